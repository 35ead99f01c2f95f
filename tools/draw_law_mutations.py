#!/usr/bin/env python3
"""What the law tests of the random draws (tests/test_oracle_draw_laws.py) resolve, shown on mutants.

Copies oracle/ (with the two headers and the table generator its Makefile names) into a temporary
directory, applies ONE named substitution at a time, builds, draws in C and runs the statistics of
tests/draw_laws.py on every regime of tests/draw_cases.py.  Prints, per mutant, which statistics fall
below the pass line and with what p.  Not a test; the suite does not run it.

    python tools/draw_law_mutations.py                    # every mutant, to stdout
    python tools/draw_law_mutations.py --only ptrd_2.53   # one
    python tools/draw_law_mutations.py --record profiles/draw_laws   # writes mutations.txt and oracle_p_values.txt

The instrument catches gross errors and whole wrong branches, not fifth digits: the mutants under
BEYOND REACH move the law by less than 4 000 000 draws resolve, or only the sampler's efficiency.
Nobody should read the suite as pinning them."""
import argparse
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import draw_cases as dc  # noqa: E402
import draw_laws as dl  # noqa: E402

SRC = "oracle/modle_oracle.c"
ZIG = "oracle/zig_tables.h"


def _swap_zig_rows(i, j):
    """rows i and j of ZIG_NORM_X change places"""
    def edit(text):
        m = re.search(r"(static const double ZIG_NORM_X\[129\] = \{)(.*?)(\};)", text, re.S)
        lits = re.findall(r"0x[0-9a-f.]+p[+-]\d+", m.group(2))
        body = m.group(2).replace(lits[i], "@A@").replace(lits[j], lits[i]).replace("@A@", lits[j])
        return text[:m.start(2)] + body + text[m.end(2):]
    return edit


# name -> (must be caught?, file, [(old, new, occurrences)] or a function of the text, what it is)
MUTANTS = [
    ("ptrd_btrd_2.53", True, SRC, [("2.53 * ", "2.35 * ", 2)], "2.53 -> 2.35 in b of both PTRD and BTRD"),
    ("ptrd_1.1239", True, SRC, [("1.1239 + ", "1.2139 + ", 1)], "1.1239 -> 1.2139 in PTRD's 1 / alpha"),
    ("log_fact_6", True, SRC, [("6.5792512120101012", "6.5972512120101012", 1)],
     "log_fact[6]: two digits swapped (6.5792 -> 6.5972)"),
    ("zig_norm_x_rows_10_100", True, ZIG, _swap_zig_rows(10, 100), "rows 10 and 100 of zig_norm_x swapped"),
    ("bucket_increment", True, SRC, [("  if (UINT64_MAX % (range + 1) == range) ++bucket;\n", "", 1)],
     "++bucket removed from the bucket rule of uniform_int"),
    ("binomial_mirror", True, SRC, [("return (0.5 < p_) ? t - x : x;", "return x;", 1),
                                    ("return (0.5 < p_) ? t - k : k;", "return k;", 1)],
     "the mirror t - k dropped for p > 0.5"),
    ("zig_norm_x_rows_40_41", False, ZIG, _swap_zig_rows(40, 41),
     "rows 40 and 41 of zig_norm_x swapped: neighbours differ by 1 % in one layer of 128"),
    ("ptrd_0.445", False, SRC, [("+ 0.445)", "+ 0.455)", 2)], "0.445 -> 0.455 in PTRD's k"),
    ("ptrd_3.6224", False, SRC, [("3.6224 / ", "3.2624 / ", 1)], "3.6224 -> 3.2624 in PTRD's v_r"),
    ("btrd_0.0248", False, SRC, [("0.0248 * b", "0.0284 * b", 1)], "0.0248 -> 0.0284 in BTRD's a"),
    ("binom_fc_2", False, SRC, [("0.02767792568499834", "0.02776792568499834", 1)],
     "binom_fc table entry 2 off by 9e-5"),
]


def copy_oracle(dst):
    shutil.copytree(os.path.join(ROOT, "oracle"), os.path.join(dst, "oracle"),
                    ignore=shutil.ignore_patterns("*.so", "__pycache__", "_ref"))
    os.makedirs(os.path.join(dst, "modle_amd", "csrc"))
    for h in ("modle_math.h", "modle_math_tables.h"):
        shutil.copy2(os.path.join(ROOT, "modle_amd", "csrc", h), os.path.join(dst, "modle_amd", "csrc", h))
    os.makedirs(os.path.join(dst, "tools"))
    shutil.copy2(os.path.join(ROOT, "tools", "gen_ziggurat_tables.py"), os.path.join(dst, "tools"))


def build_mutant(dst, path, edits):
    full = os.path.join(dst, path)
    text = open(full).read()
    if callable(edits):
        new = edits(text)
        assert new != text
    else:
        new = text
        for old, repl, count in edits:
            assert new.count(old) == count, f"{old!r} occurs {new.count(old)} times in {path}, expected {count}"
            new = new.replace(old, repl)
    with open(full, "w") as f:
        f.write(new)
    subprocess.run(["make", "-C", os.path.join(dst, "oracle"), "libmodle_oracle.so"], check=True, capture_output=True)
    return load(os.path.join(dst, "oracle", "libmodle_oracle.so"))


def load(so):
    L = C.CDLL(so)
    u64p = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")
    L.mo_draw_many.argtypes = [C.c_uint32, u64p, C.c_uint64, C.c_size_t, u64p, C.POINTER(C.c_uint64)]
    L.mo_draw_many.restype = C.c_int
    L.mo_binom_fc.argtypes = [C.c_int64]
    L.mo_binom_fc.restype = C.c_double
    L.mo_uniform_int_bucket.argtypes = [C.c_uint64]
    L.mo_uniform_int_bucket.restype = C.c_uint64
    return L


def draw_many(L, regime, seed, n):
    out = np.zeros(n, dtype=np.uint64)
    consumed = C.c_uint64(0)
    assert L.mo_draw_many(regime.kind, np.array(regime.words, dtype=np.uint64), seed, n, out, C.byref(consumed)) == 0
    return out, consumed.value


def run_all(L, zig):
    """every statistic of the law tests on library L: [(regime or check, statistic, p)]"""
    res = []
    for regime in dc.REGIMES:
        draws, consumed = draw_many(L, regime, dl.SEED, dl.N_DRAWS)
        for name, p in dl.statistics(regime, draws, consumed, zig).items():
            res.append((regime.name, name, p))
    normal = next(r for r in dc.REGIMES if r.name == "normal_0_1")
    ratios = [draw_many(L, normal, 1000 + s, 10_000)[1] / 10_000 for s in range(400)]
    res.append(("normal_outputs_per_draw", "ratio_z", dl.normal_outputs_ratio_p(ratios, zig)))
    dev = dl.binom_fc_deviation(L.mo_binom_fc)
    res.append(("binom_fc (deterministic)", f"deviation {dev:.3g} <= {dl.FC_LIMIT:.3g}", 1.0 if dev <= dl.FC_LIMIT else 0.0))
    ok = all(L.mo_uniform_int_bucket(r) == dc.bucket_of(r) for r in dc.RANGES)
    res.append(("bucket rule (deterministic)", "equals Python's integers", 1.0 if ok else 0.0))
    return res, dev, float(np.mean(ratios))


def describe(res):
    failing = [(r, s, p) for r, s, p in res if p < dl.P_LINE]
    sampled = [(r, s, p) for r, s, p in res if "deterministic" not in r]
    return failing, min(sampled, key=lambda t: t[2])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--only", help="name of one mutant")
    ap.add_argument("--record", help="directory to write mutations.txt and oracle_p_values.txt into")
    args = ap.parse_args()
    lines, plines = [], []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    with tempfile.TemporaryDirectory() as base:
        clean = os.path.join(base, "clean")
        copy_oracle(clean)
        zig = dl.read_zig_tables(os.path.join(clean, ZIG))  # the statistics read the UNMUTATED table
        say(f"{dl.N_DRAWS} draws per regime, seed {dl.SEED}; a statistic fails below p = {dl.P_LINE:g}.")
        say("The instrument catches gross errors and whole wrong branches, not fifth digits.")
        say()
        L = build_mutant(clean, SRC, [])
        base_res, dev, ratio = run_all(L, zig)
        failing, (r, s, p) = describe(base_res)
        say(f"UNMUTATED: {len(failing)} statistics below the line; smallest p {p:.3g} ({r}: {s})")
        assert not failing, failing
        say()
        plines.append(f"The unmutated oracle: smallest p per regime ({dl.N_DRAWS} draws, seed {dl.SEED}; pass line {dl.P_LINE:g})")
        for name in [x.name for x in dc.REGIMES] + ["normal_outputs_per_draw"]:
            mine = [(s, p) for r, s, p in base_res if r == name]
            s, p = min(mine, key=lambda t: t[1])
            plines.append(f"  {name:28s} {p:9.3g}  ({s}; " + ", ".join(f"{a} {b:.3g}" for a, b in mine) + ")")
        plines.append("")
        plines.append(f"engine outputs per normal draw: {dl.normal_outputs_per_draw(zig):.6f} from the table's areas, "
                      f"{ratio:.6f} in 400 samples of 10 000 draws")
        plines.append(f"binom_fc against the Stirling remainder at 50 digits, k = 0..20 and 10^6: largest deviation "
                      f"{dev:.3g}, limit {dl.FC_LIMIT:.3g}")
        import mpmath

        worst_table = max(abs(mpmath.mpf(L.mo_binom_fc(k)) - dl.stirling_remainder(k)) for k in range(10))
        plines.append(f"  (the ten table literals alone: {float(worst_table):.3g})")
        # udiv_by_uniform (the device's division of a raw output by a bucket) on the inputs of tests/draw_cases.py
        L.mo_udiv_by_uniform.argtypes = [C.c_uint64, C.c_uint64, C.c_double]
        L.mo_udiv_by_uniform.restype = C.c_uint64
        pairs = [(e[0], e[1]) for e in dc.FORMS[5][2]] + [(e[1], dc.bucket_of(e[0])) for e in dc.FORMS[2][2]]
        inside = [(raw, d) for raw, d in pairs if dc.udiv_within_bound(raw, d)]
        beyond = [(raw, d) for raw, d in pairs if not dc.udiv_within_bound(raw, d)]
        wrong = [(raw, d) for raw, d in beyond if L.mo_udiv_by_uniform(raw, d, 1.0 / d) != raw // d]
        assert all(L.mo_udiv_by_uniform(raw, d, 1.0 / d) == raw // d for raw, d in inside)
        plines.append(f"udiv_by_uniform against Python's integers: {len(inside)} inputs inside its stated bound (d <= 2^62, "
                      f"quotient < 2^40), all exact; {len(beyond)} beyond it, of which {len(wrong)} are not the plain quotient"
                      + (f" (the first: raw {wrong[0][0]:#x}, d {wrong[0][1]:#x})" if wrong else ""))
        before = {(r, s): p for r, s, p in base_res}
        for heading, want in (("MUST BE CAUGHT", True), ("BEYOND REACH of the sample", False)):
            say(f"---- {heading}")
            for name, caught, path, edits, what in MUTANTS:
                if caught != want or (args.only and args.only != name):
                    continue
                dst = os.path.join(base, name)
                copy_oracle(dst)
                res, _, _ = run_all(build_mutant(dst, path, edits), zig)
                failing, _ = describe(res)
                # the statistics the mutant moved at all (the others drew the same numbers as before)
                moved = [(r, s, p) for r, s, p in res if "deterministic" not in r and before.get((r, s)) != p]
                say(f"{name}: {what}")
                if moved:
                    r, s, p = min(moved, key=lambda t: t[2])
                    say(f"    {len(moved)} sampled statistics moved; the smallest p among them {p:.3g} ({r}: {s}; "
                        f"unmutated {before.get((r, s), float('nan')):.3g})")
                else:
                    say("    no sampled statistic moved")
                for r, s, p in failing:
                    say(f"    FAILS  {r}: {s}  p = {p:.3g}")
                if want:
                    assert failing, f"{name} must be caught"
                elif not [f for f in failing if "deterministic" not in f[0]]:
                    say("    NOT CAUGHT by any sampled statistic")
            say()
    if args.record and not args.only:
        os.makedirs(args.record, exist_ok=True)
        with open(os.path.join(args.record, "mutations.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        with open(os.path.join(args.record, "oracle_p_values.txt"), "w") as f:
            f.write("\n".join(plines) + "\n")


if __name__ == "__main__":
    main()
