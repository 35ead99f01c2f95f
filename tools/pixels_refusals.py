#!/usr/bin/env python3
"""What libmodle_pixels.so refuses before its first HIP call, as a table (include/modle_pixels.h).

    python tools/pixels_refusals.py modle_amd/libmodle_pixels.so tests/golden/pixels_refusals.json

Every case calls one entry point with arguments that the library refuses on the host, so neither a device nor a
real context is needed: the handle, the bands and the device arrays are addresses inside one host array that the
library never follows.  Every `const T**` output is preset to a sentinel.  Recorded per case: the return code,
the message, and what became of each output pointer ("kept", "null" or "other").  tests/test_pixels_refusals.py
holds the current library against the table written from the library of the commit before a change of the
host layer."""
import ctypes as C
import json
import sys

NROWS, NCOLS = 23, 70
FACTOR, FIRST_BIN = 2, 0  # the coarse band is 12 x 35
SENTINEL = 0x5A5A5A5A5A5A5A50
U64, I64 = C.c_uint64, C.c_int64


class Arena:
    """fake device addresses: 256-byte aligned offsets into one host array"""

    def __init__(self):
        self.buf = (C.c_uint8 * (1 << 20))()
        self.base = (C.addressof(self.buf) + 255) & ~255

    def at(self, offset):
        return self.base + offset


ARENA = Arena()
HANDLE, BAND, BAND2 = ARENA.at(0), ARENA.at(1 << 16), ARENA.at(2 << 16)
OUT, OUT2, OUT3 = ARENA.at(3 << 16), ARENA.at(4 << 16), ARENA.at(5 << 16)
LIST1, LIST2, LIST3 = ARENA.at(6 << 16), ARENA.at(7 << 16), ARENA.at(8 << 16)
BAND_BYTES = (NROWS * NCOLS + 1) * 4

# host tables of the analyses (read by the library's checks)
ONES = (C.c_double * (4 * NROWS))(*([1.0] * (4 * NROWS)))
EDGES = (C.c_double * 2)(1.0, 2.0)
THR = (C.c_uint32 * 12)(*([1] * 12))
WINDOWS = (U64 * 2)(1, 2)
ANCHOR1, ANCHOR2 = (I64 * 3)(3, 4, 5), (I64 * 3)(4, 6, 8)
STATS = (C.c_uint64 * 4)()       # modle_pixels_stats
BAND_STATS = (C.c_uint64 * 12)()  # modle_pixels_band_stats, with room


def ptr(x):
    return C.c_void_p(x if isinstance(x, int) else C.addressof(x))


class Out:
    """the name of a `const T**` output of a call"""

    def __init__(self, name):
        self.name = name


PIXEL_OUTS = [Out("bin1"), Out("bin2"), Out("count"), Out("bin1_offset")]


def entry_points():
    """name -> (arguments by name in call order, the analysis' own refusals as {case: {argument: value}})"""
    shape = [("h", HANDLE), ("d_band", BAND), ("nrows", NROWS), ("ncols", NCOLS)]
    coarse = shape + [("factor", FACTOR), ("first_bin", FIRST_BIN)]
    pix = [("bin_offset", I64(7))] + [(o.name, o) for o in PIXEL_OUTS] + [("stats", STATS), ("stream", None)]
    dots = [("w", 1), ("p", 0), ("min_diag", 0), ("min_count", 1), ("scale", ONES)]
    hist = [("w", 1), ("p", 0), ("min_diag", 0), ("lam", ONES), ("edges", EDGES), ("n_edges", 2), ("n_obs", 33)]
    fdr = [("w", 1), ("p", 0), ("min_diag", 0), ("min_count", 1), ("lam", ONES), ("edges", EDGES), ("n_edges", 2),
           ("thr", THR), ("scale", ONES)]
    wins = [("windows", WINDOWS), ("n_windows", 2), ("min_diag", 1)]
    pile = [("flank", 1), ("bin_offset", I64(0)), ("bin1", ANCHOR1), ("bin2", ANCHOR2), ("n", 3)]
    resc = [("size", 2), ("bin_offset", I64(0)), ("start", ANCHOR1), ("end", ANCHOR2), ("n", 3)]
    one = lambda *names: [(n, Out(n)) for n in names] + [("stream", None)]
    pair = [("h", HANDLE), ("d_ref", BAND), ("d_tgt", BAND2), ("nrows", NROWS), ("ncols", NCOLS)]
    p_ge_w = {"p >= w": {"p": 1}}
    table = {}
    for stem, args, own in [
            ("to_host", pix, {"bin_offset < 0": {"bin_offset": I64(-1)}}),
            ("marginals_to_host", [("min_diag", 1)] + one("diag_sum", "coverage"), {}),
            ("insulation_to_host", wins + one("ins_sum"), {"no window": {"n_windows": 0}}),
            ("dots_to_host", dots + pix, p_ge_w),
            ("dot_hist_to_host", hist + one("hist"), {**p_ge_w, "n_obs == 1": {"n_obs": 1}, "n_edges == 0": {"n_edges": 0}}),
            ("dots_fdr_to_host", fdr + pix, {**p_ge_w, "n_edges == 0": {"n_edges": 0}}),
            ("pileup_to_host", pile + one("pile", "n_used"), {"flank 33": {"flank": 33}}),
            ("rescale_to_host", resc + one("pile", "area", "n_used"), {"size 129": {"size": 129}})]:
        table["modle_pixels_" + stem] = (shape + args, own)
        table["modle_pixels_coarse_" + stem] = (coarse + args, {"factor == 1": {"factor": 1}, **own})
    table["modle_pixels_stripes_to_host"] = (pair + [("what", 1)] + one("rows"), {"what == 0": {"what": 0}})
    table["modle_pixels_scc_to_host"] = (pair + [("smooth", 0), ("min_diag", 1), ("max_diag", 5)] + one("rows"),
                                         {"min_diag > max_diag": {"min_diag": 6}})
    # the forms that enqueue: their outputs are device arrays, and an output that shares a byte with an input or
    # with another output is refused
    dev = [("stream", None)]
    table["modle_pixels_marginals"] = (
        shape + [("min_diag", 1), ("d_diag_sum", OUT), ("d_coverage", OUT2)] + dev,
        {"diag_sum on the band": {"d_diag_sum": BAND + BAND_BYTES - 8}, "coverage on the band": {"d_coverage": BAND},
         "misaligned": {"d_coverage": OUT2 + 2}})
    table["modle_pixels_insulation"] = (
        shape + wins + [("d_out", OUT), ("out_words", 2 * NCOLS)] + dev,
        {"no window": {"n_windows": 0}, "out on the band": {"d_out": BAND + 8}})
    table["modle_pixels_dots"] = (
        shape + dots + [("d_cand", OUT), ("d_sums", OUT2)] + dev,
        {**p_ge_w, "cand on the band": {"d_cand": BAND + BAND_BYTES - 4}, "sums on the band": {"d_sums": BAND + 8},
         "sums on cand": {"d_sums": OUT + 8}, "sums on the band, no cand": {"d_cand": None, "d_sums": BAND}})
    table["modle_pixels_dot_hist"] = (
        shape + hist + [("d_hist", OUT)] + dev,
        {**p_ge_w, "n_obs == 1": {"n_obs": 1}, "n_edges == 0": {"n_edges": 0}, "hist on the band": {"d_hist": BAND + 8}})
    table["modle_pixels_dots_fdr"] = (
        shape + fdr + [("d_cand", OUT)] + dev,
        {**p_ge_w, "n_edges == 0": {"n_edges": 0}, "cand on the band": {"d_cand": BAND - 4}})
    table["modle_pixels_pileup"] = (
        shape + [("flank", 1), ("bin_offset", I64(0)), ("d_bin1", LIST1), ("d_bin2", LIST2), ("n", 3), ("d_pile", OUT),
                 ("d_n_used", OUT2)] + dev,
        {"flank 33": {"flank": 33}, "pile on the band": {"d_pile": BAND + 16}, "pile on bin1": {"d_pile": LIST1 + 16},
         "pile on bin2": {"d_pile": LIST2 - 8}, "n_used on the band": {"d_n_used": BAND}, "n_used on bin1": {"d_n_used": LIST1},
         "n_used on bin2": {"d_n_used": LIST2 + 16}, "n_used on pile": {"d_n_used": OUT + 64},
         "misaligned n_used": {"d_n_used": OUT2 + 4}})
    table["modle_pixels_rescale"] = (
        shape + [("size", 2), ("bin_offset", I64(0)), ("d_start", LIST1), ("d_end", LIST2), ("n", 3), ("d_pile", OUT),
                 ("d_area", OUT2), ("d_n_used", OUT3)] + dev,
        {"size 129": {"size": 129}, "pile on the band": {"d_pile": BAND + 16}, "pile on start": {"d_pile": LIST1 + 16},
         "area on end": {"d_area": LIST2 - 8}, "area on the band": {"d_area": BAND + (BAND_BYTES - 1) // 8 * 8},
         "n_used on the band": {"d_n_used": BAND}, "n_used on start": {"d_n_used": LIST1},
         "n_used on end": {"d_n_used": LIST2 + 16}, "n_used on pile": {"d_n_used": OUT + 24},
         "n_used on area": {"d_n_used": OUT2}, "area on pile": {"d_area": OUT + 8}})
    table["modle_pixels_sample"] = (
        shape + [("bin_offset", I64(0)), ("threshold", 1 << 31), ("seed", 1), ("salt", C.c_uint32(0)), ("stats", STATS),
                 ("d_kept", OUT), ("d_rest", OUT2)] + dev,
        {"threshold > 2^32": {"threshold": (1 << 32) + 1}, "bin_offset < 0": {"bin_offset": I64(-1)},
         "kept on the band": {"d_kept": BAND + BAND_BYTES - 4}, "rest on the band": {"d_rest": BAND - 4},
         "rest on kept": {"d_rest": OUT + 4}, "rest on the band, no kept": {"d_kept": None, "d_rest": BAND}})
    table["modle_pixels_stripes"] = (
        pair + [("what", 1), ("d_out", OUT), ("out_words", 2 * 9 * NCOLS)] + dev,
        {"what == 0": {"what": 0}, "out on ref": {"d_out": BAND + 8}, "out on tgt": {"d_out": BAND2 - 8}})
    table["modle_pixels_scc"] = (
        pair + [("smooth", 0), ("min_diag", 1), ("max_diag", 5), ("d_out", OUT), ("out_words", 11 * NROWS)] + dev,
        {"min_diag > max_diag": {"min_diag": 6}, "out on ref": {"d_out": BAND + 8}, "out on tgt": {"d_out": BAND2 - 8}})
    pixels = [("d_bin1", LIST1), ("d_bin2", LIST2), ("d_count", LIST3), ("n", 3)]
    table["modle_pixels_band_check"] = (
        [("h", HANDLE)] + pixels + [("nrows", NROWS), ("ncols", NCOLS), ("bin_offset", I64(0)), ("d_row_start", OUT),
                                    ("stats", BAND_STATS)] + dev,
        {"n >= 2^31": {"n": 1 << 31}, "row_start on bin1": {"d_row_start": LIST1 + 16},
         "row_start on bin2": {"d_row_start": LIST2 - 8}, "row_start on count": {"d_row_start": LIST3 + 8}})
    table["modle_pixels_band_fill"] = (
        [("h", HANDLE)] + pixels[1:] + [("nrows", NROWS), ("ncols", NCOLS), ("bin_offset", I64(0)), ("d_row_start", OUT2),
                                        ("d_out", OUT), ("out_words", NROWS * NCOLS + 1)] + dev,
        {"n >= 2^31": {"n": 1 << 31}, "out on bin2": {"d_out": LIST2 + 16}, "out on count": {"d_out": LIST3 - 4},
         "out on row_start": {"d_out": OUT2 + 8 * NCOLS + 4}})
    return table


def cases_of(args, own):
    """{case: {argument: value}}: the refusals every entry point shares, where it has the argument, then its own"""
    names = [n for n, _ in args]
    cases = {"null handle": {"h": None}}
    for band in ("d_band", "d_ref", "d_tgt"):
        if band in names:
            cases["null " + band] = {band: None}
    cases["nrows > ncols"] = {"nrows": NCOLS + 1}
    cases["nrows == 0"] = {"nrows": 0}
    outs = [n for n, v in args if isinstance(v, Out)]
    if outs == ["diag_sum", "coverage"]:  # either may be null, not both
        cases["null outputs"] = {"diag_sum": None, "coverage": None}
    else:
        for n in outs:
            cases["null " + n] = {n: None}
    if "stats" in names:
        cases["null stats"] = {"stats": None}
    for n in ("d_out", "d_pile", "d_hist"):
        if n in names:
            cases["null " + n] = {n: None}
    cases.update(own)
    return cases


def call(lib, name, args, change):
    slots, argv = {}, []
    for arg, value in args:
        value = change.get(arg, value)
        if isinstance(value, Out):
            slots[arg] = C.c_void_p(SENTINEL)
            argv.append(C.byref(slots[arg]))
        elif isinstance(value, int) and not isinstance(value, bool):
            # addresses and sizes alike travel as 64-bit words
            argv.append(U64(value))
        elif value is None or isinstance(value, (I64, C.c_uint32)):
            argv.append(C.c_void_p(None) if value is None else value)
        else:
            argv.append(ptr(value))
    err = C.create_string_buffer(b"(nothing written)", 1024)
    fn = getattr(lib, name)
    fn.restype = C.c_int
    rc = fn(*argv, err, C.c_size_t(len(err)))
    state = {n: "kept" if s.value == SENTINEL else "null" if not s.value else "other" for n, s in slots.items()}
    return {"rc": rc, "message": err.value.decode(errors="replace"), "outputs": state}


def run(path):
    lib = C.CDLL(path)
    result = {}
    for name, (args, own) in entry_points().items():
        for case, change in cases_of(args, own).items():
            if not set(change) <= {n for n, _ in args}:
                raise KeyError(f"{name}: {case} names an argument the entry point does not have")
            result[f"{name}: {case}"] = call(lib, name, args, change)
    return result


def main(argv):
    if len(argv) != 3:
        sys.exit(__doc__)
    result = run(argv[1])
    accepted = [k for k, v in result.items() if v["rc"] not in (-1, -3)]
    if accepted:
        sys.exit("not refused on the host (the table must hold refusals only): " + "; ".join(accepted))
    with open(argv[2], "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(result)} cases -> {argv[2]}")


if __name__ == "__main__":
    main(sys.argv)
