#!/usr/bin/env python3
"""What the comparison of two bands diagonal by diagonal costs, on the bands tools/stripes_vs_host.py builds.

On two bands of the shape of GRCh38 chr1 at 5 kb / 3 Mb (ncols 49 792, nrows 600) in device memory whose
counts follow a distance decay -- Poisson around 600 / (d + 1), two seeds -- one process takes, after a
warm-up, HIP-event times of

  * modle_pixels_scc with a smoothing half-width of 0, 5 and 20 bins over the widest strata the band allows
    (from diagonal 1), each a launch sequence of its own into a device array (the walk and the fold);
  * modle_pixels_stripes with the mask MOMENTS on the same two bands: the other comparison of the family;
  * the count arm: modle_pixels_count on one of the bands, one pass over its words;

and the host wall time of the same sums restated in numpy on the two bands copied to the host -- the band
extended by the 2h diagonals below the main one, box sums as a running sum along the diagonals and 2h + 1
shifted adds along the bins, then one strided column per stratum -- with pixels.scc_scores on top.  The device
words are held against that restatement, word for word, before anything is timed.  No ratio is expected: the
record says what was measured.

    python tools/scc_vs_host.py [--repeats 20] [--out profiles/scc/scc_vs_host.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.pixels_vs_dense import NCOLS, NROWS  # noqa: E402
from tools.sample_vs_torch import PEAK  # noqa: E402
from tools.stripes_vs_host import make_band  # noqa: E402

SMOOTH = (0, 5, 20)


def host_rows(np, a, b, h, lo, hi):
    """uint64 [11, NROWS]: the sums of the strata lo .. hi of the host bands `a` and `b` (zero in the left-edge
    triangle), in int64 -- the counts of these bands leave it far from overflowing, which is asserted"""
    xs = []
    for band in (a, b):
        m = band[:NROWS * NCOLS].reshape(NCOLS, NROWS).astype(np.int64)
        # e[j + h, ds + 2h] = M(j - ds, j) for -2h <= ds < NROWS: below the main diagonal through the symmetry
        e = np.zeros((NCOLS + 2 * h, NROWS + 2 * h), dtype=np.int64)
        e[h:h + NCOLS, 2 * h:] = m
        for k in range(1, 2 * h + 1):
            e[h:h + NCOLS - k, 2 * h - k] = m[k:, k]
        # s[:, k] = the sum of e[:, k - 2h .. k]: the cells of one column of the matrix in a box
        c = np.cumsum(e, axis=1)
        s = c.copy()
        s[:, 2 * h + 1:] -= c[:, :-(2 * h + 1)]
        x = np.zeros((NCOLS, NROWS), dtype=np.int64)
        for dj in range(-h, h + 1):
            # the column j + dj of the matrix: its cells of the box of (j - d, j) end at diagonal d + dj + h
            x[:, lo:hi + 1] += s[h + dj:h + dj + NCOLS, lo + dj + 3 * h:hi + 1 + dj + 3 * h]
        xs.append(x)
    out = np.zeros((11, NROWS), dtype=np.uint64)
    for d in range(lo, hi + 1):
        p, q = xs[0][d:, d], xs[1][d:, d]
        assert int(p.max()) ** 2 * len(p) < 2**63 and int(q.max()) ** 2 * len(q) < 2**63
        out[0, d] = np.count_nonzero(p | q)
        for k, v in enumerate((p.sum(), q.sum(), p @ p, q @ q, p @ q)):
            out[1 + 2 * k, d] = int(v)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the record to this file")
    a = ap.parse_args()

    from modle_amd import pixels  # (loads the HIP runtime torch ships, see _lib.py)
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device and has no fallback")
    dev = torch.device("cuda", 0)
    ref, tgt = make_band(torch, dev, 7), make_band(torch, dev, 8)
    torch.cuda.synchronize()
    ex = pixels.Extractor(0)
    stream = torch.cuda.Stream(device=dev)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        """event times, ms, of `fn()` enqueued on `stream`: a.repeats after a.warmup"""
        out = []
        for it in range(a.warmup + a.repeats):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            fn()
            t1.record(stream)
            t1.synchronize()
            if it >= a.warmup:
                out.append(t0.elapsed_time(t1))
        return out

    def line(what, ms):
        med = statistics.median(ms)
        say(f"  {what:<66} median {med:8.4f} ms  min {min(ms):8.4f}  max {max(ms):8.4f}")
        return med

    stats = [ex.count(t.data_ptr(), NROWS, NCOLS, stream=stream) for t in (ref, tgt)]
    say(f"bands: nrows {NROWS}, ncols {NCOLS}, counts Poisson around {PEAK:g} / (d + 1), two seeds: sums {stats[0].sum} "
        f"and {stats[1].sum}, {4 * (NROWS * NCOLS + 1) / 1e6:.1f} MB each")
    say(f"device: {torch.cuda.get_device_name(0)}; HIP-event times on one stream, {a.repeats} runs after "
        f"{a.warmup} warm-up; at most {pixels.scc_groups()} workgroups walk a strip of 64 diagonals")

    # what is timed is right: every word against the numpy restatement on the host, whose time is the host arm
    t0 = time.perf_counter()
    h_ref, h_tgt = ref.cpu().numpy().view(np.uint32), tgt.cpu().numpy().view(np.uint32)
    copy_s = time.perf_counter() - t0
    out = torch.empty((pixels.SCC_ROWS, NROWS), dtype=torch.int64, device=dev)
    host = {}
    for h in SMOOTH:
        lo, hi = 1, NROWS - 1 - 2 * h
        ex.scc_into(ref.data_ptr(), tgt.data_ptr(), NROWS, NCOLS, h, lo, hi, out.data_ptr(), out.numel(), stream=stream)
        stream.synchronize()
        rows = out.cpu().numpy().view(np.uint64)
        t0 = time.perf_counter()
        want = host_rows(np, h_ref, h_tgt, h, lo, hi)
        sums_s = time.perf_counter() - t0
        assert np.array_equal(rows, want), f"h = {h}: the device words differ from the host's"
        t0 = time.perf_counter()
        scc = pixels.scc_scores(rows, NCOLS, lo, hi)[0]
        host[h] = (sums_s, time.perf_counter() - t0, scc, hi)
    say("checked: for every smoothing the eleven words of every stratum equal their numpy restatement on the host")

    count_ms = line("count arm: modle_pixels_count on one band (reads every word once)",
                    timed(lambda: ex.count(ref.data_ptr(), NROWS, NCOLS, stream=stream)))
    stripes_out = torch.empty((2, 9, NCOLS), dtype=torch.int64, device=dev)
    stripes_ms = line("modle_pixels_stripes, MOMENTS", timed(lambda: ex.stripes_into(
        ref.data_ptr(), tgt.data_ptr(), NROWS, NCOLS, 1, stripes_out.data_ptr(), stripes_out.numel(), stream=stream)))
    for h in SMOOTH:
        lo, hi = 1, NROWS - 1 - 2 * h
        ms = line(f"modle_pixels_scc, smooth {h}, diagonals {lo} .. {hi}", timed(lambda: ex.scc_into(
            ref.data_ptr(), tgt.data_ptr(), NROWS, NCOLS, h, lo, hi, out.data_ptr(), out.numel(), stream=stream)))
        sums_s, score_s, scc, _ = host[h]
        say(f"      {ms / stripes_ms:.2f} x the stripes' moments, {ms / count_ms:.2f} x the count arm; on the host the "
            f"same sums take {sums_s:.2f} s in numpy ({sums_s * 1e3 / ms:.0f} x) and pixels.scc_scores {score_s * 1e3:.1f} ms; "
            f"SCC {scc:.6f}")
    say(f"host arm: the two bands copied to the host in {copy_s:.2f} s, once")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
