#!/usr/bin/env python3
"""What the marginals of a band cost, on the band tools/pixels_vs_dense.py uses.

On a band of the shape of GRCh38 chr1 at 5 kb / 3 Mb (ncols 49 792, nrows 600, about 11.6 % of the
pixels non-zero) in device memory, one process takes, after a warm-up, HIP-event times of

  * modle_pixels_count on the band (two memsets, pixels_count, pixels_scan and the copy of the
    statistics): the yardstick, a kernel that reads the same words once;
  * modle_pixels_marginals into device arrays (two memsets, pixels_marginals, two copies of
    nrows + ncols words), for both results, for each alone, and with the first two diagonals left out
    of the coverage, with the achieved bytes per second: pixel words read over the time.

The results of the timed calls are checked against the statistics of the count.

    python tools/marginals_vs_count.py [--repeats 20] [--out profiles/marginals/marginals_vs_count.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.pixels_vs_dense import NCOLS, NROWS, make_band  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from modle_amd import pixels  # (loads the HIP runtime torch ships, see _lib.py)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device and has no fallback")
    dev = torch.device("cuda", 0)
    band = make_band(torch, dev)
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

    def line(what, ms, nbytes):
        med = statistics.median(ms)
        say(f"  {what:<62} median {med:8.4f} ms  min {min(ms):8.4f}  max {max(ms):8.4f}"
            f"  {nbytes / med / 1e6:8.1f} GB/s")
        return med

    pixel_words = NROWS * NCOLS - NROWS * (NROWS - 1) // 2  # without the left-edge triangle
    stats = ex.count(band.data_ptr(), NROWS, NCOLS, stream=stream)
    say(f"band: nrows {NROWS}, ncols {NCOLS}, {pixel_words} pixel words, nnz {stats.nnz}, sum {stats.sum}")
    say(f"device: {torch.cuda.get_device_name(0)}; HIP-event times on one stream, {a.repeats} runs after "
        f"{a.warmup} warm-up")
    base = line("modle_pixels_count (reads every pixel word once)",
                timed(lambda: ex.count(band.data_ptr(), NROWS, NCOLS, stream=stream)), 4 * pixel_words)
    diag = torch.empty(NROWS, dtype=torch.int64, device=dev)
    cov = torch.empty(NCOLS, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    for what, min_diag, d_diag, d_cov in (("diag_sum and coverage", 0, diag, cov), ("diag_sum alone", 0, diag, None),
                                          ("coverage alone", 0, None, cov),
                                          ("diag_sum and coverage, min_diag 2", 2, diag, cov)):
        ms = timed(lambda: ex.marginals_into(band.data_ptr(), NROWS, NCOLS, min_diag,
                                             None if d_diag is None else d_diag.data_ptr(),
                                             None if d_cov is None else d_cov.data_ptr(), stream=stream))
        med = line(f"modle_pixels_marginals: {what}", ms, 4 * pixel_words)
        say(f"      = {med / base:.2f} x the count")
        stream.synchronize()
        d = [int(x) for x in diag.tolist()]
        assert sum(d) == stats.sum
        if d_cov is not None:  # every kept pixel counts twice, one of the main diagonal once
            assert int(cov.sum()) == 2 * sum(d[max(min_diag, 1):]) + (d[0] if min_diag == 0 else 0)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
