#!/usr/bin/env python3
"""What the statistical test of the dot calling costs, on the band tools/dots_vs_count.py uses.

On a band of the shape of GRCh38 chr1 at 5 kb / 3 Mb (ncols 49 792, nrows 600) in device memory, one process
takes, after a warm-up, HIP-event times of

  * modle_pixels_count on the band: a kernel that reads every pixel word once;
  * modle_pixels_dots into d_cand alone (the fold decision), re-measured here;
  * modle_pixels_dot_hist into a table on the device (the copy of the tables and the kernel: the LDS counts of a
    workgroup flushed with 64-bit integer atomics, the one flush form that was built), HiCCUPS' 40 edges, n_obs =
    min(the largest count + 2, 16384);
  * modle_pixels_dots_fdr into d_cand (the threshold decision with the fold test on), against thresholds that
    pixels.dot_thresholds takes from that table at a rate of 0.1

for window half-widths of 5, 10 and 20 bins (peak 2, 4, 7), on three bands: the distance-decay band of the other
records; a constant band of 3, where every pixel of a workgroup hits the same few LDS words; and a constant band
of 40, where every pixel goes to the same few words of the table in device memory -- the worst cases of the
counting.  The table of every timed histogram call is checked: it holds the valid pixels once per call.

    python tools/dots_fdr_vs_dots.py [--repeats 20] [--out profiles/dots_fdr/dots_fdr_vs_dots.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.pixels_vs_dense import NCOLS, NROWS, make_band  # noqa: E402

WINDOWS = ((5, 2), (10, 4), (20, 7))  # (w, p)
MIN_DIAG, MIN_COUNT, FDR = 2, 1, 0.1


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
    ex = pixels.Extractor(0)
    stream = torch.cuda.Stream(device=dev)
    edges = pixels.dot_lambda_edges()
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
        say(f"  {what:<58} median {med:8.4f} ms  min {min(ms):8.4f}  max {max(ms):8.4f}")
        return med

    decay = make_band(torch, dev)
    words = NROWS * NCOLS
    say(f"device: {torch.cuda.get_device_name(0)}; HIP-event times on one stream, {a.repeats} runs after {a.warmup} "
        f"warm-up; min_diag {MIN_DIAG}, min_count {MIN_COUNT}, HiCCUPS' folds and {len(edges)} edges, fdr {FDR}")
    say("flush form: 64-bit integer atomics into the table (the only one built)")
    for name, band in (("distance-decay band", decay), ("constant band of 3", torch.full_like(decay, 3)),
                       ("constant band of 40", torch.full_like(decay, 40))):
        stats = ex.count(band.data_ptr(), NROWS, NCOLS, stream=stream)
        n_obs = min(int(stats.max_count) + 2, pixels.MAX_DOT_OBS)
        diag_sum, _ = ex.marginals(band.data_ptr(), NROWS, NCOLS, stream=stream)
        say(f"{name}: nrows {NROWS}, ncols {NCOLS}, nnz {stats.nnz}, sum {stats.sum}, largest count {stats.max_count}, "
            f"n_obs {n_obs}")
        count_ms = line("modle_pixels_count", timed(lambda: ex.count(band.data_ptr(), NROWS, NCOLS, stream=stream)))
        cand = torch.empty(words + 1, dtype=torch.int32, device=dev)
        for w, p in WINDOWS:
            scale = pixels.dot_scales(diag_sum, NCOLS, w, p, pixels.DOT_FOLDS, MIN_DIAG)
            lam = pixels.dot_scales(diag_sum, NCOLS, w, p, (1.0, 1.0, 1.0, 1.0), MIN_DIAG)
            valid = sum(max(0, NCOLS - 2 * w - d) for d in range(2 * w + MIN_DIAG, NROWS - 2 * w))
            table = torch.zeros((4, len(edges) + 1, n_obs), dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            fold_ms = line(f"w {w:2}, p {p}: modle_pixels_dots, d_cand alone",
                           timed(lambda: ex.dots_into(band.data_ptr(), NROWS, NCOLS, w, p, MIN_DIAG, MIN_COUNT, scale,
                                                      cand.data_ptr(), None, stream=stream)))
            n_fold = ex.count(cand.data_ptr(), NROWS, NCOLS, stream=stream).nnz
            hist_ms = line(f"w {w:2}, p {p}: modle_pixels_dot_hist",
                           timed(lambda: ex.dot_hist_into(band.data_ptr(), NROWS, NCOLS, w, p, MIN_DIAG, lam, edges, n_obs,
                                                          table.data_ptr(), stream=stream)))
            stream.synchronize()
            hist = table.cpu().numpy().view(np.uint64)
            calls = a.warmup + a.repeats
            assert all(int(hist[k].sum()) == calls * valid for k in range(4)) and not (hist % np.uint64(calls)).any()
            hist //= np.uint64(calls)
            thr = pixels.dot_thresholds(hist, edges, FDR)
            fdr_ms = line(f"w {w:2}, p {p}: modle_pixels_dots_fdr, fold test on",
                          timed(lambda: ex.dots_fdr_into(band.data_ptr(), NROWS, NCOLS, w, p, MIN_DIAG, MIN_COUNT, lam,
                                                         edges, thr, scale, cand.data_ptr(), stream=stream)))
            n_fdr = ex.count(cand.data_ptr(), NROWS, NCOLS, stream=stream).nnz
            say(f"      histogram = {hist_ms / fold_ms:.2f} x the fold decision, {hist_ms / count_ms:.2f} x the count; "
                f"threshold decision = {fdr_ms / fold_ms:.2f} x the fold decision, {fdr_ms / count_ms:.2f} x the count")
            say(f"      {valid} valid pixels counted once per call in {np.count_nonzero(hist[0].sum(axis=1))} chunks "
                f"(donut); thresholds set in {np.count_nonzero(thr)} of {thr.size} chunks; {n_fold} candidates by fold "
                f"alone, {n_fdr} with the thresholds")
        del cand
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
