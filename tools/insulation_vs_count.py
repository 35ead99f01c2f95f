#!/usr/bin/env python3
"""What the insulation sums of a band cost, on the band tools/pixels_vs_dense.py uses.

On a band of the shape of GRCh38 chr1 at 5 kb / 3 Mb (ncols 49 792, nrows 600, about 11.6 % of the
pixels non-zero) in device memory, one process takes, after a warm-up, HIP-event times of

  * modle_pixels_count on the band (two memsets, pixels_count, pixels_scan and the copy of the
    statistics): the yardstick, a kernel that reads every pixel word once;
  * modle_pixels_insulation into a device array (one kernel, nothing else) for windows of 20, 100 and 300
    bins, each alone and all three in one call, with the words of the band the call addresses: of each
    column the first 2 w - 1 words, once per group of 64 bins that needs the column, (63 + w) / 64 times.

The results of the timed calls are checked against the diagonal sums of modle_pixels_marginals.

    python tools/insulation_vs_count.py [--repeats 20] [--out profiles/insulation/insulation_vs_count.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.pixels_vs_dense import NCOLS, NROWS, make_band  # noqa: E402

WINDOWS = (20, 100, 300)
MIN_DIAG = 2


def words_addressed(windows):
    """the band words one call loads: per group of 64 bins and column of its halo, what the windows that
    still reach the column need (modle_insulation.hip); the left edge and the last group are not trimmed"""
    wmax, total = max(windows), 0
    for jj in range(63 + wmax):
        tmin = max(jj - 63, 0)
        total += max(min(jj, w - 1) + w - 1 for w in windows if w > tmin) + 1
    return total * ((NCOLS + 63) // 64)


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
    diag_sum, _ = ex.marginals(band.data_ptr(), NROWS, NCOLS, stream=stream)
    say(f"band: nrows {NROWS}, ncols {NCOLS}, {pixel_words} pixel words, nnz {stats.nnz}, sum {stats.sum}")
    say(f"device: {torch.cuda.get_device_name(0)}; HIP-event times on one stream, {a.repeats} runs after "
        f"{a.warmup} warm-up; min_diag {MIN_DIAG}")
    base = line("modle_pixels_count (reads every pixel word once)",
                timed(lambda: ex.count(band.data_ptr(), NROWS, NCOLS, stream=stream)), 4 * pixel_words)
    for windows in [(w,) for w in WINDOWS] + [WINDOWS]:
        out = torch.empty((len(windows), NCOLS), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        ms = timed(lambda: ex.insulation_into(band.data_ptr(), NROWS, NCOLS, windows, MIN_DIAG, out.data_ptr(),
                                              out.numel(), stream=stream))
        words = words_addressed(windows)
        med = line(f"modle_pixels_insulation: windows {', '.join(map(str, windows))}", ms, 4 * words)
        say(f"      = {med / base:.2f} x the count; {words} words addressed = {words / pixel_words:.2f} x the band's "
            f"pixel words, column halo (63 + wmax) / 64 = {(63 + max(windows)) / 64:.2f}")
        stream.synchronize()
        got = out.cpu().tolist()
        for k, w in enumerate(windows):
            want = sum(min(d + 1, 2 * w - 1 - d) * int(diag_sum[d]) for d in range(MIN_DIAG, 2 * w - 1))
            assert sum(got[k]) == want, (w, sum(got[k]), want)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
