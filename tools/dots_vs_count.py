#!/usr/bin/env python3
"""What dot calling on a band costs, on the band tools/pixels_vs_dense.py uses.

On a band of the shape of GRCh38 chr1 at 5 kb / 3 Mb (ncols 49 792, nrows 600, about 11.6 % of the
pixels non-zero) in device memory, one process takes, after a warm-up, HIP-event times of

  * modle_pixels_count on the band (two memsets, pixels_count, pixels_scan and the copy of the
    statistics): a kernel that reads every pixel word once;
  * a device-to-device copy of the band's size: what moving the band once costs;
  * modle_pixels_dots for window half-widths of 5, 10 and 20 bins (peak 2, 4, 7), into d_cand alone (the
    copy of the scale table, the clearing of one word and the kernel) and into d_cand and d_sums, with
    the halo factor ((T + 2 w) / T)^2 of the kernel's T = 64 block and the bytes the call stores.

The sums of the timed calls are checked on a strip of the band against a numpy summed-area table.

    python tools/dots_vs_count.py [--repeats 20] [--out profiles/dots/dots_vs_count.txt]
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
MIN_DIAG, MIN_COUNT, T = 2, 1, 64
STRIP = 900  # the first columns of the band, checked on the host


def strip_sums(band, w, p):
    """O_k of the valid pixels (j - d, j), j + w < STRIP, of the band's first STRIP columns: uint64
    [4, STRIP, NROWS], from a summed-area table of the upper triangle (the definition in
    include/modle_pixels.h)"""
    upper = np.zeros((STRIP, STRIP), dtype=np.uint64)
    for d in range(NROWS):
        j = np.arange(d, STRIP)
        upper[j - d, j] = band[j * NROWS + d]
    sat = np.zeros((STRIP + 1, STRIP + 1), dtype=np.uint64)
    sat[1:, 1:] = upper.cumsum(axis=0, dtype=np.uint64).cumsum(axis=1, dtype=np.uint64)
    jj, dd = np.arange(STRIP)[:, None], np.arange(NROWS)[None, :]
    J, D = np.nonzero((jj - dd >= w) & (jj + w < STRIP) & (dd >= 2 * w + MIN_DIAG) & (dd <= NROWS - 1 - 2 * w))
    i, j = J - D, J

    def rect(ra, rb, ca, cb):
        return sat[rb + 1, cb + 1] - sat[ra, cb + 1] - sat[rb + 1, ca] + sat[ra, ca]

    out = np.zeros((4, STRIP, NROWS), dtype=np.uint64)
    out[0, J, D] = (rect(i - w, i + w, j - w, j + w) - rect(i - p, i + p, j - p, j + p)
                    - rect(i, i, j - w, j - p - 1) - rect(i, i, j + p + 1, j + w)
                    - rect(i - w, i - p - 1, j, j) - rect(i + p + 1, i + w, j, j))
    out[1, J, D] = rect(i + 1, i + w, j - w, j - 1) - rect(i + 1, i + p, j - p, j - 1)
    out[2, J, D] = rect(i - 1, i + 1, j - w, j - p - 1) + rect(i - 1, i + 1, j + p + 1, j + w)
    out[3, J, D] = rect(i - w, i - p - 1, j - 1, j + 1) + rect(i + p + 1, i + w, j - 1, j + 1)
    return out, (J, D)


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

    words = NROWS * NCOLS
    pixel_words = words - NROWS * (NROWS - 1) // 2  # without the left-edge triangle
    stats = ex.count(band.data_ptr(), NROWS, NCOLS, stream=stream)
    diag_sum, _ = ex.marginals(band.data_ptr(), NROWS, NCOLS, stream=stream)
    host_strip = band[:STRIP * NROWS].cpu().numpy().view(np.uint32)
    say(f"band: nrows {NROWS}, ncols {NCOLS}, {pixel_words} pixel words, nnz {stats.nnz}, sum {stats.sum}")
    say(f"device: {torch.cuda.get_device_name(0)}; HIP-event times on one stream, {a.repeats} runs after "
        f"{a.warmup} warm-up; min_diag {MIN_DIAG}, min_count {MIN_COUNT}, HiCCUPS' folds")
    count_ms = line("modle_pixels_count (reads every pixel word once)",
                    timed(lambda: ex.count(band.data_ptr(), NROWS, NCOLS, stream=stream)), 4 * pixel_words)
    twin = torch.empty_like(band)
    with torch.cuda.stream(stream):
        copy_ms = line("device-to-device copy of the band (reads and writes it once)",
                       timed(lambda: twin.copy_(band, non_blocking=True)), 8 * (words + 1))
    del twin
    cand = torch.empty(words + 1, dtype=torch.int32, device=dev)
    sums = torch.empty((4, NCOLS, NROWS), dtype=torch.int64, device=dev)
    for w, p in WINDOWS:
        scale = pixels.dot_scales(diag_sum, NCOLS, w, p, pixels.DOT_FOLDS, MIN_DIAG)
        halo = ((T + 2 * w) / T) ** 2
        valid = sum(max(0, NCOLS - 2 * w - d) for d in range(2 * w + MIN_DIAG, NROWS - 2 * w))
        for both in (False, True):
            torch.cuda.synchronize()
            ms = timed(lambda: ex.dots_into(band.data_ptr(), NROWS, NCOLS, w, p, MIN_DIAG, MIN_COUNT, scale,
                                            cand.data_ptr(), sums.data_ptr() if both else None, stream=stream))
            stored = 4 * words + (32 * words if both else 0)
            med = line(f"modle_pixels_dots: w {w}, p {p}, d_cand{' and d_sums' if both else ' alone'}", ms,
                       4 * halo * pixel_words + stored)
            say(f"      = {med / count_ms:.2f} x the count, {med / copy_ms:.2f} x the copy; halo factor "
                f"((T + 2 w) / T)^2 = {halo:.2f}: {halo * pixel_words:.0f} words addressed, {stored} bytes stored, "
                f"{valid} valid pixels")
        stream.synchronize()
        want, (J, D) = strip_sums(host_strip, w, p)
        got = sums[:, :STRIP, :].cpu().numpy().view(np.uint64)
        assert np.array_equal(got[:, J, D], want[:, J, D]), (w, p)
        nnz = ex.count(cand.data_ptr(), NROWS, NCOLS, stream=stream).nnz
        say(f"      checked {len(J)} pixels of the first {STRIP} columns against numpy; {nnz} candidates")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
