#!/usr/bin/env python3
"""What unpacking dense regions costs, on the band tools/pixels_vs_dense.py uses.

On a band of the shape of GRCh38 chr1 at 5 kb / 3 Mb (ncols 49 792, nrows 600) in device memory, one
process takes, after a warm-up, HIP-event times on one stream of

  * modle_pixels_count on the band (for continuity with profiles/mcool/mcool_vs_cool.txt);
  * modle_pixels_dense_tiles for tiles of 512 bins at step 256 across the whole band (193 tiles,
    202 MB of output) and for one region of 2048 bins, with the achieved bytes per second:
    (pixel words read + words written) over the time;
  * the yardstick of each: hipMemcpyAsync, device to device, of a buffer of the output's size on
    the same stream.  The copy writes the same bytes and reads as many again, at least twice what
    the kernel can read (a tile's pixels lie in its upper triangle).

Before anything is timed the outputs are compared, word for word, with the definition evaluated by
torch indexing on the device.

    python tools/dense_vs_copy.py [--repeats 20] [--out profiles/dense/dense_vs_copy.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.pixels_vs_dense import NCOLS, NROWS, make_band  # noqa: E402

TILE, STEP, REGION, REGION_LO = 512, 256, 2048, 20_000
HIP_MEMCPY_DEVICE_TO_DEVICE = 3


def hip_runtime():
    """the HIP runtime this process has loaded (modle_amd/_lib.py: one per process)"""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    if len(paths) != 1:
        raise SystemExit(f"expected one loaded HIP runtime, found {sorted(paths)}")
    rt = C.CDLL(paths.pop())
    rt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return rt


def pixel_words(size):
    """band words one tile of `size` bins is made of: the (a, b), a <= b, with b - a < NROWS"""
    return sum(size - d for d in range(min(NROWS, size)))


def definition(torch, band, lo, size):
    """include/modle_pixels.h: out[r][c] = d < nrows ? band[j * nrows + d] : 0, by torch indexing"""
    a = (lo + torch.arange(size, device=band.device, dtype=torch.int64)).unsqueeze(1)
    b = a.t()
    d, j = (a - b).abs(), torch.maximum(a, b)
    inside = d < NROWS
    words = band[torch.where(inside, j * NROWS + d, torch.zeros_like(d))]
    return torch.where(inside, words, torch.zeros_like(words))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from modle_amd import pixels  # (loads the HIP runtime torch ships, see _lib.py)

    pixels.lib()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device and has no fallback")
    rt = hip_runtime()
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
        say(f"  {what:<62} median {med:8.4f} ms  min {min(ms):8.4f}  max {max(ms):8.4f}  "
            f"{nbytes / med / 1e6:8.1f} GB/s")
        return med

    def copy(dst, src):
        rc = rt.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), 4 * src.numel(), HIP_MEMCPY_DEVICE_TO_DEVICE,
                               stream.cuda_stream)
        assert rc == 0, rc

    stats = ex.count(band.data_ptr(), NROWS, NCOLS, stream=stream)
    band_pixels = NROWS * NCOLS - NROWS * (NROWS - 1) // 2
    say(f"band: nrows {NROWS}, ncols {NCOLS}, {band_pixels} pixel words, nnz {stats.nnz}, sum {stats.sum}")
    say(f"device: {torch.cuda.get_device_name(0)}; HIP-event times on one stream, {a.repeats} runs after "
        f"{a.warmup} warm-up")
    line("modle_pixels_count (reads every pixel word once)",
         timed(lambda: ex.count(band.data_ptr(), NROWS, NCOLS, stream=stream)), 4 * band_pixels)

    count = pixels.tiles_fit(NCOLS, 0, TILE, STEP)
    for what, first, size, step, n in ((f"{count} tiles of {TILE} bins at step {STEP}", 0, TILE, STEP, count),
                                       (f"one region of {REGION} bins", REGION_LO, REGION, 1, 1)):
        out = torch.full((n, size, size), -1, dtype=torch.int32, device=dev)
        other = torch.empty_like(out)
        torch.cuda.synchronize()

        def unpack():
            ex.dense_tiles_into(band.data_ptr(), NROWS, NCOLS, first, size, step, n, out.data_ptr(), out.numel(),
                                stream=stream)

        unpack()
        stream.synchronize()
        for t in sorted({0, n // 2, n - 1}):  # (the same words as the definition, at the size that is timed)
            assert torch.equal(out[t], definition(torch, band, first + t * step, size)), (what, t)
        words = n * size * size
        say(f"{what}: {words} output words ({4 * words / 1e6:.1f} MB), {n * pixel_words(size)} pixel words read")
        k = line("modle_pixels_dense_tiles (pixel words read + words written)", timed(unpack),
                 4 * (n * pixel_words(size) + words))
        c = line("hipMemcpyAsync device to device, same size (read + written)", timed(lambda: copy(other, out)),
                 8 * words)
        say(f"      kernel = {k / c:.2f} x the copy")
        assert torch.equal(other, out)
        del out, other

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
