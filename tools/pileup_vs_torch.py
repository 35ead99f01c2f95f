#!/usr/bin/env python3
"""What a pileup on a band costs, on the band tools/pixels_vs_dense.py uses.

On a band of the shape of GRCh38 chr1 at 5 kb / 3 Mb (ncols 49 792, nrows 600, about 11.6 % of the
pixels non-zero) in device memory, with seeded anchors that the kernel accepts (uniform distances
0 .. nrows - 1 - 2 f, uniform positions), n = 1 000 and 100 000, and flanks of 5, 10 and 32 bins, one
process takes, after a warm-up, HIP-event times of

  * modle_pixels_pileup on device anchors (pixels_pileup and pixels_pileup_sum): the gather of
    n * S * S words, S = 2 f + 1;
  * the plain torch formulation on the device: the index arithmetic of n * S * S int64 indices,
    band[idx] and .sum(0) -- in chunks of 16 384 anchors, so that its temporaries stay below a few
    GiB at f = 32;
  * modle_pixels_count on the same band: a kernel that reads every pixel word once.

The two piles are compared word for word on the device before anything is timed.

    python tools/pileup_vs_torch.py [--repeats 20] [--out profiles/pileup/pileup_vs_torch.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.pixels_vs_dense import NCOLS, NROWS, make_band  # noqa: E402

COUNTS = (1_000, 100_000)
FLANKS = (5, 10, 32)
CHUNK = 16_384  # anchors per step of the torch formulation


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

    def torch_pileup(b1, b2, f):
        """the plain formulation: indices, a gather, a sum; int64 [S, S]"""
        off = torch.arange(-f, f + 1, device=dev, dtype=torch.int64)
        pile = torch.zeros((2 * f + 1, 2 * f + 1), dtype=torch.int64, device=dev)
        for lo in range(0, len(b1), CHUNK):
            x = b1[lo:lo + CHUNK, None, None] + off[None, :, None]
            y = b2[lo:lo + CHUNK, None, None] + off[None, None, :]
            j = torch.maximum(x, y)
            idx = j * NROWS + (j - torch.minimum(x, y))
            pile += (band[idx].to(torch.int64) & 0xFFFFFFFF).sum(0)
        return pile

    pixel_words = NROWS * NCOLS - NROWS * (NROWS - 1) // 2  # without the left-edge triangle
    stats = ex.count(band.data_ptr(), NROWS, NCOLS, stream=stream)
    say(f"band: nrows {NROWS}, ncols {NCOLS}, {pixel_words} pixel words, nnz {stats.nnz}, sum {stats.sum}")
    say(f"device: {torch.cuda.get_device_name(0)}; HIP-event times on one stream, {a.repeats} runs after "
        f"{a.warmup} warm-up; at most {pixels.PILEUP_GROUPS} workgroups of 256 lanes")
    count_ms = line("modle_pixels_count (reads every pixel word once)",
                    timed(lambda: ex.count(band.data_ptr(), NROWS, NCOLS, stream=stream)), 4 * pixel_words)
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    for f in FLANKS:
        s = 2 * f + 1
        for n in COUNTS:
            d = torch.randint(0, NROWS - 2 * f, (n,), generator=g, device=dev, dtype=torch.int64)
            b1 = f + (torch.rand(n, generator=g, device=dev, dtype=torch.float64) * (NCOLS - 2 * f - d)).to(torch.int64)
            b2 = b1 + d
            pile = torch.empty((s, s), dtype=torch.int64, device=dev)
            used = torch.empty(1, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()

            def kernel():
                ex.pileup_into(band.data_ptr(), NROWS, NCOLS, f, b1.data_ptr(), b2.data_ptr(), n, pile.data_ptr(),
                               used.data_ptr(), stream=stream)

            kernel()
            stream.synchronize()
            with torch.cuda.stream(stream):
                want = torch_pileup(b1, b2, f)
            stream.synchronize()
            assert int(used[0]) == n and torch.equal(pile, want), (f, n)
            say(f"flank {f} ({s} x {s} cells), {n} anchors, all accepted; the two piles agree, their sum is {int(pile.sum())}")
            gathered = 4 * n * s * s
            k_ms = line("modle_pixels_pileup (gathers n * S * S words)", timed(kernel), gathered)
            with torch.cuda.stream(stream):
                t_ms = line("torch: index arithmetic, band[idx], .sum(0)", timed(lambda: torch_pileup(b1, b2, f)), gathered)
            say(f"      the kernels take {k_ms / t_ms:.3f} x the torch form ({t_ms / k_ms:.1f} x faster) and "
                f"{k_ms / count_ms:.2f} x the count")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
