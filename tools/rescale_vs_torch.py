#!/usr/bin/env python3
"""What a rescaled pileup on a band costs, on the band tools/pixels_vs_dense.py uses.

On a band of the shape of GRCh38 chr1 at 5 kb / 3 Mb (ncols 49 792, nrows 600, about 11.6 % of the
pixels non-zero) in device memory, with seeded windows on the diagonal (uniform widths 60 .. nrows, uniform
positions), n = 1 000 and 100 000, and grids of 30, 60 and 128 cells a side (a window narrower than the grid
is rejected by both arms), one process takes, after a warm-up, HIP-event times of

  * modle_pixels_rescale on device windows (pixels_rescale and pixels_rescale_sum): the upper triangle
    of every accepted window, W (W + 1) / 2 words, read once;
  * the plain torch formulation on the device: per chunk of windows (about 2^24 source pixels) the index
    arithmetic of every (x, y) of every window -- its window, its cell, its band word -- band[idx] and
    index_add_ into an int64 pile: W * W words per window;
  * modle_pixels_count on the same band: a kernel that reads every pixel word once.

The two piles, the two areas and the count of accepted windows are compared word for word on the device
before anything is timed.  An arm whose first run takes longer than SLOW_MS is timed with SLOW_REPEATS runs
after that one warm-up, and its line says so: the torch arm at 100 000 windows takes seconds a run.

    python tools/rescale_vs_torch.py [--repeats 20] [--out profiles/rescale/rescale_vs_torch.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.pixels_vs_dense import NCOLS, NROWS, make_band  # noqa: E402

COUNTS = (1_000, 100_000)
SIZES = (30, 60, 128)
MIN_WIDTH = 60
CHUNK = 1 << 24  # source pixels per step of the torch formulation
SLOW_MS, SLOW_REPEATS = 500.0, 2  # an arm slower than this a run is timed with that many runs after one


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

    def once(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        fn()
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1)

    def timed(fn):
        """event times, ms, of `fn()` enqueued on `stream`: a.repeats after a.warmup, or, when the first run is
        slow, SLOW_REPEATS after it"""
        first = once(fn)
        if first > SLOW_MS:
            return [once(fn) for _ in range(SLOW_REPEATS)]
        for _ in range(a.warmup - 1):
            once(fn)
        return [once(fn) for _ in range(a.repeats)]

    def line(what, ms, nbytes):
        med = statistics.median(ms)
        say(f"  {what:<62} median {med:10.4f} ms  min {min(ms):10.4f}  max {max(ms):10.4f}  ({len(ms):2d} runs)"
            f"  {nbytes / med / 1e6:8.1f} GB/s")
        return med

    def torch_rescale(start, end, r):
        """the plain formulation: (pile, area, n_used), int64"""
        w = end - start
        ok = (start >= 0) & (end <= NCOLS) & (w >= r) & (w <= NROWS)
        s, w = start[ok], w[ok]
        pile = torch.zeros(r * r, dtype=torch.int64, device=dev)
        area = torch.zeros(r * r, dtype=torch.int64, device=dev)
        sq = w * w
        ends = torch.cumsum(sq, 0)
        lo = 0
        while lo < len(s):
            base = int(ends[lo - 1]) if lo else 0
            hi = max(lo + 1, int(torch.searchsorted(ends, torch.tensor(base + CHUNK, device=dev), right=True)))
            cs, cw, csq = s[lo:hi], w[lo:hi], sq[lo:hi]
            t = torch.repeat_interleave(torch.arange(hi - lo, device=dev), csq)
            p = torch.arange(len(t), device=dev) - (torch.cumsum(csq, 0) - csq)[t]
            wt = cw[t]
            x, y = p // wt, p % wt
            cell = (x * r // wt) * r + y * r // wt
            j = cs[t] + torch.maximum(x, y)
            idx = j * NROWS + (torch.maximum(x, y) - torch.minimum(x, y))
            pile.index_add_(0, cell, band[idx].to(torch.int64) & 0xFFFFFFFF)
            area.index_add_(0, cell, torch.ones_like(cell))
            lo = hi
        return pile.view(r, r), area.view(r, r), int(ok.sum())

    pixel_words = NROWS * NCOLS - NROWS * (NROWS - 1) // 2  # without the left-edge triangle
    stats = ex.count(band.data_ptr(), NROWS, NCOLS, stream=stream)
    say(f"band: nrows {NROWS}, ncols {NCOLS}, {pixel_words} pixel words, nnz {stats.nnz}, sum {stats.sum}")
    say(f"device: {torch.cuda.get_device_name(0)}; HIP-event times on one stream, {a.repeats} runs after "
        f"{a.warmup} warm-up (an arm slower than {SLOW_MS:g} ms a run: {SLOW_REPEATS} after 1); at most "
        f"{pixels.rescale_groups()} workgroups of 1024 lanes")
    count_ms = line("modle_pixels_count (reads every pixel word once)",
                    timed(lambda: ex.count(band.data_ptr(), NROWS, NCOLS, stream=stream)), 4 * pixel_words)
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    for r in SIZES:
        for n in COUNTS:
            w = torch.randint(MIN_WIDTH, NROWS + 1, (n,), generator=g, device=dev, dtype=torch.int64)
            start = (torch.rand(n, generator=g, device=dev, dtype=torch.float64) * (NCOLS - w + 1)).to(torch.int64)
            end = start + w
            pile = torch.empty((r, r), dtype=torch.int64, device=dev)
            area = torch.empty((r, r), dtype=torch.int64, device=dev)
            used = torch.empty(1, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()

            def kernel():
                ex.rescale_into(band.data_ptr(), NROWS, NCOLS, r, start.data_ptr(), end.data_ptr(), n, pile.data_ptr(),
                                area.data_ptr(), used.data_ptr(), stream=stream)

            kernel()
            stream.synchronize()
            with torch.cuda.stream(stream):
                want, want_area, want_used = torch_rescale(start, end, r)
            stream.synchronize()
            assert int(used[0]) == want_used and torch.equal(pile, want) and torch.equal(area, want_area), (r, n)
            acc = w[w >= r]
            upper, square = int((acc * (acc + 1) // 2).sum()), int((acc * acc).sum())
            say(f"grid {r} x {r}, {n} windows, {want_used} accepted; the two piles and areas agree, the pile sums to "
                f"{int(pile.sum())} over {square} source pixels")
            k_ms = line("modle_pixels_rescale (reads W (W + 1) / 2 words a window)", timed(kernel), 4 * upper)
            with torch.cuda.stream(stream):
                t_ms = line("torch: index arithmetic, band[idx], index_add_ (W * W words)",
                            timed(lambda: torch_rescale(start, end, r)), 4 * square)
            say(f"      the kernels take {k_ms / t_ms:.4f} x the torch form ({t_ms / k_ms:.1f} x faster) and "
                f"{k_ms / count_ms:.2f} x the count")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
