#!/usr/bin/env python3
"""What the triangle sums of a band cost, on a band of the shape tools/pixels_vs_dense.py uses.

On a band of the shape of GRCh38 chr1 at 5 kb / 3 Mb (ncols 49 792, nrows 600) in device memory whose counts
follow a distance decay -- Poisson around 600 / (d + 1), the recipe of tools/stripes_vs_host.py -- one process
takes, after a warm-up, HIP-event times of

  * modle_pixels_triangles at the largest width W = 100, 400 and 600, each a launch sequence of its own (two
    kernels) into a device array of W x ncols 64-bit words;
  * the count arm: modle_pixels_count on the same band, one pass over its words;
  * the plain torch form of the same table on the same device: the first W diagonals of the band as int64,
    cumsum along the depth, the sheared gather (column s + k, diagonal k, for start s and width k + 1, over a
    view padded with zeros), then cumsum along k.

Before anything is timed every word of the kernels' output is held against the torch form's.  No ratio is fixed
in advance: the record says what was measured.  Not measured: a cold pass (every arm runs on a band that the
warm-up has just read), the coarse form, more than one rank.

    python tools/triangles_vs_torch.py [--repeats 20] [--out profiles/triangles/triangles_vs_torch.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.pixels_vs_dense import NCOLS, NROWS  # noqa: E402
from tools.sample_vs_torch import PEAK  # noqa: E402
from tools.stripes_vs_host import make_band  # noqa: E402

WIDTHS = (100, 400, 600)
MIN_DIAG = 2


def torch_triangles(torch, band, width, d0):
    """int64 [width, NCOLS]: the table by cumulative sums in torch.  The band holds zeros where it has no pixel,
    so a prefix needs no clipping at the left edge of the matrix."""
    cols = band[:-1].view(NCOLS, NROWS)[:, :width].to(torch.int64)
    cols[:, :d0] = 0
    prefix = cols.cumsum(1)  # P[c][k]
    padded = torch.cat([prefix.reshape(-1), torch.zeros(width * width, dtype=torch.int64, device=band.device)])
    # (k, s) -> P[s + k][k], zeros beyond the last column
    sheared = torch.as_strided(padded, (width, NCOLS), (width + 1, width))
    return sheared.cumsum(0)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the record to this file")
    a = ap.parse_args()

    from modle_amd import pixels  # (loads the HIP runtime torch ships, see _lib.py)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device and has no fallback")
    dev = torch.device("cuda", 0)
    band = make_band(torch, dev, 7)
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
        with torch.cuda.stream(stream):
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
        say(f"  {what:<70} median {med:8.4f} ms  min {min(ms):8.4f}  max {max(ms):8.4f}")
        return med

    stats = ex.count(band.data_ptr(), NROWS, NCOLS, stream=stream)
    say(f"band: nrows {NROWS}, ncols {NCOLS}, counts Poisson around {PEAK:g} / (d + 1): sum {stats.sum}, "
        f"{4 * (NROWS * NCOLS + 1) / 1e6:.1f} MB; min_diag {MIN_DIAG}")
    say(f"device: {torch.cuda.get_device_name(0)}; HIP-event times on one stream, {a.repeats} runs after "
        f"{a.warmup} warm-up")

    # what is timed is right: every word against the torch form
    for width in WIDTHS:
        out = torch.empty((width, NCOLS), dtype=torch.int64, device=dev)
        ex.triangles_into(band.data_ptr(), NROWS, NCOLS, width, MIN_DIAG, out.data_ptr(), out.numel(), stream=stream)
        stream.synchronize()
        with torch.cuda.stream(stream):
            want = torch_triangles(torch, band, width, MIN_DIAG)
        stream.synchronize()
        assert torch.equal(out, want), width
        del want
    say(f"checked: for W = {', '.join(map(str, WIDTHS))} every word of the kernels' output equals the torch form's")

    count_ms = line("count arm: modle_pixels_count on the band (reads every word once)",
                    timed(lambda: ex.count(band.data_ptr(), NROWS, NCOLS, stream=stream)))
    for width in WIDTHS:
        out = torch.empty((width, NCOLS), dtype=torch.int64, device=dev)
        med = line(f"modle_pixels_triangles, W = {width} ({out.numel() * 8 / 1e6:.1f} MB of sums)",
                   timed(lambda: ex.triangles_into(band.data_ptr(), NROWS, NCOLS, width, MIN_DIAG, out.data_ptr(),
                                                   out.numel(), stream=stream)))
        tmed = line(f"the torch form, W = {width}", timed(lambda: torch_triangles(torch, band, width, MIN_DIAG)))
        say(f"      the kernels take {med / count_ms:.2f} x the count arm and {med / tmed:.3f} x the torch form "
            f"({'faster' if med < tmed else 'NOT faster'})")
        del out
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
