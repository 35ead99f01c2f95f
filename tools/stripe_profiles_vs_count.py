#!/usr/bin/env python3
"""What the stripe profiles of a band cost, on a band of the shape tools/pixels_vs_dense.py uses.

On a band of the shape of GRCh38 chr1 at 5 kb / 3 Mb (ncols 49 792, nrows 600) in device memory whose counts
follow a distance decay -- Poisson around 600 / (d + 1), the recipe of tools/stripes_vs_host.py -- one process
takes, after a warm-up, HIP-event times of

  * modle_pixels_stripe_profiles for the largest offset m = 0, 4, 8 and K = 1 and 4 lengths, each a launch
    sequence of its own (two kernels) into a device array;
  * the count arm: modle_pixels_count on the band, one pass over its words -- the profiles read the band twice,
    once per direction;
  * the moments of the comparison, modle_pixels_stripes with MOMENTS on two bands: two passes over two bands;
  * the plain torch form of the same numbers: band[:-1].view(ncols, nrows).to(int64).cumsum(1) read off at the
    cut points for V, and the same over a sheared view of the band (row r, diagonal e at r * nrows + e * (nrows +
    1)) for H.

Before anything is timed every word of the kernels' output is held against the torch form's.  No time is fixed
in advance: the record says what was measured.  Not measured: a cold pass (every arm runs on a band that the
warm-up has just read), the coarse form, more than one rank.

    python tools/stripe_profiles_vs_count.py [--repeats 20] [--out profiles/stripe_profiles/stripe_profiles_vs_count.txt]
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

LENGTHS = {1: [400], 4: [40, 80, 160, 400]}  # bins of 5 kb: 2 Mb alone; 200 kb, 400 kb, 800 kb and 2 Mb


def torch_profiles(torch, band, m, lengths, d0):
    """int64 [2, K, 2 m + 1, NCOLS]: the profiles by cumulative sums in torch.  The band holds zeros where it has
    no pixel, so a prefix needs no clipping at the edges of the matrix."""
    flat = band[:-1]
    zero = torch.zeros((NCOLS, 1), dtype=torch.int64, device=band.device)
    # P[q][t]: the sum of the words below t of column q
    cols = torch.cat([zero, flat.view(NCOLS, NROWS).to(torch.int64).cumsum(1)], dim=1)
    # Q[r][t]: the sum of the diagonals below t of row r, over a sheared view of the band padded with zeros
    padded = torch.cat([flat, torch.zeros(NROWS * (NROWS + 1), dtype=flat.dtype, device=band.device)])
    rows = torch.cat([zero, torch.as_strided(padded, (NCOLS, NROWS), (NROWS, NROWS + 1)).to(torch.int64).cumsum(1)], dim=1)
    out = torch.zeros((2, len(lengths), 2 * m + 1, NCOLS), dtype=torch.int64, device=band.device)
    for k, length in enumerate(lengths):
        for o in range(-m, m + 1):
            lo, hi = max(0, -o), min(NCOLS, NCOLS - o)  # the anchors c with 0 <= c + o < NCOLS
            out[0, k, o + m, lo:hi] = cols[lo + o:hi + o, length + o] - cols[lo + o:hi + o, d0 + o]
            out[1, k, o + m, lo:hi] = rows[lo + o:hi + o, length - o] - rows[lo + o:hi + o, d0 - o]
    return out


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
    band, other = make_band(torch, dev, 7), make_band(torch, dev, 8)
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
        f"{4 * (NROWS * NCOLS + 1) / 1e6:.1f} MB")
    say(f"device: {torch.cuda.get_device_name(0)}; HIP-event times on one stream, {a.repeats} runs after "
        f"{a.warmup} warm-up")

    # what is timed is right: every word against the torch form
    for m in (0, 4, 8):
        for n_lengths, lengths in LENGTHS.items():
            d0 = max(m, 1)
            out = torch.empty((2, n_lengths, 2 * m + 1, NCOLS), dtype=torch.int64, device=dev)
            ex.stripe_profiles_into(band.data_ptr(), NROWS, NCOLS, m, lengths, d0, out.data_ptr(), out.numel(), stream=stream)
            stream.synchronize()
            with torch.cuda.stream(stream):
                want = torch_profiles(torch, band, m, lengths, d0)
            stream.synchronize()
            assert torch.equal(out, want), (m, lengths)
    say("checked: for m = 0, 4, 8 and K = 1, 4 every word of the kernels' output equals the torch form's")

    count_ms = line("count arm: modle_pixels_count on the band (reads every word once)",
                    timed(lambda: ex.count(band.data_ptr(), NROWS, NCOLS, stream=stream)))
    mom = torch.empty((2, 9, NCOLS), dtype=torch.int64, device=dev)
    mom_ms = line("modle_pixels_stripes, MOMENTS, on two bands (two passes over each)",
                  timed(lambda: ex.stripes_into(band.data_ptr(), other.data_ptr(), NROWS, NCOLS, 1, mom.data_ptr(),
                                                mom.numel(), stream=stream)))
    for m in (0, 4, 8):
        for n_lengths, lengths in LENGTHS.items():
            d0 = max(m, 1)
            out = torch.empty((2, n_lengths, 2 * m + 1, NCOLS), dtype=torch.int64, device=dev)
            med = line(f"modle_pixels_stripe_profiles, m = {m}, K = {n_lengths} ({out.numel() * 8 / 1e6:.1f} MB of sums)",
                       timed(lambda: ex.stripe_profiles_into(band.data_ptr(), NROWS, NCOLS, m, lengths, d0, out.data_ptr(),
                                                             out.numel(), stream=stream)))
            tmed = line(f"the torch form, m = {m}, K = {n_lengths}",
                        timed(lambda: torch_profiles(torch, band, m, lengths, d0)))
            say(f"      the kernels take {med / count_ms:.2f} x the count arm, {med / mom_ms:.2f} x the moments of the "
                f"comparison and {med / tmed:.3f} x the torch form ({'faster' if med < tmed else 'NOT faster'})")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
