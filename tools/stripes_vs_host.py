#!/usr/bin/env python3
"""What the comparison of two bands stripe by stripe costs, on bands of the shape tools/pixels_vs_dense.py uses.

On two bands of the shape of GRCh38 chr1 at 5 kb / 3 Mb (ncols 49 792, nrows 600) in device memory whose
counts follow a distance decay -- Poisson around 600 / (d + 1), the recipe of tools/sample_vs_torch.py with
two seeds -- one process takes, after a warm-up, HIP-event times of

  * modle_pixels_stripes with the mask MOMENTS, with MOMENTS | MASKED and with all three blocks, each a
    launch sequence of its own into a device array (two kernels for the moments, one more for the ranks);
  * the count arm: modle_pixels_count on one of the bands, one pass over its words -- half of what the
    moments have to read;

and the host wall time of evaluate.compare on the same two bands copied to the host, Pearson and Spearman,
both directions each: what `evaluate` and a fitting loop pay today (its copy over the bus is timed apart).

Before anything is timed the moments of a sample of bins are formed again on the host in Python integers, and
the device scores of every bin are held against evaluate.compare's.  No ratio is expected: the record says
what was measured.

    python tools/stripes_vs_host.py [--repeats 20] [--out profiles/stripes/stripes_vs_host.txt]
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


def make_band(torch, dev, seed):
    """tools/sample_vs_torch.py's band with a seed of its own: Poisson counts around PEAK / (d + 1), zero in
    the left-edge triangle and the trailing word"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    d = torch.arange(NROWS, device=dev, dtype=torch.float32)
    mean = (PEAK / (d + 1.0)).unsqueeze(0).expand(NCOLS, NROWS).contiguous()
    band = torch.poisson(mean, generator=g).to(torch.int32)
    j = torch.arange(NCOLS, device=dev).unsqueeze(1)
    band = torch.where(d.unsqueeze(0) <= j, band, torch.zeros_like(band))
    out = torch.zeros(NROWS * NCOLS + 1, dtype=torch.int32, device=dev)
    out[:-1] = band.reshape(-1)
    return out


def host_moments(a, b, c, direction):
    """(n, Sa, Sb, Saa, Sbb, Sab) of bin c in Python integers, from the host bands"""
    if direction == 0:
        idx = [c * NROWS + i for i in range(min(c + 1, NROWS))]
    else:
        idx = [(c + i) * NROWS + i for i in range(min(NROWS, NCOLS - c))]
    x, y = [int(a[k]) for k in idx], [int(b[k]) for k in idx]
    return [NROWS, sum(x), sum(y), sum(v * v for v in x), sum(v * v for v in y), sum(v * w for v, w in zip(x, y))]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the record to this file")
    ap.add_argument("--no-host", action="store_true", help="leave out the host arm (evaluate.compare)")
    a = ap.parse_args()

    from modle_amd import evaluate, pixels  # (loads the HIP runtime torch ships, see _lib.py)
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
        f"{a.warmup} warm-up")

    # what is timed is right: the sums of a sample of bins in Python integers, every score against the host's
    out = torch.empty((2, 21, NCOLS), dtype=torch.int64, device=dev)
    ex.stripes_into(ref.data_ptr(), tgt.data_ptr(), NROWS, NCOLS, 7, out.data_ptr(), out.numel(), stream=stream)
    stream.synchronize()
    rows = out.cpu().numpy().view(np.uint64)
    t0 = time.perf_counter()
    h_ref, h_tgt = ref.cpu().numpy().view(np.uint32), tgt.cpu().numpy().view(np.uint32)
    copy_s = time.perf_counter() - t0
    for d in (0, 1):
        assert int(rows[d, 1].sum()) == stats[0].sum and int(rows[d, 2].sum()) == stats[1].sum
        for c in (0, 1, 63, 64, 599, 600, 20000, NCOLS - 600, NCOLS - 599, NCOLS - 1):
            m = host_moments(h_ref, h_tgt, c, d)
            got = [int(rows[d, k, c]) for k in range(3)] + [int(rows[d, k, c]) | (int(rows[d, k + 1, c]) << 64)
                                                            for k in (3, 5, 7)]
            assert got == m, (d, c, got, m)
    say("checked: in both directions the Sa and Sb of the bins add up to the bands' sums, and the moments of ten "
        "bins equal their sums in Python integers")

    count_ms = line("count arm: modle_pixels_count on one band (reads every word once)",
                    timed(lambda: ex.count(ref.data_ptr(), NROWS, NCOLS, stream=stream)))
    med = {}
    for what, name in ((1, "MOMENTS"), (3, "MOMENTS | MASKED"), (7, "MOMENTS | MASKED | RANKS")):
        words = 2 * pixels.stripes_rows(what) * NCOLS
        med[what] = line(f"modle_pixels_stripes, {name}", timed(lambda: ex.stripes_into(
            ref.data_ptr(), tgt.data_ptr(), NROWS, NCOLS, what, out.data_ptr(), words, stream=stream)))
    say(f"      the moments take {med[1] / count_ms:.2f} x the count arm (they read two bands, twice: once per direction); "
        f"the ranks add {med[7] - med[3]:.3f} ms, {(med[7] - med[3]) * 1e3 / (2 * NCOLS):.3f} us per stripe pair")
    gbytes = 2 * 2 * 4 * NROWS * NCOLS / 1e9
    say(f"      {gbytes / (med[1] * 1e-3):.0f} GB/s over the {gbytes:.2f} GB the two moment kernels read")

    if not a.no_host:
        say(f"host arm: the two bands copied to the host in {copy_s:.2f} s; evaluate.compare, both directions, wall time")
        for metric, mask in (("pearson", 1), ("spearman", 5)):
            t0 = time.perf_counter()
            host = [evaluate.compare(h_ref, h_tgt, NROWS, NCOLS, metric, direction)[0]
                    for direction in ("vertical", "horizontal")]
            wall = time.perf_counter() - t0
            picked = np.concatenate([rows[:, :9], rows[:, 18:]], axis=1) if mask == 5 else rows[:, :9]
            t0 = time.perf_counter()
            mine = [pixels.stripe_scores(picked[d], metric) for d in (0, 1)]
            score_s = time.perf_counter() - t0
            worst = 0.0
            for x, y in zip(mine, host):
                assert np.array_equal(np.isnan(x), np.isnan(y))
                worst = max(worst, float(np.nanmax(np.abs(x - y))))
            device_ms = med[1] if mask == 1 else med[7] - med[3] + med[1]
            say(f"  evaluate.compare {metric:<9} {wall:8.2f} s on the host; on the device the sums take about "
                f"{device_ms:.3f} ms and pixels.stripe_scores {score_s:.2f} s for the {2 * NCOLS} stripes; the scores "
                f"differ by at most {worst:.2e}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
