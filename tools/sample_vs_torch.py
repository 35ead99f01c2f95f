#!/usr/bin/env python3
"""What the random sampling of a band costs, on a band of the shape tools/pixels_vs_dense.py uses.

On a band of the shape of GRCh38 chr1 at 5 kb / 3 Mb (ncols 49 792, nrows 600) in device memory whose
counts follow a distance decay -- Poisson around 600 / (d + 1), seeded: a column's first few words hold
most of its contacts -- one process takes, after a warm-up, HIP-event times of

  * modle_pixels_sample at the fractions 0.1 and 0.5, into the kept band alone and into both bands (one
    Philox call per four contacts: the work is proportional to the band's sum);
  * the torch arm, what a torch user writes today: torch.binomial(band.float(), p) on the same device.
    It does not reproduce the definition: its draw depends on the generator's state and on the launch,
    not on the pixel, and a series of fractions is not nested;
  * the count arm: modle_pixels_count on the same band, one pass over the words -- the floor.

Before anything is timed, kept + rest == band is checked on the device for every word and 4 096 pixels
(the heaviest column among them) are drawn again on the host with pixels.sample_pixels.  The last lines
give the measured trials per second and what MODLE_PIXELS_MAX_SAMPLE_TRIALS lasts at that rate.
`--lib` times another build of the library (a tier boundary built with -DMODLE_SAMPLE_TIER1_BLOCKS=N) in
a process of its own.

    python tools/sample_vs_torch.py [--repeats 20] [--out profiles/sample/sample_vs_torch.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.pixels_vs_dense import NCOLS, NROWS  # noqa: E402

FRACTIONS = (0.1, 0.5)
PEAK = 600.0  # the mean count on the diagonal
SEED = 2026


def make_band(torch, dev):
    """Poisson counts around PEAK / (d + 1), zero in the left-edge triangle and the trailing word"""
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    d = torch.arange(NROWS, device=dev, dtype=torch.float32)
    mean = (PEAK / (d + 1.0)).unsqueeze(0).expand(NCOLS, NROWS).contiguous()
    band = torch.poisson(mean, generator=g).to(torch.int32)
    j = torch.arange(NCOLS, device=dev).unsqueeze(1)
    band = torch.where(d.unsqueeze(0) <= j, band, torch.zeros_like(band))
    out = torch.zeros(NROWS * NCOLS + 1, dtype=torch.int32, device=dev)
    out[:-1] = band.reshape(-1)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the record to this file")
    ap.add_argument("--lib", default=None, help="another build of libmodle_pixels.so to time")
    ap.add_argument("--label", default=None, help="what the record calls that build")
    ap.add_argument("--kernel-only", action="store_true", help="leave out the torch and the count arm")
    a = ap.parse_args()

    from modle_amd import pixels  # (loads the HIP runtime torch ships, see _lib.py)
    if a.lib:
        pixels.SO_PATH = os.path.abspath(a.lib)
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device and has no fallback")
    dev = torch.device("cuda", 0)
    band = make_band(torch, dev)
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

    words = NROWS * NCOLS + 1
    stats = ex.count(band.data_ptr(), NROWS, NCOLS, stream=stream)
    say(f"build: {a.label or f'the library as built: a lane draws the first {pixels.SAMPLE_TIER1_TRIALS} trials of its pixel'}")
    say(f"band: nrows {NROWS}, ncols {NCOLS}, counts Poisson around {PEAK:g} / (d + 1): nnz {stats.nnz}, sum {stats.sum} "
        f"({stats.sum / 4e6:.1f} M Philox calls at least), max {stats.max_count}")
    say(f"device: {torch.cuda.get_device_name(0)}; HIP-event times on one stream, {a.repeats} runs after "
        f"{a.warmup} warm-up")
    kept = torch.empty(words, dtype=torch.int32, device=dev)
    rest = torch.empty(words, dtype=torch.int32, device=dev)
    count_ms = None
    if not a.kernel_only:
        count_ms = line("count arm: modle_pixels_count (reads every word once)",
                        timed(lambda: ex.count(band.data_ptr(), NROWS, NCOLS, stream=stream)))
    rates = []
    for frac in FRACTIONS:
        thr = pixels.sample_threshold(frac)
        ex.sample_into(band.data_ptr(), NROWS, NCOLS, thr, SEED, stats, kept.data_ptr(), rest.data_ptr(), stream=stream)
        stream.synchronize()
        assert torch.equal(kept + rest, band) and int(kept.min()) >= 0
        g = np.random.default_rng(1)
        w = np.concatenate([np.arange(5000 * NROWS, 5000 * NROWS + NROWS), g.integers(NROWS * NROWS, words - 1, 4096 - NROWS)])
        j, d = w // NROWS, w % NROWS
        idx = torch.from_numpy(w).to(dev)
        want = pixels.sample_pixels(j - d, j, band[idx].cpu().numpy(), thr, SEED)
        assert np.array_equal(kept[idx].cpu().numpy().astype(np.uint32), want)
        total = int(kept.sum())
        say(f"fraction {frac}: threshold {thr}; kept {total} of {stats.sum} ({total / stats.sum:.5f}); kept + rest == band "
            "word for word, 4096 pixels agree with the host statement")
        k_ms = line("modle_pixels_sample, kept band only", timed(lambda: ex.sample_into(
            band.data_ptr(), NROWS, NCOLS, thr, SEED, stats, kept.data_ptr(), None, stream=stream)))
        b_ms = line("modle_pixels_sample, kept and rest band", timed(lambda: ex.sample_into(
            band.data_ptr(), NROWS, NCOLS, thr, SEED, stats, kept.data_ptr(), rest.data_ptr(), stream=stream)))
        rates.append(stats.sum / (b_ms * 1e-3))
        say(f"      {stats.sum / (b_ms * 1e-3) / 1e9:.1f} G trials/s, {stats.sum / 4 / (b_ms * 1e-3) / 1e9:.2f} G Philox calls/s")
        if not a.kernel_only:
            p = torch.full((words,), frac, dtype=torch.float32, device=dev)
            with torch.cuda.stream(stream):
                as_float = band.float()
                t_ms = line("torch arm: torch.binomial(band.float(), p) (another draw)",
                            timed(lambda: torch.binomial(as_float, p)))
            say(f"      the kernel takes {b_ms / t_ms:.3f} x the torch arm and {b_ms / count_ms:.2f} x the count arm")
    # one pixel of 2^20 + 3 contacts in an empty band of the same shape: what a pixel costs that one wave
    # draws alone (it is not spread over the waves of a workgroup)
    empty = torch.zeros(words, dtype=torch.int32, device=dev)
    giant = torch.zeros(words, dtype=torch.int32, device=dev)
    giant[5000 * NROWS] = 2**20 + 3
    torch.cuda.synchronize()
    g_stats = ex.count(giant.data_ptr(), NROWS, NCOLS, stream=stream)
    thr = pixels.sample_threshold(0.5)
    e_ms = line("an empty band of the same shape", timed(lambda: ex.sample_into(
        empty.data_ptr(), NROWS, NCOLS, thr, SEED, pixels.Stats(0, 0, 0), kept.data_ptr(), None, stream=stream)))
    g_ms = line("the same with one pixel of 2^20 + 3 contacts, drawn by one wave", timed(lambda: ex.sample_into(
        giant.data_ptr(), NROWS, NCOLS, thr, SEED, g_stats, kept.data_ptr(), None, stream=stream)))
    assert int(kept[5000 * NROWS]) == int(pixels.sample_pixels([5000], [5000], [2**20 + 3], thr, SEED)[0])
    say(f"      the giant pixel adds {g_ms - e_ms:.4f} ms")
    rate = min(rates)
    cap = pixels.MAX_SAMPLE_TRIALS
    say(f"throughput: {rate / 1e9:.1f} G trials/s at the slower fraction; MODLE_PIXELS_MAX_SAMPLE_TRIALS = 2^{cap.bit_length() - 1} "
        f"trials last {cap / rate:.2f} s at that rate (2^36: {2**36 / rate:.2f} s)")
    say(f"one wave alone draws {(2**20 + 3) / ((g_ms - e_ms) * 1e-3) / 1e9:.2f} G trials/s: a band whose contacts sit in a "
        "handful of pixels is drawn at that rate, not at the band's")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
