#!/usr/bin/env python3
"""What the coarse resolutions of an .mcool cost, on the band tools/pixels_vs_dense.py uses.

On a band of the shape of GRCh38 chr1 at 5 kb / 3 Mb (ncols 49 792, nrows 600, about 11.6 % of the
pixels non-zero) in device memory, one process takes, after a warm-up, HIP-event times of

  * modle_pixels_count on the fine band (two memsets, pixels_count, pixels_scan and the copy of the
    statistics): the yardstick, a kernel that reads the same words once;
  * the coarsen kernel (modle_pixels_coarsen) for the factors 2, 5 and 20, with the achieved bytes
    per second: (pixel words read + words written) over the time;

and then the wall time of `simulate` on a small synthetic genome with and without
`--mcool-resolutions 10kb,25kb,100kb`, alternating.

    python tools/mcool_vs_cool.py [--repeats 20] [--out profiles/mcool/mcool_vs_cool.txt]
"""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.pixels_vs_dense import NCOLS, NROWS, make_band  # noqa: E402

FACTORS = (2, 5, 20)
FIRST_BIN = 3  # a phase for every factor


def write_genome(tmp):
    """two chromosomes of 8 and 4 Mb with a barrier every 100 kb or so"""
    rng = np.random.default_rng(11)
    sizes = (("chrA", 8_000_000), ("chrB", 4_000_000))
    with open(os.path.join(tmp, "g.chrom.sizes"), "w") as f:
        f.writelines(f"{n}\t{s}\n" for n, s in sizes)
    with open(os.path.join(tmp, "b.bed"), "w") as f:
        for n, s in sizes:
            for p in sorted(rng.choice(s - 100, size=s // 100_000, replace=False)):
                f.write(f"{n}\t{p}\t{p + 19}\t.\t{rng.uniform(0.6, 1.0):.3f}\t{'+' if rng.random() < 0.5 else '-'}\n")
    return os.path.join(tmp, "g.chrom.sizes"), os.path.join(tmp, "b.bed")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--simulate-repeats", type=int, default=3, help="0 skips the simulate runs")
    ap.add_argument("--ncells", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from modle_amd import cli, pixels  # (loads the HIP runtime torch ships, see _lib.py)
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

    def line(what, ms, nbytes=None):
        med = statistics.median(ms)
        rate = "" if nbytes is None else f"  {nbytes / med / 1e6:8.1f} GB/s"
        say(f"  {what:<58} median {med:8.4f} ms  min {min(ms):8.4f}  max {max(ms):8.4f}{rate}")
        return med

    words = NROWS * NCOLS
    pixel_words = words - NROWS * (NROWS - 1) // 2  # without the left-edge triangle
    stats = ex.count(band.data_ptr(), NROWS, NCOLS, stream=stream)
    say(f"band: nrows {NROWS}, ncols {NCOLS}, {pixel_words} pixel words, nnz {stats.nnz}, sum {stats.sum}")
    say(f"device: {torch.cuda.get_device_name(0)}; HIP-event times on one stream, {a.repeats} runs after "
        f"{a.warmup} warm-up")
    base = line("modle_pixels_count (fine band; reads every pixel word once)",
                timed(lambda: ex.count(band.data_ptr(), NROWS, NCOLS, stream=stream)), 4 * pixel_words)
    for k in FACTORS:
        nr, nc = pixels.coarse_shape(NROWS, NCOLS, k, FIRST_BIN)
        out = torch.empty(nr * nc + 1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ms = timed(lambda: ex.coarsen_into(band.data_ptr(), NROWS, NCOLS, k, FIRST_BIN, out.data_ptr(),
                                           nr * nc + 1, stream=stream))
        med = line(f"modle_pixels_coarsen factor {k:2d} -> {nr} x {nc}", ms, 4 * (pixel_words + nr * nc + 1))
        say(f"      = {med / base:.2f} x the count")
        assert int(out[:-1].sum(dtype=torch.int64)) == stats.sum  # (every contact is in the coarse band)

    if a.simulate_repeats > 0:
        tmp = tempfile.mkdtemp(prefix="mcool_vs_cool_")
        sizes, bed = write_genome(tmp)
        argv = ["simulate", "-c", sizes, "-b", bed, "-r", "5kb", "--ncells", str(a.ncells), "--seed", "3", "-q",
                "--force", "-o"]
        extra = ["--mcool-resolutions", "10kb,25kb,100kb"]
        t = {"cool": [], "mcool": []}
        for it in range(1 + a.simulate_repeats):
            for kind, more in (("cool", []), ("mcool", extra)):
                t0 = time.perf_counter()
                assert cli.main(argv + [os.path.join(tmp, kind, "run")] + more) == 0
                if it >= 1:
                    t[kind].append(time.perf_counter() - t0)
        say(f"simulate, chrA 8 Mb + chrB 4 Mb, {a.ncells} cells, 5 kb, wall seconds of the whole command "
            f"(alternating, {a.simulate_repeats} runs after 1 warm-up):")
        for kind, what in (("cool", "<prefix>.cool"), ("mcool", "<prefix>.mcool with 10kb,25kb,100kb")):
            say(f"  {what:<40} median {statistics.median(t[kind]):7.3f}  [{', '.join(f'{x:.3f}' for x in t[kind])}]  "
                f"file {os.path.getsize(os.path.join(tmp, kind, 'run.' + kind))} bytes")
        shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
