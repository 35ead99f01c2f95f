#!/usr/bin/env python3
"""Sparse pixels from the device against the dense copy, on a chr1-shaped band.

Builds a band of the shape of GRCh38 chr1 at 5 kb / 3 Mb (ncols 49 792, nrows 600, about 11.6 %
of the pixels non-zero) on the device and times, in one process, after a
warm-up, alternating:

  (a) the dense path: the device-to-host copy of the whole band into a fresh pageable array (what
      Simulator.copy_outputs does) plus modle_cool_append_matrix, which scans it on one host thread;
  (b) the pixel path: modle_pixels_to_host (count + scan + extract on the device and the copy of the
      triples to the host) plus modle_cool_append_pixels, which validates them.

Both append into a cooler file of their own, so both include the same HDF5 work (deflate of the
same pixel table); the parts are reported separately.  Times are host clocks around calls that end
in a device synchronise.  With --kernels-only nothing is written and the extraction runs a few times
(for a `rocprofv3 --kernel-trace --stats` run of its own).

    python tools/pixels_vs_dense.py [--repeats 3] [--out profiles/pixels/pixels_vs_dense.txt]
"""
import argparse
import ctypes as C
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NROWS, NCOLS, DENSITY, BIN_SIZE = 600, 49_792, 0.116, 5000


def make_band(torch, dev):
    """counts that fall off with the distance from the diagonal like a contact matrix's do: the
    probability of a non-zero word decreases with d, 11.6 % over the whole band"""
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    d = torch.arange(NROWS, device=dev, dtype=torch.float32)
    p = 1.0 / (1.0 + d / 12.0)
    p = p * (DENSITY * NROWS / p.sum())
    p = p.clamp(max=1.0)
    u = torch.rand((NCOLS, NROWS), generator=g, device=dev)
    v = torch.randint(1, 40, (NCOLS, NROWS), generator=g, device=dev, dtype=torch.int32)
    band = torch.where(u < p, v, torch.zeros_like(v))
    j = torch.arange(NCOLS, device=dev).unsqueeze(1)
    band = torch.where(d.unsqueeze(0) <= j, band, torch.zeros_like(band))  # left-edge triangle
    out = torch.zeros(NROWS * NCOLS + 1, dtype=torch.int32, device=dev)
    out[:-1] = band.reshape(-1)
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from modle_amd import cooler, pixels  # (loads the HIP runtime torch ships, see _lib.py)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device and has no fallback")
    dev = torch.device("cuda", 0)
    band = make_band(torch, dev)
    ex = pixels.Extractor(0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    if a.kernels_only:
        for _ in range(5):
            ex.extract(band.data_ptr(), NROWS, NCOLS)
        return 0

    chroms = [("chr1", NCOLS * BIN_SIZE)]
    tmp = tempfile.mkdtemp(prefix="pixels_vs_dense_")
    t = {k: [] for k in ("a_copy", "a_append", "b_extract", "b_numpy", "b_append")}
    stats = None
    for it in range(a.warmup + a.repeats):
        keep = it >= a.warmup
        # (a)
        t0 = time.perf_counter()
        dense = band.cpu().numpy().view(np.uint32)  # (synchronises)
        t1 = time.perf_counter()
        with cooler.CoolerWriter(os.path.join(tmp, "dense.cool"), chroms, BIN_SIZE, force_overwrite=True) as w:
            t2 = time.perf_counter()
            w.append("chr1", dense, NROWS, NCOLS)
            t3 = time.perf_counter()
        # (b)
        t4 = time.perf_counter()
        p1, p2, pc, po = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        st = pixels._CStats()
        err = C.create_string_buffer(512)
        rc = ex._L.modle_pixels_to_host(ex._h, band.data_ptr(), NROWS, NCOLS, 0, C.byref(p1), C.byref(p2),
                                        C.byref(pc), C.byref(po), C.byref(st), None, err, len(err))
        assert rc == 0, err.value
        t5 = time.perf_counter()
        n = int(st.nnz)
        b1 = pixels._host_array(p1.value, n, np.int64)
        b2 = pixels._host_array(p2.value, n, np.int64)
        cn = pixels._host_array(pc.value, n, np.int32)
        off = pixels._host_array(po.value, NCOLS + 1, np.int64)
        t6 = time.perf_counter()
        with cooler.CoolerWriter(os.path.join(tmp, "sparse.cool"), chroms, BIN_SIZE, force_overwrite=True) as w:
            t7 = time.perf_counter()
            w.append_pixels("chr1", NCOLS, b1, b2, cn, bin1_offset=off)
            t8 = time.perf_counter()
        stats = st
        if keep:
            for k, v in (("a_copy", t1 - t0), ("a_append", t3 - t2), ("b_extract", t5 - t4),
                         ("b_numpy", t6 - t5), ("b_append", t8 - t7)):
                t[k].append(v * 1e3)
        # the two paths found the same pixels
        assert int(np.count_nonzero(dense[:NROWS * NCOLS])) == n and int(dense[:NROWS * NCOLS].sum(dtype=np.uint64)) == st.sum

    shutil.rmtree(tmp, ignore_errors=True)

    def med(k):
        return statistics.median(t[k])

    words = NROWS * NCOLS
    say(f"band: nrows {NROWS}, ncols {NCOLS}, {words} words, nnz {stats.nnz} "
        f"({100.0 * stats.nnz / words:.2f} % of the words), sum {stats.sum}, max {stats.max_count}")
    say(f"device: {torch.cuda.get_device_name(0)}; medians of {a.repeats} runs after {a.warmup} warm-up, ms "
        "(all runs in brackets)")
    for k, what in (("a_copy", "(a) dense device-to-host copy into a fresh pageable array"),
                    ("a_append", "(a) modle_cool_append_matrix (host scan + HDF5)"),
                    ("b_extract", "(b) modle_pixels_to_host (count + scan + extract + copy of the triples)"),
                    ("b_numpy", "(b) copy of the pinned result into numpy arrays (Python binding only)"),
                    ("b_append", "(b) modle_cool_append_pixels (validation + HDF5)")):
        say(f"  {what:<82} {med(k):9.2f}  [{', '.join(f'{x:.2f}' for x in t[k])}]")
    ta, tb = med("a_copy") + med("a_append"), med("b_extract") + med("b_numpy") + med("b_append")
    say(f"  (a) total {ta:.2f} ms   (b) total {tb:.2f} ms   (b) / (a) = {tb / ta:.3f}")
    say(f"  up to the host arrays only: (a) {med('a_copy'):.2f} ms (pixels not yet found), "
        f"(b) {med('b_extract') + med('b_numpy'):.2f} ms (pixels found)")
    say("bytes moved device -> host: "
        f"(a) {4 * (words + 1)}   (b) {20 * stats.nnz + 8 * (NCOLS + 1) + 24}")
    say(f"bytes the kernels read / write in device memory (from the shapes): read 2 x {4 * words} (count, extract) "
        f"+ {8 * 3 * (NCOLS + 1)} (row counts, scan), write {20 * stats.nnz} (triples) + {8 * 2 * (NCOLS + 1)}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
