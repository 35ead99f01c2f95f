#!/usr/bin/env python3
"""What the way from sorted pixels back to a band costs, on the band tools/pixels_vs_dense.py uses.

On a band of the shape of GRCh38 chr1 at 5 kb / 3 Mb (ncols 49 792, nrows 600, about 11.6 % of the pixels
non-zero) and its pixels, extracted on the device, one process takes, after a warm-up,

  1. HIP-event times of modle_pixels_band_check (one pass over the list and the binary searches of the row
     starts; the call waits, so its time holds the copy of the statistics) and of modle_pixels_band_fill, each
     on its own;
  2. of the plain torch form on the same device arrays: the index arithmetic (bin2 - off) * nrows +
     (bin2 - bin1), torch.zeros and index_put_;
  3. of modle_pixels_count on the same band, the family's yardstick: a kernel that reads every pixel word
     once;
  4. host-clock times around a synchronise of the two ways a band gets from the host to the device: its
     pixels from pinned memory through modle_pixels_band_from_host (copy, check, fill), and the dense band
     from pinned memory, which is how the evaluator's reader would feed a device.

The bands of the kernel and of the torch form are compared word for word with the source band before
anything is timed.

    python tools/band_vs_torch.py [--repeats 20] [--out profiles/band/band_vs_torch.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.pixels_vs_dense import NCOLS, NROWS, make_band  # noqa: E402


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
    words = NROWS * NCOLS + 1
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

    def clocked(fn):
        """host-clock times, ms, of `fn()` between two synchronises"""
        out = []
        for it in range(a.warmup + a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= a.warmup:
                out.append(1e3 * (time.perf_counter() - t0))
        return out

    def line(what, ms, nbytes):
        med = statistics.median(ms)
        say(f"  {what:<66} median {med:8.4f} ms  min {min(ms):8.4f}  max {max(ms):8.4f}"
            f"  {nbytes / med / 1e6:8.1f} GB/s")
        return med

    # the pixels of the band, on the device: count + extract
    off = 1234  # (a bin offset, as a chromosome inside a file has one)
    rows_x = torch.empty(NCOLS + 1, dtype=torch.int64, device=dev)
    stats = ex.count(band.data_ptr(), NROWS, NCOLS, rows_x.data_ptr(), stream)
    n = int(stats.nnz)
    bin1 = torch.empty(n, dtype=torch.int64, device=dev)
    bin2 = torch.empty(n, dtype=torch.int64, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    ex.extract_into(band.data_ptr(), NROWS, NCOLS, off, rows_x.data_ptr(), bin1.data_ptr(), bin2.data_ptr(),
                    count.data_ptr(), n, stream)
    stream.synchronize()
    pixel_bytes, band_bytes = 20 * n, 4 * words
    pixel_words = NROWS * NCOLS - NROWS * (NROWS - 1) // 2
    say(f"band: nrows {NROWS}, ncols {NCOLS}, {words} words ({band_bytes / 1e6:.1f} MB), {pixel_words} pixel words, "
        f"nnz {n} ({pixel_bytes / 1e6:.1f} MB of pixels), sum {stats.sum}")
    say(f"device: {torch.cuda.get_device_name(0)}; HIP-event times on one stream unless a host clock is named, "
        f"{a.repeats} runs after {a.warmup} warm-up; the fill's tile is {pixels.BAND_TILE_COLS} columns x "
        f"{pixels.BAND_TILE_DIAGS} diagonals")

    rows = torch.empty(NCOLS + 1, dtype=torch.int64, device=dev)
    out = torch.full((words,), -1, dtype=torch.int32, device=dev)  # (the caller does not pre-zero)
    torch.cuda.synchronize()

    def check():
        return ex.band_check(bin1.data_ptr(), bin2.data_ptr(), count.data_ptr(), n, NROWS, NCOLS, off, rows.data_ptr(),
                             stream)

    def fill():
        ex.band_fill_into(bin2.data_ptr(), count.data_ptr(), n, NROWS, NCOLS, off, rows.data_ptr(), out.data_ptr(),
                          words, stream)

    def torch_form():
        idx = (bin2 - off) * NROWS + (bin2 - bin1)
        t = torch.zeros(words, dtype=torch.int32, device=dev)
        t.index_put_((idx,), count)
        return t

    st = check()
    fill()
    stream.synchronize()
    with torch.cuda.stream(stream):
        want = torch_form()
    stream.synchronize()
    assert torch.equal(out, band) and torch.equal(want, band)
    assert (st.n_in, st.nnz_in, st.sum_in, st.n_beyond, st.n_outside) == (n, n, stats.sum, 0, 0)
    say("the band of the kernel, the band of the torch form and the source band agree word for word")

    count_ms = line("modle_pixels_count (reads every pixel word once)",
                    timed(lambda: ex.count(band.data_ptr(), NROWS, NCOLS, stream=stream)), 4 * pixel_words)
    check_ms = line("modle_pixels_band_check (one pass over the list, row starts; waits)", timed(check), pixel_bytes)
    fill_ms = line("modle_pixels_band_fill (reads bin2 and count, stores every word)", timed(fill),
                   12 * n + band_bytes)
    with torch.cuda.stream(stream):
        torch_ms = line("torch: index arithmetic, torch.zeros, index_put_", timed(torch_form), pixel_bytes + band_bytes)
    say(f"      the fill takes {fill_ms / torch_ms:.3f} x the torch form ({torch_ms / fill_ms:.2f} x "
        f"{'faster' if fill_ms < torch_ms else 'the speed: it is SLOWER'}), check + fill {(check_ms + fill_ms) / torch_ms:.3f} x; "
        f"the fill is {fill_ms / count_ms:.2f} x the count")

    # host to device: the pixels against the dense band, both from pinned memory
    h1, h2, hc = bin1.cpu().pin_memory(), bin2.cpu().pin_memory(), count.cpu().pin_memory()
    hband = band.cpu().pin_memory()
    dband = torch.empty_like(band)

    def pixels_up():
        ex.band_from_host(h1.numpy(), h2.numpy(), hc.numpy(), NROWS, NCOLS, off, out.data_ptr(), words)

    def dense_up():
        dband.copy_(hband, non_blocking=True)

    out.fill_(-1)
    pixels_up()
    dense_up()
    torch.cuda.synchronize()
    assert torch.equal(out, band) and torch.equal(dband, band)
    up_ms = line("host clock: pinned pixels -> modle_pixels_band_from_host -> band", clocked(pixels_up), pixel_bytes)
    dense_ms = line("host clock: pinned dense band -> device (one copy)", clocked(dense_up), band_bytes)
    say(f"      the pixels take {up_ms / dense_ms:.3f} x the dense copy "
        f"({'faster' if up_ms < dense_ms else 'SLOWER'}); they are {pixel_bytes / band_bytes:.3f} x its bytes")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
