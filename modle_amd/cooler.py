"""ctypes view of the cooler (v3) writer, include/modle_cooler.h.  The product path is the C
library (modle_amd/libmodle_cooler.so, built by `make -C modle_amd/csrc cooler`); this module
mirrors how the reference's IO thread uses it (simulation.cpp:117-168, 217-269): create the file
with every chromosome, append the interval matrices in genome order, close.  CoolerReader is the way
back (include/modle_cooler_read.h): a chromosome's pixels as they lie in the file."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(_HERE, "libmodle_cooler.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run `make -C modle_amd/csrc cooler` "
                               "(python -c 'import __graft_entry__ as g; g.build()')")
        lb = ctypes.CDLL(path)
        lb.modle_cool_create.restype = ctypes.c_int
        lb.modle_cool_create.argtypes = [
            ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p),
            ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t, ctypes.c_uint32, ctypes.c_char_p,
            ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_char_p,
            ctypes.c_size_t]
        lb.modle_cool_append_matrix.restype = ctypes.c_int
        lb.modle_cool_append_matrix.argtypes = [
            ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
            ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t]
        lb.modle_cool_bin_offset.restype = ctypes.c_int  # include/modle_cooler_pixels.h
        lb.modle_cool_bin_offset.argtypes = [
            ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.POINTER(ctypes.c_int64),
            ctypes.c_char_p, ctypes.c_size_t]
        lb.modle_cool_append_pixels.restype = ctypes.c_int
        lb.modle_cool_append_pixels.argtypes = [
            ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_char_p,
            ctypes.c_size_t]
        lb.modle_cool_close.restype = ctypes.c_int
        lb.modle_cool_close.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        lb.modle_mcool_create.restype = ctypes.c_int  # include/modle_mcool.h
        lb.modle_mcool_create.argtypes = [
            ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p),
            ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32),
            ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
            ctypes.POINTER(ctypes.c_void_p), ctypes.c_char_p, ctypes.c_size_t]
        lb.modle_mcool_resolution.restype = ctypes.c_void_p
        lb.modle_mcool_resolution.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
        lb.modle_mcool_close.restype = ctypes.c_int
        lb.modle_mcool_close.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        vpp = ctypes.POINTER(ctypes.c_void_p)  # include/modle_cooler_read.h
        lb.modle_cool_reader_open.restype = ctypes.c_int
        lb.modle_cool_reader_open.argtypes = [ctypes.c_char_p, vpp, ctypes.c_char_p, ctypes.c_size_t]
        lb.modle_cool_reader_info.restype = ctypes.c_int
        lb.modle_cool_reader_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32),
                                              ctypes.POINTER(ctypes.c_size_t)]
        lb.modle_cool_reader_chrom.restype = ctypes.c_int
        lb.modle_cool_reader_chrom.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_char_p),
                                               ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int64),
                                               ctypes.POINTER(ctypes.c_uint64)]
        lb.modle_cool_reader_indexes.restype = ctypes.c_int
        lb.modle_cool_reader_indexes.argtypes = [ctypes.c_void_p, vpp, vpp, ctypes.POINTER(ctypes.c_uint64)]
        lb.modle_cool_reader_pixels.restype = ctypes.c_int
        lb.modle_cool_reader_pixels.argtypes = [ctypes.c_void_p, ctypes.c_size_t, vpp, vpp, vpp,
                                                ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int64),
                                                ctypes.c_char_p, ctypes.c_size_t]
        lb.modle_cool_reader_close.restype = None
        lb.modle_cool_reader_close.argtypes = [ctypes.c_void_p]
        _LIB = lb
    return _LIB


class CoolerError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"modle_cooler error {code}: {message}")
        self.code = code


def _marshal_chroms(chroms):
    """[(name, size)] as the (names, sizes, count) arguments of the create calls"""
    names = (ctypes.c_char_p * len(chroms))(*[n.encode() for n, _ in chroms])
    sizes = (ctypes.c_uint32 * len(chroms))(*[int(s) for _, s in chroms])
    return names, sizes, len(chroms)


class _Handle:
    """A handle of the library with its error buffer and the chromosomes' indexes.  `_close_fn` names
    the call that finishes a handle this object owns; a borrowed one (one resolution of a
    multi-resolution file) has none and is only let go of."""
    _close_fn = None

    def __init__(self, handle, chroms):
        self._h = handle
        self._err = ctypes.create_string_buffer(512)
        self._index = {n: i for i, (n, _) in enumerate(chroms)}

    def _cid(self, chrom):
        return self._index[chrom] if isinstance(chrom, str) else int(chrom)

    def _call(self, fn, *args):
        rc = fn(*args, self._err, len(self._err))
        if rc != 0:
            raise CoolerError(rc, self._err.value.decode())

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            if self._close_fn is not None:
                self._call(getattr(lib(), self._close_fn), h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class _Cooler(_Handle):
    """One cooler behind a modle_cool_file handle: a file of its own (CoolerWriter) or one
    resolution of a multi-resolution file (McoolWriter.resolution)."""

    def append(self, chrom, band, nrows, ncols, offset_bp=0):
        """band: uint32 array of nrows * ncols (+1) words in the layout of the HIP library"""
        import numpy as np
        band = np.ascontiguousarray(band, dtype=np.uint32)
        if band.size < nrows * ncols:
            raise ValueError("band matrix smaller than nrows * ncols")
        self._call(lib().modle_cool_append_matrix, self._h, self._cid(chrom), int(offset_bp),
                   band.ctypes.data, int(nrows), int(ncols))

    def bin_offset(self, chrom, offset_bp=0):
        """first bin id, within the file, of the interval of `chrom` that starts at `offset_bp`:
        what the pixels of that interval are extracted with (pixels.extract(bin_offset=...))"""
        out = ctypes.c_int64(0)
        self._call(lib().modle_cool_bin_offset, self._h, self._cid(chrom), int(offset_bp), ctypes.byref(out))
        return out.value

    def append_pixels(self, chrom, ncols, bin1, bin2, count, bin1_offset=None, offset_bp=0):
        """the sorted non-zero pixels of one interval of `ncols` bins (modle_cool_append_pixels):
        int64 file-wide bin ids, int32 counts, and optionally the interval's bin1_offset index
        (ncols + 1 entries), which is then checked against the pixels"""
        import numpy as np
        bin1 = np.ascontiguousarray(bin1, dtype=np.int64)
        bin2 = np.ascontiguousarray(bin2, dtype=np.int64)
        count = np.ascontiguousarray(count, dtype=np.int32)
        if not (bin1.ndim == bin2.ndim == count.ndim == 1 and len(bin1) == len(bin2) == len(count)):
            raise ValueError("bin1, bin2 and count must be 1-D arrays of one length")
        off = None
        if bin1_offset is not None:
            off = np.ascontiguousarray(bin1_offset, dtype=np.int64)
            if off.shape != (int(ncols) + 1,):
                raise ValueError("bin1_offset must hold ncols + 1 entries")
        self._call(lib().modle_cool_append_pixels, self._h, self._cid(chrom), int(offset_bp), int(ncols),
                   bin1.ctypes.data, bin2.ctypes.data, count.ctypes.data, len(bin1),
                   off.ctypes.data if off is not None else None)


class CoolerWriter(_Cooler):
    """`chroms`: list of (name, size); matrices are appended in ascending chromosome order.  It is
    the one-resolution case of McoolWriter: `bin_sizes == [bin_size]`, `resolution(bin_size)` is the
    writer itself."""
    _close_fn = "modle_cool_close"

    def __init__(self, path, chroms, bin_size, assembly="unknown", generated_by="modle-hip",
                 metadata_json="", force_overwrite=False):
        super().__init__(ctypes.c_void_p(), chroms)
        self._call(lib().modle_cool_create, os.fsencode(path), int(force_overwrite), *_marshal_chroms(chroms),
                   int(bin_size), assembly.encode(), generated_by.encode(), metadata_json.encode(),
                   ctypes.byref(self._h))
        self.bin_sizes = [int(bin_size)]

    def resolution(self, bin_size):
        if int(bin_size) != self.bin_sizes[0]:
            raise KeyError(bin_size)
        return self


class McoolWriter(_Handle):
    """A multi-resolution cooler (include/modle_mcool.h): one cooler per entry of `bin_sizes`
    (ascending, distinct multiples of the first) under /resolutions/<bin size>.  `resolution(b)`
    is written like a CoolerWriter of bin size `b` (bin_offset, append_pixels, append), in genome
    order per resolution; `close` finishes all of them."""
    _close_fn = "modle_mcool_close"

    def __init__(self, path, chroms, bin_sizes, assembly="unknown", generated_by="modle-hip",
                 metadata_json="", force_overwrite=False):
        bin_sizes = [int(b) for b in bin_sizes]
        if any(not 0 <= b < 2**32 for b in bin_sizes):
            raise CoolerError(-1, "modle_mcool_create: a bin size does not fit 32 bits")
        res = (ctypes.c_uint32 * len(bin_sizes))(*bin_sizes)
        super().__init__(ctypes.c_void_p(), chroms)
        self._call(lib().modle_mcool_create, os.fsencode(path), int(force_overwrite), *_marshal_chroms(chroms),
                   res, len(bin_sizes), assembly.encode(), generated_by.encode(), metadata_json.encode(),
                   ctypes.byref(self._h))
        self.bin_sizes = bin_sizes
        self._res = {b: _Cooler(ctypes.c_void_p(lib().modle_mcool_resolution(self._h, k)), chroms)
                     for k, b in enumerate(bin_sizes)}

    def resolution(self, bin_size):
        return self._res[int(bin_size)]

    def close(self):
        for r in self._res.values():
            r.close()  # borrowed handles: gone with the file
        super().close()


def _copy_array(ptr, n, ctype, dtype):
    import numpy as np
    if n == 0 or not ptr:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctype)), shape=(n,)).copy()


class CoolerReader:
    """A cooler opened for reading (include/modle_cooler_read.h): `uri` is `path`, the cooler at the root of
    the file, or `path::/resolutions/10000`, that group of an .mcool.  `bin_size`, `chroms` ([(name, size)]) and
    `chrom_offset` (the first bin of every chromosome and the number of bins) are read on opening; `pixels(chrom)`
    hands over a chromosome's pixels as they lie in the file.  A bin-type other than "fixed", counts that are no
    integers and indexes of the wrong length are refused with a CoolerError; balancing weights are ignored."""

    def __init__(self, uri):
        self.uri = os.fspath(uri)
        self._h = ctypes.c_void_p()
        self._err = ctypes.create_string_buffer(1024)
        rc = lib().modle_cool_reader_open(os.fsencode(self.uri), ctypes.byref(self._h), self._err, len(self._err))
        if rc != 0:
            self._h = None
            raise CoolerError(rc, self._err.value.decode(errors="replace"))
        bs, n = ctypes.c_uint32(), ctypes.c_size_t()
        lib().modle_cool_reader_info(self._h, ctypes.byref(bs), ctypes.byref(n))
        self.bin_size = bs.value
        self.chroms, self.chrom_offset = [], []
        for c in range(n.value):
            name, size, first, bins = ctypes.c_char_p(), ctypes.c_uint64(), ctypes.c_int64(), ctypes.c_uint64()
            lib().modle_cool_reader_chrom(self._h, c, ctypes.byref(name), ctypes.byref(size), ctypes.byref(first),
                                          ctypes.byref(bins))
            self.chroms.append((name.value.decode(), size.value))
            self.chrom_offset.append(first.value)
        self.chrom_offset.append(self.chrom_offset[-1] + bins.value if self.chroms else 0)
        self._index = {name: i for i, (name, _) in enumerate(self.chroms)}

    def _cid(self, chrom):
        if isinstance(chrom, str):
            if chrom not in self._index:
                raise KeyError(f"chromosome {chrom!r} is not in {self.uri}")
            return self._index[chrom]
        return int(chrom)

    def n_bins(self, chrom):
        c = self._cid(chrom)
        return self.chrom_offset[c + 1] - self.chrom_offset[c]

    def bin1_offset(self):
        """the file's indexes/bin1_offset, numpy int64 with one entry per bin and one more"""
        import numpy as np
        p, n = ctypes.c_void_p(), ctypes.c_uint64()
        lib().modle_cool_reader_indexes(self._h, None, ctypes.byref(p), ctypes.byref(n))
        return _copy_array(p.value, n.value + 1, ctypes.c_int64, np.int64)

    def pixels(self, chrom):
        """(bin1, bin2, count, first_bin) of the pixels whose bin1 lies in `chrom` (a name or an index): numpy
        int64, int64 and int32 arrays the caller owns, with the file's bin ids, in the file's order, the trans
        pixels included, and the id of the chromosome's first bin"""
        import numpy as np
        p1, p2, pc = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        n, first = ctypes.c_uint64(), ctypes.c_int64()
        rc = lib().modle_cool_reader_pixels(self._h, self._cid(chrom), ctypes.byref(p1), ctypes.byref(p2),
                                            ctypes.byref(pc), ctypes.byref(n), ctypes.byref(first), self._err,
                                            len(self._err))
        if rc != 0:
            raise CoolerError(rc, self._err.value.decode(errors="replace"))
        return (_copy_array(p1.value, n.value, ctypes.c_int64, np.int64),
                _copy_array(p2.value, n.value, ctypes.c_int64, np.int64),
                _copy_array(pc.value, n.value, ctypes.c_int32, np.int32), first.value)

    def close(self):
        if self._h:
            h, self._h = self._h, None
            lib().modle_cool_reader_close(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
