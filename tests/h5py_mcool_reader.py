"""Independent reader of one cooler inside an HDF5 file: prints the tables of the group at
`group` (`/` for a plain .cool, `/resolutions/<bin size>` for one resolution of an .mcool) as JSON,
with the file's root attributes next to them.

Run by tests/test_mcool_writer.py and tests/test_gpu_coarsen.py under an interpreter that has
h5py (the image's conda Python 3.9; the suite's own interpreter has no HDF5 binding).  Pixels are
fetched chromosome by chromosome THROUGH the indexes of that group (chrom_offset -> bin1_offset ->
pixel rows), like tests/h5py_cooler_reader.py does for a whole file, so that a wrong index shows
up as wrong pixels."""
import json
import sys

import h5py

DATASETS = ("chroms/length", "bins/chrom", "bins/start", "bins/end", "pixels/bin1_id",
            "pixels/bin2_id", "pixels/count", "indexes/bin1_offset", "indexes/chrom_offset")


def attrs_of(obj):
    return {k: (v.decode() if isinstance(v, bytes) else (v.item() if hasattr(v, "item") else v))
            for k, v in obj.attrs.items()}


def main(path, group):
    out = {}
    with h5py.File(path, "r") as f:
        out["root_attrs"] = attrs_of(f)
        out["root_attr_dtypes"] = {k: str(f.attrs.get_id(k).dtype) for k in f.attrs}
        out["root_members"] = sorted(f.keys())
        out["resolutions"] = sorted(f["resolutions"].keys(), key=int) if "resolutions" in f else []
        g = f[group]
        out["members"] = sorted(g.keys())
        out["attrs"] = attrs_of(g)
        out["attr_dtypes"] = {k: str(g.attrs.get_id(k).dtype) for k in g.attrs}
        out["dtypes"] = {name: str(g[name].dtype) for name in DATASETS}
        out["filters"] = {name: {"compression": g[name].compression, "opts": g[name].compression_opts,
                                 "chunks": list(g[name].chunks or [])} for name in DATASETS}
        out["name_dtype"] = str(g["chroms/name"].dtype)
        names = [n.decode().rstrip("\x00") for n in g["chroms/name"][:]]
        out["chroms"] = list(zip(names, [int(x) for x in g["chroms/length"][:]]))
        out["bins"] = [[int(a), int(b), int(c)] for a, b, c in
                       zip(g["bins/chrom"][:], g["bins/start"][:], g["bins/end"][:])]
        chrom_offset = g["indexes/chrom_offset"][:]
        bin1_offset = g["indexes/bin1_offset"][:]
        out["chrom_offset"] = [int(x) for x in chrom_offset]
        out["bin1_offset"] = [int(x) for x in bin1_offset]
        all_b1 = g["pixels/bin1_id"][:]
        fetched = {}
        for k, name in enumerate(names):
            for b in range(int(chrom_offset[k]), int(chrom_offset[k + 1])):
                p0, p1 = int(bin1_offset[b]), int(bin1_offset[b + 1])
                assert (all_b1[p0:p1] == b).all(), f"bin1_offset[{b}] does not delimit the pixels of bin {b}"
            lo, hi = int(bin1_offset[chrom_offset[k]]), int(bin1_offset[chrom_offset[k + 1]])
            fetched[name] = [[int(a), int(b), int(c)] for a, b, c in
                             zip(all_b1[lo:hi], g["pixels/bin2_id"][lo:hi], g["pixels/count"][lo:hi])]
        out["pixels_by_chrom"] = fetched
        out["n_pixels"] = int(g["pixels/count"].shape[0])
    json.dump(out, sys.stdout)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "/")
