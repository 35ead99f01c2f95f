"""Spoils a cooler (v3) file in place, for the refusals of the reader (tests/test_band_outputs.py).

Run under an interpreter that has h5py (the image's conda Python 3.9, like tests/h5py_cooler_reader.py):

    h5py_cooler_spoil.py FILE WHAT [GROUP]

WHAT: `bin-type` sets the attribute to "variable"; `float-count` replaces pixels/count by float64;
`short-index` drops the last entry of indexes/bin1_offset."""
import sys

import h5py
import numpy as np


def main(path, what, group="/"):
    with h5py.File(path, "r+") as f:
        g = f[group]
        if what == "bin-type":
            g.attrs["bin-type"] = "variable"
        elif what == "float-count":
            counts = g["pixels/count"][:].astype(np.float64)
            del g["pixels/count"]
            g["pixels"].create_dataset("count", data=counts)
        elif what == "short-index":
            index = g["indexes/bin1_offset"][:-1]
            del g["indexes/bin1_offset"]
            g["indexes"].create_dataset("bin1_offset", data=index)
        else:
            raise SystemExit(f"unknown: {what}")


if __name__ == "__main__":
    main(*sys.argv[1:])
