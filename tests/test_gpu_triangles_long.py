"""The triangle sums of long bands (tests/test_gpu_triangles.py has the shapes around the tiles): 70 000 columns
on 8 diagonals, word for word against pixels.triangle_sums_host, and a band of one diagonal whose 2^26 + 70 columns
take the launches of both kernels, 64 columns or starts to a workgroup, past the 2^20 workgroups of a grid's x: the
workgroups beyond go to y, and no loop strides by the grid.  There the table at the largest width 1 is the band
itself, and it is compared on the device."""
import numpy as np
import pytest

from test_gpu_marginals import Guarded, make_band
from test_gpu_stripe_profiles import FilledOut

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ex():
    from modle_amd import pixels

    with pixels.Extractor(0) as e:
        yield e


@pytest.mark.parametrize("width,d0", [(1, 0), (8, 0), (8, 2), (7, 6)])
def test_the_table_of_a_long_band(ex, width, d0):
    from modle_amd import pixels

    nrows, ncols = 8, 70_000
    band = make_band(nrows, ncols, "tenth")
    want = pixels.triangle_sums_host(band, nrows, ncols, width, d0)
    src = Guarded(band)
    d_out = FilledOut(width * ncols)
    ex.triangles_into(src.data_ptr(), nrows, ncols, width, d0, d_out.data_ptr(), width * ncols)
    got = d_out.sums((width, ncols))
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert d_out.guards_intact() and src.unchanged()
    assert np.array_equal(ex.triangles_to_host(src.data_ptr(), nrows, ncols, width, d0), want)


def test_both_launches_pass_the_two_to_the_twenty_workgroups_of_a_grid_s_x(ex):
    import torch

    ncols = 64 * 2**20 + 70  # 2^20 + 2 workgroups of 64 columns, and as many of 64 starts
    dev = torch.device("cuda", 0)
    band = (torch.arange(ncols + 1, dtype=torch.int64, device=dev) * 2654435761) & 0xFFFFFFFF  # one pixel per column
    want = band[:ncols].clone()
    band = band.to(torch.int32)  # (the low 32 bits, bit for bit)
    band[ncols] = -1             # the word beyond the band is never read
    out = torch.full((1, ncols), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev)  # 0xA5 bytes
    torch.cuda.synchronize()
    ex.triangles_into(band.data_ptr(), 1, ncols, 1, 0, out.data_ptr(), ncols)
    torch.cuda.synchronize()
    assert torch.equal(out[0], want)
    assert int(want[2**26:].count_nonzero()) == 70  # the columns of the workgroups in y are not all alike
    # one diagonal ignored: zeros, stored in every word
    out.fill_(-0x5A5A5A5A5A5A5A5B)
    ex.triangles_into(band.data_ptr(), 1, ncols, 1, 1, out.data_ptr(), ncols)
    torch.cuda.synchronize()
    assert int(out.count_nonzero()) == 0
