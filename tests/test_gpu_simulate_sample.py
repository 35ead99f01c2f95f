"""`simulate --subsample-frac / --subsample-to` end to end, on the genome, the cell count and the options of
tests/test_gpu_simulate_ranks.py and with an .mcool of two coarse levels: the kept and the other pixels read
back out of <prefix>_sampled.mcool and <prefix>_sampled_rest.mcool add up to the pixels of the .mcool the
same run wrote; the kept ones are what the numpy restatement of tests/test_sample_outputs.py draws at the
file's global bin ids with the run's seed; every coarse level is the numpy coarsening of its own base
level; a target above the total writes the unsampled matrix with a warning; and a second run writes the
same pixels.  Each run is a fresh child process with one rank, made once per module."""
import numpy as np
import pytest

import test_gpu_simulate_ranks as ranks
from test_gpu_simulate_marginals import CHROMS, SIMULATED, pixels_of
from test_mcool_writer import read_group
from test_sample_outputs import reference_sample

from modle_amd import pixels

pytestmark = pytest.mark.gpu

BASE, COARSE = 5000, (10000, 25000)
SEED = 5  # ranks.COMMON's --seed: the default of --subsample-seed
BASIC = ["--ncells", str(ranks.NCELLS), "--no-track-1d-lef-position", "--mcool-resolutions", "10kb,25kb"]
OPTIONS = BASIC + ["--subsample-frac", "0.5", "--subsample-split"]
FILES = ["run.mcool", "run_sampled.mcool", "run_sampled_rest.mcool"]


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("sample"))


@pytest.fixture(scope="module")
def one(workdir):
    return ranks.simulate(workdir, "one", 1, 0, OPTIONS)


@pytest.fixture(scope="module")
def again(workdir, one):  # (after the first run has ended)
    return ranks.simulate(workdir, "again", 1, 0, OPTIONS)


def global_pixels(mcool, bin_size=BASE):
    """{(bin1, bin2): count} of one resolution, the ids as the file has them"""
    group = read_group(mcool, f"/resolutions/{bin_size}")
    out = {}
    for name, _ in CHROMS:
        for b1, b2, c in group["pixels_by_chrom"][name]:
            out[(b1, b2)] = c
    assert len(out) == group["n_pixels"]
    return out


@pytest.fixture(scope="module")
def base_pixels(one):
    prefix = one[0]
    return tuple(global_pixels(prefix + suffix) for suffix in (".mcool", "_sampled.mcool", "_sampled_rest.mcool"))


def test_the_files_of_the_run(one):
    assert ranks.files_of(one[0]) == FILES
    written = [l for l in one[2].splitlines() if l.startswith("written ")]
    assert [l.split()[1].rsplit("/", 1)[1] for l in written] == FILES
    assert f"(threshold {2**31} of 2^32)" in written[1] and f"(threshold {2**31} of 2^32)" in written[2]


def test_kept_and_rest_add_up_to_the_matrix(base_pixels):
    whole, kept, rest = base_pixels
    assert len(whole) > 1000 and 0 < len(kept) <= len(whole) and 0 < len(rest) <= len(whole)
    assert min(kept.values()) > 0 and min(rest.values()) > 0
    assert set(kept) | set(rest) == set(whole)
    for key, n in whole.items():
        assert kept.get(key, 0) + rest.get(key, 0) == n, key


def test_the_kept_pixels_are_the_restatement_at_the_global_ids(base_pixels):
    whole, kept, _ = base_pixels
    keys = sorted(whole)
    b1, b2 = np.array([k[0] for k in keys]), np.array([k[1] for k in keys])
    assert b1.max() >= 500  # chrC's bins lie behind chrA's and chrB's: the ids are the file's, not the interval's
    want = reference_sample(b1, b2, np.array([whole[k] for k in keys]), pixels.sample_threshold(0.5), SEED)
    assert np.array_equal(np.array([kept.get(k, 0) for k in keys]), want)
    assert 0 < int(want.sum()) < sum(whole.values())


@pytest.mark.parametrize("suffix", ["_sampled.mcool", "_sampled_rest.mcool"])
def test_every_coarse_level_is_the_coarsening_of_its_own_base_level(one, suffix):
    fine = pixels_of(one[0] + suffix, BASE)
    for bin_size in COARSE:
        k = bin_size // BASE
        level = pixels_of(one[0] + suffix, bin_size)
        for name in SIMULATED:  # (whole chromosomes: the coarse bins start with the fine ones)
            _, b1, b2, count = fine[name]
            want = {}
            for key, c in zip(zip((b1 // k).tolist(), (b2 // k).tolist()), count.tolist()):
                want[key] = want.get(key, 0) + c
            _, c1, c2, got = level[name]
            assert list(zip(c1.tolist(), c2.tolist())) == sorted(want), (bin_size, name)
            assert got.tolist() == [want[key] for key in sorted(want)], (bin_size, name)
        assert len(level["chrB"][3]) == 0


def test_a_target_above_the_total_writes_the_unsampled_matrix_with_a_warning(workdir, one, base_pixels):
    total = sum(base_pixels[0].values())
    prefix, _, stderr = ranks.simulate(workdir, "all", 1, 0, BASIC + ["--subsample-to", str(total)])
    assert ranks.files_of(prefix) == FILES[:2]
    assert (f"warning: --subsample-to {total} is not below the {total} contacts of the matrix: the sampled file holds "
            "the unsampled matrix") in stderr.splitlines()
    for bin_size in (BASE,) + COARSE:
        assert global_pixels(prefix + "_sampled.mcool", bin_size) == global_pixels(prefix + ".mcool", bin_size)
    assert global_pixels(prefix + ".mcool") == base_pixels[0]


def test_a_second_run_writes_the_same_pixels(one, again, base_pixels):
    assert ranks.files_of(again[0]) == FILES
    for suffix, want in zip((".mcool", "_sampled.mcool", "_sampled_rest.mcool"), base_pixels):
        assert global_pixels(again[0] + suffix) == want
    for bin_size in COARSE:
        assert global_pixels(again[0] + "_sampled.mcool", bin_size) == global_pixels(one[0] + "_sampled.mcool", bin_size)
