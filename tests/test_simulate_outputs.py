"""The front end's output path without a GPU: cli.preflight (which files a run plans, and the
refuse-to-overwrite rule) and driver.write_pixels (one writer for .cool and .mcool), driven by a
numpy-only callback.  The expected files come from driver.write_cooler on the dense bands and from
cooler.CoolerWriter on the restated coarse pixel tables of test_mcool_writer, with bin offsets worked
out here, never from what write_pixels hands its callback."""
import os

import numpy as np
import pytest

from test_cooler_pixels import assert_same_cooler, random_band
from test_mcool_writer import assert_same_group, coarsen_pixels, fine_pixels, read_group

from modle_amd import api, cli, driver, pixels

# ---- preflight ----------------------------------------------------------------------------------

SUFFIXES = {"cool": ".cool", "mcool": ".mcool", "bw": "_lef_1d_occupancy.bw", "npz": "_dense.npz"}
TRACK, NO_TRACK = ["--track-1d-lef-position"], ["--no-track-1d-lef-position"]
MCOOL, REGION = ["--mcool-resolutions", "10kb,25kb"], ["--dense-region", "chrA"]


@pytest.fixture
def prefix(tmp_path, monkeypatch):
    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(name, raising=False)
    return str(tmp_path / "out" / "p")


def run_preflight(prefix, *extra):
    a = cli.build_parser().parse_args(["simulate", "-c", "g.chrom.sizes", "-b", "b.bed", "-o", prefix,
                                       "-r", "5kb", *extra])
    return cli.preflight(a, cli.config_from_args(a))


def touch(prefix, *which):
    os.makedirs(os.path.dirname(prefix), exist_ok=True)
    for w in which:
        with open(prefix + SUFFIXES[w], "wb") as fh:
            fh.write(b"precious " + w.encode())


def snapshot(prefix):
    out = {}
    for w, suffix in SUFFIXES.items():
        st = os.stat(prefix + suffix) if os.path.exists(prefix + suffix) else None
        out[w] = None if st is None else (st.st_size, st.st_mtime_ns)
    return out


def test_preflight_plans_the_files_of_the_run(prefix):
    pre = run_preflight(prefix, *TRACK)
    assert pre.bin_sizes is None and (pre.rank, pre.world, pre.device) == (0, 1, 0)
    assert pre.outputs == cli.Outputs(prefix + ".cool", prefix + "_lef_1d_occupancy.bw", None, None)
    assert os.path.isdir(os.path.dirname(prefix)) and snapshot(prefix) == dict.fromkeys(SUFFIXES)
    pre = run_preflight(prefix, *NO_TRACK, *MCOOL)
    assert pre.bin_sizes == [5000, 10000, 25000]
    assert pre.outputs == cli.Outputs(prefix + ".mcool", None, None, None)
    pre = run_preflight(prefix, *TRACK, *REGION, "--log-model-internal-state", "--device", "3")
    assert pre.device == 3
    assert pre.outputs == cli.Outputs(prefix + ".cool", prefix + "_lef_1d_occupancy.bw", prefix + "_dense.npz",
                                      prefix + "_internal_state.log.gz")
    assert snapshot(prefix) == dict.fromkeys(SUFFIXES)  # planning writes nothing


def test_preflight_reads_rank_world_and_device_from_the_launcher(prefix, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "4")
    monkeypatch.setenv("RANK", "2")
    monkeypatch.setenv("LOCAL_RANK", "1")
    touch(prefix, "cool")  # only rank 0 looks at the files
    pre = run_preflight(prefix, "--log-model-internal-state")
    assert (pre.rank, pre.world, pre.device) == (2, 4, 1)
    assert pre.outputs.state_log == prefix + "_internal_state.rank2.log.gz"


def test_dist_backend_parses_defaults_to_nccl_and_refuses_other_values(prefix, capsys):
    def parse(*extra):
        return cli.build_parser().parse_args(["simulate", "-c", "g.chrom.sizes", "-b", "b.bed", "-o", prefix, *extra])

    assert parse().dist_backend == "nccl"
    assert parse("--dist-backend", "nccl").dist_backend == "nccl"
    assert parse("--dist-backend", "gloo").dist_backend == "gloo"
    for bad in ("mpi", "GLOO", "rccl", ""):
        with pytest.raises(SystemExit) as e:
            parse("--dist-backend", bad)
        assert e.value.code == 2 and "--dist-backend" in capsys.readouterr().err
    # the backend settles nothing that preflight settles
    for options in (TRACK, NO_TRACK + MCOOL, TRACK + REGION + ["--log-model-internal-state", "--device", "3"]):
        assert run_preflight(prefix, *options, "--dist-backend", "gloo") == run_preflight(prefix, *options)


# (files present, options, the file the refusal names -- None: the run may go on)
CASES = [
    (["cool"], TRACK, "cool"),
    (["cool"], TRACK + MCOOL, None),      # an .mcool run does not write <prefix>.cool
    (["mcool"], TRACK + MCOOL, "mcool"),
    (["mcool"], TRACK, None),
    (["bw"], TRACK, "bw"),
    (["bw"], NO_TRACK, None),
    (["npz"], TRACK + REGION, "npz"),
    (["npz"], TRACK, None),
    (["cool", "bw", "npz"], TRACK + REGION, "cool"),   # the order: cooler, bigwig, .npz
    (["bw", "npz"], TRACK + REGION, "bw"),
    (["mcool", "bw", "npz"], TRACK + MCOOL + REGION, "mcool"),
]


@pytest.mark.parametrize("present,options,named", CASES)
def test_preflight_refuses_to_overwrite_and_harms_nothing(prefix, present, options, named):
    touch(prefix, *present)
    before = snapshot(prefix)
    if named is None:
        run_preflight(prefix, *options)
    else:
        with pytest.raises(SystemExit) as e:
            run_preflight(prefix, *options)
        assert str(e.value) == f"refusing to overwrite {prefix + SUFFIXES[named]}: pass --force to overwrite"
    assert snapshot(prefix) == before
    # --force passes in every case, and --skip-output looks at nothing and plans nothing
    assert run_preflight(prefix, *options, "--force").outputs.cooler is not None
    assert run_preflight(prefix, *options, "--skip-output").outputs == cli.Outputs(None, None, None, None)
    assert snapshot(prefix) == before


def test_preflight_with_skip_output_does_not_make_the_directory(prefix):
    run_preflight(prefix, "--skip-output", *REGION, "--log-model-internal-state")
    assert not os.path.exists(os.path.dirname(prefix))


def test_a_bad_resolution_list_is_refused_before_the_files_are_looked_at(prefix):
    with pytest.raises(SystemExit) as e:
        run_preflight(prefix, "--mcool-resolutions", "10kb,12kb")
    assert "--mcool-resolutions" in str(e.value) and "12000" in str(e.value)
    assert not os.path.exists(os.path.dirname(prefix))


def test_the_missing_interactions_warning_starts_at_one_percent():
    said = []
    for total, missed in ((0, 0), (1000, 0), (991, 9), (990, 10), (0, 5)):
        driver.warn_missing("chrA", total, missed, said.append)
    assert said == ["warning: 1.00% missing interactions for chrA", "warning: 100.00% missing interactions for chrA"]


# ---- write_pixels -------------------------------------------------------------------------------

BASE = 5000
BIN_SIZES = [BASE, 2 * BASE, 5 * BASE]
CHROMS = [("chrA", 1_003_000), ("chrB", 600_000)]
# (chromosome, start, nrows, ncols, skipped): the first interval starts at fine bin 21, a multiple of
# neither factor; the second is skipped (it has no matrix); the third is a whole chromosome
INTERVALS = [("chrA", 105_000, 12, 30, False), ("chrA", 500_000, 40, 90, True), ("chrB", 0, 20, 120, False)]
KW = dict(assembly="asm", generated_by="gen", metadata_json='{"k": 1}')


def chrom_offset(name, bin_size):
    off = 0
    for n, size in CHROMS:
        if n == name:
            return off
        off += -(-size // bin_size)


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(77)
    cfg = api.make_config(bin_size=BASE)
    plan, bands = [], []
    for name, start, nrows, ncols, skipped in INTERVALS:
        iv = {"name": name, "size": dict(CHROMS)[name], "start": start, "end": start + ncols * BASE}
        plan.append({"interval": iv, "nrows": nrows, "ncols": ncols, "tasks": None, "skipped": skipped})
        bands.append(random_band(rng, nrows, ncols, 0.4))
    return cfg, plan, bands


def expected_table(plan, bands, k, b):
    """(first bin of the interval within the file at bin size `b`, its bins there, bin1, bin2, count)
    of plan entry k, from this module's own arithmetic"""
    iv, nrows, ncols = plan[k]["interval"], plan[k]["nrows"], plan[k]["ncols"]
    first, factor = iv["start"] // BASE, b // BASE
    px = fine_pixels(bands[k], nrows, ncols, first)  # ids within the chromosome
    if factor > 1:
        px = coarsen_pixels(*px, 0, 0, factor)
    off = chrom_offset(iv["name"], b)
    n_bins = (first + ncols - 1) // factor - first // factor + 1
    return off + first // factor, n_bins, px[0] + off, px[1] + off, px[2]


def numpy_extract(plan, bands, calls):
    def extract(k, factor, first_bin, bin_offset):
        calls.append((k, factor))
        assert not plan[k]["skipped"] and first_bin == plan[k]["interval"]["start"] // BASE
        want_offset, n_bins, b1, b2, cn = expected_table(plan, bands, k, factor * BASE)
        assert bin_offset == want_offset
        index = np.searchsorted(b1 - bin_offset, np.arange(n_bins + 1)).astype(np.int64)
        return pixels.Pixels(b1, b2, cn, index, pixels.Stats(len(cn), int(cn.sum()), int(cn.max())))
    return extract


@pytest.fixture(scope="module")
def written(tmp_path_factory, case):
    """the dense-band .cool, and the .cool and .mcool of write_pixels, written once"""
    cfg, plan, bands = case
    d = tmp_path_factory.mktemp("written")
    paths = {w: str(d / w) for w in ("dense.cool", "sparse.cool", "out.mcool")}
    calls = {"sparse.cool": [], "out.mcool": []}
    driver.write_cooler(paths["dense.cool"], cfg, plan, bands, chroms=CHROMS, **KW)
    driver.write_pixels(paths["sparse.cool"], cfg, plan, numpy_extract(plan, bands, calls["sparse.cool"]),
                        chroms=CHROMS, **KW)
    driver.write_pixels(paths["out.mcool"], cfg, plan, numpy_extract(plan, bands, calls["out.mcool"]), BIN_SIZES,
                        chroms=CHROMS, **KW)
    return paths, calls


def test_without_bin_sizes_the_file_is_the_one_from_the_dense_bands(case, written):
    _, plan, bands = case
    paths, calls = written
    assert calls["sparse.cool"] == [(0, 1), (2, 1)]  # genome order, the skipped entry is never asked for
    got = assert_same_cooler(paths["dense.cool"], paths["sparse.cool"])
    assert got["attrs"]["nnz"] == sum(len(expected_table(plan, bands, k, BASE)[2]) for k in (0, 2)) > 500


def test_with_bin_sizes_the_base_resolution_is_that_same_file(case, written, tmp_path):
    cfg, plan, _ = case
    paths, calls = written
    assert driver.mcool_collision(plan, BASE, BIN_SIZES) is None
    assert calls["out.mcool"] == [(k, f) for k in (0, 2) for f in (1, 2, 5)]
    fine = read_group(paths["out.mcool"], f"/resolutions/{BASE}")
    assert fine["resolutions"] == [str(b) for b in BIN_SIZES] and fine["root_attrs"]["format"] == "HDF5::MCOOL"
    assert_same_group(fine, read_group(paths["dense.cool"]))
    with pytest.raises(ValueError):  # the list starts with the simulation's bin size
        driver.write_pixels(str(tmp_path / "bad.mcool"), cfg, plan, None, BIN_SIZES[1:], chroms=CHROMS)
    assert not os.path.exists(str(tmp_path / "bad.mcool"))


@pytest.mark.parametrize("b", BIN_SIZES[1:])
def test_with_bin_sizes_a_coarse_resolution_is_the_restated_cooler(case, written, tmp_path, b):
    from modle_amd import cooler

    _, plan, bands = case
    alone = str(tmp_path / "alone.cool")
    with cooler.CoolerWriter(alone, CHROMS, b, **KW) as w:
        for k in (0, 2):
            _, n_bins, b1, b2, cn = expected_table(plan, bands, k, b)
            w.append_pixels(plan[k]["interval"]["name"], n_bins, b1, b2, cn, offset_bp=plan[k]["interval"]["start"])
    got = read_group(written[0]["out.mcool"], f"/resolutions/{b}")
    assert_same_group(got, read_group(alone))
    want_sum = sum(int(expected_table(plan, bands, k, BASE)[4].sum()) for k in (0, 2))
    assert got["attrs"]["bin-size"] == b and got["attrs"]["sum"] == want_sum and got["n_pixels"] > 100
