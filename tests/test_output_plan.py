"""The plan of a run and the output stage that follows it, without a GPU: cli.preflight makes the whole plan
once (every analysis with its file, the reference cooler opened one time), cli.check_plan judges that plan and
nothing else, driver.write_outputs writes rank 0's files in their order from a stand-in simulator over a numpy
band, driver.bin_span is the one form of a bin's clipped ends, and the front end's limits are the library's."""
import functools
import os

import numpy as np
import pytest

from test_cooler_pixels import reference_pixels
from test_gpu_analyze import analysis_options
from test_gpu_marginals import make_band, reference_marginals
from test_gpu_simulate_ranks import COMMON
from test_insulation_outputs import brute_n_valid, prefix_insulation
from test_stripes_outputs import CHROMS, entry

from modle_amd import api, cli, cooler, driver, pixels


@pytest.fixture
def prefix(tmp_path, monkeypatch):
    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(name, raising=False)
    return str(tmp_path / "out" / "p")


@pytest.fixture
def ref(tmp_path):
    """a .cool at 5 kb of CHROMS, without a pixel"""
    path = str(tmp_path / "ref.cool")
    with cooler.CoolerWriter(path, CHROMS, 5000):
        pass
    return path


def parse(prefix, *extra):
    a = cli.build_parser().parse_args(["simulate", "-c", "g.chrom.sizes", "-b", "b.bed", "-o", prefix, "-r", "5kb",
                                       "--no-track-1d-lef-position", *extra])
    return a, cli.config_from_args(a)


# ---- the plan ---------------------------------------------------------------------------------------------

def test_the_reference_is_read_once_before_the_launch(prefix, ref, monkeypatch):
    made, real = [], cooler.CoolerReader

    def counted(*args, **kw):
        made.append(args)
        return real(*args, **kw)

    monkeypatch.setattr(cooler, "CoolerReader", counted)
    plan = [entry("chrA", 0, 100_000, 8, 20), entry("chrB", 0, 40_000, 8, 8, skipped=True)]
    a, cfg = parse(prefix, "--compare-to", ref, "--compare-metrics", "spearman")
    pre = cli.preflight(a, cfg)
    assert cli.check_plan(a, cfg, pre, plan, CHROMS) == []
    assert made == [(ref,)]
    assert pre.stripes == cli.Stripes(prefix + "_stripes.tsv", ref, 5000, ["spearman"], False, 5000, CHROMS)
    # check_plan judges the Stripes of the plan, not one it makes from the arguments: a doctored one is refused
    doctored = pre._replace(stripes=pre.stripes._replace(ref_chroms=[("chrB", 40_000)]))
    with pytest.raises(SystemExit) as e:
        cli.check_plan(a, cfg, doctored, plan, CHROMS)
    assert str(e.value) == f"--compare-to {ref}: the file has no chromosome chrA"
    assert made == [(ref,)]


def test_the_preflight_is_the_whole_plan(prefix, ref, tmp_path):
    bedpe = str(tmp_path / "loops.bedpe")  # (named, not read: check_plan reads it)
    a = cli.build_parser().parse_args(
        ["simulate", "-c", "g.chrom.sizes", "-b", "b.bed", "-o", prefix, *COMMON, "--no-track-1d-lef-position",
         *analysis_options(bedpe), "--subsample-split", "--coverage-ignore-diags", "3", "--compare-to", ref])
    cfg = cli.config_from_args(a)
    pre = cli.preflight(a, cfg)
    kept_path, rest_path = cli.sampled_paths(prefix, mcool=True)
    assert pre.bin_sizes == [5000, 10000, 25000] and (pre.rank, pre.world, pre.device) == (0, 1, 0)
    assert pre.outputs == cli.Outputs(cli.output_paths(prefix, mcool=True)[0], None, cli.dense_path(prefix), None,
                                      cli.expected_path(prefix), cli.coverage_path(prefix))
    assert pre.coverage_min_diag == 3
    for record, path in ((pre.insulation, cli.insulation_path(prefix)), (pre.dots, cli.dots_path(prefix)),
                         (pre.pileup, cli.pileup_path(prefix)), (pre.subsample, kept_path),
                         (pre.stripes, cli.stripes_path(prefix))):
        assert record is not None and record.path == path
    assert pre.insulation.windows == a.insulation_windows and pre.dots.folds == a.dots_folds
    assert pre.pileup.sources == ["dots", bedpe] and pre.pileup.flank == 25_000
    assert pre.subsample == cli.Subsample(kept_path, rest_path, 0.5, None, int(cfg.seed), True)
    assert pre.stripes == cli.Stripes(cli.stripes_path(prefix), ref, 5000, ["pearson"], False, 5000, CHROMS)
    assert cli.preflight(a, cfg) == pre
    assert os.listdir(os.path.dirname(prefix)) == []  # the directory is made and nothing in it


def test_the_limits_of_the_front_end_are_the_library_s():
    assert cli.MAX_INSULATION_WINDOWS is pixels.MAX_WINDOWS and cli.MAX_INSULATION_WINDOW_BINS is pixels.MAX_WINDOW
    assert cli.MAX_DOT_WINDOW_BINS is pixels.MAX_DOT_WINDOW and cli.MAX_PILEUP_FLANK_BINS is pixels.MAX_PILEUP_FLANK
    assert cli.DOT_FOLDS is pixels.DOT_FOLDS and cli.COMPARE_METRICS is pixels.STRIPE_METRICS


# ---- the ends of a bin --------------------------------------------------------------------------------------

def inlined_span(start, end, base, k, c):
    """the form insulation_lines, dots_lines and stripes_lines each spelled out"""
    p = (start // base) % k
    return start + max(0, c * k - p) * base, min(end, start + ((c + 1) * k - p) * base)


@pytest.mark.parametrize("start,base,factor", [(0, 5000, 1), (15_000, 5000, 2), (20_000, 5000, 3)])
def test_bin_span_is_the_inlined_form(start, base, factor):
    end = start + 13 * base + 3000  # not on a bin boundary
    iv = {"name": "chrA", "start": start, "end": end}
    n_bins = (end - 1) // (base * factor) - start // (base * factor) + 1
    spans = [driver.bin_span(iv, base, factor, c) for c in range(n_bins)]
    assert spans == [inlined_span(start, end, base, factor, c) for c in range(n_bins)]
    # the bins tile the interval: the first starts with it, the last ends with it, none is empty or longer than a bin
    assert spans[0][0] == start and spans[-1][1] == end
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:])) and all(0 < hi - lo <= base * factor for lo, hi in spans)
    assert all(lo % (base * factor) == 0 for lo, _ in spans[1:])  # coarse bins are anchored at the chromosome's start


def test_bin_span_on_the_cases_the_lines_tests_pin():
    span = driver.bin_span
    iv = {"name": "chrA", "start": 10_000, "end": 23_000}  # insulation_lines
    assert [span(iv, 5000, 1, c) for c in range(3)] == [(10_000, 15_000), (15_000, 20_000), (20_000, 23_000)]
    iv = {"name": "chrA", "start": 15_000, "end": 28_000}
    assert [span(iv, 5000, 2, c) for c in range(2)] == [(15_000, 20_000), (20_000, 28_000)]
    iv = {"name": "chrA", "start": 10_000, "end": 123_000}  # dots_lines
    assert [span(iv, 5000, 1, c) for c in (2, 3, 10, 22)] == [(20_000, 25_000), (25_000, 30_000), (60_000, 65_000),
                                                             (120_000, 123_000)]
    iv = {"name": "chrA", "start": 15_000, "end": 128_000}
    assert [span(iv, 5000, 2, c) for c in (0, 1)] == [(15_000, 20_000), (20_000, 30_000)]
    iv = {"name": "chrA", "start": 25_000, "end": 52_000}  # stripes_lines
    assert [span(iv, 10_000, 1, c) for c in range(3)] == [(25_000, 35_000), (35_000, 45_000), (45_000, 52_000)]
    assert [span(iv, 5000, 2, c) for c in range(3)] == [(25_000, 30_000), (30_000, 40_000), (40_000, 50_000)]


# ---- the file stage -----------------------------------------------------------------------------------------

NROWS, NCOLS, IID = 4, 6, 7


class FakeSim:
    """what write_outputs asks of a simulator for a cooler, the marginals and an insulation track: one band,
    held in numpy, under the interval id IID"""
    device = 0

    def __init__(self, band, occupancy):
        self.band, self.occupancy, self.calls = band, occupancy, []

    def copy_outputs(self, interval_id, want_contacts=True):
        assert interval_id == IID and not want_contacts
        self.calls.append("copy_outputs")
        return None, 0, self.occupancy

    def outputs(self, interval_id):
        assert interval_id == IID
        return 0x1000, None, NROWS, NCOLS

    def pixels(self, interval_id, bin_offset=0, stream=None, factor=1, first_bin=0):
        assert (interval_id, factor, first_bin) == (IID, 1, 0)
        self.calls.append("pixels")
        b1, b2, cn, index = reference_pixels(self.band, NROWS, NCOLS, bin_offset)
        return pixels.Pixels(b1, b2, cn, index, pixels.Stats(len(cn), int(cn.sum()), int(cn.max())))

    def marginals(self, interval_id, min_diag=0, factor=1, first_bin=0):
        assert (interval_id, factor, first_bin) == (IID, 1, 0)
        self.calls.append("marginals")
        return reference_marginals(self.band, NROWS, NCOLS, min_diag)

    def insulation(self, interval_id, windows, min_diag=2, factor=1, first_bin=0):
        assert (interval_id, factor, first_bin) == (IID, 1, 0)
        self.calls.append("insulation")
        n_valid = np.array([brute_n_valid(NCOLS, w, min_diag) for w in windows], dtype=np.uint64)
        return prefix_insulation(self.band, NROWS, NCOLS, windows, min_diag), n_valid


def planned(d, rank=0):
    """a plan with the cooler, the expected, the coverage and the insulation file in the directory `d`"""
    p = str(d / "p")
    return cli.Preflight(None, cli.Outputs(p + ".cool", None, None, None, cli.expected_path(p), cli.coverage_path(p)),
                         rank, 1, 0, cli.Insulation(cli.insulation_path(p), 5000, [10_000, 5000], 1), coverage_min_diag=1)


def test_the_file_stage_writes_rank_0_s_files_in_their_order(tmp_path):
    cfg = api.make_config(bin_size=5000)
    chroms = [("chrA", 28_000), ("chrB", 28_000)]
    plan = [entry("chrA", 0, 28_000, NROWS, NCOLS), entry("chrB", 0, 28_000, NROWS, NCOLS)]
    ids = [IID, None]  # chrB has no matrix
    band = make_band(NROWS, NCOLS, "full", limit=1000, seed=5)
    occupancy = np.arange(NCOLS, dtype=np.uint64)
    sim, said = FakeSim(band, occupancy), []
    (tmp_path / "zero").mkdir()
    pre = planned(tmp_path / "zero")
    got = driver.write_outputs(sim, cfg, plan, ids, None, pre, (), said.append, chroms=chroms)
    assert len(got) == 2 and got[0] is occupancy and got[1] is None
    assert said == [f"written {pre.outputs.cooler}", f"written {pre.outputs.expected}", f"written {pre.outputs.coverage}",
                    f"written {pre.insulation.path}"]
    assert sim.calls == ["copy_outputs", "pixels", "marginals", "insulation"]  # the two files share the marginals
    assert sorted(os.listdir(tmp_path / "zero")) == ["p.cool", "p_coverage.bedgraph", "p_expected.tsv", "p_insulation.tsv"]
    # the cooler holds the band's pixels, through the library's writer
    b1, b2, cn, _ = reference_pixels(band, NROWS, NCOLS)
    with cooler.CoolerReader(pre.outputs.cooler) as reader:
        assert reader.chroms == chroms and reader.bin_size == 5000
        for name, want in (("chrA", (b1, b2, cn)), ("chrB", (b1[:0], b2[:0], cn[:0]))):
            px = reader.pixels(name)
            assert all(np.array_equal(x, y) for x, y in zip(px[:3], want)), name
    # the texts are what the writers make of the same callbacks
    marginals = functools.partial(driver._interval_marginals, sim, plan, ids, {0: int(cn.sum())}, 1, {})
    insulation = functools.partial(driver._interval_insulation, sim, plan, ids, [2, 1], 1, marginals)
    alone = {w: str(tmp_path / w) for w in ("expected", "coverage", "insulation")}
    driver.write_expected(alone["expected"], plan, 5000, None, marginals)
    driver.write_coverage(alone["coverage"], plan, 5000, marginals)
    driver.write_insulation(alone["insulation"], plan, 5000, 5000, [10_000, 5000], insulation)
    for w, path in (("expected", pre.outputs.expected), ("coverage", pre.outputs.coverage),
                    ("insulation", pre.insulation.path)):
        text = open(path, "rb").read()
        assert text == open(alone[w], "rb").read() and text.count(b"\n") >= NROWS and b"chrB" not in text, w
    assert open(pre.outputs.coverage).readlines()[-1].startswith("chrA\t25000\t28000\t")
    # another rank collects and writes nothing
    (tmp_path / "one").mkdir()
    sim, said = FakeSim(band, occupancy), []
    got = driver.write_outputs(sim, cfg, plan, ids, None, planned(tmp_path / "one", rank=1), (), said.append, chroms=chroms)
    assert len(got) == 2 and got[0] is occupancy and got[1] is None
    assert said == [] and sim.calls == ["copy_outputs"] and os.listdir(tmp_path / "one") == []
