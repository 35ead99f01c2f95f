"""Dense regions, the parts that need no GPU: the REGION strings of `simulate --dense-region`, their
mapping to (plan entry, columns of its band, name of the array) by driver.dense_regions on a plan
built from text inputs, the host-only modle_pixels_tiles_fit, and the parser."""
import argparse

import pytest

from modle_amd import api, cli, driver, genome, pixels

BIN = 5000
# chrA's size is no multiple of the bin: its last bin, 240, is 2.5 kb long.  The interval of chrA
# starts at fine bin 5; chrC has an interval but no barrier, so it is skipped; chrD has no interval.
SIZES = "chrA\t1202500\nchrB\t400000\nchrC\t300000\nchrD\t100000\n"
INTERVALS = "chrA\t25000\t1202500\nchrB\t0\t400000\nchrC\t0\t300000\n"
BARRIERS = "chrA\t100000\t100019\t.\t0.9\t+\nchrA\t700000\t700019\t.\t0.9\t-\nchrB\t200000\t200019\t.\t0.8\t+\n"


@pytest.fixture(scope="module")
def planned():
    cfg = api.make_config(bin_size=BIN, num_cells=2)
    chroms, ivs, _ = genome.import_genome_text(cfg, SIZES, BARRIERS, INTERVALS)
    plan = driver.plan_genome(cfg, ivs)
    assert [(e["interval"]["name"], e["interval"]["start"], e["ncols"], e["skipped"]) for e in plan] == \
        [("chrA", 25000, 236, False), ("chrB", 0, 80, False), ("chrC", 0, 60, True)]
    return plan, chroms


def test_region_strings_parse():
    assert cli.dense_region("chrA") == ("chrA", None, None)
    assert cli.dense_region("chrA:25000-1025000") == ("chrA", 25000, 1025000)
    assert cli.dense_region("chrA:25kb-1.025mb") == ("chrA", 25000, 1025000)
    assert cli.dense_region("chrA:1,000-2,000") == ("chrA", 1000, 2000)


@pytest.mark.parametrize("text", ["", "chrA:", ":1-2", "chrA:100", "chrA:100-", "chrA:-100", "chrA:1-2-3",
                                  "chrA:a-b", "chrA:1.5-2", "chrA:10-20parsecs"])
def test_malformed_region_strings_are_rejected(text):
    with pytest.raises(argparse.ArgumentTypeError):
        cli.dense_region(text)


def test_regions_map_to_the_entry_the_columns_and_the_key(planned):
    plan, chroms = planned
    # inside the interval that starts at fine bin 5: columns are relative to the interval's band
    assert driver.dense_regions(plan, BIN, chroms, [("chrA", 100000, 600000)]) == \
        [(0, 15, 115, "chrA:100000-600000")]
    # snapped outward: 101 000 lies in bin 20, 599 000 in bin 119
    assert driver.dense_regions(plan, BIN, chroms, [("chrA", 101000, 599000)]) == \
        [(0, 15, 115, "chrA:100000-600000")]
    assert driver.dense_regions(plan, BIN, chroms, [("chrA", 25000, 25001)]) == [(0, 0, 1, "chrA:25000-30000")]
    # the key is clipped at the chromosome's end: bin 240 ends at 1 205 000, chrA at 1 202 500
    assert driver.dense_regions(plan, BIN, chroms, [("chrA", 1200000, 1202500)]) == \
        [(0, 235, 236, "chrA:1200000-1202500")]
    # a whole chromosome, and several regions in the order given
    assert driver.dense_regions(plan, BIN, chroms, [("chrB", None, None), ("chrA", 100000, 600000)]) == \
        [(1, 0, 80, "chrB:0-400000"), (0, 15, 115, "chrA:100000-600000")]
    assert driver.dense_regions(plan, BIN, chroms, []) == []


@pytest.mark.parametrize("what,regions", [
    ("unknown chromosome", [("chrZ", 0, 5000)]),
    ("start == end", [("chrA", 100000, 100000)]),
    ("start > end", [("chrA", 200000, 100000)]),
    ("beyond the chromosome", [("chrB", 300000, 400001)]),
    ("before the interval of -g", [("chrA", 0, 100000)]),
    ("one bin before the interval of -g", [("chrA", 24999, 100000)]),
    ("whole chromosome, of which -g has a part", [("chrA", None, None)]),
    ("an interval skipped for having no barriers", [("chrC", 0, 100000)]),
    ("a chromosome without an interval", [("chrD", None, None)]),
    ("a duplicate", [("chrA", 100000, 600000), ("chrB", None, None), ("chrA", 100000, 600000)]),
    ("a duplicate after snapping", [("chrA", 100000, 600000), ("chrA", 101000, 599000)]),
])
def test_bad_regions_end_the_run(planned, what, regions):
    plan, chroms = planned
    with pytest.raises(SystemExit) as e:
        driver.dense_regions(plan, BIN, chroms, regions)
    assert "--dense-region" in str(e.value), what


def test_a_region_across_two_intervals_is_refused():
    cfg = api.make_config(bin_size=BIN, num_cells=2)
    chroms, ivs, _ = genome.import_genome_text(cfg, SIZES, BARRIERS, "chrA\t0\t500000\nchrA\t500000\t1000000\n")
    plan = driver.plan_genome(cfg, ivs)
    assert driver.dense_regions(plan, BIN, chroms, [("chrA", 500000, 600000)]) == [(1, 0, 20, "chrA:500000-600000")]
    with pytest.raises(SystemExit):
        driver.dense_regions(plan, BIN, chroms, [("chrA", 495000, 600000)])


def test_tiles_fit():
    assert pixels.tiles_fit(130, 1, 65, 32) == 3
    assert pixels.tiles_fit(7, 2, 3, 1) == 3
    assert pixels.tiles_fit(10, 7, 3, 5) == 1  # first + size == ncols
    assert pixels.tiles_fit(49792, 0, 512, 256) == 193
    for what, args in [("size 0", (7, 2, 0, 1)), ("step 0", (7, 2, 3, 0)), ("first + size > ncols", (7, 5, 3, 1)),
                       ("first + size overflows", (7, 2**64 - 1, 3, 1))]:
        with pytest.raises(pixels.PixelsError) as e:
            pixels.tiles_fit(*args)
        assert e.value.code == pixels.ERR_ARG, what
    for name in ("modle_pixels_tiles_fit", "modle_pixels_dense_tiles", "modle_pixels_dense_to_host"):
        assert name in pixels.EXPORTS and hasattr(pixels.lib(), name)


def test_the_parser_takes_the_option_repeatedly():
    common = ["simulate", "-c", "g.chrom.sizes", "-b", "b.bed", "-o", "out/run"]
    assert cli.build_parser().parse_args(common).dense_region is None
    a = cli.build_parser().parse_args(common + ["--dense-region", "chrB", "--dense-region", "chrA:100kb-600kb"])
    assert a.dense_region == [("chrB", None, None), ("chrA", 100000, 600000)]
    assert cli.dense_path(a.output_prefix) == "out/run_dense.npz"
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(common + ["--dense-region", "chrA:100kb"])
