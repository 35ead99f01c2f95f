"""Random sampling of a band (include/modle_pixels.h: modle_pixels_sample*; modle_amd/pixels.py; the
--subsample-* options of simulate), as far as it goes without a GPU.  `reference_sample` restates the
definition in numpy, vectorised over (pixel, Philox block), and shares no code with the library: it is held
against Random123's known answers, and pixels.sample_pixels -- the host statement compiled from the kernel's
own Philox function -- against it, word for word.  The properties that follow from the definition (nesting,
kept <= n, a binomial total) are tested on the restatement's side of that equality.  Then the front end:
what the parser and preflight refuse, the names of the files, the threshold of --subsample-to and the
check that runs before a sampled file is closed.  Nothing here has a tolerance but the binomial total,
whose bound is six standard deviations of the definition's own distribution."""
import json
import os

import numpy as np
import pytest

from modle_amd import pixels

HERE = os.path.dirname(os.path.abspath(__file__))
M32 = np.uint64(0xFFFFFFFF)
TWO32 = 1 << 32
T1 = pixels.SAMPLE_TIER1_TRIALS
THRESHOLDS = [0, 1, 2**31, 2**32 - 1, 2**32, pixels.sample_threshold(0.1)]
SEEDS = [7, 0x9E3779B97F4A7C15]  # the second is above 2^32: both key words count
SALTS = [0, 0xDEADBEEF]


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on numpy uint64 arrays that hold 32-bit words"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2  # 32 x 32 bits: no wrap in 64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def reference_sample(i, j, n, threshold, seed, salt=0):
    """kept of the pixels (i, j) with n trials, numpy uint32: trial t is kept when word t & 3 of
    philox4x32_10((i, j, t >> 2, salt), (seed & 0xFFFFFFFF, seed >> 32)) is below `threshold`"""
    i, j, n = (np.asarray(a, dtype=np.uint64).reshape(-1) for a in (i, j, n))
    blocks = (n + np.uint64(3)) // np.uint64(4)
    first = np.concatenate([[0], np.cumsum(blocks)]).astype(np.int64)
    pix = np.repeat(np.arange(len(n)), blocks.astype(np.int64))  # one row per (pixel, block)
    blk = (np.arange(first[-1]) - first[pix]).astype(np.uint64)
    words = philox4x32_10(i[pix], j[pix], blk, np.full(len(pix), int(salt), dtype=np.uint64), int(seed) & 0xFFFFFFFF,
                          int(seed) >> 32)
    hit = np.zeros(len(pix), dtype=np.int64)
    for k, w in enumerate(words):
        hit += (w < np.uint64(int(threshold))) & (np.uint64(4) * blk + np.uint64(k) < n[pix])
    kept = np.zeros(len(n), dtype=np.int64)
    np.add.at(kept, pix, hit)
    return kept.astype(np.uint32)


def test_the_restatement_reproduces_random123s_known_answers():
    with open(os.path.join(HERE, "golden", "random123_philox_kats.json")) as fh:
        vectors = json.load(fh)["vectors"]
    assert len(vectors) == 3
    for v in vectors:
        c, k = [int(x, 16) for x in v["counter"]], [int(x, 16) for x in v["key"]]
        got = philox4x32_10(*[np.array([x]) for x in c], *k)
        assert [f"{int(w[0]):08x}" for w in got] == v["expected"]


def edge_pixels():
    """(i, j, n): random pixels with the small counts, the counts around the tier boundary and around a
    wave's stride of 256 trials, one giant, and the ids at both ends of their range"""
    rng = np.random.default_rng(11)
    counts = [0, 1, 3, 4, 5, T1 - 1, T1, T1 + 1, 255, 256, 257, 2**20 + 3]
    n = np.array(counts * 3, dtype=np.uint64)
    i = rng.integers(0, 2**32, size=len(n), dtype=np.uint64)
    j = rng.integers(0, 2**32, size=len(n), dtype=np.uint64)
    i, j = np.minimum(i, j), np.maximum(i, j)
    k = len(counts)
    i[k:2 * k], j[k:2 * k] = 0, 0
    i[2 * k:], j[2 * k:] = 2**32 - 1, 2**32 - 1
    i[0], j[0] = 0, 2**32 - 1
    return i, j, n


@pytest.fixture(scope="module")
def edges():
    return edge_pixels()


@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_the_host_statement_equals_the_restatement(edges, threshold):
    i, j, n = edges
    for seed in SEEDS:
        for salt in SALTS:
            want = reference_sample(i, j, n, threshold, seed, salt)
            got = pixels.sample_pixels(i.astype(np.int64), j.astype(np.int64), n, threshold, seed, salt)
            assert got.dtype == np.uint32 and np.array_equal(got, want), (threshold, seed, salt)
    if threshold == 2**32:
        assert np.array_equal(want, n.astype(np.uint32))
    if threshold == 0:
        assert not want.any()


def test_seed_salt_and_both_key_words_change_the_draw(edges):
    i, j, n = edges
    base = reference_sample(i, j, n, 2**31, 7, 0)
    for seed, salt in ((8, 0), (7 + 2**32, 0), (7, 1)):
        assert not np.array_equal(reference_sample(i, j, n, 2**31, seed, salt), base)


def test_the_offset_shifts_the_ids():
    i, j, n = np.array([3, 2**32 - 50]), np.array([9, 2**32 - 40]), np.array([77, 1000])
    want = reference_sample(i + 39, j + 39, n, 2**30, 5, 2)
    assert np.array_equal(pixels.sample_pixels(i, j, n, 2**30, 5, 2, bin_offset=39), want)
    assert np.array_equal(pixels.sample_pixels(i + 39, j + 39, n, 2**30, 5, 2), want)
    assert np.array_equal(pixels.sample_pixels(i + 100, j + 100, n, 2**30, 5, 2, bin_offset=-61), want)


def test_the_host_statement_refuses():
    one = np.array([1])
    for args, code in [((one, one, one, 2**32 + 1, 0), pixels.ERR_ARG),
                       ((one, one, one, -1, 0), pixels.ERR_ARG),
                       ((one, one, one, 5, 2**64), pixels.ERR_ARG),
                       ((one, one, one, 5, 0, 2**32), pixels.ERR_ARG),
                       ((one, one, np.array([1, 2]), 5, 0), pixels.ERR_ARG),
                       ((one, np.array([1, 2]), one, 5, 0), pixels.ERR_ARG),
                       ((one, one, np.array([-1]), 5, 0), pixels.ERR_RANGE),
                       ((one, one, np.array([2**32]), 5, 0), pixels.ERR_RANGE),
                       ((np.array([2**32]), np.array([2**32]), one, 5, 0), pixels.ERR_RANGE),
                       ((np.array([-1]), one, one, 5, 0), pixels.ERR_RANGE),
                       ((one, np.array([2**63 - 1]), one, 5, 0, 0, 2**63 - 1), pixels.ERR_RANGE)]:
        with pytest.raises(pixels.PixelsError) as e:
            pixels.sample_pixels(*args)
        assert e.value.code == code, args
    assert len(pixels.sample_pixels([], [], [], 5, 0)) == 0


def test_sample_threshold_at_its_edges_and_its_refusals():
    assert pixels.sample_threshold(0) == 0 and pixels.sample_threshold(1) == 2**32
    assert pixels.sample_threshold(0.5) == 2**31 and pixels.sample_threshold(2.0**-32) == 1
    assert pixels.sample_threshold(2.0**-33) == 0
    assert pixels.sample_threshold(np.nextafter(1.0, 0.0)) == 2**32 - 1
    assert pixels.sample_threshold(0.1) == 429496729  # floor(0.1 * 2^32), 0.1 the double
    assert isinstance(pixels.sample_threshold(np.float32(0.25)), int)
    for bad in (-1e-300, np.nextafter(1.0, 2.0), float("nan"), float("inf"), -float("inf"), 1.5):
        with pytest.raises(ValueError):
            pixels.sample_threshold(bad)


def test_a_series_of_depths_is_nested_and_never_above_the_count(edges):
    i, j, n = edges
    before = np.zeros(len(n), dtype=np.uint32)
    for threshold in sorted(THRESHOLDS):
        kept = reference_sample(i, j, n, threshold, SEEDS[1], SALTS[1])
        assert (kept >= before).all() and (kept <= n).all()
        before = kept
    assert np.array_equal(before, n.astype(np.uint32))


def test_the_kept_total_is_binomial():
    """about 10^6 trials over 20 000 pixels: the total lies within six standard deviations,
    sqrt(N p (1 - p)), of N p -- a property of the definition"""
    rng = np.random.default_rng(3)
    j = rng.integers(0, 2**20, size=20_000)
    i = j - rng.integers(0, 600, size=20_000).clip(max=j)
    n = rng.integers(0, 101, size=20_000)
    total = int(n.sum())
    assert 900_000 < total < 1_100_000
    for frac in (0.1, 0.5):
        threshold = pixels.sample_threshold(frac)
        p = threshold / 2**32
        kept = pixels.sample_pixels(i, j, n, threshold, 2026)
        assert np.array_equal(kept, reference_sample(i, j, n, threshold, 2026))
        assert abs(int(kept.sum()) - total * p) <= 6 * (total * p * (1 - p)) ** 0.5


# ---- the options, preflight and the output stage ----------------------------------------------------

@pytest.fixture
def prefix(tmp_path, monkeypatch):
    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(name, raising=False)
    return str(tmp_path / "out" / "p")


def parse(prefix, *extra):
    from modle_amd import cli

    a = cli.build_parser().parse_args(["simulate", "-c", "g.chrom.sizes", "-b", "b.bed", "-o", prefix, "-r", "5kb",
                                       "--no-track-1d-lef-position", *extra])
    return a, cli.config_from_args(a)


def test_the_options_parse_and_the_files_are_planned(prefix):
    from modle_amd import cli

    a, cfg = parse(prefix)
    before = cli.preflight(a, cfg)
    assert before.subsample is None
    a, cfg = parse(prefix, "--subsample-frac", "0.25", "--seed", "77")
    assert cli.preflight(a, cfg)._replace(subsample=None) == before  # that field changes and nothing else
    assert cli.preflight(a, cfg).subsample == cli.Subsample(prefix + "_sampled.cool", prefix + "_sampled_rest.cool", 0.25,
                                                            None, 77, False)
    a, cfg = parse(prefix, "--subsample-to", "1000000", "--subsample-seed", str(2**64 - 1), "--subsample-split",
                   "--mcool-resolutions", "10kb,50kb")
    assert cli.preflight(a, cfg).subsample == cli.Subsample(prefix + "_sampled.mcool", prefix + "_sampled_rest.mcool", None,
                                                            1_000_000, 2**64 - 1, True)
    assert cli.sampled_paths("x/y") == ("x/y_sampled.cool", "x/y_sampled_rest.cool")
    assert cli.sampled_paths("x/y", mcool=True) == ("x/y_sampled.mcool", "x/y_sampled_rest.mcool")
    assert cli.preflight(*parse(prefix, "--subsample-frac", "1")).subsample.frac == 1.0
    assert cli.preflight(*parse(prefix, "--subsample-to", "0")).subsample.target == 0


SUBSAMPLE_REFUSED = [
    (["--subsample-seed", "3"], "--subsample-seed needs --subsample-frac or --subsample-to"),
    (["--subsample-split"], "--subsample-split needs --subsample-frac or --subsample-to"),
    (["--subsample-frac", "0"], "--subsample-frac: 0.0 is not in (0, 1]"),
    (["--subsample-frac", "-0.5"], "--subsample-frac: -0.5 is not in (0, 1]"),
    (["--subsample-frac", "1.0000001"], "--subsample-frac: 1.0000001 is not in (0, 1]"),
    (["--subsample-frac", "nan"], "--subsample-frac: nan is not in (0, 1]"),
    (["--subsample-frac", "inf"], "--subsample-frac: inf is not in (0, 1]"),
    (["--subsample-to", "-1"], "--subsample-to: -1 is negative"),
    (["--subsample-frac", "0.5", "--subsample-seed", "-1"], "--subsample-seed: -1 is no unsigned 64-bit number"),
    (["--subsample-frac", "0.5", "--subsample-seed", str(2**64)], "--subsample-seed: 18446744073709551616 is no"),
    (["--subsample-frac", "0.5", "--skip-output"], "--subsample-frac needs the cooler: it excludes --skip-output"),
    (["--subsample-to", "5", "--skip-output"], "--subsample-to needs the cooler: it excludes --skip-output"),
]


@pytest.mark.parametrize("options,message", SUBSAMPLE_REFUSED)
def test_preflight_refuses_before_anything_is_made(prefix, options, message):
    from modle_amd import cli

    with pytest.raises(SystemExit) as e:
        cli.preflight(*parse(prefix, *options))
    assert str(e.value).startswith(message)
    assert not os.path.exists(os.path.dirname(prefix))


def test_the_parser_refuses_two_depths_and_a_missing_target(prefix, capsys):
    for options in (["--subsample-frac", "0.5", "--subsample-to", "10"], ["--subsample-to"], ["--subsample-frac"],
                    ["--subsample-to", "many"], ["--subsample-to", "1.5"]):
        with pytest.raises(SystemExit) as e:
            parse(prefix, *options)
        assert e.value.code == 2
    assert "not allowed with argument" in capsys.readouterr().err


def test_the_sampled_files_are_not_overwritten_without_force(prefix):
    from modle_amd import cli

    os.makedirs(os.path.dirname(prefix))
    with open(prefix + "_sampled_rest.cool", "wb") as fh:
        fh.write(b"precious")
    cli.preflight(*parse(prefix, "--subsample-frac", "0.5"))  # the second file is not planned
    with pytest.raises(SystemExit) as e:
        cli.preflight(*parse(prefix, "--subsample-frac", "0.5", "--subsample-split"))
    assert str(e.value) == f"refusing to overwrite {prefix}_sampled_rest.cool: pass --force to overwrite"
    with open(prefix + "_sampled.cool", "wb") as fh:
        fh.write(b"precious")
    with pytest.raises(SystemExit) as e:
        cli.preflight(*parse(prefix, "--subsample-to", "5", "--subsample-split"))
    assert str(e.value) == f"refusing to overwrite {prefix}_sampled.cool: pass --force to overwrite"
    cli.preflight(*parse(prefix, "--subsample-to", "5", "--subsample-split", "--force"))
    cli.preflight(*parse(prefix))  # without the options: nobody's business
    assert open(prefix + "_sampled.cool", "rb").read() == b"precious"


def test_the_threshold_of_a_target():
    from modle_amd import driver

    assert driver.subsample_threshold(0, 10) == 0
    assert driver.subsample_threshold(5, 10) == 2**31
    assert driver.subsample_threshold(1, 3) == (2**32) // 3
    assert driver.subsample_threshold(9, 10) == (9 * 2**32) // 10
    assert driver.subsample_threshold(10, 10) == 2**32 and driver.subsample_threshold(11, 10) == 2**32
    assert driver.subsample_threshold(0, 0) == 2**32  # an empty job: nothing to draw
    big = 2**62 + 12345  # no double holds it
    assert driver.subsample_threshold(big - 1, big) == ((big - 1) << 32) // big == 2**32 - 1
    assert driver.subsample_threshold(1, big) == 0
    with pytest.raises(ValueError):
        driver.subsample_threshold(-1, 10)


def sampled_pixels(threshold, seed):
    """(stats, kept, rest) of a made-up interval whose pixels carry global ids, as the output stage sees them"""
    rng = np.random.default_rng(8)
    ids = np.unique(rng.integers(0, 300 * 40, size=5000))
    b1 = 4_000_000_000 + ids // 40
    b2, n = b1 + ids % 40, rng.integers(1, 60, size=len(ids))
    kept = reference_sample(b1, b2, n, threshold, seed).astype(np.int64)

    def px(count):
        on = count != 0
        return pixels.Pixels(b1[on], b2[on], count[on].astype(np.int32), None,
                             pixels.Stats(int(on.sum()), int(count.sum()), int(count.max(initial=0))))

    return pixels.Stats(len(n), int(n.sum()), int(n.max())), px(kept), px(n - kept)


def test_the_check_accepts_the_definition_and_names_a_tampered_pixel():
    from modle_amd import driver

    threshold, seed = pixels.sample_threshold(0.4), 2**33 + 1
    stats, kept, rest = sampled_pixels(threshold, seed)
    assert len(kept.count) > driver.SAMPLE_CHECKED_PIXELS / 2 and len(rest.count) < stats.nnz
    driver.check_sample("chrA:0-1", stats, kept, rest, threshold, seed)
    driver.check_sample("chrA:0-1", pixels.Stats(0, 0, 0), kept._replace(bin1=kept.bin1[:0], bin2=kept.bin2[:0],
                                                                         count=kept.count[:0]),
                        kept._replace(bin1=kept.bin1[:0], bin2=kept.bin2[:0], count=kept.count[:0]), threshold, seed)
    with pytest.raises(RuntimeError, match="chrA:0-1: the sampled halves hold"):
        driver.check_sample("chrA:0-1", stats._replace(sum=stats.sum + 1), kept, rest, threshold, seed)
    with pytest.raises(RuntimeError, match="kept pixels, the interval has"):
        driver.check_sample("chrA:0-1", stats._replace(nnz=len(kept.count) - 1), kept, rest, threshold, seed)
    with pytest.raises(RuntimeError, match="by the definition"):
        driver.check_sample("chrA:0-1", stats, kept, rest, threshold, seed + 1)  # another draw
    with pytest.raises(RuntimeError, match="by the definition"):
        driver.check_sample("chrA:0-1", stats, kept, rest, threshold + 2**28, seed)
    # one contact moved from the first kept pixel to the first other pixel: the sums still agree
    moved_k, moved_r = kept.count.copy(), rest.count.copy()
    moved_k[0] -= 1
    moved_r[0] += 1
    assert moved_k[0] > 0
    with pytest.raises(RuntimeError, match=rf"chrA:0-1: pixel \({kept.bin1[0]}, {kept.bin2[0]}\)"):
        driver.check_sample("chrA:0-1", stats, kept._replace(count=moved_k), rest._replace(count=moved_r), threshold, seed)
