"""`simulate` under torch.distributed.run: the front end's multi-rank output stage (cli.run_plan's
torch tensors, driver.write_outputs' reduces, rank 0's pixels, coarsening and dense regions from the
reduced tensor) with two ranks that share this GPU and reduce on host copies (--dist-backend gloo),
against the single-rank run of the same arguments.  Cells are independent and the sums are integer
sums, so every file and every warning must be the single-rank run's, byte for byte where the format
allows; nothing here has a tolerance.  Each run is a fresh child process; a pair of runs is made once
per module and several tests read its files."""
import gzip
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from bigwig_reader import BigWig
from test_cooler_pixels import read_cooler
from test_mcool_writer import FILE_LEVEL, read_group

from modle_amd import driver

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCELLS = 5  # two ranks: shards of 3 and 2 cells
# The diagonal width.  The reference's default is 3 Mb; with 200 kb (40 rows of 5 kb bins) the contacts of
# the longer loops fall outside the band.  (matrix sum, missed updates) per chromosome of the whole job,
# from the CPU oracle (oracle.simulate_interval on cli.config_from_args / genome.import_genome /
# driver.plan_genome of these arguments, the way tests/test_sharding_gloo.py::_simulate_shard calls it):
# a missing share, missed / (sum + missed), of 6.25 % and 6.12 % in pair A (5 cells), 9.84 % and 6.33 % in
# pair B (5 cells, no occupancy track: other draws), 9.53 % and 7.29 % in pair C (1 cell), all well above
# the 1 % at which the warning starts.  (Rank 0's shard of A alone: 1784 + 136 and 1359 + 81, so its own
# missed updates against the whole matrix would read 4.34 % and 3.47 %.)
DIAGONAL_WIDTH = "200kb"
ORACLE = {"a": {"chrA": (3000, 200), "chrC": (2253, 147)}, "b": {"chrA": (2885, 315), "chrC": (2248, 152)},
          "c": {"chrA": (2895, 305), "chrC": (2225, 175)}}
COMMON = ["-r", "5kb", "-w", DIAGONAL_WIDTH, "--target-contact-density", "0.2", "--seed", "5"]
RUN_KEYS = ("output_prefix", "dist_backend", "device")  # the metadata's keys that name the run
WARNING = re.compile(r"^warning: \d+\.\d\d% missing interactions for \S+$")
PORT = 35500 + os.getpid() % 2000  # (+ 0, 1, 2: one per two-rank run; no other test's range)


def genome_files(d):
    """chrA (2 Mb, 24 stranded barriers), chrB (500 kb, none: skipped), chrC (1.5 Mb, 17 barriers)"""
    sizes, bed = os.path.join(d, "g.chrom.sizes"), os.path.join(d, "b.bed")
    with open(sizes, "w") as fh:
        fh.write("chrA\t2000000\nchrB\t500000\nchrC\t1500000\n")
    with open(bed, "w") as fh:
        for name, first, step, n in (("chrA", 41_000, 80_000, 24), ("chrC", 63_000, 83_000, 17)):
            for i in range(n):
                p = first + i * step + (i * 37 % 11) * 1000
                fh.write(f"{name}\t{p}\t{p + 19}\t.\t{0.6 + 0.08 * (i % 5):.2f}\t{'+-+--+'[i % 6]}\n")
    return sizes, bed


_failed = []  # once a child has failed nothing more is started on the GPU


def simulate(d, name, world, port, options):
    """one run in a directory of its own: (prefix, the warning lines of its stderr, all of its stderr)"""
    if _failed:
        pytest.fail(f"not started: the run {_failed[0]} failed before")
    os.makedirs(os.path.join(d, "in"), exist_ok=True)
    sizes, bed = genome_files(os.path.join(d, "in"))
    prefix = os.path.join(d, name, "run")
    args = ["-m", "modle_amd", "simulate", "-c", sizes, "-b", bed, "-o", prefix, *COMMON, *options]
    cmd = [sys.executable, *args]
    if world > 1:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
               "--master-addr", "127.0.0.1", "--master-port", str(port), *args,
               "--dist-backend", "gloo", "--device", "0"]
    env = {k: v for k, v in os.environ.items() if k not in ("MODLE_HIP_LIB", "MODLE_PIXELS_LIB")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    try:
        p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _failed.append(name)
        raise
    if p.returncode != 0:
        _failed.append(name)
    assert p.returncode == 0, f"{name}: exit code {p.returncode}\n{p.stderr[-3000:]}"
    return prefix, [l for l in p.stderr.splitlines() if WARNING.match(l)], p.stderr


def pair(d, name, options, port):
    one = simulate(d, name + "_one", 1, 0, options)
    two = simulate(d, name + "_two", 2, port, options)
    return one, two


def oracle_warnings(which):
    return [f"warning: {100.0 * m / (s + m):.2f}% missing interactions for {name}"
            for name, (s, m) in ORACLE[which].items()]


def files_of(prefix):
    d = os.path.dirname(prefix)
    return sorted(os.listdir(d)) if os.path.exists(d) else None


def without_run_keys(metadata):
    return {k: v for k, v in json.loads(metadata).items() if k not in RUN_KEYS}


def comparable(cooler):
    """a reader's output without what may differ: the creation date, and in the metadata the run's keys"""
    out = {k: v for k, v in cooler.items() if k not in FILE_LEVEL}
    out["attrs"] = {k: v for k, v in cooler["attrs"].items() if k != "creation-date"}
    out["attrs"]["metadata"] = without_run_keys(cooler["attrs"]["metadata"])
    return out


def assert_same_tables(a, b):
    a, b = comparable(a), comparable(b)
    assert a.keys() == b.keys()
    for key in a:
        assert a[key] == b[key], key
    return a


def assert_same_npz(path_a, path_b, n_regions):
    with np.load(path_a) as a, np.load(path_b) as b:
        assert sorted(a.files) == sorted(b.files) and len(a.files) == n_regions
        for key in a.files:
            assert a[key].dtype == b[key].dtype == np.int32 and a[key].shape == b[key].shape, key
            assert np.array_equal(a[key], b[key]), key
            assert a[key].sum() > 0, key


def state_log(path):
    with gzip.open(path, "rt") as fh:
        lines = fh.read().splitlines()
    return lines[0], lines[1:]


# ---- A: .cool, bigWig, two dense regions, state logs ----------------------------------------------

@pytest.fixture(scope="module")
def pair_a(tmp_path_factory):
    return pair(str(tmp_path_factory.mktemp("a")), "a",
                ["--ncells", str(NCELLS), "--track-1d-lef-position", "--dense-region", "chrA:500kb-1.2mb",
                 "--dense-region", "chrC", "--log-model-internal-state"], PORT)


def test_a_the_warnings_are_the_single_rank_run_s(pair_a):
    (_, warned, _), (_, warned2, err2) = pair_a
    assert len(warned) >= 1, "the single-rank run did not warn: the diagonal width proves nothing"
    assert warned == oracle_warnings("a")
    assert warned2 == warned, err2[-3000:]


def test_a_the_files_of_each_run_and_nothing_else(pair_a):
    (one, _, _), (two, _, _) = pair_a
    rest = ["run.cool", "run_dense.npz", "run_lef_1d_occupancy.bw"]
    assert files_of(one) == sorted(rest + ["run_internal_state.log.gz"])
    # (rank 1 leaves its state log and nothing else; no un-ranked log)
    assert files_of(two) == sorted(rest + ["run_internal_state.rank0.log.gz", "run_internal_state.rank1.log.gz"])


def test_a_cooler(pair_a):
    (one, _, _), (two, _, _) = pair_a
    got = assert_same_tables(read_cooler(one + ".cool"), read_cooler(two + ".cool"))
    assert got["attrs"]["sum"] == sum(s for s, _ in ORACLE["a"].values()) > got["attrs"]["nnz"] > 0
    assert got["pixels_by_chrom"]["chrA"] and not got["pixels_by_chrom"]["chrB"] and got["pixels_by_chrom"]["chrC"]
    meta = json.loads(read_cooler(two + ".cool")["attrs"]["metadata"])
    assert (meta["output_prefix"], meta["dist_backend"], meta["device"]) == (two, "gloo", 0)


def test_a_bigwig(pair_a):
    (one, _, _), (two, _, _) = pair_a
    a, b = BigWig(one + "_lef_1d_occupancy.bw"), BigWig(two + "_lef_1d_occupancy.bw")
    assert a.chroms == b.chroms == [("chrA", 2_000_000), ("chrB", 500_000), ("chrC", 1_500_000)]
    assert a.summary == b.summary and a.summary["sum"] > 0
    assert a.sections() == b.sections() and len(a.sections()) >= 2


def test_a_dense_regions(pair_a):
    (one, _, _), (two, _, _) = pair_a
    assert_same_npz(one + "_dense.npz", two + "_dense.npz", 2)
    with np.load(two + "_dense.npz") as z:
        assert sorted(z.files) == ["chrA:500000-1200000", "chrC:0-1500000"]
        assert z["chrA:500000-1200000"].shape == (140, 140) and z["chrC:0-1500000"].shape == (300, 300)


def test_a_state_logs(pair_a):
    (one, _, _), (two, _, _) = pair_a
    header, single = state_log(one + "_internal_state.log.gz")
    assert header == driver.STATE_LOG_HEADER.rstrip("\n")
    assert {l.split("\t")[2] for l in single} == {str(c) for c in range(NCELLS)}
    both = []
    for r in range(2):
        h, lines = state_log(f"{two}_internal_state.rank{r}.log.gz")
        assert h == header
        assert {l.split("\t")[2] for l in lines} == {str(c) for c in range(*driver.shard_bounds(NCELLS, r, 2))}
        assert {l.split("\t")[3] for l in lines} == {"chrA", "chrC"}
        both += lines
    assert sorted(both) == sorted(single) and len(set(single)) == len(single)


# ---- B: .mcool, one dense region, no bigWig -------------------------------------------------------

@pytest.fixture(scope="module")
def pair_b(tmp_path_factory):
    return pair(str(tmp_path_factory.mktemp("b")), "b",
                ["--ncells", str(NCELLS), "--no-track-1d-lef-position", "--mcool-resolutions", "10kb,25kb",
                 "--dense-region", "chrC:200kb-900kb"], PORT + 1)


def test_b_every_resolution_and_the_root(pair_b):
    (one, warned, _), (two, warned2, err2) = pair_b
    assert files_of(one) == files_of(two) == ["run.mcool", "run_dense.npz"]
    assert warned == oracle_warnings("b") and warned2 == warned, err2[-3000:]
    sums = []
    for b in (5000, 10000, 25000):
        a, c = read_group(one + ".mcool", f"/resolutions/{b}"), read_group(two + ".mcool", f"/resolutions/{b}")
        got = assert_same_tables(a, c)
        assert got["attrs"]["bin-size"] == b and got["n_pixels"] > 100
        sums.append(got["attrs"]["sum"])
        for key in FILE_LEVEL:
            assert a[key] == c[key], key
        assert a["resolutions"] == ["5000", "10000", "25000"]
    assert sums[0] == sums[1] == sums[2] == sum(s for s, _ in ORACLE["b"].values())


def test_b_dense_region(pair_b):
    (one, _, _), (two, _, _) = pair_b
    assert_same_npz(one + "_dense.npz", two + "_dense.npz", 1)


# ---- C: --skip-output with one cell: rank 1's shard is empty for every interval -------------------

@pytest.fixture(scope="module")
def pair_c(tmp_path_factory):
    return pair(str(tmp_path_factory.mktemp("c")), "c", ["--ncells", "1", "--skip-output"], PORT + 2)


def test_c_an_empty_shard_and_no_output(pair_c):
    (one, warned, err1), (two, warned2, err2) = pair_c
    assert files_of(one) is None and files_of(two) is None  # not even the directory
    assert len(warned) >= 1, "the single-rank run did not warn: the diagonal width proves nothing"
    assert warned == oracle_warnings("c")
    assert warned2 == warned, err2[-3000:]
    assert "simulating 2 (interval, cell) tasks on device 0 (rank 0 of 1)" in err1
    assert "simulating 2 (interval, cell) tasks on device 0 (rank 0 of 2)" in err2
    assert "simulating 0 (interval, cell) tasks on device 0 (rank 1 of 2)" in err2
