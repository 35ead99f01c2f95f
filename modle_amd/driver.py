"""Host driver standing in for `Simulation::run_simulate` (reference:
src/libmodle/cpu/scheduler_simulate.cpp:43-170) on top of the C ABI.

For every interval in genome order it derives the per-cell tasks exactly like the reference
(seed hash, one PRNG jump per cell, target-contact split), keeps the cells of this rank's shard,
registers the interval with the simulator and enqueues the tasks.  One launch then processes the
tasks of all intervals together (the reference's workers also drain one queue that mixes
intervals).  Cells are independent, so sharding them over ranks needs no data-path collective;
the per-rank contact matrices are summed afterwards (`reduce_outputs`).

`write_outputs` is the front end's output stage after the launch.
"""
import functools
import inspect
import math

import numpy as np

from . import api


def shard_bounds(num_cells, rank, world):
    """Contiguous cell-id range [lo, hi) owned by `rank` (any partition gives the same result:
    every cell's PRNG state is fixed by its cell id)."""
    base, rem = divmod(num_cells, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def plan_genome(cfg, genome, rank=0, world=1):
    """Task derivation for every interval of `genome` (list of dicts, see synthetic.py).

    Returns a list of {interval, tasks (this rank's shard), nrows, ncols, skipped}."""
    plan = []
    task_id = 0
    for iv in genome:
        size = iv["end"] - iv["start"]
        nrows, ncols = api.matrix_shape(cfg, size)
        entry = {"interval": iv, "nrows": nrows, "ncols": ncols, "tasks": None, "skipped": False}
        if not cfg.simulate_chromosomes_wo_barriers and len(iv["bar_pos"]) == 0:
            # scheduler_simulate.cpp:111-124: intervals without barriers are skipped
            entry["skipped"] = True
            plan.append(entry)
            continue
        tasks = api.make_tasks(cfg, iv["name"], iv["size"], iv["start"], iv["end"], task_id)
        task_id += int(cfg.num_cells)
        lo, hi = shard_bounds(int(cfg.num_cells), rank, world)
        entry["tasks"] = api.slice_tasks(tasks, lo, hi)
        plan.append(entry)
    return plan


def interval_stps(cfg, iv):
    """self-transition probabilities of an interval's barriers: as imported (genome.py), or
    derived from BED-score-like occupancies (synthetic.py)"""
    if "bar_stp_active" in iv:
        return iv["bar_stp_active"], iv["bar_stp_inactive"]
    return api.barrier_stps(cfg, iv["bar_occupancy"])


def enqueue_plan(sim, cfg, plan, device_buffers=None):
    """Registers intervals + tasks of a plan with `sim`.  `device_buffers`: optional list of
    (contacts_ptr, occupancy_ptr) device pointers per plan entry (e.g. torch tensors)."""
    ids = []
    for k, entry in enumerate(plan):
        if entry["skipped"]:
            ids.append(None)
            continue
        iv = entry["interval"]
        stp_active, stp_inactive = interval_stps(cfg, iv)
        dc, do = (None, None) if device_buffers is None else device_buffers[k]
        iid = sim.add_interval(iv["start"], iv["end"], iv["bar_pos"], iv["bar_dir"], stp_active,
                               stp_inactive, dc, do)
        if len(entry["tasks"]) != 0:
            sim.submit(iid, entry["tasks"])
        ids.append(iid)
    return ids


def algorithmic_bytes(results, n_barriers, track_1d=True):
    """ALGORITHMIC HBM bytes of a set of finished cells of one interval:
    per simulated epoch 40 B per active LEF (read+write of rev/fwd position, binding epoch and
    the two ranks), 22 B per barrier (position, two transition probabilities, state read+write)
    and 64 B of PRNG state; per sampling event 8 B (contact read-modify-write) and, with the 1-D
    occupancy track, 16 B."""
    total = 0
    for r in results:
        total += 40 * r.sum_active_lefs + (22 * n_barriers + 64) * r.sim_epochs
        total += (8 + (16 if track_1d else 0)) * r.sampling_events
    return total


def read_missed(sim, ids):
    """missed-update counters of every registered interval (they accumulate over launches)"""
    return [None if iid is None else sim.copy_outputs(iid, want_contacts=False)[1] for iid in ids]


def verify_outputs(sim, cfg, plan, ids, matrix_sums, missed_delta, occupancy_sums=None):
    """Self-check of one launch's outputs (what a caller can assert without an oracle):

    * every registered contact is in the band matrix or was counted as a missed update
      (ContactMatrixDense::add, contact_matrix_dense_safe_impl.hpp:55-68);
    * with a target contact density, every cell stops exactly on its share of the target
      (stop condition, simulation.cpp:925-931; split, scheduler_simulate.cpp:129-141);
    * the 1-D occupancy track holds at most two entries per sampling event, an even number;
    * burn-in: all LEFs activated before it can end, and at least one epoch simulated.

    `matrix_sums[k]` / `occupancy_sums[k]`: sum of the interval's matrix / occupancy words of this
    launch (this rank's shard, before any reduce); `missed_delta[k]`: missed updates of this
    launch.  Uses the results of the LAST launch.  Raises AssertionError; returns a summary."""
    n_tasks = n_contacts = n_missed = 0
    for k, (entry, iid) in enumerate(zip(plan, ids)):
        if iid is None:
            continue
        name = entry["interval"]["name"]
        ntasks = len(entry["tasks"])
        res = sim.results(iid)
        last = res[len(res) - ntasks:]
        contacts = sum(r.num_contacts for r in last)
        assert int(matrix_sums[k]) + int(missed_delta[k]) == contacts, \
            f"{name}: {int(matrix_sums[k])} matrix + {int(missed_delta[k])} missed != {contacts} contacts"
        if cfg.target_contact_density >= 0:
            got = [r.num_contacts for r in last]
            want = [t.num_target_contacts for t in entry["tasks"]]
            assert got == want, f"{name}: per-cell contacts differ from the target split"
        if occupancy_sums is not None and cfg.track_1d_lef_position:
            occ = int(occupancy_sums[k])
            assert occ % 2 == 0 and occ <= 2 * sum(r.sampling_events for r in last), \
                f"{name}: occupancy track inconsistent with the sampling events"
        for r, t in zip(last, entry["tasks"]):
            if t.num_target_contacts != 0 and not cfg.skip_burnin and cfg.target_contact_density >= 0:
                assert r.burnin_epochs >= 1 and r.epochs >= r.sim_epochs >= 1, f"{name}: epoch counters"
        n_tasks += ntasks
        n_contacts += contacts
        n_missed += int(missed_delta[k])
    return {"tasks": n_tasks, "contacts": n_contacts, "missed_updates": n_missed}


def _chroms_of_plan(plan):
    chroms = []
    for entry in plan:
        iv = entry["interval"]
        if not chroms or chroms[-1][0] != iv["name"]:
            chroms.append((iv["name"], int(iv["size"])))
    return chroms


def write_cooler(path, cfg, plan, matrices, assembly="unknown", generated_by="modle-hip",
                 metadata_json="", force_overwrite=False, chroms=None):
    """Writes the (reduced) contact matrices of a plan to a cooler file the way the reference's
    IO thread does (simulation.cpp:117-168, 217-269): every chromosome of the genome is in the
    file, intervals are appended in genome order, skipped intervals and intervals without a
    matrix contribute no pixels.  `matrices[k]`: band matrix of plan entry k (uint32,
    nrows * ncols [+1] words, layout of modle_hip_interval_outputs) or None.
    `chroms`: [(name, size)] of the WHOLE genome (chrom.sizes order).  The reference creates the
    file from genome.chromosomes() (init_cooler_file, simulation.cpp:205-214), so a chromosome that
    --genomic-intervals leaves out still has its bins; without `chroms` only the chromosomes of
    the plan are known."""
    from . import cooler

    if chroms is None:
        chroms = _chroms_of_plan(plan)
    with cooler.CoolerWriter(path, chroms, int(cfg.bin_size), assembly=assembly,
                             generated_by=generated_by, metadata_json=metadata_json,
                             force_overwrite=force_overwrite) as w:
        for entry, m in zip(plan, matrices):
            if entry["skipped"] or m is None:
                continue
            iv = entry["interval"]
            w.append(iv["name"], m, entry["nrows"], entry["ncols"], offset_bp=int(iv["start"]))


def coarse_bin_range(first_bin, ncols, factor):
    """first and last coarse bin, within the chromosome, of the `ncols` fine bins from `first_bin`
    (coarse bins are anchored at the chromosome's start: include/modle_pixels.h)"""
    return first_bin // factor, (first_bin + ncols - 1) // factor


def mcool_collision(plan, base, bin_sizes):
    """The first (resolution, name of interval a, name of interval b) at which two intervals of one
    chromosome that have a matrix touch the same coarse bin -- the pixel table of that resolution
    would not be sorted and unique -- or None.  Names are `chrom:start-end`."""
    for b in bin_sizes:
        last = None  # (chromosome, last coarse bin, name) of the interval before
        for entry in plan:
            iv = entry["interval"]
            if entry["skipped"] or entry["ncols"] == 0:
                continue
            lo, hi = coarse_bin_range(int(iv["start"]) // base, entry["ncols"], b // base)
            name = f"{iv['name']}:{iv['start']}-{iv['end']}"
            if last is not None and last[0] == iv["name"] and lo <= last[1]:
                return b, last[2], name
            last = (iv["name"], hi, name)
    return None


def write_pixels(path, cfg, plan, extract, bin_sizes=None, assembly="unknown", generated_by="modle-hip",
                 metadata_json="", force_overwrite=False, chroms=None):
    """write_cooler from sparse pixels, without a dense matrix on the host.  `bin_sizes=None`: the
    .cool write_cooler writes (dataset for dataset, attribute for attribute).  A list (ascending; the
    first is cfg.bin_size, the others multiples of it): a multi-resolution file with one such cooler
    per entry under /resolutions/<bin size>.  For every entry of the plan that is not skipped, in
    genome order, `extract(k, factor, first_bin, bin_offset)` is called once per resolution and returns
    the sorted non-zero pixels of plan entry k at `factor` times the bin size, with `bin_offset` (the
    interval's first bin within that resolution) added to the ids -- a pixels.Pixels, what
    api.Simulator.pixels returns -- or None for an entry without a matrix.  `first_bin` is the
    interval's first fine bin within its chromosome.  One interval's pixels of one resolution are on
    the host at a time.  (An entry that is not skipped has a column: plan_genome refuses an empty interval.)"""
    from . import cooler

    base = int(cfg.bin_size)
    if chroms is None:
        chroms = _chroms_of_plan(plan)
    kw = dict(assembly=assembly, generated_by=generated_by, metadata_json=metadata_json,
              force_overwrite=force_overwrite)
    if bin_sizes is None:
        writer = cooler.CoolerWriter(path, chroms, base, **kw)
    else:
        if not bin_sizes or int(bin_sizes[0]) != base:
            raise ValueError("write_pixels: bin_sizes must start with the simulation's bin size")
        writer = cooler.McoolWriter(path, chroms, bin_sizes, **kw)
    with writer as w:
        for k, entry in enumerate(plan):
            if entry["skipped"]:
                continue
            iv = entry["interval"]
            first_bin = int(iv["start"]) // base
            for b in w.bin_sizes:
                res, factor = w.resolution(b), b // base
                px = extract(k, factor, first_bin, res.bin_offset(iv["name"], int(iv["start"])))
                if px is None:
                    continue
                lo, hi = coarse_bin_range(first_bin, entry["ncols"], factor)
                res.append_pixels(iv["name"], hi - lo + 1, px.bin1, px.bin2, px.count,
                                  bin1_offset=px.bin1_offset, offset_bp=int(iv["start"]))


def dense_regions(plan, bin_size, chroms, regions):
    """Maps every region of --dense-region to (k, lo, hi, key): the index k of the plan entry whose
    matrix holds it, the columns [lo, hi) of that entry's band, and the name of its array,
    `chrom:start-end` of the bins it covers (the end clipped at the chromosome's).  `regions`:
    (chrom, start, end) in base pairs, or (chrom, None, None) for the whole chromosome; positions are
    snapped outward to whole bins of `bin_size`.  `chroms`: [(name, size)] of the genome.  Needs no
    GPU.  SystemExit: an unknown chromosome, start >= end, a region beyond the chromosome, a region
    that does not lie inside exactly one simulated interval (one skipped for having no barriers is
    not simulated), a duplicate."""
    bin_size, sizes = int(bin_size), dict(chroms)
    out, seen = [], set()
    for chrom, start, end in regions:
        what = chrom if start is None else f"{chrom}:{start}-{end}"
        if chrom not in sizes:
            raise SystemExit(f"--dense-region {what}: unknown chromosome {chrom}")
        if start is None:
            start, end = 0, int(sizes[chrom])
        if start >= end:
            raise SystemExit(f"--dense-region {what}: the start is not below the end")
        if end > sizes[chrom]:
            raise SystemExit(f"--dense-region {what}: beyond the end of {chrom} ({sizes[chrom]})")
        lo, hi = start // bin_size, (end + bin_size - 1) // bin_size  # bins within the chromosome
        hits = []
        for k, entry in enumerate(plan):
            iv = entry["interval"]
            first = int(iv["start"]) // bin_size
            if iv["name"] == chrom and first <= lo and hi <= first + entry["ncols"]:
                hits.append((k, first))
        if len(hits) != 1 or plan[hits[0][0]]["skipped"]:
            why = "lies in an interval that is skipped for having no barriers" if len(hits) == 1 else \
                "does not lie inside exactly one simulated interval"
            raise SystemExit(f"--dense-region {what}: bins {lo}..{hi - 1} of {chrom}: the region {why}")
        key = f"{chrom}:{lo * bin_size}-{min(hi * bin_size, int(sizes[chrom]))}"
        if key in seen:
            raise SystemExit(f"--dense-region {what}: {key} is requested twice")
        seen.add(key)
        k, first = hits[0]
        out.append((k, lo - first, hi - first, key))
    return out


def write_bigwig(path, cfg, plan, occupancies, chroms=None, force_overwrite=False):
    """Writes the 1-D LEF occupancy of every simulated interval the way the reference's IO thread
    does (simulation.cpp:130-141, 170-197): every chromosome of the genome in the header, one
    range per interval in genome order with values = counts / max(counts) as float32, span = step =
    bin size.  `occupancies[k]`: uint64 counts of plan entry k (ncols words) or None."""
    from . import bigwig

    if chroms is None:
        chroms = _chroms_of_plan(plan)
    with bigwig.BigWigWriter(path, chroms, force_overwrite=force_overwrite) as w:
        for entry, occ in zip(plan, occupancies):
            if entry["skipped"] or occ is None or entry["ncols"] == 0:
                continue
            iv = entry["interval"]
            w.write_occupancy(iv["name"], occ[:entry["ncols"]], int(cfg.bin_size), int(iv["start"]))


STATE_LOG_HEADER = ("task_id\tepoch\tcell_id\tchrom\tstart\tend\tburnin\tbarrier_occupancy\t"
                    "num_active_lefs\tnum_stalls_rev\tnum_stalls_fwd\tnum_stalls_both\t"
                    "num_lef_bar_collisions\tnum_primary_lef_lef_collisions\t"
                    "num_secondary_lef_lef_collisions\tavg_loop_size\n")


def format_state_log(task, interval, n_barriers, records):
    """lines of the model-internal-state log for one task, in the column order of
    Simulation::dump_stats (simulation.cpp:1040-1054): ids, interval, burn-in flag, effective
    barrier occupancy (occupied / all), active LEFs, units stalled rev / fwd, LEFs stalled at both
    ends, LEF-BAR / primary / secondary collisions, mean loop size"""
    out = []
    for rec in records:
        epoch = int(rec[0]) & ((1 << 63) - 1)
        burnin = bool(int(rec[0]) >> 63)
        n = int(rec[2])
        occ = (int(rec[1]) / n_barriers) if n_barriers else float("nan")
        avg = int(rec[9]) / n if n else float("nan")
        out.append(f"{task.id}\t{epoch}\t{task.cell_id}\t{interval['name']}\t{interval['start']}\t"
                   f"{interval['end']}\t{'True' if burnin else 'False'}\t{occ!r}\t{n}\t{int(rec[3])}\t"
                   f"{int(rec[4])}\t{int(rec[5])}\t{int(rec[6])}\t{int(rec[7])}\t{int(rec[8])}\t{avg!r}\n")
    return out


def write_state_log(path, sim, plan, ids):
    """<prefix>_internal_state.log.gz: the records of every task of every registered interval"""
    import gzip

    with gzip.open(path, "wt") as fh:
        fh.write(STATE_LOG_HEADER)
        for entry, iid in zip(plan, ids):
            if iid is None:
                continue
            iv = entry["interval"]
            for k, task in enumerate(entry["tasks"]):
                fh.writelines(format_state_log(task, iv, len(iv["bar_pos"]), sim.state_log(iid, k)))


def warn_missing(name, total, missed, log):
    """simulation.cpp:153-157: 1% or more of an interval's interactions fell outside its matrix"""
    if total + missed > 0 and missed / (total + missed) >= 0.01:
        log(f"warning: {100.0 * missed / (total + missed):.2f}% missing interactions for {name}")


def _needs_matrix(fn):
    """An _interval_* callback answers None for a plan entry without a matrix, `ids[k] is None`; the two
    are found by name among its positional arguments."""
    names = list(inspect.signature(fn).parameters)
    at_ids, at_k = names.index("ids"), names.index("k")

    @functools.wraps(fn)
    def guarded(*args, **kw):
        return None if args[at_ids][args[at_k]] is None else fn(*args, **kw)
    return guarded


@_needs_matrix
def _interval_pixels(sim, plan, ids, missed, log, k, factor, first_bin, bin_offset, sums=None):
    """write_pixels' callback: every resolution from the same matrix on the device (with several
    ranks: the reduced tensor); the base resolution's sum feeds the missing-interactions warning and
    is kept in `sums[k]`, for the check of the marginals"""
    px = sim.pixels(ids[k], bin_offset, factor=factor, first_bin=first_bin)
    if factor == 1:
        warn_missing(plan[k]["interval"]["name"], px.stats.sum, missed[k], log)
        if sums is not None:
            sums[k] = int(px.stats.sum)
    return px


def subsample_threshold(target, total):
    """The threshold (of 2^32) that brings a job of `total` contacts to about `target`: floor(target *
    2^32 / total) in integers; 2^32, which keeps everything, when the target is not below the total (an
    empty job included).  The kept total is binomial around the target, not equal to it."""
    target, total = int(target), int(total)
    if target < 0:
        raise ValueError(f"subsample: the target {target} is negative")
    return 1 << 32 if target >= total else (target << 32) // total


SAMPLE_CHECKED_PIXELS = 4096  # how many kept pixels of an interval check_sample draws again on the host


def check_sample(name, stats, kept, rest, threshold, seed, salt=0):
    """What the kept and the rest pixels of an interval (pixels.Pixels with the file's global bin ids)
    must satisfy before they are written, against the pixels.Stats `stats` of the interval's matrix: the
    two sums add up to the interval's, neither has more pixels than the interval, and for up to
    SAMPLE_CHECKED_PIXELS evenly spaced kept pixels the count n = kept + rest, with the rest looked up in
    the rest pixels, gives the kept count again through the host statement of the draw
    (pixels.sample_pixels).  RuntimeError, naming the interval and what fails."""
    from . import pixels

    k_sum, r_sum = int(kept.count.sum(dtype=np.int64)), int(rest.count.sum(dtype=np.int64))
    if k_sum + r_sum != int(stats.sum):
        raise RuntimeError(f"{name}: the sampled halves hold {k_sum} + {r_sum} contacts, the interval {int(stats.sum)}")
    for what, px in (("kept", kept), ("other", rest)):
        if len(px.count) > int(stats.nnz):
            raise RuntimeError(f"{name}: {len(px.count)} {what} pixels, the interval has {int(stats.nnz)}")
    n = len(kept.count)
    if n == 0:
        return
    pick = np.unique(np.linspace(0, n - 1, min(n, SAMPLE_CHECKED_PIXELS)).astype(np.int64))
    b1, b2, c = kept.bin1[pick], kept.bin2[pick], kept.count[pick].astype(np.int64)
    key = (rest.bin1.astype(np.uint64) << np.uint64(32)) | rest.bin2.astype(np.uint64)  # (sorted: cooler order)
    want = (b1.astype(np.uint64) << np.uint64(32)) | b2.astype(np.uint64)
    at = np.searchsorted(key, want)
    found = at < len(key)
    found[found] = key[at[found]] == want[found]
    others = np.zeros(len(pick), dtype=np.int64)
    others[found] = rest.count[at[found]]
    again = pixels.sample_pixels(b1, b2, c + others, threshold, seed, salt).astype(np.int64)
    bad = np.nonzero(again != c)[0]
    if len(bad):
        t = int(bad[0])
        raise RuntimeError(f"{name}: pixel ({int(b1[t])}, {int(b2[t])}) of {int(c[t] + others[t])} contacts keeps "
                           f"{int(c[t])} in the file and {int(again[t])} by the definition")


@_needs_matrix
def _interval_sampled(sim, plan, ids, threshold, seed, cache, want_rest, k, factor, first_bin, bin_offset):
    """write_pixels' callback for a sampled file (`want_rest`: for the file of the other half).  At the
    base bin size, which write_pixels asks for first, plan entry k is sampled once with the file's global
    bin ids -- `bin_offset` is the interval's first bin in the file, so a pixel's draw does not depend on
    how the genome was cut into intervals --, both halves are extracted and checked (check_sample) and the
    bands are kept in `cache`; the other levels are coarsened from the kept (or the other) band, so that
    the levels of the file agree.  `cache` holds the two bands of one interval at a time."""
    import torch

    from . import pixels

    d_band, _, nrows, ncols = sim.outputs(ids[k])
    ex = pixels.extractor(sim.device)
    if factor != 1:
        if cache.get("k") != k:
            raise RuntimeError("a sampled file is written from its base bin size upwards")
        band = cache["bands"][1 if want_rest else 0]
        return ex.coarse_extract(band.data_ptr(), nrows, ncols, factor, first_bin, bin_offset)
    cache.clear()  # (the bands of the interval before go)
    dev = torch.device("cuda", sim.device)
    bands = (torch.empty(nrows * ncols + 1, dtype=torch.int32, device=dev),
             torch.empty(nrows * ncols + 1, dtype=torch.int32, device=dev))
    stats = ex.count(d_band, nrows, ncols)
    ex.sample_into(d_band, nrows, ncols, threshold, seed, stats, bands[0].data_ptr(), bands[1].data_ptr(), 0,
                   bin_offset)
    halves = tuple(ex.extract(b.data_ptr(), nrows, ncols, bin_offset) for b in bands)
    check_sample(interval_name(plan[k]["interval"]), stats, halves[0], halves[1], threshold, seed)
    cache.update(k=k, bands=bands)
    return halves[1 if want_rest else 0]


EXPECTED_HEADER ="chrom\tstart\tend\tbin_size\tdist\tdist_bp\tn_valid\tcount_sum\tcount_avg\n"


def interval_name(iv):
    return f"{iv['name']}:{iv['start']}-{iv['end']}"


def bin_span(iv, base, factor, c):
    """[lo, hi) in base pairs of bin `c` of the interval's band at `factor` times the bin size `base`.  Fine bins
    count from the interval's start and coarse bins are anchored at the chromosome's, so the first and the last
    bin are clipped to the interval."""
    start, base, k = int(iv["start"]), int(base), int(factor)
    p = (start // base) % k
    return start + max(0, c * k - p) * base, min(int(iv["end"]), start + ((c + 1) * k - p) * base)


def check_marginals(name, total, diag_sum, coverage, min_diag=0):
    """What ties the marginals of a band (api.Simulator.marginals) to the sum of its pixels, `total`
    (pixels.Stats.sum), in exact integers: the diagonals add up to the total, and the coverage counts
    every pixel of the diagonals it keeps twice, those of the main diagonal once -- with min_diag == 0
    that is 2 * total - diag_sum[0].  RuntimeError, naming the interval, when one does not hold."""
    diag = [int(x) for x in diag_sum]
    if sum(diag) != int(total):
        raise RuntimeError(f"{name}: the diagonal sums add up to {sum(diag)}, the pixels to {int(total)}")
    m = int(min_diag)
    want = 2 * sum(diag[max(m, 1):]) + (diag[0] if m == 0 else 0)
    got = sum(int(x) for x in coverage)
    if got != want:
        raise RuntimeError(f"{name}: the coverage adds up to {got}, the diagonals from {m} on give {want}")


def expected_lines(iv, bin_size, diag_sum, n_valid):
    """the rows of <prefix>_expected.tsv for one interval at one bin size, one per diagonal d:
    chrom, start, end, bin_size, dist (d), dist_bp, n_valid, count_sum, count_avg (the repr of the
    quotient of the two integers)"""
    head = f"{iv['name']}\t{iv['start']}\t{iv['end']}\t{int(bin_size)}"
    return [f"{head}\t{d}\t{d * int(bin_size)}\t{int(n)}\t{int(s)}\t{int(s) / int(n)!r}\n"
            for d, (s, n) in enumerate(zip(diag_sum, n_valid))]


def coverage_lines(iv, bin_size, coverage):
    """the lines of <prefix>_coverage.bedgraph for one interval: chrom, start, end, value per bin;
    bin i starts i bins after the interval's start and the last one ends with the interval (bin_span)"""
    spans = (bin_span(iv, bin_size, 1, i) for i in range(len(coverage)))
    return [f"{iv['name']}\t{lo}\t{hi}\t{int(c)}\n" for (lo, hi), c in zip(spans, coverage)]


def write_expected(path, plan, base, bin_sizes, marginals):
    """<prefix>_expected.tsv: the distance-decay curve of every entry of the plan that is not skipped,
    in plan order, then by ascending bin size (`bin_sizes`; None: the base only), then by diagonal.
    `marginals(k, factor, first_bin)` returns (diag_sum, coverage) of plan entry k at `factor` times
    the bin size `base` -- what api.Simulator.marginals returns -- or None for an entry without a
    matrix; the number of pixels of diagonal d is the number of bins less d."""
    with open(path, "w") as fh:
        fh.write(EXPECTED_HEADER)
        for k, entry, first_bin, _, _ in plan_bands(plan, base):
            for b in (bin_sizes or [int(base)]):
                got = marginals(k, int(b) // int(base), first_bin)
                if got is not None:
                    diag_sum, coverage = got
                    n_valid = api.expected_n_valid(len(diag_sum), len(coverage))
                    fh.writelines(expected_lines(entry["interval"], b, diag_sum, n_valid))


def write_coverage(path, plan, base, marginals):
    """<prefix>_coverage.bedgraph: the coverage of every bin of every entry of the plan that is not
    skipped, in plan order, at the bin size `base`; `marginals` as for write_expected"""
    with open(path, "w") as fh:
        for k, entry, first_bin, factor, _ in plan_bands(plan, base):
            got = marginals(k, factor, first_bin)
            if got is not None:
                fh.writelines(coverage_lines(entry["interval"], base, got[1]))


@_needs_matrix
def _interval_marginals(sim, plan, ids, sums, min_diag, cache, k, factor, first_bin):
    """write_expected's and write_coverage's callback: summed on the device from the matrix where it
    lies (with several ranks: the reduced tensor) and checked against the sum of the interval's
    pixels.  `min_diag` holds at the base bin size, whose result both files share (the diagonal sums
    do not depend on it); a coarse level keeps every diagonal."""
    if factor == 1 and k in cache:
        return cache[k]
    m = min_diag if factor == 1 else 0
    diag_sum, coverage = sim.marginals(ids[k], m, factor, first_bin)
    check_marginals(interval_name(plan[k]["interval"]), sums[k], diag_sum, coverage, m)
    if factor == 1:
        cache[k] = (diag_sum, coverage)
    return diag_sum, coverage


def insulation_shape(nrows, ncols, first_bin, factor):
    """(nrows', ncols') of a band of plan shape at `factor` times the bin size, the interval starting at
    fine bin `first_bin` of its chromosome (modle_pixels_coarse_shape; factor 1: the band itself)"""
    if int(factor) == 1:
        return int(nrows), int(ncols)
    lo, hi = coarse_bin_range(int(first_bin), int(ncols), int(factor))
    nc = hi - lo + 1
    return min(nc, (int(nrows) - 1 + int(factor) - 1) // int(factor) + 1), nc


def plan_bands(plan, base, resolution=None):
    """(k, entry, first_bin, factor, (nrows', ncols')) of every entry of the plan that is not skipped, in plan
    order: the interval's first bin of `base` bp within its chromosome, `resolution` // `base` (None: 1) and
    the shape of its band at that factor (insulation_shape)"""
    base, factor = int(base), 1 if resolution is None else int(resolution) // int(base)
    for k, entry in enumerate(plan):
        if not entry["skipped"]:
            first_bin = int(entry["interval"]["start"]) // base
            yield k, entry, first_bin, factor, insulation_shape(entry["nrows"], entry["ncols"], first_bin, factor)


def insulation_misfit(plan, base, resolution, windows):
    """The first (name of the interval, window in bp, its bins, diagonals of the band, largest window
    in bp that fits) of an entry of the plan that has a matrix and a window of `windows` (bp, multiples
    of `resolution`) whose diamond leaves the band at `resolution`, 2 * w - 1 > nrows' -- or None."""
    res = int(resolution)
    for _, entry, _, _, (nr, _) in plan_bands(plan, base, res):
        for w in windows:
            if entry["ncols"] != 0 and 2 * (int(w) // res) - 1 > nr:
                return interval_name(entry["interval"]), int(w), int(w) // res, nr, (nr + 1) // 2 * res
    return None


def check_insulation(name, windows, min_diag, ins_sum, diag_sum):
    """What ties the insulation sums of a band (api.Simulator.insulation) to its diagonal sums
    (api.Simulator.marginals, at the same bin size), in exact integers: a pixel (a, c) of diagonal
    d = c - a lies in the diamonds of the bins a .. c that are within w of both, min(d + 1, 2 w - 1 - d)
    of them whatever the interval's edges, so for every window
        sum over b of ins_sum[b] = sum over d = min_diag .. 2 w - 2 of min(d + 1, 2 w - 1 - d) * diag_sum[d].
    RuntimeError, naming the interval and the window (in bins), when it does not hold."""
    diag = [int(x) for x in diag_sum]
    for w, row in zip(windows, ins_sum):
        w = int(w)
        if 2 * w - 1 > len(diag):
            raise RuntimeError(f"{name}: the diamond of the window of {w} bins leaves the {len(diag)} diagonals")
        want = sum(min(d + 1, 2 * w - 1 - d) * diag[d] for d in range(int(min_diag), 2 * w - 1))
        got = sum(int(x) for x in row)
        if got != want:
            raise RuntimeError(f"{name}: the insulation sums of the window of {w} bins add up to {got}, "
                               f"the diagonals from {int(min_diag)} on give {want}")


def insulation_header(windows):
    """the header line of <prefix>_insulation.tsv for the `windows` in base pairs"""
    return "chrom\tstart\tend" + "".join(f"\tsum_{w}\tn_valid_{w}\tlog2_insulation_score_{w}"
                                         for w in map(int, windows)) + "\n"


def insulation_lines(iv, base, factor, ins_sum, n_valid, score):
    """the rows of <prefix>_insulation.tsv for one interval, one per bin of `factor` * `base` base pairs:
    chrom, start, end, then per window (the rows of the three arrays) the sum, the number of pixels and
    the repr of the score.  The bins are bin_span's."""
    out = []
    for c in range(len(ins_sum[0]) if len(ins_sum) else 0):
        lo, hi = bin_span(iv, base, factor, c)
        out.append(f"{iv['name']}\t{lo}\t{hi}" + "".join(
            f"\t{int(s[c])}\t{int(n[c])}\t{float(x[c])!r}" for s, n, x in zip(ins_sum, n_valid, score)) + "\n")
    return out


def write_insulation(path, plan, base, resolution, windows, insulation):
    """<prefix>_insulation.tsv: a header, then the insulation of every bin of every entry of the plan
    that is not skipped, in plan order, at the bin size `resolution` (a multiple of `base`) for the
    `windows` in base pairs.  `insulation(k, factor, first_bin)` returns (ins_sum, n_valid) of plan
    entry k -- what api.Simulator.insulation returns -- or None for an entry without a matrix."""
    with open(path, "w") as fh:
        fh.write(insulation_header(windows))
        for k, entry, first_bin, factor, _ in plan_bands(plan, base, resolution):
            got = insulation(k, factor, first_bin)
            if got is not None:
                ins_sum, n_valid = got
                fh.writelines(insulation_lines(entry["interval"], base, factor, ins_sum, n_valid,
                                               api.insulation_score(ins_sum, n_valid)))


@_needs_matrix
def _interval_insulation(sim, plan, ids, windows, min_diag, marginals, k, factor, first_bin):
    """write_insulation's callback: summed on the device from the matrix where it lies (with several
    ranks: the reduced tensor) for the `windows` in bins, and checked against the diagonal sums of the
    marginals pass at the same bin size (`marginals`: _interval_marginals, whose base result the
    expected and the coverage file share)"""
    ins_sum, n_valid = sim.insulation(ids[k], windows, min_diag, factor, first_bin)
    check_insulation(interval_name(plan[k]["interval"]), windows, min_diag, ins_sum,
                     marginals(k, factor, first_bin)[0])
    return ins_sum, n_valid


def dots_misfit(plan, base, resolution, window, min_diag):
    """The first (name of the interval, window in bp, its bins, diagonals of the band, largest window in
    bp that fits or 0) of an entry of the plan that has a matrix in whose band at `resolution` no pixel
    can hold the whole window of `window` bp (a multiple of `resolution`) on or above diagonal
    `min_diag`, 4 * w + 1 + min_diag > nrows' -- or None."""
    res, w = int(resolution), int(window) // int(resolution)
    for _, entry, _, _, (nr, _) in plan_bands(plan, base, res):
        if entry["ncols"] != 0 and 4 * w + 1 + int(min_diag) > nr:
            return interval_name(entry["interval"]), int(window), w, nr, max(0, (nr - 1 - int(min_diag)) // 4) * res
    return None


def check_dots(name, nrows, ncols, w, min_diag, min_count, bin1, bin2, count):
    """What the candidates of a band of `nrows` x `ncols` (api.Simulator.dots) must satisfy before a row
    is written: strictly ascending in (bin1, bin2), every one a valid pixel -- bin1 >= w, bin2 + w <
    ncols, 2 w + min_diag <= bin2 - bin1 <= nrows - 1 - 2 w -- and count >= min_count.  RuntimeError,
    naming the interval and the first candidate that fails."""
    w, lo, hi = int(w), 2 * int(w) + int(min_diag), int(nrows) - 1 - 2 * int(w)
    last = None
    for b1, b2, c in zip(map(int, bin1), map(int, bin2), map(int, count)):
        if last is not None and (b1, b2) <= last:
            raise RuntimeError(f"{name}: the dot candidate ({b1}, {b2}) does not follow {last} in (bin1, bin2) order")
        if b1 < w or b2 + w >= int(ncols) or not lo <= b2 - b1 <= hi:
            raise RuntimeError(f"{name}: the dot candidate ({b1}, {b2}) is no valid pixel for a window of {w} bins "
                               f"(diagonals {lo} .. {hi}, {int(ncols)} bins)")
        if c < int(min_count):
            raise RuntimeError(f"{name}: the dot candidate ({b1}, {b2}) has count {c}, below {int(min_count)}")
        last = (b1, b2)


def dots_header():
    """the header line of <prefix>_dots.bedpe"""
    return "#chrom1\tstart1\tend1\tchrom2\tstart2\tend2\tcount\texpected\tobserved_over_expected\n"


def dots_lines(iv, base, factor, bin1, bin2, count, expected):
    """the rows of <prefix>_dots.bedpe for one interval, one per dot, in the order given: chrom, start
    and end of bin1, the same of bin2, the count, the repr of the expected count at that distance and
    the repr of their quotient.  The bins are of `factor` * `base` base pairs, with bin_span's ends."""
    out = []
    for b1, b2, c, e in zip(map(int, bin1), map(int, bin2), map(int, count), map(float, expected)):
        (lo1, hi1), (lo2, hi2) = bin_span(iv, base, factor, b1), bin_span(iv, base, factor, b2)
        ratio = c / e if e > 0 else float("inf")
        out.append(f"{iv['name']}\t{lo1}\t{hi1}\t{iv['name']}\t{lo2}\t{hi2}\t{c}\t{e!r}\t{ratio!r}\n")
    return out


def write_dots(path, plan, base, resolution, dots):
    """<prefix>_dots.bedpe: the header, then the dots of every entry of the plan that is not skipped, in
    plan order, at the bin size `resolution` (a multiple of `base`).  `dots(k, factor, first_bin)`
    returns (bin1, bin2, count, expected) of plan entry k -- the clustered candidates, interval-relative
    bins -- or None for an entry without a matrix."""
    with open(path, "w") as fh:
        fh.write(dots_header())
        for k, entry, first_bin, factor, _ in plan_bands(plan, base, resolution):
            got = dots(k, factor, first_bin)
            if got is not None:
                fh.writelines(dots_lines(entry["interval"], base, factor, *got))


@_needs_matrix
def _interval_dots(sim, plan, ids, w, p, min_count, folds, min_diag, radius, k, factor, first_bin, fdr=None):
    """write_dots' callback: the candidates found on the device in the matrix where it lies (with several
    ranks: the reduced tensor) for `w`, `p`, `radius` in bins, verified (check_dots) and thinned to local
    maxima (api.cluster_dots).  `fdr`: None, or (thresholds, edges) of dot_thresholds_of_plan, which the
    candidates must clear as well."""
    more = {} if fdr is None else {"thresholds": fdr[0], "edges": fdr[1]}
    bin1, bin2, count, expected = sim.dots(ids[k], w=w, p=p, min_count=min_count, folds=folds, min_diag=min_diag,
                                           factor=factor, first_bin=first_bin, **more)
    entry = plan[k]
    nr, nc = insulation_shape(entry["nrows"], entry["ncols"], first_bin, factor)
    check_dots(interval_name(entry["interval"]), nr, nc, w, min_diag, min_count, bin1, bin2, count)
    keep = api.cluster_dots(bin1, bin2, count, radius)
    return bin1[keep], bin2[keep], count[keep], expected[keep]


DOT_NEIGHBOURHOODS = ("donut", "lower_left", "horizontal", "vertical")


def dot_valid_pixels(nrows, ncols, w, min_diag):
    """the number of valid pixels of a band for dots with a window of `w` bins (include/modle_pixels.h): on
    diagonal d = 2 w + min_diag .. nrows - 1 - 2 w the bins j with j - d >= w and j + w < ncols"""
    w = int(w)
    return sum(max(0, int(ncols) - 2 * w - d) for d in range(2 * w + int(min_diag), int(nrows) - 2 * w))


def check_dot_hist(hist, n_valid):
    """What the lambda-chunk histogram of a plan (uint64 [4, n_chunks, n_obs], api.BandAnalyses.dot_histogram
    summed over the entries) must satisfy before thresholds are taken from it, in exact integers: for every
    neighbourhood the table sums to `n_valid`, the valid pixels of the plan, and summed over the chunks it is the
    same vector of counts for all four.  RuntimeError when it does not hold."""
    h = np.asarray(hist)
    if h.ndim != 3 or h.shape[0] != 4:
        raise RuntimeError(f"the dot histogram has shape {h.shape}, not (4, chunks, counts)")
    by_count = [[int(x) for x in h[k].astype(np.uint64).sum(axis=0, dtype=np.uint64)] for k in range(4)]
    for k, name in enumerate(DOT_NEIGHBOURHOODS):
        if sum(by_count[k]) != int(n_valid):
            raise RuntimeError(f"the dot histogram of the {name} neighbourhood holds {sum(by_count[k])} pixels, the "
                               f"plan has {int(n_valid)} valid ones")
        if by_count[k] != by_count[0]:
            o = next(o for o in range(h.shape[2]) if by_count[k][o] != by_count[0][o])
            raise RuntimeError(f"the dot histogram of the {name} neighbourhood holds {by_count[k][o]} pixels with "
                               f"count {o}, that of the {DOT_NEIGHBOURHOODS[0]} neighbourhood {by_count[0][o]}")


def dot_thresholds_header():
    """the header line of <prefix>_dots_thresholds.tsv"""
    return "resolution\tneighbourhood\tchunk\tupper_edge\tpixels\tthreshold\n"


def dot_thresholds_lines(resolution, edges, hist, thresholds):
    """the rows of <prefix>_dots_thresholds.tsv: per neighbourhood and lambda chunk the bin size, the
    neighbourhood's name, the chunk, the repr of its upper edge (inf: the top chunk), its pixels and its count
    threshold (0: never)"""
    uppers = [float(e) for e in edges] + [float("inf")]
    return [f"{int(resolution)}\t{name}\t{c}\t{uppers[c]!r}\t{int(np.asarray(hist[k][c], dtype=np.uint64).sum(dtype=np.uint64))}\t"
            f"{int(thresholds[k][c])}\n" for k, name in enumerate(DOT_NEIGHBOURHOODS) for c in range(len(uppers))]


def dot_thresholds_of_plan(sim, plan, ids, base, resolution, w, p, min_diag, fdr, chunks, log):
    """The statistical test's first pass over every entry of the plan that has a matrix, at the bin size
    `resolution`: their lambda-chunk histograms added into one table on the device (with several ranks: of the
    reduced tensors), n_obs = min(the largest count of any band + 2, 16384); check_dot_hist; then
    pixels.dot_thresholds at the rate `fdr`.  Returns (thresholds, edges, the table); a chunk with pixels and no
    threshold is named in the log."""
    from . import pixels

    edges = pixels.dot_lambda_edges(chunks)
    bands = [(ids[k], first_bin, factor, shape) for k, _, first_bin, factor, shape in plan_bands(plan, base, resolution)
             if ids[k] is not None]
    largest = max((int(sim.contact_max(iid, factor, first_bin)) for iid, first_bin, factor, _ in bands), default=0)
    n_obs = min(largest + 2, pixels.MAX_DOT_OBS)
    table, n_valid = None, 0
    for iid, first_bin, factor, (nr, nc) in bands:
        table = sim.dot_histogram_tensor(iid, w, p, edges, n_obs, min_diag, factor, first_bin, into=table)
        n_valid += dot_valid_pixels(nr, nc, w, min_diag)
    if table is None:
        hist = np.zeros((4, len(edges) + 1, n_obs), dtype=np.uint64)
    else:
        import torch

        torch.cuda.synchronize(table.device)
        hist = table.cpu().numpy().view(np.uint64)
    check_dot_hist(hist, n_valid)
    thresholds = pixels.dot_thresholds(hist, edges, fdr)
    for k, name in enumerate(DOT_NEIGHBOURHOODS):
        never = [c for c in range(len(edges)) if thresholds[k][c] == 0 and hist[k][c].any()]
        if never:
            log(f"--dots-fdr: the {name} neighbourhood has no threshold up to a count of {n_obs - 1} in the lambda "
                f"chunks {', '.join(map(str, never))}: no dot is called there")
    return thresholds, edges, hist


def read_bedpe(path):
    """The pairs of a BEDPE file as a list of (chrom1, mid1, chrom2, mid2): the first six columns of every
    line that is neither empty nor starts with `#`, mid = (start + end) // 2 of each side.  OSError when
    the file cannot be opened, ValueError, naming the line, for one with fewer than six columns or a
    coordinate that is no non-negative integer or ends before it starts."""
    pairs = []
    with open(path) as fh:
        for n, line in enumerate(fh, 1):
            if not line.strip() or line.startswith("#"):
                continue
            cols = line.rstrip("\r\n").split("\t")
            if len(cols) < 6:
                cols = line.split()
            try:
                if len(cols) < 6:
                    raise ValueError("fewer than six columns")
                s1, e1, s2, e2 = int(cols[1]), int(cols[2]), int(cols[4]), int(cols[5])
                if min(s1, s2) < 0 or e1 < s1 or e2 < s2:
                    raise ValueError("a negative start or an end before its start")
            except ValueError as e:
                raise ValueError(f"{path}, line {n}: {e}") from None
            pairs.append((cols[0], (s1 + e1) // 2, cols[3], (s2 + e2) // 2))
    return pairs


def place_pairs(plan, base, resolution, pairs):
    """Where the pairs of read_bedpe lie in the plan at the bin size `resolution` (a multiple of `base`):
    ({k: (a, b)}, trans, outside).  A cis pair goes to the first entry k of the plan that has a matrix, is
    of its chromosome and contains both midpoints; its columns in that entry's band are mid // resolution
    - (start // base) // factor, swapped so that a <= b (int64 arrays, in file order).  `trans` counts the
    pairs of two chromosomes, `outside` the cis pairs that no such entry contains."""
    base, res = int(base), int(resolution)
    factor = res // base
    placed, trans, outside = {}, 0, 0
    for c1, m1, c2, m2 in pairs:
        if c1 != c2:
            trans += 1
            continue
        for k, entry in enumerate(plan):
            iv = entry["interval"]
            if entry["skipped"] or entry["ncols"] == 0 or iv["name"] != c1:
                continue
            if int(iv["start"]) <= min(m1, m2) and max(m1, m2) < int(iv["end"]):
                first = (int(iv["start"]) // base) // factor
                a, b = sorted((m1 // res - first, m2 // res - first))
                placed.setdefault(k, ([], []))
                placed[k][0].append(a), placed[k][1].append(b)
                break
        else:
            outside += 1
    return ({k: (np.array(a, dtype=np.int64), np.array(b, dtype=np.int64)) for k, (a, b) in placed.items()},
            trans, outside)


def barrier_anchors(iv, base, resolution):
    """the on-diagonal anchors of an interval's barriers at the bin size `resolution`: a = b = the column
    of every barrier in the interval's band, ascending (int64)"""
    res = int(resolution)
    first = (int(iv["start"]) // int(base)) // (res // int(base))
    bins = np.sort(np.asarray(iv["bar_pos"], dtype=np.uint64).astype(np.int64) // res - first)
    return bins, bins.copy()


def pileup_misfit(plan, base, resolution, flank, sources=()):
    """What refuses a pileup before anything is simulated, or None: ("bedpe", path, why) for the first
    source (other than `dots` and `barriers`) that read_bedpe cannot read, else ("flank", name of the
    interval, flank in bp, its bins, diagonals of the band, largest flank in bp that fits) for the first
    entry of the plan that has a matrix in whose band at `resolution` no window of 2 f + 1 bins fits,
    2 * f + 1 > nrows'."""
    for what in sources:
        if what not in ("dots", "barriers"):
            try:
                read_bedpe(what)
            except (OSError, ValueError) as e:
                return "bedpe", what, str(e)
    res, f = int(resolution), int(flank) // int(resolution)
    for _, entry, _, _, (nr, _) in plan_bands(plan, base, res):
        if entry["ncols"] != 0 and 2 * f + 1 > nr:
            return "flank", interval_name(entry["interval"]), int(flank), f, nr, (nr - 1) // 2 * res
    return None


def check_pileup(name, source, flank, pile, n_used, dist_hist, max_count, centre=None):
    """What a pileup of a band (api.Simulator.pileup) must satisfy before a row is written, in exact
    integers: n_used is the sum of dist_hist; the whole pile is at most n_used * S * S times the largest
    pixel of the band, `max_count`; and, with `centre` (the on-diagonal anchors of `barriers`: the sum of
    M(b, b) over the accepted barriers, from the extracted pixels), the centre cell equals it.
    RuntimeError, naming the interval and the source, when one does not hold."""
    f = int(flank)
    s = 2 * f + 1
    cells = [int(x) for x in np.asarray(pile).reshape(-1)]
    if len(cells) != s * s:
        raise RuntimeError(f"{name}: the pileup at {source} has {len(cells)} cells, not {s} x {s}")
    total = sum(int(x) for x in dist_hist)
    if int(n_used) != total:
        raise RuntimeError(f"{name}: the pileup at {source} used {int(n_used)} anchors, their distances count {total}")
    if sum(cells) > int(n_used) * s * s * int(max_count):
        raise RuntimeError(f"{name}: the pileup at {source} sums to {sum(cells)}, above {int(n_used)} windows of "
                           f"{s * s} pixels of at most {int(max_count)}")
    if centre is not None and cells[f * s + f] != int(centre):
        raise RuntimeError(f"{name}: the centre of the pileup at {source} is {cells[f * s + f]}, the diagonal "
                           f"pixels of the used anchors add up to {int(centre)}")


PILEUP_SCORES = ("peak", "p2ll", "p2ul", "p2ur", "p2lr", "z_ll")


def pileup_header(source, resolution, flank, corner, given, placed, used, scores):
    """the `#` line in front of a source's block of <prefix>_pileup.tsv: the source, the bin size, the
    flank and the corner of the scores in base pairs, the anchors given, placed in an interval and used
    (accepted by the kernel), and the six scores of api.apa_scores on the observed pile, as reprs"""
    return (f"#source={source}\tresolution={int(resolution)}\tflank={int(flank)}\tcorner={int(corner)}"
            f"\tgiven={int(given)}\tplaced={int(placed)}\tused={int(used)}" +
            "".join(f"\t{key}={float(scores[key])!r}" for key in PILEUP_SCORES) + "\n")


def pileup_lines(source, resolution, flank, observed, expected):
    """the rows of a source's block, one per cell, row-major: source, the row's and the column's offset
    from the anchor in base pairs, the observed sum (an integer) and the repr of the expected one.
    `observed`, `expected`: S * S values, S = 2 * (flank // resolution) + 1."""
    res, f = int(resolution), int(flank) // int(resolution)
    s = 2 * f + 1
    return [f"{source}\t{(q // s - f) * res}\t{(q % s - f) * res}\t{int(o)}\t{float(e)!r}\n"
            for q, (o, e) in enumerate(zip(observed, expected))]


def write_pileup(path, plan, base, resolution, flank, corner, sources, anchors, pileup, unplaced=None):
    """<prefix>_pileup.tsv: one block per source of `sources` (names: `dots`, `barriers` or a BEDPE path), in
    the order given: pileup_header, then pileup_lines, at the bin size `resolution` (a multiple of
    `base`), `flank` and `corner` in base pairs.  `anchors(name, k, factor, first_bin)` returns the anchors
    (a, b) of source `name` in plan entry k, columns of its band, or None; `pileup(name, k, factor,
    first_bin, a, b)` returns (pile, n_used, terms) of them -- what api.Simulator.pileup returns and the
    terms of api.pileup_expected_terms for its dist_hist -- or None for an entry without a matrix.  The
    observed pile is the sum over the entries in Python ints, the expected one math.fsum over the entries
    of the terms.  `unplaced`: {name: the pairs given that lie in no entry}.  Returns [(name, given,
    placed, used)]."""
    res = int(resolution)
    s = 2 * (int(flank) // res) + 1
    done = []
    with open(path, "w") as fh:
        for name in sources:
            observed, terms = [0] * (s * s), [[] for _ in range(s * s)]
            placed = used = 0
            for k, _, first_bin, factor, _ in plan_bands(plan, base, res):
                ab = anchors(name, k, factor, first_bin)
                if ab is None:
                    continue
                got = pileup(name, k, factor, first_bin, ab[0], ab[1])
                if got is None:
                    continue
                placed += len(ab[0])
                used += int(got[1])
                for q, x in enumerate(np.asarray(got[0]).reshape(-1)):
                    observed[q] += int(x)
                for q, t in enumerate(got[2]):
                    terms[q] += list(t)
            given = placed + int((unplaced or {}).get(name, 0))
            scores = api.apa_scores(np.array(observed, dtype=np.float64).reshape(s, s), int(corner) // res)
            fh.write(pileup_header(name, res, flank, corner, given, placed, used, scores))
            fh.writelines(pileup_lines(name, res, flank, observed, [math.fsum(t) for t in terms]))
            done.append((name, given, placed, used))
    return done


@_needs_matrix
def _interval_anchors(plan, ids, base, resolution, dots, placed, name, k, factor, first_bin):
    """write_pileup's first callback: the run's own clustered dots (`dots`: write_dots' callback), the
    interval's barriers, or the pairs of a BEDPE file that place_pairs put into entry k"""
    if name == "dots":
        got = dots(k, factor, first_bin)
        return None if got is None else (np.asarray(got[0], dtype=np.int64), np.asarray(got[1], dtype=np.int64))
    if name == "barriers":
        return barrier_anchors(plan[k]["interval"], base, resolution)
    return placed[name].get(k, (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)))


@_needs_matrix
def _interval_pileup(sim, plan, ids, marginals, cache, flank, name, k, factor, first_bin, a, b):
    """write_pileup's second callback: summed on the device from the matrix where it lies (with several
    ranks: the reduced tensor) for `flank` in bins, and verified (check_pileup) against the pixels of the
    band at that bin size, extracted once per entry (`cache`): their largest count and, for `barriers`,
    their diagonal.  The terms of the expected pile come from the diagonal sums of the marginals pass
    (`marginals`: _interval_marginals)."""
    from . import pixels

    entry = plan[k]
    nr, nc = insulation_shape(entry["nrows"], entry["ncols"], first_bin, factor)
    pile, n_used, dist_hist = sim.pileup(ids[k], a, b, flank, factor, first_bin)
    if k not in cache:
        px = sim.pixels(ids[k], 0, factor=factor, first_bin=first_bin)
        diagonal = np.zeros(nc, dtype=np.int64)
        on = px.bin1 == px.bin2
        diagonal[px.bin1[on]] = px.count[on]
        cache[k] = (int(px.stats.max_count), diagonal)
    max_count, diagonal = cache[k]
    centre = None
    if name == "barriers":
        ok = pixels.pileup_accepts(nr, nc, flank, a, b)
        centre = sum(int(diagonal[x]) for x in np.asarray(a)[ok])
    check_pileup(interval_name(entry["interval"]), name, flank, pile, n_used, dist_hist, max_count, centre)
    diag_sum = marginals(k, factor, first_bin)[0]
    return pile, n_used, api.pileup_expected_terms(dist_hist, diag_sum, nc, flank)


def read_bed(path):
    """The domains of a BED file as a list of (chrom, start, end): the first three columns of every line that is
    neither empty nor starts with `#`.  OSError when the file cannot be opened, ValueError, naming the line, for
    one with fewer than three columns or a coordinate that is no non-negative integer or ends before it
    starts."""
    domains = []
    with open(path) as fh:
        for n, line in enumerate(fh, 1):
            if not line.strip() or line.startswith("#"):
                continue
            cols = line.rstrip("\r\n").split("\t")
            if len(cols) < 3:
                cols = line.split()
            try:
                if len(cols) < 3:
                    raise ValueError("fewer than three columns")
                s, e = int(cols[1]), int(cols[2])
                if s < 0 or e < s:
                    raise ValueError("a negative start or an end before its start")
            except ValueError as e:
                raise ValueError(f"{path}, line {n}: {e}") from None
            domains.append((cols[0], s, e))
    return domains


def place_domains(plan, base, resolution, flank_percent, domains):
    """Where the domains of read_bed lie in the plan at the bin size `resolution` (a multiple of `base`), each
    padded by `flank_percent` of its bins on either side: ({k: (start, end)}, unplaced).  A domain goes to the
    first entry k of the plan that has a matrix, is of its chromosome and contains it; in the columns of that
    entry's band it covers [s, e), s = start // resolution - first, e = max(s + 1, ceil(end / resolution) -
    first), first = (start of the interval // base) // factor, and its window is [s - pad, e + pad) with
    pad = (e - s) * flank_percent // 100 (int64 arrays, in file order).  A window that leaves the band is not
    clipped: the kernel's rule rejects it.  `unplaced` counts the domains that no such entry contains."""
    base, res, percent = int(base), int(resolution), int(flank_percent)
    factor = res // base
    placed, unplaced = {}, 0
    for chrom, start, end in domains:
        for k, entry in enumerate(plan):
            iv = entry["interval"]
            if entry["skipped"] or entry["ncols"] == 0 or iv["name"] != chrom:
                continue
            if int(iv["start"]) <= start and end <= int(iv["end"]):
                first = (int(iv["start"]) // base) // factor
                s = start // res - first
                e = max(s + 1, -(-end // res) - first)
                pad = (e - s) * percent // 100
                placed.setdefault(k, ([], []))
                placed[k][0].append(s - pad), placed[k][1].append(e + pad)
                break
        else:
            unplaced += 1
    return {k: (np.array(s, dtype=np.int64), np.array(e, dtype=np.int64)) for k, (s, e) in placed.items()}, unplaced


CALLED_DOMAINS = "called"  # the source of --domains-at that, with --call-domains, stands for the domains just called


def domains_misfit(plan, base, resolution, size, sources=()):
    """What refuses the average domain before anything is simulated, or None: ("bed", path, why) for the first
    source that read_bed cannot read, else ("size", the grid side, the diagonals of the deepest band) when the
    plan has matrices and no window reaches `size` bins in any of them at `resolution`, size > nrows' of every
    band."""
    for what in sources:
        try:
            read_bed(what)
        except (OSError, ValueError) as e:
            return "bed", what, str(e)
    depths = [nr for _, entry, _, _, (nr, _) in plan_bands(plan, base, int(resolution)) if entry["ncols"] != 0]
    if depths and int(size) > max(depths):
        return "size", int(size), max(depths)
    return None


RESCALE_CHECKED_WINDOWS = 4096  # how many accepted windows of an interval check_rescaled piles again, each alone


def window_total(px, s, e):
    """the sum of the symmetric matrix over the square [s, e) x [s, e) from the extracted pixels `px`
    (pixels.Pixels with the band's own columns as bin ids): a diagonal pixel once, another one twice"""
    lo, hi = int(px.bin1_offset[s]), int(px.bin1_offset[e])
    b1, b2, c = px.bin1[lo:hi], px.bin2[lo:hi], px.count[lo:hi].astype(np.int64)
    inside = b2 < e
    on = inside & (b1 == b2)
    return 2 * int(c[inside].sum()) - int(c[on].sum())


def check_rescaled(name, source, size, pile, area, n_used, width_hist, windows=(), totals=(), alone=None):
    """What a rescaled pileup of a band (api.Simulator.rescaled_pileup) must satisfy before a row is written, in
    exact integers: n_used is the sum of width_hist; the area equals the closed form of the widths
    (api.rescaled_area), word for word; pile and area are symmetric; and for every (s, e) of `windows` (accepted
    ones; the caller gives RESCALE_CHECKED_WINDOWS at most) the window's total from the extracted pixels,
    `totals`, equals the sum of what `alone(s, e)`, the window piled alone, returns.  RuntimeError, naming the
    interval and the source, when one does not hold."""
    r = int(size)
    p, ar = np.asarray(pile), np.asarray(area)
    if p.shape != (r, r) or ar.shape != (r, r):
        raise RuntimeError(f"{name}: the rescaled pileup at {source} has the shapes {p.shape} and {ar.shape}, not "
                           f"{r} x {r}")
    total = sum(int(x) for x in width_hist)
    if int(n_used) != total:
        raise RuntimeError(f"{name}: the rescaled pileup at {source} used {int(n_used)} windows, their widths count "
                           f"{total}")
    want = api.rescaled_area(width_hist, r)
    if not np.array_equal(ar.astype(np.uint64), want):
        u, v = (int(x[0]) for x in np.nonzero(ar.astype(np.uint64) != want))
        raise RuntimeError(f"{name}: cell ({u}, {v}) of the rescaled pileup at {source} took {int(ar[u, v])} source "
                           f"pixels, the widths of the used windows give {int(want[u, v])}")
    for what, m in (("pile", p), ("area", ar)):
        if not np.array_equal(m, m.T):
            raise RuntimeError(f"{name}: the {what} of the rescaled pileup at {source} is not symmetric")
    for (s, e), t in zip(windows, totals):
        got = sum(int(x) for x in np.asarray(alone(s, e)).reshape(-1))
        if got != int(t):
            raise RuntimeError(f"{name}: the window [{int(s)}, {int(e)}) of the rescaled pileup at {source} piles "
                               f"{got} alone, its pixels add up to {int(t)}")


def domains_header(source, resolution, size, flank_percent, given, placed, used, strength):
    """the `#` line in front of a source's block of <prefix>_domains.tsv: the source, the bin size, the side of
    the grid, the padding in percent, the domains given, placed in an interval and used (accepted by the kernel),
    and the repr of api.domain_strength of the block"""
    return (f"#source={source}\tresolution={int(resolution)}\tsize={int(size)}\tflank_percent={int(flank_percent)}"
            f"\tgiven={int(given)}\tplaced={int(placed)}\tused={int(used)}\tstrength={float(strength)!r}\n")


def domains_lines(size, observed, area, expected):
    """the rows of a source's block, one per cell, row-major: the row, the column, the observed sum and the
    number of source pixels (integers) and the repr of the expected sum.  `observed`, `area`, `expected`:
    size * size values."""
    r = int(size)
    return [f"{q // r}\t{q % r}\t{int(o)}\t{int(a)}\t{float(e)!r}\n"
            for q, (o, a, e) in enumerate(zip(observed, area, expected))]


def write_domains(path, plan, base, resolution, size, flank_percent, sources, windows, rescaled, unplaced=None):
    """<prefix>_domains.tsv: one block per BED file of `sources`, in the order given: domains_header, then
    domains_lines, at the bin size `resolution` (a multiple of `base`).  `windows(name, k)` returns the windows
    (start, end) of source `name` in plan entry k, columns of its band, or None; `rescaled(name, k, factor,
    first_bin, start, end)` returns (pile, area, n_used, terms) of them -- what api.Simulator.rescaled_pileup
    returns and the terms of api.rescaled_expected_terms for its width_hist -- or None for an entry without a
    matrix.  The observed pile and the area are sums over the entries in Python ints, the expected pile
    math.fsum over the entries of the terms.  `unplaced`: {name: the domains given that lie in no entry}.
    Returns [(name, given, placed, used)]."""
    res, r = int(resolution), int(size)
    done = []
    with open(path, "w") as fh:
        for name in sources:
            observed, area, terms = [0] * (r * r), [0] * (r * r), [[] for _ in range(r * r)]
            placed = used = 0
            for k, _, first_bin, factor, _ in plan_bands(plan, base, res):
                se = windows(name, k)
                if se is None:
                    continue
                got = rescaled(name, k, factor, first_bin, se[0], se[1])
                if got is None:
                    continue
                placed += len(se[0])
                used += int(got[2])
                for q, x in enumerate(np.asarray(got[0]).reshape(-1)):
                    observed[q] += int(x)
                for q, x in enumerate(np.asarray(got[1]).reshape(-1)):
                    area[q] += int(x)
                for q, t in enumerate(got[3]):
                    terms[q] += list(t)
            given = placed + int((unplaced or {}).get(name, 0))
            expected = [math.fsum(t) for t in terms]
            strength = api.domain_strength(np.array(observed, dtype=object).reshape(r, r),
                                           np.array(expected, dtype=np.float64).reshape(r, r), r, flank_percent)
            fh.write(domains_header(name, res, r, flank_percent, given, placed, used, strength))
            fh.writelines(domains_lines(r, observed, area, expected))
            done.append((name, given, placed, used))
    return done


@_needs_matrix
def _interval_windows(plan, ids, placed, name, k):
    """write_domains' first callback: the windows of a BED file that place_domains put into entry k"""
    return placed[name].get(k, (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)))


@_needs_matrix
def _interval_rescaled(sim, plan, ids, marginals, cache, size, name, k, factor, first_bin, start, end):
    """write_domains' second callback: summed on the device from the matrix where it lies (with several ranks:
    the reduced tensor) on a grid of `size`, and verified (check_rescaled) against the pixels of the band at
    that bin size, extracted once per entry (`cache`): up to RESCALE_CHECKED_WINDOWS evenly spaced accepted
    windows are piled again, each alone.  The terms of the expected pile come from the diagonal sums of the
    marginals pass (`marginals`: _interval_marginals)."""
    from . import pixels

    entry = plan[k]
    nr, nc = insulation_shape(entry["nrows"], entry["ncols"], first_bin, factor)
    pile, area, n_used, width_hist = sim.rescaled_pileup(ids[k], start, end, size, factor, first_bin)
    if k not in cache:
        cache[k] = sim.pixels(ids[k], 0, factor=factor, first_bin=first_bin)
    px = cache[k]
    ok = np.flatnonzero(pixels.rescale_accepts(nr, nc, size, start, end))
    if len(ok) > RESCALE_CHECKED_WINDOWS:
        ok = ok[np.unique(np.linspace(0, len(ok) - 1, RESCALE_CHECKED_WINDOWS).astype(np.int64))]
    picked = [(int(start[t]), int(end[t])) for t in ok]
    check_rescaled(interval_name(entry["interval"]), name, size, pile, area, n_used, width_hist, picked,
                   [window_total(px, s, e) for s, e in picked],
                   lambda s, e: sim.rescaled_pileup(ids[k], [s], [e], size, factor, first_bin)[0])
    diag_sum = marginals(k, factor, first_bin)[0]
    return pile, area, n_used, api.rescaled_expected_terms(width_hist, diag_sum, nc, size)


def stripes_what(metrics, exclude_zero):
    """the mask of pixels.stripes for the `metrics` of --compare-metrics: the moments always (check_stripes
    reads them), the masked moments with --compare-exclude-zero-pixels, the rank sums for spearman"""
    from . import pixels

    return pixels.STRIPES_MOMENTS | (pixels.STRIPES_MASKED if exclude_zero else 0) | \
        (pixels.STRIPES_RANKS if "spearman" in metrics else 0)


def stripes_misfit(plan, base, resolution, metrics, ref_bin_size, ref_chroms, chroms=None):
    """What keeps the run from being compared with a reference cooler of `ref_bin_size` and the chromosomes
    `ref_chroms` ([(name, size)]) at `resolution`, as a sentence, or None: another bin size; a chromosome of an
    entry of the plan that has a matrix which the file lacks or holds with another length (`chroms`: the
    run's [(name, size)]; None: the sizes the plan carries); spearman on a band deeper than
    pixels.MAX_STRIPE diagonals at `resolution`."""
    from . import pixels

    if int(ref_bin_size) != int(resolution):
        return f"the file has a bin size of {int(ref_bin_size)}, the comparison runs at {int(resolution)}"
    have, sizes = dict(ref_chroms), dict(chroms if chroms is not None else _chroms_of_plan(plan))
    for _, entry, _, _, (nr, _) in plan_bands(plan, base, resolution):
        name = entry["interval"]["name"]
        if name not in have:
            return f"the file has no chromosome {name}"
        if int(have[name]) != int(sizes[name]):
            return f"chromosome {name} has {int(have[name])} bp in the file and {int(sizes[name])} in the run"
        if "spearman" in metrics and nr > pixels.MAX_STRIPE:
            return (f"spearman ranks stripes of at most {pixels.MAX_STRIPE} entries, the band of "
                    f"{interval_name(entry['interval'])} has {nr} diagonals at {int(resolution)}")
    return None


def check_stripes(name, rows, nrows, ref_sum, run_sum):
    """What ties the sums of the stripes (api.BandAnalyses.stripe_moments with pixels.STRIPES_MOMENTS among
    the blocks, which then come first) to the two bands, in exact integers, before a row is written: every
    pixel lies in one vertical and in one horizontal stripe, so in either direction the Sa of the bins add up
    to the contacts of the reference band, `ref_sum`, and the Sb to those of the run's, `run_sum`; and every n
    is the depth of the band, `nrows`.  RuntimeError, naming the interval and what fails."""
    for d, direction in enumerate(("vertical", "horizontal")):
        n, sa, sb = ([int(x) for x in rows[d][k]] for k in range(3))
        if any(x != int(nrows) for x in n):
            raise RuntimeError(f"{name}: a {direction} stripe counts {next(x for x in n if x != int(nrows))} entries, "
                               f"the band has {int(nrows)} diagonals")
        for what, got, want in (("reference", sum(sa), int(ref_sum)), ("run", sum(sb), int(run_sum))):
            if got != want:
                raise RuntimeError(f"{name}: the {direction} stripes of the {what} add up to {got} contacts, "
                                   f"its band holds {want}")


def stripes_header(reference, resolution, exclude_zero, metrics):
    """the two header lines of <prefix>_stripes.tsv: what was compared, then the columns"""
    return (f"# reference={reference} resolution={int(resolution)} "
            f"exclude_zero_pixels={'yes' if exclude_zero else 'no'}\n"
            "chrom\tstart\tend" + "".join(f"\t{m}_vertical\t{m}_horizontal" for m in metrics) + "\n")


def stripes_lines(iv, base, factor, scores):
    """the rows of <prefix>_stripes.tsv for one interval, one per bin of `factor` * `base` base pairs: chrom,
    start, end (bin_span's), then per metric the repr of the score of
    the vertical and of the horizontal stripe, NaN as `nan`.  `scores`: per metric the (vertical, horizontal)
    pair of api.BandAnalyses.stripe_scores, in the order of the columns."""
    out = []
    for c in range(len(scores[0][0]) if scores else 0):
        lo, hi = bin_span(iv, base, factor, c)
        out.append(f"{iv['name']}\t{lo}\t{hi}" + "".join(f"\t{float(v[c])!r}\t{float(h[c])!r}" for v, h in scores)
                   + "\n")
    return out


def write_stripes(path, plan, base, reference, resolution, exclude_zero, metrics, stripes):
    """<prefix>_stripes.tsv: the header, then the scores of every bin of every entry of the plan that is not
    skipped, in plan order, at the bin size `resolution` (a multiple of `base`).  `stripes(k, factor,
    first_bin)` returns the scores of plan entry k per metric -- what stripes_lines takes -- or None for an
    entry without a matrix."""
    with open(path, "w") as fh:
        fh.write(stripes_header(reference, resolution, exclude_zero, metrics))
        for k, entry, first_bin, factor, _ in plan_bands(plan, base, resolution):
            got = stripes(k, factor, first_bin)
            if got is not None:
                fh.writelines(stripes_lines(entry["interval"], base, factor, got))


def scc_strata(nrows, resolution, smooth, max_distance, min_diag):
    """(h, lo, hi): the half-width of the smoothing box in bins and the strata of a band of `nrows` diagonals
    at `resolution` for the `smooth`, `max_distance` (bp; None: the widest the band allows) and `min_diag` of
    a cli.Scc: hi = min(nrows - 1 - 2 h, max_distance // resolution), so that no box leaves the band.  lo > hi:
    no stratum is left."""
    h = int(smooth) // int(resolution)
    hi = int(nrows) - 1 - 2 * h
    if max_distance is not None:
        hi = min(hi, int(max_distance) // int(resolution))
    return h, int(min_diag), hi


def scc_misfit(plan, base, resolution, smooth, max_distance, min_diag):
    """What keeps the SCC from being formed at `resolution`, as a sentence that names the interval, or None: an
    entry of the plan that has a matrix in whose band scc_strata leaves no stratum."""
    for _, entry, _, _, (nr, _) in plan_bands(plan, base, resolution):
        h, lo, hi = scc_strata(nr, resolution, smooth, max_distance, min_diag)
        if lo > hi:
            return (f"no diagonal is left in the band of {interval_name(entry['interval'])} ({nr} diagonals at "
                    f"{int(resolution)}): with a smoothing of {h} bins the last one is {hi}, the first one {lo}")
    return None


def check_scc(name, rows, ncols, h, lo, hi, ref_diag, run_diag):
    """What ties the sums of the strata (api.BandAnalyses.scc_moments) to the two bands, in exact integers,
    before a row is written.  For every stratum lo <= d <= hi: n is at most its ncols - d entries; Sab^2 <=
    Saa * Sbb (Cauchy-Schwarz); and, as the (2h + 1 - |k|) cells of a box on the diagonal d + k run over
    different pixels of that diagonal while the box moves along the stratum,
        Sa(d) <= sum over |k| <= 2h of (2h + 1 - |k|) * diag_sum_A(|d + k|)
    against the sums per diagonal of the reference band, `ref_diag`, with equality at h == 0; the same for Sb
    and the run's, `run_diag` (the marginals).  RuntimeError, naming the interval, the stratum and what fails."""
    h = int(h)
    for d in range(int(lo), int(hi) + 1):
        w = [int(rows[k][d]) for k in range(11)]
        n = w[0]
        sa, sb, saa, sbb, sab = (w[k] | (w[k + 1] << 64) for k in (1, 3, 5, 7, 9))
        if n > int(ncols) - d:
            raise RuntimeError(f"{name}: diagonal {d} counts {n} entries, it has {int(ncols) - d} pixels")
        if sab * sab > saa * sbb:
            raise RuntimeError(f"{name}: diagonal {d} has Sab^2 = {sab * sab} above Saa * Sbb = {saa * sbb}")
        for what, got, diag in (("reference", sa, ref_diag), ("run", sb, run_diag)):
            most = sum((2 * h + 1 - abs(k)) * int(diag[abs(d + k)]) for k in range(-2 * h, 2 * h + 1))
            if got > most or (h == 0 and got != most):
                raise RuntimeError(f"{name}: diagonal {d} of the {what} adds up to {got} contacts, the diagonals "
                                   f"its boxes reach allow {'exactly' if h == 0 else 'at most'} {most}")


def _g17(x):
    return "nan" if x != x else "%.17g" % x


def scc_header(reference, resolution, smooth, include_zeros):
    """the two header lines of <prefix>_scc.tsv: what was compared, then the columns"""
    return (f"# reference={reference} resolution={int(resolution)} smooth={int(smooth)} "
            f"include_zeros={'yes' if include_zeros else 'no'}\n"
            "distance\tn\trho\tweight\n")


def scc_lines(iv, base, factor, ncols, h, lo, hi, rows, include_zeros):
    """the rows of <prefix>_scc.tsv for one interval: a `#` line with the chromosome, start, end, the bin size,
    the half-width of the box in bins, the strata and the SCC, then per stratum its distance in base pairs, the
    number of samples, its correlation and its weight (pixels.scc_scores of `rows`), floats as %.17g, NaN as
    `nan`"""
    from . import pixels

    scc, rho, weight = pixels.scc_scores(rows, ncols, lo, hi, include_zeros)
    res = int(base) * int(factor)
    out = [f"# chrom={iv['name']} start={int(iv['start'])} end={int(iv['end'])} bin_size={res} smooth_bins={int(h)} "
           f"min_diag={int(lo)} max_diag={int(hi)} scc={_g17(scc)}\n"]
    for d in range(int(lo), int(hi) + 1):
        n = int(ncols) - d if include_zeros else int(rows[0][d])
        out.append(f"{d * res}\t{n}\t{_g17(float(rho[d - lo]))}\t{_g17(float(weight[d - lo]))}\n")
    return out


def write_scc(path, plan, base, reference, resolution, smooth, include_zeros, taken):
    """<prefix>_scc.tsv: the header, then scc_lines of every entry of the plan that is not skipped, in plan
    order.  `taken(k)` returns (ncols, h, lo, hi, rows) of plan entry k -- the strata and the sums
    _interval_scc formed -- or None for an entry without a matrix."""
    with open(path, "w") as fh:
        fh.write(scc_header(reference, resolution, smooth, include_zeros))
        for k, entry, _, factor, _ in plan_bands(plan, base, resolution):
            got = taken(k)
            if got is not None:
                fh.writelines(scc_lines(entry["interval"], base, factor, *got, include_zeros))


def _interval_scc(sim, plan, ids, marginals, scc, resolution, taken, k, ref, rid, nr, nc, factor, first_bin):
    """What _interval_stripes does for --scc while the reference band `rid` of `ref` lies on the device: the sums
    of the strata (scc_strata of the cli.Scc `scc` at the comparison's `resolution`) of the two bands are formed
    where they lie, checked (check_scc) against the diagonal sums of both, and kept in `taken[k]` for write_scc."""
    h, lo, hi = scc_strata(nr, resolution, scc.smooth, scc.max_distance, scc.min_diag)
    rows = sim.scc_moments(ids[k], ref, rid, h, lo, hi, factor, first_bin)
    check_scc(interval_name(plan[k]["interval"]), rows, nc, h, lo, hi, ref.marginals(rid)[0],
              marginals(k, factor, first_bin)[0])
    taken[k] = (nc, h, lo, hi, rows)


@_needs_matrix
def _interval_stripes(sim, plan, ids, reader, metrics, exclude_zero, sums, k, factor, first_bin, scc=None):
    """write_stripes' callback.  The reference's pixels of the interval's chromosome are scattered into a band
    of the interval's own shape at the comparison's bin size on the device (api.LoadedBands.load_pixels at the
    interval's first bin in the file), the run's band is coarsened there where `factor` is above 1, the sums of
    the stripes are formed from the two where they lie and checked (check_stripes) against the contacts the
    reference band was loaded with and those of the run's band -- `sums[k]` of the cooler at the base bin size,
    else counted on the coarse band --, and the reference band is let go.  Before it goes, `scc(k, ref, rid,
    nrows, ncols, factor, first_bin)` is called where it is given (_interval_scc): the reference is loaded once."""
    from . import pixels

    entry = plan[k]
    iv = entry["interval"]
    nr, nc = insulation_shape(entry["nrows"], entry["ncols"], first_bin, factor)
    bin1, bin2, count, chrom_first = reader.pixels(iv["name"])
    ref = api.LoadedBands(sim.device)
    try:
        rid, st = ref.load_pixels(bin1, bin2, count, nr, nc, chrom_first + coarse_bin_range(first_bin, entry["ncols"],
                                                                                            factor)[0])
        del bin1, bin2, count
        rows = sim.stripe_moments(ids[k], ref, rid, stripes_what(metrics, exclude_zero), factor, first_bin)
        run_sum = sums[k] if factor == 1 and k in sums else sim.contact_sum(ids[k], factor, first_bin)
        check_stripes(interval_name(iv), rows, nr, st.sum_in, run_sum)
        if scc is not None:
            scc(k, ref, rid, nr, nc, factor, first_bin)
    finally:
        ref.close()
    return [tuple(pixels.stripe_scores(rows[d], m, exclude_zero) for d in (0, 1)) for m in metrics]


def stripe_calls_bins(calls):
    """(m, h, lengths, min_diag, radius) in bins of the cli.StripeCalls `calls`"""
    res = int(calls.resolution)
    return int(calls.flank) // res, (int(calls.width) // res - 1) // 2, [int(x) // res for x in calls.lengths], \
        int(calls.min_diag), int(calls.radius) // res


def stripe_calls_misfit(plan, base, resolution, lengths, flank):
    """What an entry of the plan that has a matrix cannot hold of the stripe profiles, or None: the longest of
    `lengths` and the `flank` (bp, multiples of `resolution`) need L_K + m <= nrows' diagonals of its band at
    `resolution`"""
    res = int(resolution)
    need = max(int(x) for x in lengths) // res + int(flank) // res
    for _, entry, _, _, (nr, _) in plan_bands(plan, base, res):
        if entry["ncols"] != 0 and need > nr:
            return (f"the length of {max(int(x) for x in lengths)} with the flank of {int(flank)} needs {need} diagonals "
                    f"of {res}, the band of {interval_name(entry['interval'])} has {nr}")
    return None


def check_stripe_profiles(name, profiles, max_offset, lengths, min_diag, diag_sum):
    """What ties the stripe profiles of a band (api.BandAnalyses.stripe_profiles) to its diagonal sums (marginals,
    at the same bin size), in exact integers.  The cell of V[k][o][c] at distance d is the pixel (x, y) = (c - d,
    c + o) of diagonal d + o.  For o >= 0 every pixel of that diagonal has its anchor inside the chromosome, 0 <= x
    + d = c = y - o < ncols, so
        sum over c of V[k][o][c] = sum over d0 <= d < L_k of diag_sum[d + o]             (o >= 0)
    and likewise the cell (c + o, c + d) of H, of diagonal d - o, has 0 <= x - o = c = y - d < ncols for o <= 0:
        sum over c of H[k][o][c] = sum over d0 <= d < L_k of diag_sum[d - o]             (o <= 0).
    The other signs lose edge pixels: for o < 0 the anchor of a pixel in one of the last |o| columns, c = y + |o|,
    lies beyond the chromosome, and for o > 0 that of a pixel in one of the first o rows, c = x - o, before it; such
    a pixel is in no profile, and the sum falls short of the diagonals by what those pixels hold.
    RuntimeError, naming the interval, the direction, the length and the offset, when one does not hold."""
    diag = [int(x) for x in diag_sum]
    m, d0 = int(max_offset), int(min_diag)
    if max(int(x) for x in lengths) + m > len(diag):
        raise RuntimeError(f"{name}: the length of {max(lengths)} bins with the offset {m} leaves the {len(diag)} diagonals")
    for direction, word in enumerate(("upstream", "downstream")):
        for k, length in enumerate(lengths):
            for o in range(m + 1):
                row = profiles[direction][k][m + o if direction == 0 else m - o]
                got, want = sum(int(x) for x in row), sum(diag[d + o] for d in range(d0, int(length)))
                if got != want:
                    raise RuntimeError(f"{name}: the {word} profiles of length {int(length)} at offset "
                                       f"{o if direction == 0 else -o} add up to {got}, the diagonals {d0 + o} to "
                                       f"{int(length) + o - 1} give {want}")


def stripe_calls_header(calls):
    """the two header lines of <prefix>_stripe_calls.bedpe: the options of the cli.StripeCalls `calls`, then the
    columns"""
    return (f"# resolution={int(calls.resolution)} lengths={','.join(str(int(x)) for x in calls.lengths)} "
            f"flank={int(calls.flank)} width={int(calls.width)} fold={float(calls.fold)!r} min_count={int(calls.min_count)} "
            f"ignore_diags={int(calls.min_diag)} radius={int(calls.radius)}\n"
            "#chrom1\tstart1\tend1\tchrom2\tstart2\tend2\tdirection\tlength\tcentre_sum\tcentre_cells\tleft_mean\t"
            "right_mean\tenrichment\tobserved_over_expected\n")


def stripe_calls_lines(iv, base, factor, half_width, min_diag, rows):
    """the rows of <prefix>_stripe_calls.bedpe for one interval, one per api.StripeRow, sorted by anchor, then
    direction: the anchor (the bins of the centre), the extent of the stripe (the bins at the distances min_diag ..
    length - 1 from the anchor bin: before it for `up`, behind it for `down`), the direction, the length in base
    pairs, the sum and the cells of the centre, the means of the two shoulders, the enrichment and the centre over
    what the distance decay expects, floats as %.17g.  The bins are of `factor` * `base` base pairs, with
    bin_span's ends."""
    out = []
    res, h, d0 = int(base) * int(factor), int(half_width), int(min_diag)
    for r in sorted(rows, key=lambda r: (r.bin, r.direction)):
        near, far = (r.bin - r.length + 1, r.bin - d0) if r.direction == 0 else (r.bin + d0, r.bin + r.length - 1)
        lo1, hi1 = bin_span(iv, base, factor, r.bin - h)[0], bin_span(iv, base, factor, r.bin + h)[1]
        lo2, hi2 = bin_span(iv, base, factor, near)[0], bin_span(iv, base, factor, far)[1]
        out.append(f"{iv['name']}\t{lo1}\t{hi1}\t{iv['name']}\t{lo2}\t{hi2}\t{('up', 'down')[r.direction]}\t"
                   f"{r.length * res}\t{r.centre}\t{r.n_centre}\t{_g17(r.left_mean)}\t{_g17(r.right_mean)}\t"
                   f"{_g17(r.enrichment)}\t{_g17(r.obs_over_exp)}\n")
    return out


def write_stripe_calls(path, plan, base, calls, each):
    """<prefix>_stripe_calls.bedpe: the header, then the calls of every entry of the plan that is not skipped, in
    plan order (the plan is sorted by chromosome), at the bin size of the cli.StripeCalls `calls`.  `each(k, factor,
    first_bin)` returns the api.StripeRows of plan entry k, or None for an entry without a matrix."""
    _, h, _, d0, _ = stripe_calls_bins(calls)
    with open(path, "w") as fh:
        fh.write(stripe_calls_header(calls))
        for k, entry, first_bin, factor, _ in plan_bands(plan, base, calls.resolution):
            got = each(k, factor, first_bin)
            if got is not None:
                fh.writelines(stripe_calls_lines(entry["interval"], base, factor, h, d0, got))


@_needs_matrix
def _interval_stripe_calls(sim, plan, ids, marginals, calls, k, factor, first_bin):
    """write_stripe_calls' callback: the profiles summed on the device from the matrix where it lies (with several
    ranks: the reduced tensor), checked against the diagonal sums of the marginals pass at the same bin size
    (check_stripe_profiles) before a row is made of them (api.stripe_rows)"""
    m, h, lengths, d0, radius = stripe_calls_bins(calls)
    profiles, _ = sim.stripe_profiles(ids[k], m, lengths, d0, factor, first_bin)
    diag_sum = marginals(k, factor, first_bin)[0]
    check_stripe_profiles(interval_name(plan[k]["interval"]), profiles, m, lengths, d0, diag_sum)
    return api.stripe_rows(profiles, diag_sum, m, lengths, d0, h, calls.fold, calls.min_count, radius)


def stripe_calls_file(sim, cfg, plan, ids, sums, marginals, log, calls):
    """<prefix>_stripe_calls.bedpe of the cli.StripeCalls `calls`"""
    write_stripe_calls(calls.path, plan, int(cfg.bin_size), calls,
                       functools.partial(_interval_stripe_calls, sim, plan, ids, marginals, calls))
    log(f"written {calls.path}")


def domain_calls_bins(calls):
    """(max_width, min_width, min_diag) in bins of the cli.DomainCalls `calls`"""
    res = int(calls.resolution)
    return int(calls.max_width) // res, int(calls.min_width) // res, int(calls.min_diag)


def domain_calls_table_bytes(plan, base, calls):
    """the device memory of the largest triangle table --call-domains forms: over the entries of the plan that
    have a matrix, 8 bytes times the widths (the largest width, clamped to the nrows' diagonals of the band at
    the resolution of the calls) times the ncols' bins"""
    width = domain_calls_bins(calls)[0]
    return max((8 * min(width, nr) * nc for _, entry, _, _, (nr, nc) in plan_bands(plan, base, calls.resolution)
                if entry["ncols"] != 0), default=0)


def _row_sums(table):
    """the sum of every row of a uint64 table as Python integers: the two halves of the words summed apart, so
    that no sum wraps"""
    tab = np.asarray(table, dtype=np.uint64)
    lo = (tab & np.uint64(0xFFFFFFFF)).sum(axis=1, dtype=np.uint64)
    hi = (tab >> np.uint64(32)).sum(axis=1, dtype=np.uint64)
    return [(int(h) << 32) + int(l) for h, l in zip(hi, lo)]


def check_triangles(name, table, min_diag, diag_sum, windows=(), ins_sum=None):
    """What ties the triangle table of a band (api.BandAnalyses.triangle_sums, uint64 [W, ncols]) to its diagonal
    sums (marginals, at the same bin size), in exact integers.  The window of k + 1 bins at s, less the windows of
    k bins at s and at s + 1, plus the window of k - 1 bins at s + 1 that both share, leaves the one pixel (s, s +
    k) of diagonal k, so for every k < W
        sum over s of T[k][s] - T[k - 1][s] - T[k - 1][s + 1] + T[k - 2][s + 1] = diag_sum[k]   (0 for k < min_diag),
    rows -1 and -2 and column ncols counting 0; where the chromosome's end clips the windows the four terms
    cancel.  With `windows` (bins) and `ins_sum`, the insulation sums of the same band at the same `min_diag`
    (api.BandAnalyses.insulation): every window with 2 w - 1 <= W equals api.insulation_from_triangles of the
    table word for word.  RuntimeError, naming the interval and the width or the window, when one does not hold."""
    tab = np.asarray(table)
    diag = [int(x) for x in diag_sum]
    width, d0 = tab.shape[0], int(min_diag)
    if width > len(diag):
        raise RuntimeError(f"{name}: the triangle table has {width} widths, the band {len(diag)} diagonals")
    rows = _row_sums(tab)
    first = [int(x) for x in tab[:, 0]] if tab.shape[1] else [0] * width

    def shifted(k):  # the sum over s of T[k][s + 1]
        return rows[k] - first[k] if k >= 0 else 0

    for k in range(width):
        got = rows[k] - (rows[k - 1] if k >= 1 else 0) - shifted(k - 1) + shifted(k - 2)
        want = diag[k] if k >= d0 else 0
        if got != want:
            raise RuntimeError(f"{name}: the windows of {k + 1} bins hold {got} contacts on diagonal {k} beyond those "
                               f"of {k} bins, the diagonal sums give {want}")
    if ins_sum is not None:
        for w, row in zip(windows, ins_sum):
            if 2 * int(w) - 1 <= width and not np.array_equal(api.insulation_from_triangles(tab, [int(w)])[0],
                                                               np.asarray(row, dtype=np.uint64)):
                raise RuntimeError(f"{name}: the insulation sums of the window of {int(w)} bins are not the "
                                   "difference of three triangles of the table")


def domain_calls_header(calls):
    """the two header lines of <prefix>_domain_calls.bed: the options of the cli.DomainCalls `calls`, then the
    columns"""
    return (f"# resolution={int(calls.resolution)} max_width={int(calls.max_width)} min_width={int(calls.min_width)} "
            f"gamma={float(calls.gamma)!r} ignore_diags={int(calls.min_diag)}\n"
            "#chrom\tstart\tend\tname\tscore\tstrength\n")


def domain_calls_lines(iv, base, factor, rows):
    """the rows of <prefix>_domain_calls.bed for one interval, one per pixels.DomainCall, in the order of their
    starts: the chromosome, the start of the first and the end of the last bin of the domain (bins of `factor` *
    `base` base pairs with bin_span's ends), a name made of the three, the score and the strength as %.17g"""
    out = []
    for r in rows:
        lo, hi = bin_span(iv, base, factor, r.start)[0], bin_span(iv, base, factor, r.end - 1)[1]
        out.append(f"{iv['name']}\t{lo}\t{hi}\t{iv['name']}:{lo}-{hi}\t{_g17(r.score)}\t{_g17(r.strength)}\n")
    return out


def write_domain_calls(path, plan, base, calls, each):
    """<prefix>_domain_calls.bed: the header, then the domains of every entry of the plan that is not skipped, in
    plan order (the plan is sorted by chromosome), at the bin size of the cli.DomainCalls `calls`.  `each(k,
    factor, first_bin)` returns the pixels.DomainCalls of plan entry k, or None for an entry without a matrix.
    read_bed reads the file as it is."""
    with open(path, "w") as fh:
        fh.write(domain_calls_header(calls))
        for k, entry, first_bin, factor, _ in plan_bands(plan, base, calls.resolution):
            got = each(k, factor, first_bin)
            if got is not None:
                fh.writelines(domain_calls_lines(entry["interval"], base, factor, got))


@_needs_matrix
def _interval_domain_calls(sim, plan, ids, marginals, calls, insulation, k, factor, first_bin):
    """write_domain_calls' callback: the triangle table formed on the device from the matrix where it lies (with
    several ranks: the reduced tensor), the largest width clamped to the band, checked against the diagonal sums
    of the marginals pass at the same bin size and, when `insulation` (a cli.Insulation or None) ran at the same
    bin size and with the same diagonals ignored, against its sums (check_triangles) before a row is made of it
    (pixels.domain_calls)"""
    from . import pixels

    width, least, d0 = domain_calls_bins(calls)
    _, _, nrows, ncols = sim.outputs(ids[k])
    nr, _ = pixels.band_shape(nrows, ncols, factor, first_bin)
    width = min(width, nr)
    table = sim.triangle_sums(ids[k], width, d0, factor, first_bin)
    windows, ins_sum = (), None
    if insulation is not None and int(insulation.resolution) == int(calls.resolution) and int(insulation.min_diag) == d0:
        windows = [int(w) // int(insulation.resolution) for w in insulation.windows]
        ins_sum, _ = sim.insulation(ids[k], windows, d0, factor, first_bin)
    check_triangles(interval_name(plan[k]["interval"]), table, d0, marginals(k, factor, first_bin)[0], windows, ins_sum)
    try:
        return pixels.domain_calls(table, pixels.triangle_cells(table.shape[1], width, d0), gamma=calls.gamma,
                                   min_width=least)
    except ValueError as e:
        raise RuntimeError(f"{interval_name(plan[k]['interval'])}: {e}") from None


def domain_calls_file(sim, cfg, plan, ids, sums, marginals, log, calls, insulation=None):
    """<prefix>_domain_calls.bed of the cli.DomainCalls `calls`"""
    write_domain_calls(calls.path, plan, int(cfg.bin_size), calls,
                       functools.partial(_interval_domain_calls, sim, plan, ids, marginals, calls, insulation))
    log(f"written {calls.path}")


def sample_matrices(sim, cfg, plan, ids, total, subsample, bin_sizes, log, **attrs):
    """Writes `subsample.path`, the cooler (or .mcool) of the kept contacts, and with `subsample.split`
    `subsample.rest_path`, that of the others.  The threshold is that of `subsample.frac`, or with
    `subsample.target` the one that brings the job's `total` contacts at the base bin size to about the
    target; a target that is not below the total keeps everything, with a warning.  The ids of the draw
    are the file's global bin ids, the salt is 0, the seed `subsample.seed`.  With --subsample-split every
    interval is drawn a second time, for the second file: the draw is a function of its arguments."""
    from . import pixels

    if subsample.target is not None:
        threshold = subsample_threshold(subsample.target, total)
        if int(subsample.target) >= int(total):
            log(f"warning: --subsample-to {int(subsample.target)} is not below the {int(total)} contacts of the "
                "matrix: the sampled file holds the unsampled matrix")
    else:
        threshold = pixels.sample_threshold(subsample.frac)
    for path, want_rest in ((subsample.path, False), (subsample.rest_path, True)):
        if want_rest and not subsample.split:
            continue
        write_pixels(path, cfg, plan,
                     functools.partial(_interval_sampled, sim, plan, ids, threshold, int(subsample.seed), {}, want_rest),
                     bin_sizes, **attrs)
        log(f"written {path} (threshold {threshold} of 2^32)")


def reduce_to_rank0(t, backend, rank):
    """Sum of the ranks' tensors `t` into rank 0's, in place (the other ranks' tensors are unspecified
    afterwards).  `nccl` (= RCCL): on the device tensors.  `gloo`: on host copies -- the rehearsal with
    several ranks on one GPU; the copy synchronises the current stream.  int32 / int64 words that hold
    unsigned counts stay exact modulo 2^32 / 2^64 (two's complement sums)."""
    import torch.distributed as dist

    if backend == "nccl":
        dist.reduce(t, dst=0, op=dist.ReduceOp.SUM)
    else:
        h = t.cpu()
        dist.reduce(h, dst=0, op=dist.ReduceOp.SUM)
        if rank == 0:
            t.copy_(h)


def reduce_missed(missed, backend, rank, device=None):
    """The missed-update counts per plan entry (None: an entry without a matrix, zero) summed over
    the ranks, as ints on rank 0: one reduce of one int64 vector, whatever the ranks' shards hold.
    `device`: the torch device of the vector under `nccl`."""
    import torch

    t = torch.tensor([0 if m is None else int(m) for m in missed], dtype=torch.int64,
                     device=device if backend == "nccl" else "cpu")
    if len(missed) != 0:
        reduce_to_rank0(t, backend, rank)
    return [int(m) for m in t.tolist()]


def collect_outputs(sim, plan, ids, tensors, outputs, rank, log, backend):
    """What every rank does after a launch: its state log `outputs.state_log`, then per registered interval
    the occupancy and the missed-update count, and with several ranks (`tensors`) the reduces onto rank 0
    (reduce_to_rank0 with `backend`: contacts, then occupancy, per interval; then reduce_missed).  Every rank
    issues the same collectives in the same order; an entry that is skipped costs none.  Returns (the
    occupancies per plan entry, the missed updates per plan entry: on rank 0 the whole job's)."""
    if outputs.state_log is not None:
        write_state_log(outputs.state_log, sim, plan, ids)
        log(f"written {outputs.state_log}")
    occupancies, missed = [], []
    for k, iid in enumerate(ids):
        if iid is None:
            occupancies.append(None)
            missed.append(0)
            continue
        _, n_missed, occ = sim.copy_outputs(iid, want_contacts=False)
        if tensors is not None:
            tc, to = tensors[k]
            reduce_to_rank0(tc, backend, rank)
            reduce_to_rank0(to, backend, rank)
            occ = to.cpu().numpy().view(np.uint64) if occ is not None else None
        occupancies.append(occ)
        missed.append(n_missed)
    if tensors is not None:
        import torch

        dev = torch.device("cuda", sim.device)
        missed = reduce_missed(missed, backend, rank, dev)
        torch.cuda.synchronize(dev)
    return occupancies, missed


def warn_without_files(sim, plan, ids, missed, log):
    """--skip-output: the matrices are only summed where they lie, for the missing-interactions warnings"""
    from . import pixels

    for k, iid in enumerate(ids):
        if iid is not None:
            d_contacts, _, nrows, ncols = sim.outputs(iid)
            stats = pixels.extractor(sim.device).count(d_contacts, nrows, ncols)
            warn_missing(plan[k]["interval"]["name"], stats.sum, missed[k], log)


def insulation_file(sim, cfg, plan, ids, sums, marginals, log, insulation):
    """<prefix>_insulation.tsv of the cli.Insulation `insulation`"""
    bins = [int(w) // int(insulation.resolution) for w in insulation.windows]
    write_insulation(insulation.path, plan, int(cfg.bin_size), insulation.resolution, insulation.windows,
                     functools.partial(_interval_insulation, sim, plan, ids, bins, int(insulation.min_diag), marginals))
    log(f"written {insulation.path}")


def dots_file(sim, cfg, plan, ids, sums, marginals, log, dots):
    """<prefix>_dots.bedpe of the cli.Dots `dots`; returns write_dots' callback, which keeps the dots per entry:
    a pileup at the dots reads them again"""
    res = int(dots.resolution)
    each = functools.partial(_interval_dots, sim, plan, ids, int(dots.window) // res, int(dots.peak) // res,
                             int(dots.min_count), list(dots.folds), int(dots.min_diag), int(dots.radius) // res)
    if getattr(dots, "fdr", None) is not None:
        # the statistical test: one histogram over the whole plan, its thresholds, then the candidates per entry
        thresholds, edges, hist = dot_thresholds_of_plan(sim, plan, ids, int(cfg.bin_size), res, int(dots.window) // res,
                                                         int(dots.peak) // res, int(dots.min_diag), float(dots.fdr),
                                                         int(dots.chunks), log)
        with open(dots.thresholds_path, "w") as fh:
            fh.write(dot_thresholds_header())
            fh.writelines(dot_thresholds_lines(res, edges, hist, thresholds))
        log(f"written {dots.thresholds_path}")
        each = functools.partial(each, fdr=(thresholds, edges))
    interval_dots = functools.lru_cache(maxsize=None)(each)
    write_dots(dots.path, plan, int(cfg.bin_size), res, interval_dots)
    log(f"written {dots.path}")
    return interval_dots


def pileup_file(sim, cfg, plan, ids, sums, marginals, log, pileup, interval_dots):
    """<prefix>_pileup.tsv of the cli.Pileup `pileup`; its source `dots` piles the dots just written
    (`interval_dots`: what dots_file returned)"""
    base, res = int(cfg.bin_size), int(pileup.resolution)
    placed, unplaced = {}, {}
    for what in pileup.sources:
        if what not in ("dots", "barriers") and what not in placed:
            placed[what], trans, outside = place_pairs(plan, base, res, read_bedpe(what))
            unplaced[what] = trans + outside
            if trans + outside:
                log(f"--pileup-at {what}: {trans + outside} pairs are not placed ({trans} between two "
                    f"chromosomes, {outside} in no simulated interval)")
    write_pileup(pileup.path, plan, base, res, pileup.flank, pileup.corner, pileup.sources,
                 functools.partial(_interval_anchors, plan, ids, base, res, interval_dots, placed),
                 functools.partial(_interval_pileup, sim, plan, ids, marginals, {}, int(pileup.flank) // res),
                 unplaced)
    log(f"written {pileup.path}")


def domains_file(sim, cfg, plan, ids, sums, marginals, log, domains, called=None):
    """<prefix>_domains.tsv of the cli.Domains `domains`; with `called`, the <prefix>_domain_calls.bed that
    domain_calls_file has just written, the source `called` stands for that file"""
    base, res = int(cfg.bin_size), int(domains.resolution)
    placed, unplaced = {}, {}
    for what in domains.sources:
        if what not in placed:
            bed = called if called is not None and what == CALLED_DOMAINS else what
            placed[what], unplaced[what] = place_domains(plan, base, res, domains.flank_percent, read_bed(bed))
            if unplaced[what]:
                log(f"--domains-at {what}: {unplaced[what]} domains lie in no simulated interval")
    write_domains(domains.path, plan, base, res, domains.size, domains.flank_percent, domains.sources,
                  functools.partial(_interval_windows, plan, ids, placed),
                  functools.partial(_interval_rescaled, sim, plan, ids, marginals, {}, int(domains.size)), unplaced)
    log(f"written {domains.path}")


def stripes_file(sim, cfg, plan, ids, sums, marginals, log, stripes, scc=None):
    """<prefix>_stripes.tsv of the cli.Stripes `stripes`: the reference cooler is opened here, the one time after
    the launch, for its pixels.  With a cli.Scc `scc` the sums of the strata are taken while every reference
    band lies on the device, and <prefix>_scc.tsv is written after the stripes."""
    from . import cooler

    taken = {}
    each = None if scc is None else functools.partial(_interval_scc, sim, plan, ids, marginals, scc,
                                                      int(stripes.resolution), taken)
    with cooler.CoolerReader(stripes.reference) as reader:
        write_stripes(stripes.path, plan, int(cfg.bin_size), stripes.reference, stripes.resolution,
                      stripes.exclude_zero, stripes.metrics,
                      functools.partial(_interval_stripes, sim, plan, ids, reader, list(stripes.metrics),
                                        bool(stripes.exclude_zero), sums, scc=each))
    log(f"written {stripes.path}")
    if scc is not None:
        write_scc(scc.path, plan, int(cfg.bin_size), stripes.reference, stripes.resolution, scc.smooth,
                  scc.include_zeros, taken.get)
        log(f"written {scc.path}")


def write_files(sim, cfg, plan, ids, missed, pre, regions, log, **attrs):
    """Rank 0's files of the plan `pre`, in this order: the cooler or .mcool with the missing-interactions
    warnings (`missed`: of collect_outputs), the sampled matrices (sample_matrices), the dense `regions`, the
    distance-decay curves at every bin size of the file, the coverage without the diagonals below
    `pre.coverage_min_diag`, then insulation_file, dots_file, pileup_file, domain_calls_file, domains_file (whose source
    `called` reads the domain calls back), stripes_file (with `pre.scc` the SCC file too) and
    stripe_calls_file.  All of them read
    the matrices where they lie (with several ranks: the reduced tensors), after the cooler's INT32 range check
    has passed.  `attrs`: write_pixels' keywords."""
    outputs, bin_sizes = pre.outputs, pre.bin_sizes
    sums = {}  # the sum of the pixels per plan entry, at the base bin size
    write_pixels(outputs.cooler, cfg, plan,
                 functools.partial(_interval_pixels, sim, plan, ids, missed, log, sums=sums), bin_sizes, **attrs)
    log(f"written {outputs.cooler}")
    if pre.subsample is not None:
        sample_matrices(sim, cfg, plan, ids, sum(sums.values()), pre.subsample, bin_sizes, log, **attrs)
    if outputs.dense is not None:
        # (the uint32 words are int32 counts: the range check)
        np.savez(outputs.dense, **{key: sim.dense(ids[k], lo, hi).view(np.int32) for k, lo, hi, key in regions})
        log(f"written {outputs.dense}")
    marginals = functools.partial(_interval_marginals, sim, plan, ids, sums, int(pre.coverage_min_diag), {})
    if outputs.expected is not None:
        write_expected(outputs.expected, plan, int(cfg.bin_size), bin_sizes, marginals)
        log(f"written {outputs.expected}")
    if outputs.coverage is not None:
        write_coverage(outputs.coverage, plan, int(cfg.bin_size), marginals)
        log(f"written {outputs.coverage}")
    shared = (sim, cfg, plan, ids, sums, marginals, log)
    if pre.insulation is not None:
        insulation_file(*shared, pre.insulation)
    interval_dots = dots_file(*shared, pre.dots) if pre.dots is not None else None
    if pre.pileup is not None:
        pileup_file(*shared, pre.pileup, interval_dots)
    called = getattr(pre, "domain_calls", None)  # (an attribute of cli.Preflight, not a field)
    if called is not None:
        domain_calls_file(*shared, called, pre.insulation)
    if pre.domains is not None:
        domains_file(*shared, pre.domains, None if called is None else called.path)
    if pre.stripes is not None:
        stripes_file(*shared, pre.stripes, pre.scc)
    if getattr(pre, "stripe_calls", None) is not None:  # (an attribute of cli.Preflight, not a field)
        stripe_calls_file(*shared, pre.stripe_calls)


def write_outputs(sim, cfg, plan, ids, tensors, pre, regions=(), log=print, backend="nccl", **attrs):
    """The output stage of a finished launch, while the simulator is open, for the plan `pre` (a
    cli.Preflight): collect_outputs on every rank; then on rank 0 write_files, or without a cooler
    (--skip-output, under which no record of `pre` has a path) warn_without_files.  `tensors`: with several
    ranks the (contacts, occupancy) torch tensors per plan entry, which are reduced in place onto rank 0;
    the missed-update counts are summed over the ranks as well, so that the warnings weigh the whole job's
    missed updates against the whole job's matrix.  `regions`: of dense_regions.  `attrs`: write_pixels'
    keywords.  Returns the occupancies per plan entry, for write_bigwig."""
    occupancies, missed = collect_outputs(sim, plan, ids, tensors, pre.outputs, pre.rank, log, backend)
    if pre.rank == 0 and pre.outputs.cooler is not None:
        write_files(sim, cfg, plan, ids, missed, pre, regions, log, **attrs)
    elif pre.rank == 0:
        warn_without_files(sim, plan, ids, missed, log)
    return occupancies


# ---------------------------------------------------------------------------------------------
# what an N > 1 bench line says about itself (bench.py)
# ---------------------------------------------------------------------------------------------
def check_distinct_devices(devices, world):
    """`devices`: one (hostname, device index or uuid) pair per rank, all-gathered.  An RCCL job of N ranks
    on N GPUs has N distinct pairs; two ranks that ended up on one GPU (a launcher that did not set
    LOCAL_RANK, a CUDA_VISIBLE_DEVICES mask) would still finish and report N x the cells."""
    if len(devices) != world:
        raise RuntimeError(f"{len(devices)} device records for {world} ranks")
    if len(set(devices)) != world:
        raise RuntimeError(f"ranks share a GPU: {devices}")
    return True


def scaling_report(world, scaling, total_cells, cells_per_gpu, reduce_ms, prediction=None):
    """The keys an N > 1 line adds.  `prediction`: the parsed profiles/r05zs/scale_prediction.json
    (one-GPU rehearsal of the strong-scaling job: every rank's shard run one after the other), or None.
    Strong scaling at the predicted job size: the predicted speed-up over N = 1 (with the reduce serial
    behind the kernel); weak scaling: N minus the same serial reduce, i.e. what `value` should be a multiple of
    the N = 1 value by.  Always labelled a prediction: the measured one is value(N) / value(1), which only the
    driver, holding both lines, can compute."""
    out = {"scaling": scaling, "total_cells": int(total_cells), "cells_per_gpu": int(cells_per_gpu),
           "reduce_ms": reduce_ms,
           "scaling_means": ("strong: total_cells fixed, each GPU simulates total_cells / N cells of every chromosome "
                             "(north_star's '>= 6 x at 8 vs 1'; BASELINE configs[3] with --total-cells 16384)"
                             if scaling == "strong" else
                             "weak: cells_per_gpu fixed, the job grows with N; the reference splits a fixed number of "
                             "target contacts over the cells, so a cell of the N-GPU job samples 1/N of the contacts "
                             "(compare cell_epochs_per_s, not only value)")}
    pred = None
    if prediction is not None and world > 1:
        w = prediction.get("worlds", {}).get(str(world))
        if w is not None:
            if scaling == "strong" and int(prediction.get("total_cells", -1)) == int(total_cells):
                pred = {"predicted_speedup": w["predicted_speedup_with_serial_reduce"],
                        "predicted_speedup_kernel_only": w["predicted_speedup_kernel_only"]}
            elif scaling == "weak":
                single = prediction.get("single", {})
                k1 = single.get("kernel_ms") if isinstance(single, dict) else None
                if k1:
                    red = prediction.get("reduce_ms_at_one_xgmi_link", 0.0)
                    # (weak scaling of independent cells: N x, less the serial reduce of one launch)
                    pred = {"predicted_speedup": world * w["max_kernel_ms"] / (w["max_kernel_ms"] + red),
                            "predicted_speedup_kernel_only": float(world)}
            if pred is not None:
                pred["prediction_source"] = ("profiles/r05zs/scale_prediction.json (one-GPU rehearsal, "
                                             "unmeasured on multi-GPU hardware)")
    out["predicted"] = pred
    return out
