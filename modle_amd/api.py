"""Thin Python view of the C ABI (include/modle_hip.h).

Host-side logic (Config defaults, derived parameters, task generation) and the device path are
both implemented natively in libmodle_hip.so; this module only marshals arguments.  Names follow
the reference: `Config` (simulation_config.hpp), `Task` / `State` results (simulation.hpp:59-135),
`run_simulate`'s task generation (scheduler_simulate.cpp:104-160).
"""
import ctypes as C
import math
from collections import namedtuple

import numpy as np

from ._lib import lib
from .params import CellResult, Config, LaunchInfo, Task


Config = Config  # re-exported: `api.Config` is the ctypes mirror of modle_hip_config


ERR_ARG, ERR_DEVICE, ERR_UNSUPPORTED, ERR_STATE, ERR_CANCELLED, ERR_TIMEOUT = -1, -2, -3, -4, -5, -6


class ModleHipError(RuntimeError):
    """a negative return code of the C ABI (`code`: MODLE_HIP_ERR_*)"""

    def __init__(self, message, code=None):
        super().__init__(message)
        self.code = code


def _check(rc, err):
    if rc < 0:
        raise ModleHipError(f"modle_hip error {rc}: {err.value.decode(errors='replace')}", rc)
    return rc


def _errbuf():
    return C.create_string_buffer(512)


# ---------------------------------------------------------------------------------------------
# host logic
# ---------------------------------------------------------------------------------------------
def default_config(**overrides):
    """Config with the reference defaults; `overrides` set raw (pre-transform) fields."""
    cfg = Config()
    lib().modle_hip_config_default(C.byref(cfg))
    for k, v in overrides.items():
        if not hasattr(cfg, k):
            raise AttributeError(f"unknown Config field {k}")
        setattr(cfg, k, v)
    return cfg


def transform_config(cfg):
    """Cli::transform_args: derive speeds, release probabilities, burn-in parameters."""
    err = _errbuf()
    _check(lib().modle_hip_config_transform(C.byref(cfg), err, len(err)), err)
    return cfg


def make_config(**overrides):
    return transform_config(default_config(**overrides))


def interval_hash(name, chrom_size, start, end, seed):
    return lib().modle_hip_interval_hash(name.encode(), chrom_size, start, end, seed)


def prng_seed(seed):
    st = (C.c_uint64 * 4)()
    lib().modle_hip_prng_seed(seed, st)
    return [int(x) for x in st]


def prng_jump(state):
    st = (C.c_uint64 * 4)(*state)
    lib().modle_hip_prng_jump(st)
    return [int(x) for x in st]


def compute_num_lefs(cfg, size_bp):
    return lib().modle_hip_compute_num_lefs(C.byref(cfg), size_bp)


def compute_contacts_per_epoch(cfg, nlefs):
    return lib().modle_hip_compute_contacts_per_epoch(C.byref(cfg), nlefs)


def matrix_shape(cfg, size_bp):
    nr, nc = C.c_uint64(), C.c_uint64()
    lib().modle_hip_matrix_shape(C.byref(cfg), size_bp, C.byref(nr), C.byref(nc))
    return nr.value, nc.value


def make_tasks(cfg, name, chrom_size, start, end, first_task_id=0):
    tasks = (Task * int(cfg.num_cells))()
    rc = lib().modle_hip_make_tasks(C.byref(cfg), name.encode(), chrom_size, start, end,
                                    first_task_id, tasks)
    if rc < 0:
        raise ModleHipError(f"modle_hip_make_tasks failed: {rc}")
    return tasks


def plan_launch(cfg, n_tasks, num_cus, max_lefs):
    """How a launch of `n_tasks` tasks (largest cell: `max_lefs` LEFs) would be laid out on a device with `num_cus`
    compute units, environment included: a dict with the keys of `Simulator.launch_info()`, the workspace fields 0.
    No GPU needed (modle_hip_plan_launch; the rule: modle_host::plan_launch, launch_common.hpp)."""
    info = LaunchInfo()
    if lib().modle_hip_plan_launch(C.byref(cfg), int(n_tasks), int(num_cus), int(max_lefs), C.byref(info)) < 0:
        raise ModleHipError("modle_hip_plan_launch failed", ERR_ARG)
    return {name: int(getattr(info, name)) for name, _ in LaunchInfo._fields_}


def stp_active_from_occupancy(stp_inactive, occupancy):
    return lib().modle_hip_stp_active_from_occupancy(stp_inactive, occupancy)


def barrier_stps(cfg, occupancy):
    """Per-barrier self-transition probabilities from BED scores (reference: genome.cpp:260-271)."""
    occupancy = np.asarray(occupancy, dtype=np.float64)
    stp_inactive = np.full(len(occupancy), cfg.barrier_not_occupied_stp, dtype=np.float64)
    stp_active = np.array(
        [stp_active_from_occupancy(cfg.barrier_not_occupied_stp, o) if o != 0.0
         else cfg.barrier_occupied_stp for o in occupancy], dtype=np.float64)
    return stp_active, stp_inactive


def sort_barriers(bar_pos, bar_dir, stp_active, stp_inactive):
    """ExtrusionBarriers::sort: the four arrays ordered by position (copies)."""
    pos = np.array(bar_pos, dtype=np.uint64)
    dirs = np.array(bar_dir, dtype=np.uint8)
    sa = np.array(stp_active, dtype=np.float64)
    si = np.array(stp_inactive, dtype=np.float64)
    lib().modle_hip_sort_barriers(pos, dirs, sa, si, len(pos))
    return pos, dirs, sa, si


def slice_tasks(tasks, lo, hi):
    n = hi - lo
    out = (Task * n)()
    for i in range(n):
        C.memmove(C.byref(out[i]), C.byref(tasks[lo + i]), C.sizeof(Task))
    return out


def expected_n_valid(nrows, ncols):
    """the number of pixels of every diagonal d < nrows of a band of `ncols` columns: ncols - d"""
    return np.uint64(ncols) - np.arange(nrows, dtype=np.uint64)


def insulation_score(ins_sum, n_valid):
    """The log2 insulation score of integer insulation sums (Simulator.insulation), numpy float64 of
    their shape: mean = ins_sum / n_valid, and score = log2(mean / median(mean)) with the median taken,
    per window (last axis), over the bins with n_valid > 0.  nan where n_valid == 0, where ins_sum == 0
    and, everywhere, where the median is 0 (or no bin is valid)."""
    s, n = np.asarray(ins_sum, dtype=np.uint64), np.asarray(n_valid, dtype=np.uint64)
    if s.shape != n.shape or s.ndim == 0:
        raise ValueError(f"insulation_score: shapes {s.shape} and {n.shape} differ or have no bins")
    if s.size == 0:
        return np.zeros(s.shape, dtype=np.float64)
    s2, n2 = s.reshape(-1, s.shape[-1]), n.reshape(-1, n.shape[-1])
    out = np.full(s2.shape, np.nan, dtype=np.float64)
    for k in range(s2.shape[0]):
        valid = n2[k] > 0
        if not valid.any():
            continue
        mean = s2[k][valid].astype(np.float64) / n2[k][valid].astype(np.float64)
        med = float(np.median(mean))
        if med == 0.0:
            continue
        keep = mean > 0
        row = np.full(mean.shape, np.nan, dtype=np.float64)
        row[keep] = np.log2(mean[keep] / med)
        out[k][valid] = row
    return out.reshape(s.shape)


def cluster_dots(bin1, bin2, count, radius):
    """Thins dot candidates to local maxima: the ascending indexes of the candidates that stay.  A
    candidate stays unless another candidate lies within Chebyshev distance `radius` (bins, on both
    axes) and beats it: a larger count, or the same count and a smaller (bin1, bin2).  Deterministic,
    whatever the order of the input; radius 0 keeps every candidate (of distinct pixels).  This is a
    local-maximum filter, NOT HiCCUPS' greedy merge of candidates into centroids with a growing radius:
    a chain of candidates each within `radius` of the next keeps every local maximum along it."""
    b1, b2 = np.asarray(bin1, dtype=np.int64), np.asarray(bin2, dtype=np.int64)
    cnt, radius = np.asarray(count, dtype=np.int64), int(radius)
    if not (b1.shape == b2.shape == cnt.shape) or b1.ndim != 1:
        raise ValueError("cluster_dots: bin1, bin2 and count must be one-dimensional and of one length")
    if radius < 0:
        raise ValueError(f"cluster_dots: the radius {radius} is negative")
    order = np.lexsort((b2, b1))
    s1, s2, sc = b1[order], b2[order], cnt[order]
    lo = np.searchsorted(s1, s1 - radius, side="left")
    hi = np.searchsorted(s1, s1 + radius, side="right")
    keep = np.ones(len(s1), dtype=bool)
    for n in range(len(s1)):
        o1, o2, oc = s1[lo[n]:hi[n]], s2[lo[n]:hi[n]], sc[lo[n]:hi[n]]
        near = np.abs(o2 - s2[n]) <= radius
        beats = (oc > sc[n]) | ((oc == sc[n]) & ((o1 < s1[n]) | ((o1 == s1[n]) & (o2 < s2[n]))))
        keep[n] = not bool((near & beats).any())
    return np.sort(order[keep])


def pileup_expected_terms(dist_hist, diag_sum, ncols, flank):
    """The terms of pileup_expected: a list of S * S lists (cell (r, c) at r * S + c), each holding
    float(dist_hist[d]) * E[abs(d + c - r)] for the d with dist_hist[d] != 0, ascending in d, with
    E[d] = float(diag_sum[d]) / float(ncols - d)."""
    hist = [int(x) for x in np.asarray(dist_hist).reshape(-1)]
    diag = [int(x) for x in np.asarray(diag_sum).reshape(-1)]
    f, ncols = int(flank), int(ncols)
    if f < 0 or len(hist) > len(diag) or ncols < len(diag):
        raise ValueError(f"pileup_expected: flank {f}, {len(hist)} distances, {len(diag)} diagonals, {ncols} columns")
    used = [d for d, k in enumerate(hist) if k != 0]
    if used and used[-1] + 2 * f >= len(diag):
        raise ValueError(f"pileup_expected: distance {used[-1]} with a flank of {f} leaves the {len(diag)} diagonals")
    e = [float(s) / float(ncols - d) for d, s in enumerate(diag)]
    s = 2 * f + 1
    return [[float(hist[d]) * e[abs(d + c - r)] for d in used] for r in range(s) for c in range(s)]


def pileup_expected(dist_hist, diag_sum, ncols, flank):
    """What the distance-decay curve of the interval expects a pileup (Simulator.pileup) to hold, numpy
    float64 [S, S], S = 2 * flank + 1: with E[d] = float(diag_sum[d]) / float(ncols - d) (one division),
    cell (r, c) is math.fsum of float(dist_hist[d]) * E[abs(d + c - r)] over the d with dist_hist[d] != 0.
    fsum is correctly rounded, so the result does not depend on the order of the terms."""
    s = 2 * int(flank) + 1
    terms = pileup_expected_terms(dist_hist, diag_sum, ncols, flank)
    return np.array([math.fsum(t) for t in terms], dtype=np.float64).reshape(s, s)


def apa_scores(pile, corner):
    """The aggregate-peak-analysis scores of a pileup [S, S], S = 2 f + 1, as a dict of floats: `peak`, the
    centre cell; `p2ll`, `p2ul`, `p2ur`, `p2lr`, the centre over the mean of the corner x corner block in
    the lower-left (rows S - corner .., columns .. corner - 1: the corner nearest the diagonal), upper-left,
    upper-right and lower-right corner, nan where that mean is 0; `z_ll`, the centre minus the mean of
    the lower-left block over its population standard deviation, nan where that is 0.  Every cell is
    turned into a float first; a mean is math.fsum of the block over corner^2, the variance math.fsum
    of the squared differences from the mean over corner^2.  1 <= corner <= f."""
    p = np.asarray(pile)
    if p.ndim != 2 or p.shape[0] != p.shape[1] or p.shape[0] % 2 != 1:
        raise ValueError(f"apa_scores: a pile of shape {p.shape} is not [2 f + 1, 2 f + 1]")
    s, corner = p.shape[0], int(corner)
    f = s // 2
    if not 1 <= corner <= f:
        raise ValueError(f"apa_scores: the corner {corner} is not in [1, flank {f}]")
    peak = float(p[f, f])
    lo, hi = slice(0, corner), slice(s - corner, s)
    out = {"peak": peak}
    for name, rows, cols in (("p2ll", hi, lo), ("p2ul", lo, lo), ("p2ur", lo, hi), ("p2lr", hi, hi)):
        block = [float(x) for x in p[rows, cols].reshape(-1)]
        mean = math.fsum(block) / float(corner * corner)
        out[name] = peak / mean if mean != 0.0 else math.nan
        if name == "p2ll":
            sd = math.sqrt(math.fsum((x - mean) * (x - mean) for x in block) / float(corner * corner))
            out["z_ll"] = (peak - mean) / sd if sd != 0.0 else math.nan
    return out


def rescaled_block_edges(width, size):
    """lo[0 .. size] of a window of `width` bins on a grid of `size`: block u of the rescaled pileup holds the
    x with floor(x * size / width) == u, that is lo[u] <= x < lo[u + 1], lo[u] = ceil(u * width / size)"""
    w, r = int(width), int(size)
    return [-((-u * w) // r) for u in range(r + 1)]


def rescaled_area(width_hist, size):
    """The area of a rescaled pileup (Simulator.rescaled_pileup) in closed form, numpy uint64 [size, size]:
    the sum over the widths W of width_hist[W] * (the bins of block u) * (the bins of block v)."""
    r = int(size)
    area = np.zeros((r, r), dtype=np.uint64)
    for w, k in enumerate(int(x) for x in np.asarray(width_hist).reshape(-1)):
        if k != 0:
            lo = rescaled_block_edges(w, r)
            n = np.array([lo[u + 1] - lo[u] for u in range(r)], dtype=np.uint64)
            area += np.uint64(k) * np.outer(n, n)
    return area


def rescaled_expected_counts(width_hist, size):
    """cnt of rescaled_expected_terms: numpy int64 [size * (size + 1) / 2, D] over the cells u <= v (cell
    v * (v + 1) / 2 + u) and the distances d < D = the largest width in use (1 without one); cnt[q][d] is the sum
    over the widths W of width_hist[W] times the number of (x, y), 0 <= x, y < W, x in block u, y in block v, with
    abs(y - x) == d.  Block u against block v holds max(0, min(x1, y1 - k) - max(x0, y0 - k)) pairs with
    y - x == k."""
    hist = [int(x) for x in np.asarray(width_hist).reshape(-1)]
    r = int(size)
    used = [w for w, k in enumerate(hist) if k != 0]
    if r < 1 or (used and used[0] < r):
        raise ValueError(f"rescaled_expected: a grid of {r} and a width of {used[0] if used else 0}")
    uu, vv = np.triu_indices(r)
    q = vv * (vv + 1) // 2 + uu
    cnt = np.zeros((r * (r + 1) // 2, max(used[-1] if used else 1, 1)), dtype=np.int64)
    for w in used:
        lo = np.array(rescaled_block_edges(w, r), dtype=np.int64)
        x0, x1, y0, y1 = lo[uu], lo[uu + 1], lo[vv], lo[vv + 1]
        k_lo, k_hi = y0 - x1 + 1, y1 - 1 - x0  # the differences y - x a cell holds
        for j in range(int((k_hi - k_lo).max()) + 1):  # (within one j every cell is touched once)
            k = k_lo + j
            c = np.minimum(x1, y1 - k) - np.maximum(x0, y0 - k)
            on = (k <= k_hi) & (c > 0)
            cnt[q[on], np.abs(k[on])] += hist[w] * c[on]
    return cnt


def rescaled_expected_terms(width_hist, diag_sum, ncols, size):
    """The terms of rescaled_expected: a list of size * size lists (cell (u, v) at u * size + v), each holding
    float(cnt[u][v][d]) * E[d] for the d with cnt[u][v][d] != 0, ascending in d, with cnt of
    rescaled_expected_counts (exact integers) and E[d] = float(diag_sum[d]) / float(ncols - d)."""
    hist = [int(x) for x in np.asarray(width_hist).reshape(-1)]
    diag = [int(x) for x in np.asarray(diag_sum).reshape(-1)]
    r, ncols = int(size), int(ncols)
    used = [w for w, k in enumerate(hist) if k != 0]
    if ncols < len(diag) or (used and used[-1] > len(diag)):
        raise ValueError(f"rescaled_expected: widths up to {used[-1] if used else 0}, {len(diag)} diagonals, "
                         f"{ncols} columns")
    cnt = rescaled_expected_counts(hist, r)
    e = [float(s) / float(ncols - d) for d, s in enumerate(diag)]
    upper = [[float(int(row[d])) * e[d] for d in np.flatnonzero(row)] for row in cnt]
    return [upper[max(u, v) * (max(u, v) + 1) // 2 + min(u, v)] for u in range(r) for v in range(r)]


def rescaled_expected(width_hist, diag_sum, ncols, size):
    """What the distance-decay curve of the interval expects a rescaled pileup (Simulator.rescaled_pileup) to
    hold, numpy float64 [size, size]: with E[d] = float(diag_sum[d]) / float(ncols - d) (one division), cell
    (u, v) is math.fsum of float(cnt[u][v][d]) * E[d] over the d with cnt[u][v][d] != 0, cnt the number of
    source pixels of the cell at distance d over all accepted windows (rescaled_expected_counts).  fsum is
    correctly rounded, so the result does not depend on the order of the terms."""
    r = int(size)
    terms = rescaled_expected_terms(width_hist, diag_sum, ncols, size)
    return np.array([math.fsum(t) for t in terms], dtype=np.float64).reshape(r, r)


def domain_strength_blocks(size, flank_percent):
    """(g0, g1) of domain_strength: the domain itself covers the grid rows g0 <= u < g1 of a rescaled pileup
    whose windows were padded by `flank_percent` of the domain on either side:
    g0 = ceil(R P / (100 + 2 P)), g1 = floor(R (100 + P) / (100 + 2 P))"""
    r, p = int(size), int(flank_percent)
    if r < 1 or p < 0:
        raise ValueError(f"domain_strength: a grid of {r} and a flank of {p} percent")
    return -((-r * p) // (100 + 2 * p)), (r * (100 + p)) // (100 + 2 * p)


def domain_strength(pile, expected, size, flank_percent):
    """The strength of the average domain, a float: (obs_within / exp_within) / (obs_between / exp_between).
    With (g0, g1) of domain_strength_blocks, `within` is the cells g0 <= u <= v < g1 of the rescaled pileup, the
    domain's own triangle, and `between` the cells with u < g0 <= v < g1 or g0 <= u < g1 <= v, the domain
    against its two flanks.  The observed sums are Python integers of `pile`, the expected sums math.fsum of
    `expected` (rescaled_expected).  nan when flank_percent is 0, when a block is empty or when a denominator
    is 0.  This is the project's own definition, in the spirit of the TAD strength of Flyamer et al. 2017
    (observed over expected inside the domain against the same between it and its neighbourhood); it is not
    that paper's formula."""
    r = int(size)
    g0, g1 = domain_strength_blocks(r, flank_percent)
    p, e = np.asarray(pile), np.asarray(expected)
    if p.shape != (r, r) or e.shape != (r, r):
        raise ValueError(f"domain_strength: a pile of shape {p.shape}, an expected of shape {e.shape}, a grid of {r}")
    within = [(u, v) for u in range(g0, g1) for v in range(u, g1)]
    between = [(u, v) for u in range(0, g0) for v in range(g0, g1)] + \
              [(u, v) for u in range(g0, g1) for v in range(g1, r)]
    if int(flank_percent) == 0 or not within or not between:
        return math.nan
    ow, ob = sum(int(p[c]) for c in within), sum(int(p[c]) for c in between)
    ew, eb = math.fsum(float(e[c]) for c in within), math.fsum(float(e[c]) for c in between)
    if ew == 0.0 or eb == 0.0 or ob == 0:
        return math.nan
    return (float(ow) / ew) / (float(ob) / eb)


def stripe_profile_expected(diag_sum, ncols, lengths, min_diag, half_width=0):
    """What the distance-decay curve expects of the centre of a stripe profile, one float per length: the cell at
    distance d of the stripe, seen o bins to the side, lies on diagonal d + o (upstream) or d - o (downstream), so
    for either direction it is the math.fsum over min_diag <= d < L_k and |o| <= half_width of E[d + o], E[d] =
    float(diag_sum[d]) / float(ncols - d).  `diag_sum`: the sums per diagonal of the band (BandAnalyses.expected).
    ValueError when a diagonal is not held."""
    diag = [int(x) for x in np.asarray(diag_sum).reshape(-1)]
    ncols, d0, h = int(ncols), int(min_diag), int(half_width)
    ls = [int(x) for x in lengths]
    if h < 0 or d0 < h or not ls or max(ls) + h > len(diag) or ncols < len(diag):
        raise ValueError(f"stripe_profile_expected: min_diag {d0}, lengths {ls} and half width {h} on {len(diag)} "
                         f"diagonals of {ncols} columns")
    e = [float(s) / float(ncols - d) for d, s in enumerate(diag)]
    return [math.fsum(e[d + o] for d in range(d0, length) for o in range(-h, h + 1)) for length in ls]


def directionality_index(profiles, n_valid, k):
    """The directionality index of Dixon et al. (Nature 2012) of every bin from the stripe profiles of length
    class `k` (uint64 [2, K, 2 m + 1, ncols]), numpy float64 [ncols]: from the o = 0 rows, A = V the contacts with
    the L_k - min_diag bins upstream, B = H those downstream, E = (A + B) / 2 and
        DI = sign(B - A) * ((A - E)^2 + (B - E)^2) / E,
    NaN where E == 0.  A - E and B - E are formed exactly (as halves of an integer), the rest in float64.  `n_valid`
    (pixels.stripe_profile_n_valid of the same call) tells which bins have both windows whole: the index is that
    of sums, as Dixon has it, and near the ends of the chromosome one window is cut."""
    prof, nv = np.asarray(profiles), np.asarray(n_valid)
    if prof.ndim != 4 or prof.dtype != np.uint64 or prof.shape[0] != 2 or prof.shape[2] % 2 != 1 or nv.shape != prof.shape \
            or not 0 <= int(k) < prof.shape[1]:
        raise ValueError(f"directionality_index: profiles of shape {prof.shape}, valid cells of shape {nv.shape}, "
                         f"length class {k}")
    m = prof.shape[2] // 2
    out = np.empty(prof.shape[3], dtype=np.float64)
    for c in range(prof.shape[3]):
        a, b = int(prof[0, k, m, c]), int(prof[1, k, m, c])
        if a + b == 0:
            out[c] = math.nan
            continue
        # A - E = (A - B) / 2 = -(B - E): the two squares are equal
        e = (a + b) / 2
        half = (a - b) / 2
        out[c] = math.copysign((half * half + half * half) / e, b - a) if a != b else 0.0
    return out


# a call of stripe_rows: bins and sums as pixels.stripe_calls has them, the quotients as floats
StripeRow = namedtuple("StripeRow", "direction bin k length centre n_centre left_mean right_mean enrichment "
                                    "obs_over_exp")


def stripe_rows(profiles, diag_sum, max_offset, lengths, min_diag, half_width=0, fold=None, min_count=None, radius=None):
    """The stripe calls of a band as rows: pixels.stripe_calls of `profiles` and the valid cells of their call,
    each with the means of its two shoulders, its enrichment (C / nC) / max(Bl / nBl, Br / nBr) (inf over empty
    shoulders) and its centre over what the distance decay expects (stripe_profile_expected; NaN where that is
    0).  Every quotient is one division of Python integers or Fractions, rounded once.  None for `fold`,
    `min_count`, `radius`: the defaults of pixels.stripe_calls."""
    from fractions import Fraction

    from . import pixels

    prof = np.asarray(profiles)
    ncols = prof.shape[-1]
    n_valid = pixels.stripe_profile_n_valid(ncols, max_offset, lengths, min_diag)
    options = {name: v for name, v in (("fold", fold), ("min_count", min_count), ("radius", radius)) if v is not None}
    calls = pixels.stripe_calls(prof, n_valid, max_offset, lengths, min_diag, half_width, **options)
    expected = stripe_profile_expected(diag_sum, ncols, lengths, min_diag, half_width)
    rows = []
    for s in calls:
        centre, left, right = Fraction(s.centre, s.n_centre), Fraction(s.left, s.n_left), Fraction(s.right, s.n_right)
        side = max(left, right)
        rows.append(StripeRow(s.direction, s.bin, s.k, int(lengths[s.k]), s.centre, s.n_centre, float(left), float(right),
                              float(centre / side) if side else math.inf,
                              s.centre / expected[s.k] if expected[s.k] else math.nan))
    return rows


def insulation_from_triangles(table, windows):
    """The insulation sums of a band from its triangle table (BandAnalyses.triangle_sums, uint64 [W, ncols]), numpy
    uint64 [len(windows), ncols], equal word for word to BandAnalyses.insulation at the `min_diag` of the table: the
    diamond of bin b and window w, the pixels (a, c) with b - w < a <= b <= c < b + w, is the triangle of the
    window [b - w + 1, b + w) without the two triangles that lie to either side of bin b,
        ins(b, w) = T(b - w + 1, b + w) - T(b - w + 1, b) - T(b + 1, b + w),
    T(s, e) = table[e - s - 1][max(s, 0)] being the triangle of the bins [s, e), cut at the chromosome's ends, and 0
    when it is empty.  ValueError unless 1 <= w and 2 w - 1 <= W for every window."""
    tab = np.asarray(table)
    if tab.ndim != 2 or tab.dtype != np.uint64:
        raise ValueError(f"insulation_from_triangles: a table of shape {tab.shape} and type {tab.dtype} is no uint64 "
                         "[W, ncols]")
    width, ncols = tab.shape
    ws = [int(w) for w in windows]
    if any(w < 1 or 2 * w - 1 > width for w in ws):
        raise ValueError(f"insulation_from_triangles: the windows {ws} need 1 <= w and 2 w - 1 <= {width}, the widths "
                         "of the table")

    def triangle(s, e):  # arrays of starts and ends; the end is cut by the table itself
        s = np.maximum(s, 0)
        n = e - s
        some = (n > 0) & (s < ncols)
        return np.where(some, tab[np.where(some, n - 1, 0), np.where(some, s, 0)], np.uint64(0))

    b = np.arange(ncols, dtype=np.int64)
    out = np.zeros((len(ws), ncols), dtype=np.uint64)
    for i, w in enumerate(ws):
        out[i] = triangle(b - w + 1, b + w) - triangle(b - w + 1, b) - triangle(b + 1, b + w)
    return out


class BandAnalyses:
    """The analyses of a band matrix in device memory, for any owner of bands that has `device` and
    `outputs(id)` -> (device pointer of the band, occupancy pointer or None, nrows, ncols): the Simulator, whose
    bands the kernels have just written, and LoadedBands, whose bands come from a pixel list."""

    def pixels(self, interval_id, bin_offset=0, stream=None, factor=1, first_bin=0):
        """The interval's non-zero pixels in cooler order, extracted on the device from the band
        matrix where it lies (pixels.py): a pixels.Pixels of bin1, bin2, count, bin1_offset, stats.
        Call it after wait(); the dense matrix is not copied to the host.  With `factor` > 1 the band
        is first coarsened on the device (pixels.coarse_extract) and the pixels at `factor` times the
        bin size come back: `first_bin` is the interval's first bin within its chromosome (start /
        bin_size), which anchors the coarse bins at the chromosome's start, and `bin_offset` its
        first bin within the coarse file."""
        from . import pixels

        d_contacts, _, nrows, ncols = self.outputs(interval_id)
        return pixels.extractor(self.device).extract(d_contacts, nrows, ncols, bin_offset, stream, factor, first_bin)

    def coarse_pixels(self, interval_id, factor, first_bin, bin_offset=0, stream=None):
        """`pixels` at `factor` times the bin size"""
        return self.pixels(interval_id, bin_offset, stream, factor, first_bin)

    def dense(self, interval_id, lo, hi, factor=1, first_bin=0, stream=None):
        """The symmetric matrix of the bins [lo, hi) of the interval as a numpy uint32[hi - lo, hi - lo],
        unpacked on the device from the band where it lies (pixels.dense); only the region crosses to
        the host.  With `factor` > 1 the band is first coarsened on the device into a scratch band
        (`first_bin` as for coarse_pixels) and `lo`, `hi` are column indexes of that coarse band."""
        from . import pixels

        d_band, nrows, ncols, _keep = self._band(interval_id, factor, first_bin, stream)
        return pixels.dense(d_band, nrows, ncols, lo, hi, stream, device=self.device)  # (waits: a scratch may go)

    def dense_tiles(self, interval_id, first, size, step, count=None, stream=None):
        """`count` square windows of the interval (window t: the bins first + t * step .. + size - 1;
        None: all that fit) as a torch tensor [count, size, size] on the simulator's device, filled
        there by the kernel: nothing crosses to the host.  The dtype is int32 and holds the uint32
        counts bit for bit, like the tensors of the multi-rank path.  The kernel is enqueued on
        `stream` (None: the default stream, on which torch orders its own work) and not waited for."""
        import torch

        from . import pixels

        d_band, _, nrows, ncols = self.outputs(interval_id)
        if count is None:
            count = pixels.tiles_fit(ncols, first, size, step)
        out = torch.empty((int(count), int(size), int(size)), dtype=torch.int32,
                          device=torch.device("cuda", self.device))
        pixels.dense_tiles_into(d_band, nrows, ncols, first, size, step, count, out.data_ptr(), out.numel(),
                                stream, device=self.device)
        return out

    def marginals(self, interval_id, min_diag=0, factor=1, first_bin=0, stream=None):
        """(diag_sum, coverage) of the interval, numpy uint64 arrays summed on the device in one pass
        over the band (pixels.marginals; with `factor` > 1 pixels.coarse_marginals): what expected()
        and coverage() hand out one half of"""
        from . import pixels

        d_band, _, nrows, ncols = self.outputs(interval_id)
        return pixels.extractor(self.device).marginals(d_band, nrows, ncols, min_diag, stream, factor, first_bin)

    def expected(self, interval_id, factor=1, first_bin=0):
        """The distance-decay curve of the interval, summed on the device from the band where it lies
        (pixels.marginals): (diag_sum, n_valid), numpy uint64 arrays with one entry per diagonal d --
        the sum of the contacts at distance d bins and the number of pixels there, ncols - d; their
        quotient is P(s).  Call it after wait().  `factor`, `first_bin`: as for pixels(), the curve
        at `factor` times the bin size."""
        diag_sum, coverage = self.marginals(interval_id, 0, factor, first_bin)
        return diag_sum, expected_n_valid(len(diag_sum), len(coverage))

    def coverage(self, interval_id, min_diag=0, factor=1, first_bin=0):
        """The sum of every row of the interval's symmetric matrix (the diagonal pixel counted once,
        the diagonals below `min_diag` left out) as a numpy uint64 array with one entry per bin,
        summed on the device (pixels.marginals).  `factor`, `first_bin`: as for pixels()."""
        return self.marginals(interval_id, min_diag, factor, first_bin)[1]

    def marginals_tensors(self, interval_id, min_diag=0, stream=None):
        """(diag_sum, coverage) of the interval as two torch int64 tensors, [nrows] and [ncols], on
        the simulator's device, filled there by the kernel: nothing crosses to the host.  The words
        hold the uint64 sums bit for bit.  The work is enqueued on `stream` (None: the default
        stream, on which torch orders its own work) and not waited for."""
        import torch

        from . import pixels

        d_band, _, nrows, ncols = self.outputs(interval_id)
        dev = torch.device("cuda", self.device)
        diag_sum = torch.empty(nrows, dtype=torch.int64, device=dev)
        coverage = torch.empty(ncols, dtype=torch.int64, device=dev)
        pixels.marginals_into(d_band, nrows, ncols, min_diag, diag_sum.data_ptr(), coverage.data_ptr(), stream,
                              device=self.device)
        return diag_sum, coverage

    def insulation(self, interval_id, windows, min_diag=2, factor=1, first_bin=0, stream=None):
        """The insulation sums of the interval: (ins_sum, n_valid), numpy uint64 [len(windows), ncols].
        ins_sum[k][b] is the sum of the contacts that cross bin b inside the diamond of windows[k] bins
        (pixels (a, c), b - w < a <= b <= c < b + w, without the diagonals below `min_diag`), formed on
        the device from the band where it lies (pixels.insulation); n_valid the number of pixels of that
        diamond.  insulation_score() turns the two into the log2 score.  Call it after wait().  With
        `factor` > 1 the band is first coarsened on the device (`first_bin` as for pixels()) and the
        windows and `min_diag` count coarse bins."""
        from . import pixels

        d_band, _, nrows, ncols = self.outputs(interval_id)
        ins_sum = pixels.extractor(self.device).insulation(d_band, nrows, ncols, windows, min_diag, stream, factor,
                                                           first_bin)
        n_valid = np.stack([pixels.insulation_n_valid(ins_sum.shape[1], w, min_diag) for w in windows])
        return ins_sum, n_valid

    def insulation_tensor(self, interval_id, windows, min_diag=2, stream=None):
        """The insulation sums of the interval as one torch int64 tensor [len(windows), ncols] on the
        simulator's device, filled there by the kernel: nothing crosses to the host.  The words hold
        the uint64 sums bit for bit (they are below 2^52).  The kernel is enqueued on `stream` (None:
        the default stream, on which torch orders its own work) and not waited for."""
        import torch

        from . import pixels

        d_band, _, nrows, ncols = self.outputs(interval_id)
        out = torch.empty((len(windows), ncols), dtype=torch.int64, device=torch.device("cuda", self.device))
        pixels.insulation_into(d_band, nrows, ncols, windows, min_diag, out.data_ptr(), out.numel(), stream,
                               device=self.device)
        return out

    def _band(self, interval_id, factor, first_bin, stream):
        """(device pointer, nrows, ncols, what keeps it alive) of the interval's band at `factor` times
        the bin size: the band itself, or a torch scratch band the coarsening is enqueued into"""
        from . import pixels

        d_band, _, nrows, ncols = self.outputs(interval_id)
        if int(factor) == 1:
            return d_band, nrows, ncols, None
        import torch

        nr, nc = pixels.coarse_shape(nrows, ncols, factor, first_bin)
        scratch = torch.empty(nr * nc + 1, dtype=torch.int32, device=torch.device("cuda", self.device))
        pixels.extractor(self.device).coarsen_into(d_band, nrows, ncols, factor, first_bin, scratch.data_ptr(),
                                                   nr * nc + 1, stream)
        return scratch.data_ptr(), nr, nc, scratch

    def contact_sum(self, interval_id, factor=1, first_bin=0):
        """The sum of the contacts of the interval's band at `factor` times the bin size, counted on the device
        (pixels.Stats.sum of pixels.count; `first_bin` as for pixels()).  Call it after wait()."""
        from . import pixels

        d_band, nrows, ncols, _keep = self._band(interval_id, factor, first_bin, None)
        return pixels.extractor(self.device).count(d_band, nrows, ncols).sum  # (waits: a scratch may go)

    def contact_max(self, interval_id, factor=1, first_bin=0):
        """The largest count of the interval's band at `factor` times the bin size, found on the device
        (pixels.Stats.max_count of pixels.count; `first_bin` as for pixels()).  Call it after wait()."""
        from . import pixels

        d_band, nrows, ncols, _keep = self._band(interval_id, factor, first_bin, None)
        return pixels.extractor(self.device).count(d_band, nrows, ncols).max_count  # (waits: a scratch may go)

    def dot_table(self, interval_id, w, p, folds=None, min_diag=2, factor=1, first_bin=0, stream=None):
        """(scale, expected) of the interval for dots(): the table pixels.dot_scales builds from the
        diagonal sums of the marginals pass (float64 [4, nrows]) and the expected count per diagonal,
        e[d] = diag_sum[d] / (ncols - d) (float64 [nrows]), at `factor` times the bin size"""
        from . import pixels

        diag_sum, coverage = self.marginals(interval_id, 0, factor, first_bin, stream)
        ncols = len(coverage)
        scale = pixels.dot_scales(diag_sum, ncols, w, p, pixels.DOT_FOLDS if folds is None else folds, min_diag)
        e = diag_sum.astype(np.float64) / (np.float64(ncols) - np.arange(len(diag_sum), dtype=np.float64))
        return scale, e

    def dots(self, interval_id, w=5, p=2, min_count=1, folds=None, min_diag=2, factor=1, first_bin=0, stream=None,
             thresholds=None, edges=None):
        """The dot candidates of the interval: (bin1, bin2, count, expected), numpy int64, int64, int32
        and float64 arrays in cooler order.  A candidate is a pixel (bin1, bin2) whose whole window of
        half-width `w` bins lies in the band on or above diagonal `min_diag`, with count >= `min_count`
        and count >= folds[k] * e[d] * O_k / X_k for each of the four HiCCUPS neighbourhoods k (donut,
        lower-left, horizontal, vertical; peak half-width `p`): O_k the contacts of the neighbourhood,
        summed on the device, X_k what the distance-decay curve e of the interval (marginals) expects
        there; `folds` defaults to HiCCUPS' (1.75, 1.75, 1.5, 1.5).  The raw-count form of the test:
        simulated counts need no balancing.  `expected` is e at each candidate's distance.  Only the
        diagonal sums and the candidates cross to the host.  Call it after wait().  `factor`,
        `first_bin`: as for pixels(); `w`, `p`, `min_diag` then count coarse bins.  cluster_dots() thins
        the candidates to local maxima.  With `thresholds` (uint32 [4, len(edges) + 1], what dots_fdr() and
        pixels.dot_thresholds give; `edges` None: HiCCUPS' lambda chunks) a candidate must also clear, for
        every k, the threshold of the lambda chunk that e[d] * O_k / X_k falls in: the statistical test."""
        from . import pixels

        scale, e = self.dot_table(interval_id, w, p, folds, min_diag, factor, first_bin, stream)
        d_band, _, nrows, ncols = self.outputs(interval_id)
        if thresholds is None:
            px = pixels.extractor(self.device).dots(d_band, nrows, ncols, w, p, min_diag, min_count, scale, 0, stream,
                                                    factor, first_bin)
        else:
            lam = self.dot_lambda_table(interval_id, w, p, min_diag, factor, first_bin, stream)
            px = pixels.extractor(self.device).dots_fdr(d_band, nrows, ncols, w, p, min_diag, min_count, lam, edges,
                                                        thresholds, scale, 0, stream, factor, first_bin)
        return px.bin1, px.bin2, px.count, e[px.bin2 - px.bin1]

    def dots_tensors(self, interval_id, w=5, p=2, min_count=1, folds=None, min_diag=2, factor=1, first_bin=0,
                     stream=None, thresholds=None, edges=None):
        """The dot candidates of dots() as three torch tensors (bin1, bin2 int64, count int32) on the
        simulator's device: the kernel fills a candidate band there, which is counted and extracted
        into tensors of exactly nnz entries.  Only nnz and the nrows diagonal sums cross to the host."""
        import torch

        from . import pixels

        scale, _ = self.dot_table(interval_id, w, p, folds, min_diag, factor, first_bin, stream)
        lam = None if thresholds is None else self.dot_lambda_table(interval_id, w, p, min_diag, factor, first_bin,
                                                                    stream)
        d_band, nrows, ncols, keep = self._band(interval_id, factor, first_bin, stream)
        dev = torch.device("cuda", self.device)
        ex = pixels.extractor(self.device)
        cand = torch.empty(nrows * ncols + 1, dtype=torch.int32, device=dev)
        offsets = torch.empty(ncols + 1, dtype=torch.int64, device=dev)
        if thresholds is None:
            ex.dots_into(d_band, nrows, ncols, w, p, min_diag, min_count, scale, cand.data_ptr(), None, stream)
        else:
            ex.dots_fdr_into(d_band, nrows, ncols, w, p, min_diag, min_count, lam, edges, thresholds, scale,
                             cand.data_ptr(), stream)
        nnz = ex.count(cand.data_ptr(), nrows, ncols, offsets.data_ptr(), stream).nnz  # (waits)
        del keep
        bin1 = torch.empty(nnz, dtype=torch.int64, device=dev)
        bin2 = torch.empty(nnz, dtype=torch.int64, device=dev)
        count = torch.empty(nnz, dtype=torch.int32, device=dev)
        ex.extract_into(cand.data_ptr(), nrows, ncols, 0, offsets.data_ptr(), bin1.data_ptr(), bin2.data_ptr(),
                        count.data_ptr(), nnz, stream)
        torch.cuda.synchronize(dev)  # the candidate band and the index go when this returns
        return bin1, bin2, count

    def dot_lambda_table(self, interval_id, w, p, min_diag=2, factor=1, first_bin=0, stream=None):
        """The table the lambda chunks are formed with, float64 [4, nrows]: e[d] / X_k[d], pixels.dot_scales with
        folds of 1, so that O_k times it is the locally adjusted expected count of the pixel"""
        return self.dot_table(interval_id, w, p, (1.0, 1.0, 1.0, 1.0), min_diag, factor, first_bin, stream)[0]

    def dot_histogram(self, interval_id, w=5, p=2, edges=None, n_obs=None, min_diag=2, factor=1, first_bin=0,
                      stream=None):
        """The lambda-chunk histogram of the interval, numpy uint64 [4, len(edges) + 1, n_obs], counted on the
        device (pixels.dot_hist): [k][c][o] is the number of valid pixels whose locally adjusted expected count
        for neighbourhood k, e[d] * O_k / X_k, lies in chunk c = (edges[c - 1], edges[c]] and whose count is o;
        the last bin holds every count >= n_obs - 1.  `edges` None: HiCCUPS' (pixels.dot_lambda_edges); `n_obs`
        None: pixels.MAX_DOT_OBS.  The histograms of several intervals add up to the table
        pixels.dot_thresholds wants."""
        from . import pixels

        lam = self.dot_lambda_table(interval_id, w, p, min_diag, factor, first_bin, stream)
        d_band, _, nrows, ncols = self.outputs(interval_id)
        return pixels.extractor(self.device).dot_hist(d_band, nrows, ncols, w, p, min_diag, lam, edges,
                                                      pixels.MAX_DOT_OBS if n_obs is None else n_obs, stream, factor,
                                                      first_bin)

    def dot_histogram_tensor(self, interval_id, w=5, p=2, edges=None, n_obs=None, min_diag=2, factor=1, first_bin=0,
                             stream=None, into=None):
        """dot_histogram() as a torch int64 tensor [4, len(edges) + 1, n_obs] on the simulator's device, ADDED to
        `into` (a contiguous tensor of that shape there; None: a new one of zeros), which is returned: the
        intervals of a genome accumulate into one table and only the diagonal sums cross to the host.  The words
        hold the uint64 counts bit for bit."""
        import torch

        from . import pixels

        n_edges = pixels.DOT_LAMBDA_CHUNKS if edges is None else len(edges)
        n_obs = pixels.MAX_DOT_OBS if n_obs is None else int(n_obs)
        dev = torch.device("cuda", self.device)
        if into is None:
            into = torch.zeros((4, n_edges + 1, n_obs), dtype=torch.int64, device=dev)
        elif (tuple(into.shape) != (4, n_edges + 1, n_obs) or into.dtype != torch.int64 or into.device != dev
              or not into.is_contiguous()):
            raise ValueError(f"dot_histogram_tensor: `into` is not a contiguous int64 tensor of shape "
                             f"{(4, n_edges + 1, n_obs)} on {dev}")
        lam = self.dot_lambda_table(interval_id, w, p, min_diag, factor, first_bin, stream)
        d_band, nrows, ncols, keep = self._band(interval_id, factor, first_bin, stream)
        pixels.extractor(self.device).dot_hist_into(d_band, nrows, ncols, w, p, min_diag, lam, edges, n_obs,
                                                    into.data_ptr(), stream)
        if keep is not None:  # the scratch band goes when this returns
            torch.cuda.synchronize(dev)
        return into

    def dots_fdr(self, interval_ids, w=5, p=2, fdr=0.1, min_count=1, folds=None, min_diag=2, factor=1, first_bins=None,
                 edges=None, n_obs=None, stream=None):
        """The statistical test of HiCCUPS over the intervals `interval_ids` as one genome: their lambda-chunk
        histograms are added on the device, pixels.dot_thresholds turns the table into the count thresholds at
        the false discovery rate `fdr`, and every interval's candidates are found against them, with the fold
        test of dots() still on.  Returns (thresholds, {interval_id: (bin1, bin2, count, expected)}).
        `first_bins`: the first_bin of every interval at `factor` > 1 (None: 0)."""
        from . import pixels

        ids = list(interval_ids)
        firsts = [0] * len(ids) if first_bins is None else [int(f) for f in first_bins]
        if len(firsts) != len(ids):
            raise ValueError(f"dots_fdr: {len(firsts)} first bins for {len(ids)} intervals")
        e = pixels.dot_lambda_edges() if edges is None else np.asarray(edges, dtype=np.float64)
        table = None
        for iid, first in zip(ids, firsts):
            table = self.dot_histogram_tensor(iid, w, p, e, n_obs, min_diag, factor, first, stream, into=table)
        if table is None:
            return np.zeros((4, len(e) + 1), dtype=np.uint32), {}
        import torch

        torch.cuda.synchronize(table.device)
        thresholds = pixels.dot_thresholds(table.cpu().numpy().view(np.uint64), e, fdr)
        return thresholds, {iid: self.dots(iid, w, p, min_count, folds, min_diag, factor, first, stream, thresholds, e)
                            for iid, first in zip(ids, firsts)}

    def dot_sums_tensor(self, interval_id, w, p, min_diag=2, factor=1, first_bin=0, stream=None):
        """The four neighbourhood sums of every pixel of the interval as one torch int64 tensor
        [4, ncols, nrows] on the simulator's device (out[k][j][d] = O_k of pixel (j - d, j) where it is
        valid, 0 elsewhere), filled there by the kernel: nothing crosses to the host.  The words hold
        the uint64 sums bit for bit (they are below 2^43)."""
        import torch

        from . import pixels

        d_band, nrows, ncols, keep = self._band(interval_id, factor, first_bin, stream)
        out = torch.empty((4, ncols, nrows), dtype=torch.int64, device=torch.device("cuda", self.device))
        pixels.dots_into(d_band, nrows, ncols, w, p, min_diag, 1, None, None, out.data_ptr(), stream,
                         device=self.device)
        if keep is not None:  # the scratch band goes when this returns
            torch.cuda.synchronize(out.device)
        return out

    def pileup(self, interval_id, bin1, bin2, flank, factor=1, first_bin=0, bin_offset=0):
        """The pileup of the interval around the anchors (bin1[t] - bin_offset, bin2[t] - bin_offset):
        (pile, n_used, dist_hist).  pile, numpy uint64 [S, S] with S = 2 * flank + 1, is the sum of the
        windows of the symmetric matrix around the accepted anchors (a, b) -- those with a <= b whose
        window lies in the matrix and in the band (pixels.pileup_accepts) --, pile[r][c] the sum of
        M(a - flank + r, b - flank + c), formed on the device from the band where it lies
        (pixels.pileup); n_used is their number and dist_hist[d], numpy uint64 [nrows], the number of
        them with b - a == d, which pileup_expected() wants.  a == b piles windows on the diagonal.
        Only the anchors and the pile cross between host and device.  Call it after wait().  With
        `factor` > 1 the band is first coarsened on the device (`first_bin` as for pixels()) and
        `flank` and the anchors count coarse bins."""
        from . import pixels

        d_band, _, nrows, ncols = self.outputs(interval_id)
        nr, nc = pixels.band_shape(nrows, ncols, factor, first_bin)
        pile, n_used = pixels.extractor(self.device).pileup(d_band, nrows, ncols, flank, bin1, bin2, bin_offset, None,
                                                            factor, first_bin)
        b1 = np.asarray(bin1, dtype=np.int64).reshape(-1)
        b2 = np.asarray(bin2, dtype=np.int64).reshape(-1)
        ok = pixels.pileup_accepts(nr, nc, flank, b1, b2, bin_offset)
        dist_hist = np.bincount(b2[ok] - b1[ok], minlength=nr).astype(np.uint64)
        return pile, n_used, dist_hist

    def pileup_tensors(self, interval_id, bin1, bin2, flank, bin_offset=0, stream=None):
        """(pile, n_used) of pileup() for anchors that are torch int64 tensors on the simulator's
        device, as two torch int64 tensors, [S, S] and [1], on that device, filled there by the
        kernels: nothing crosses to the host, so dots_tensors() feeds in as it is.  The words hold the
        uint64 sums bit for bit.  The work is enqueued on `stream` (None: the default stream, on which
        torch orders its own work) and not waited for."""
        import torch

        from . import pixels

        d_band, _, nrows, ncols = self.outputs(interval_id)
        dev = torch.device("cuda", self.device)
        for t in (bin1, bin2):
            if t.dtype != torch.int64 or t.device != dev or t.dim() != 1:
                raise ValueError("pileup_tensors: the anchors must be one-dimensional int64 tensors on the "
                                 "simulator's device")
        if bin1.numel() != bin2.numel():
            raise ValueError(f"pileup_tensors: {bin1.numel()} first and {bin2.numel()} second anchors")
        bin1, bin2 = bin1.contiguous(), bin2.contiguous()
        s = 2 * int(flank) + 1
        pile = torch.empty((s, s), dtype=torch.int64, device=dev)
        n_used = torch.empty(1, dtype=torch.int64, device=dev)
        n = bin1.numel()
        pixels.pileup_into(d_band, nrows, ncols, flank, bin1.data_ptr() if n else None, bin2.data_ptr() if n else None,
                           n, pile.data_ptr(), n_used.data_ptr(), bin_offset, stream, device=self.device)
        return pile, n_used

    def rescaled_pileup(self, interval_id, start, end, size, factor=1, first_bin=0, bin_offset=0):
        """The rescaled pileup of the interval over the windows [start[t] - bin_offset, end[t] - bin_offset) on
        the diagonal, the average domain: (pile, area, n_used, width_hist).  An accepted window [s, e) --
        0 <= s < e <= ncols and size <= e - s <= nrows (pixels.rescale_accepts) -- of width W is cut into
        size x size blocks, block u holding the x with floor(x * size / W) == u; pile[u][v], numpy uint64
        [size, size], is the sum of the symmetric matrix over block u x block v of every accepted window, formed
        on the device from the band where it lies (pixels.rescale), and area[u][v] the number of source pixels
        it took.  pile / area is the pooled mean of a cell, in which large windows weigh more: not the mean of
        per-window interpolations.  n_used is the number of accepted windows and width_hist[W], numpy uint64
        [nrows + 1], the number of them of width W, which rescaled_expected() wants.  Only the windows and the
        results cross between host and device.  Call it after wait().  With `factor` > 1 the band is first
        coarsened on the device (`first_bin` as for pixels()) and the windows count coarse bins."""
        from . import pixels

        d_band, _, nrows, ncols = self.outputs(interval_id)
        nr, nc = pixels.band_shape(nrows, ncols, factor, first_bin)
        pile, area, n_used = pixels.extractor(self.device).rescale(d_band, nrows, ncols, size, start, end, bin_offset,
                                                                   None, factor, first_bin)
        s = np.asarray(start, dtype=np.int64).reshape(-1)
        e = np.asarray(end, dtype=np.int64).reshape(-1)
        ok = pixels.rescale_accepts(nr, nc, size, s, e, bin_offset)
        width_hist = np.bincount(e[ok] - s[ok], minlength=nr + 1).astype(np.uint64)
        return pile, area, n_used, width_hist

    def rescaled_pileup_tensors(self, interval_id, start, end, size, bin_offset=0, stream=None):
        """(pile, area, n_used) of rescaled_pileup() for windows that are torch int64 tensors on the simulator's
        device, as three torch int64 tensors, [size, size], [size, size] and [1], on that device, filled there
        by the kernels: nothing crosses to the host.  The words hold the uint64 sums bit for bit.  The work is
        enqueued on `stream` (None: the default stream, on which torch orders its own work) and not waited
        for."""
        import torch

        from . import pixels

        d_band, _, nrows, ncols = self.outputs(interval_id)
        dev = torch.device("cuda", self.device)
        for t in (start, end):
            if t.dtype != torch.int64 or t.device != dev or t.dim() != 1:
                raise ValueError("rescaled_pileup_tensors: the windows must be one-dimensional int64 tensors on the "
                                 "simulator's device")
        if start.numel() != end.numel():
            raise ValueError(f"rescaled_pileup_tensors: {start.numel()} starts and {end.numel()} ends")
        start, end = start.contiguous(), end.contiguous()
        r = int(size)
        if not 1 <= r <= pixels.MAX_RESCALE:
            raise ValueError(f"rescaled_pileup_tensors: a grid of {r} is not in [1, {pixels.MAX_RESCALE}]")
        pile = torch.empty((r, r), dtype=torch.int64, device=dev)
        area = torch.empty((r, r), dtype=torch.int64, device=dev)
        n_used = torch.empty(1, dtype=torch.int64, device=dev)
        n = start.numel()
        pixels.rescale_into(d_band, nrows, ncols, r, start.data_ptr() if n else None, end.data_ptr() if n else None,
                            n, pile.data_ptr(), area.data_ptr(), n_used.data_ptr(), bin_offset, stream,
                            device=self.device)
        return pile, area, n_used

    def sample_tensors(self, interval_id, frac, seed, salt=0, bin_offset=0, rest=False, stream=None):
        """The interval's matrix at the fraction `frac` of its depth: every contact is kept with
        probability floor(frac * 2^32) / 2^32, independently (binomial thinning, the default mode of
        `cooltools random-sample`: the total is random around its target, not equal to it).  Returns the
        kept band as a torch int32 tensor of nrows * ncols + 1 words on the simulator's device, in the
        band's layout; with `rest` the pair (kept, rest), rest = band - kept, two disjoint
        pseudo-replicates.  Trial t of pixel (i, j) is decided by the Philox word keyed by (i + bin_offset,
        j + bin_offset, t, salt) and `seed` (pixels.sample_pixels states it on the host): the same seed at
        a larger fraction keeps a superset, another salt draws anew.  Only the band's statistics cross to
        the host (the call waits for them); the kernel is enqueued on `stream` and not waited for.  A
        tensor is a band like the interval's own, and its data_ptr() goes where that goes:

            kept = sim.sample_tensors(iid, 0.25, seed=1)
            d_band, _, nrows, ncols = sim.outputs(iid)
            tiles = torch.empty((n, 256, 256), dtype=torch.int32, device=kept.device)
            pixels.dense_tiles_into(kept.data_ptr(), nrows, ncols, 0, 256, 128, n, tiles.data_ptr(), tiles.numel())
            pixels.marginals_into(kept.data_ptr(), nrows, ncols, 0, diag_sum.data_ptr(), coverage.data_ptr())
            pixels.pileup_into(kept.data_ptr(), nrows, ncols, flank, bin1.data_ptr(), bin2.data_ptr(), len(bin1),
                               pile.data_ptr())"""
        import torch

        from . import pixels

        d_band, _, nrows, ncols = self.outputs(interval_id)
        threshold = pixels.sample_threshold(frac)
        ex = pixels.extractor(self.device)
        stats = ex.count(d_band, nrows, ncols, stream=stream)
        dev = torch.device("cuda", self.device)
        kept = torch.empty(nrows * ncols + 1, dtype=torch.int32, device=dev)
        others = torch.empty(nrows * ncols + 1, dtype=torch.int32, device=dev) if rest else None
        ex.sample_into(d_band, nrows, ncols, threshold, seed, stats, kept.data_ptr(),
                       None if others is None else others.data_ptr(), salt, bin_offset, stream)
        return (kept, others) if rest else kept

    def sample(self, interval_id, frac, seed, salt=0, bin_offset=0, rest=False):
        """The non-zero pixels of the interval's matrix at the fraction `frac` of its depth, a
        pixels.Pixels like pixels() returns, with `bin_offset` added to the ids; with `rest` the pair
        (kept, rest) of two disjoint matrices that add up to the interval's.  Drawn on the device as
        sample_tensors() describes, from one draw; only the pixels cross to the host.  Call it after
        wait()."""
        from . import pixels

        d_band, _, nrows, ncols = self.outputs(interval_id)
        if not rest:
            return pixels.sample(d_band, nrows, ncols, pixels.sample_threshold(frac), seed, salt, bin_offset,
                                 device=self.device)
        bands = self.sample_tensors(interval_id, frac, seed, salt, bin_offset, rest=True)
        return tuple(pixels.extract(t.data_ptr(), nrows, ncols, bin_offset, device=self.device) for t in bands)

    def _band_pair(self, interval_id, other, other_id, factor, first_bin, other_factor, other_first_bin, stream):
        """(d_ref, d_tgt, nrows, ncols, what keeps them alive) for the stripe analyses: the band `other_id` of
        `other` is the reference and this object's `interval_id` the target, each through _band.  ValueError
        when the two lie on different devices or differ in shape."""
        if int(other.device) != int(self.device):
            raise ValueError(f"stripes: the reference lies on device {other.device}, the band on {self.device}")
        d_tgt, nrows, ncols, keep = self._band(interval_id, factor, first_bin, stream)
        d_ref, nr, nc, other_keep = other._band(other_id, other_factor, other_first_bin, stream)
        if (nr, nc) != (nrows, ncols):
            raise ValueError(f"stripes: the reference is a band of {nr} diagonals and {nc} bins, the band has "
                             f"{nrows} and {ncols}")
        return d_ref, d_tgt, nrows, ncols, (keep, other_keep)

    def stripe_moments(self, interval_id, other, other_id, what=1, factor=1, first_bin=0, other_factor=1,
                       other_first_bin=0, stream=None):
        """The interval compared stripe by stripe with band `other_id` of `other` (any owner of bands on the
        same device, a Simulator or a LoadedBands; this object itself serves): numpy uint64 [2,
        pixels.stripes_rows(what), ncols], for the vertical and the horizontal stripe of every bin the integer
        sums pixels.STRIPES_MOMENTS, _MASKED and _RANKS select (include/modle_pixels.h), formed on the device
        from the two bands where they lie (pixels.stripes).  `other` is the reference (a), the interval the
        target (b), as in evaluate.compare(ref, tgt).  Either side is first coarsened on the device when its
        factor is above 1 (`first_bin` as for pixels()); the two shapes must then be equal, else ValueError.
        Only the sums cross to the host.  Call it after wait()."""
        from . import pixels

        d_ref, d_tgt, nrows, ncols, keep = self._band_pair(interval_id, other, other_id, factor, first_bin,
                                                           other_factor, other_first_bin, stream)
        out = pixels.extractor(self.device).stripes(d_ref, d_tgt, nrows, ncols, what, stream)  # (waits)
        del keep
        return out

    def stripe_scores(self, interval_id, other, other_id, metric, exclude_zero_pixels=False, factor=1, first_bin=0,
                      other_factor=1, other_first_bin=0, stream=None):
        """(vertical, horizontal): the `metric` (pearson, spearman, rmse, eucl_dist) of every bin's stripes
        against the reference, two numpy float64 [ncols], what evaluate.compare(ref, tgt, ...) gives for the
        two directions: pixels.stripe_scores of stripe_moments with the blocks the metric needs.
        `exclude_zero_pixels`: over the entries that are non-zero in both; there is no such spearman."""
        from . import pixels

        if metric == "spearman" and exclude_zero_pixels:
            raise ValueError("stripe_scores: spearman without the zero pixels has ranks that are no integers; "
                             "evaluate.compare forms it on the host")
        what = pixels.STRIPES_MASKED if exclude_zero_pixels else pixels.STRIPES_MOMENTS
        if metric == "spearman":
            what |= pixels.STRIPES_RANKS
        rows = self.stripe_moments(interval_id, other, other_id, what, factor, first_bin, other_factor,
                                   other_first_bin, stream)
        return tuple(pixels.stripe_scores(rows[d], metric, exclude_zero_pixels) for d in (0, 1))

    def stripe_moments_tensor(self, interval_id, other, other_id, what=1, factor=1, first_bin=0, other_factor=1,
                              other_first_bin=0, stream=None):
        """The sums of stripe_moments as one torch int64 tensor [2, rows, ncols] on the device, filled there
        by the kernels: nothing crosses to the host.  The words hold the uint64 sums bit for bit.  The work is
        enqueued on `stream` (None: the default stream, on which torch orders its own work); it is waited
        for only when a side was coarsened into a scratch band, which goes when this returns."""
        import torch

        from . import pixels

        d_ref, d_tgt, nrows, ncols, keep = self._band_pair(interval_id, other, other_id, factor, first_bin,
                                                           other_factor, other_first_bin, stream)
        out = torch.empty((2, pixels.stripes_rows(what), ncols), dtype=torch.int64,
                          device=torch.device("cuda", self.device))
        pixels.stripes_into(d_ref, d_tgt, nrows, ncols, what, out.data_ptr(), out.numel(), stream,
                            device=self.device)
        if any(k is not None for k in keep):
            torch.cuda.synchronize(out.device)
        return out

    def scc_moments(self, interval_id, other, other_id, smooth=0, min_diag=1, max_diag=None, factor=1, first_bin=0,
                    other_factor=1, other_first_bin=0, stream=None):
        """The interval compared diagonal by diagonal with band `other_id` of `other` (the reference, as in
        stripe_moments): numpy uint64 [pixels.SCC_ROWS, nrows], per stratum min_diag <= d <= max_diag of the two
        matrices smoothed by a box of half-width `smooth` bins the number of entries that are non-zero in
        either and the 128-bit sums of a, b, a * a, b * b and a * b (include/modle_pixels.h), formed on the
        device from the two bands where they lie (pixels.scc); the other columns hold 0.  `max_diag` None:
        the widest the band allows, nrows - 1 - 2 * smooth.  Either side is first coarsened on the device when
        its factor is above 1; the two shapes must then be equal, else ValueError.  HiCRep compares at equal
        depth: sample the deeper band first (sample_tensors).  Only the sums cross to the host.  Call it after
        wait()."""
        from . import pixels

        d_ref, d_tgt, nrows, ncols, keep = self._band_pair(interval_id, other, other_id, factor, first_bin,
                                                           other_factor, other_first_bin, stream)
        out = pixels.extractor(self.device).scc(d_ref, d_tgt, nrows, ncols, smooth, min_diag, max_diag,
                                                stream)  # (waits)
        del keep
        return out

    def scc(self, interval_id, other, other_id, smooth=0, min_diag=1, max_diag=None, include_zeros=False, factor=1,
            first_bin=0, other_factor=1, other_first_bin=0, stream=None):
        """(scc, rho, weight): HiCRep's stratum-adjusted correlation coefficient of the interval against the
        reference, the correlation of every stratum and its weight: pixels.scc_scores of scc_moments.
        `include_zeros`: a stratum counts all its entries, not only those that are non-zero in either matrix."""
        from . import pixels

        rows = self.scc_moments(interval_id, other, other_id, smooth, min_diag, max_diag, factor, first_bin,
                                other_factor, other_first_bin, stream)
        _, _, nrows, ncols = self.outputs(interval_id)
        nrows, ncols = pixels.band_shape(nrows, ncols, factor, first_bin)
        hi = nrows - 1 - 2 * int(smooth) if max_diag is None else int(max_diag)
        return pixels.scc_scores(rows, ncols, min_diag, hi, include_zeros)

    def scc_moments_tensor(self, interval_id, other, other_id, smooth=0, min_diag=1, max_diag=None, factor=1,
                           first_bin=0, other_factor=1, other_first_bin=0, stream=None):
        """The sums of scc_moments as one torch int64 tensor [pixels.SCC_ROWS, nrows] on the device, filled there
        by the kernels: nothing crosses to the host.  The words hold the uint64 sums bit for bit.  The work is
        enqueued on `stream` (None: the default stream, on which torch orders its own work); it is waited
        for only when a side was coarsened into a scratch band, which goes when this returns."""
        import torch

        from . import pixels

        d_ref, d_tgt, nrows, ncols, keep = self._band_pair(interval_id, other, other_id, factor, first_bin,
                                                           other_factor, other_first_bin, stream)
        if max_diag is None:
            max_diag = nrows - 1 - 2 * int(smooth)
        out = torch.empty((pixels.SCC_ROWS, nrows), dtype=torch.int64, device=torch.device("cuda", self.device))
        pixels.scc_into(d_ref, d_tgt, nrows, ncols, smooth, min_diag, max_diag, out.data_ptr(), out.numel(), stream,
                        device=self.device)
        if any(k is not None for k in keep):
            torch.cuda.synchronize(out.device)
        return out

    def stripe_profiles(self, interval_id, max_offset, lengths, min_diag=None, factor=1, first_bin=0, stream=None):
        """The cross-sections of every bin's stripes: (profiles, n_valid), numpy uint64 [2, K, 2 m + 1, ncols].
        profiles[0][k][o + m][c] is the sum of the stripe that runs upstream of bin c, the cells M(c - d, c + o) at
        the distances min_diag <= d < lengths[k], seen o bins to the side; profiles[1] that of the stripe
        downstream, M(c + o, c + d) (include/modle_pixels.h), formed on the device from the band where it lies
        (pixels.stripe_profiles); n_valid the number of cells of each inside the chromosome.  `min_diag` None:
        the smallest the call accepts, max(max_offset, 1).  pixels.PROFILE_RULE is the accepted call.  Call it after
        wait().  With `factor` > 1 the band is first coarsened on the device (`first_bin` as for pixels()) and
        the lengths, the offset and `min_diag` count coarse bins."""
        from . import pixels

        if min_diag is None:
            min_diag = max(int(max_offset), 1)
        d_band, _, nrows, ncols = self.outputs(interval_id)
        prof = pixels.extractor(self.device).stripe_profiles(d_band, nrows, ncols, max_offset, lengths, min_diag, stream,
                                                             factor, first_bin)
        return prof, pixels.stripe_profile_n_valid(prof.shape[3], max_offset, lengths, min_diag)

    def stripe_profiles_tensor(self, interval_id, max_offset, lengths, min_diag=None, stream=None):
        """The sums of stripe_profiles as one torch int64 tensor [2, K, 2 m + 1, ncols] on the device, filled there
        by the kernels: nothing crosses to the host.  The words hold the uint64 sums bit for bit (they are below
        2^56).  The work is enqueued on `stream` (None: the default stream, on which torch orders its own work)
        and not waited for."""
        import torch

        from . import pixels

        if min_diag is None:
            min_diag = max(int(max_offset), 1)
        d_band, _, nrows, ncols = self.outputs(interval_id)
        out = torch.empty((2, len(lengths), 2 * int(max_offset) + 1, ncols), dtype=torch.int64,
                          device=torch.device("cuda", self.device))
        pixels.stripe_profiles_into(d_band, nrows, ncols, max_offset, lengths, min_diag, out.data_ptr(), out.numel(),
                                    stream, device=self.device)
        return out

    def call_stripes(self, interval_id, max_offset, lengths, min_diag=None, half_width=0, fold=None, min_count=None,
                     radius=None, factor=1, first_bin=0):
        """The stripes of the interval, a list of StripeRow sorted by (direction, bin): stripe_rows of
        stripe_profiles and of the sums per diagonal (marginals), both formed on the device; the decision is
        pixels.stripe_calls.  Direction 0: the stripe runs upstream of its anchor bin, 1: downstream."""
        if min_diag is None:
            min_diag = max(int(max_offset), 1)
        prof, _ = self.stripe_profiles(interval_id, max_offset, lengths, min_diag, factor, first_bin)
        diag_sum, _ = self.marginals(interval_id, 0, factor, first_bin)
        return stripe_rows(prof, diag_sum, max_offset, lengths, min_diag, half_width, fold, min_count, radius)

    def triangle_sums(self, interval_id, max_width, min_diag=0, factor=1, first_bin=0, stream=None):
        """The triangle table of the interval, numpy uint64 [max_width, ncols]: T[k][s] is the sum of the contacts
        inside the window of k + 1 bins that starts at bin s (the pixels (a, c), s <= a <= c < min(s + k + 1, ncols),
        without the diagonals below `min_diag`; include/modle_pixels.h), formed on the device from the band where it
        lies (pixels.triangles_to_host).  pixels.TRIANGLE_RULE is the accepted call, pixels.triangle_cells the number
        of pixels behind every word.  Call it after wait().  With `factor` > 1 the band is first coarsened on the
        device (`first_bin` as for pixels()) and the widths and `min_diag` count coarse bins."""
        from . import pixels

        d_band, _, nrows, ncols = self.outputs(interval_id)
        return pixels.extractor(self.device).triangles_to_host(d_band, nrows, ncols, max_width, min_diag, stream,
                                                               factor, first_bin)

    def triangle_sums_tensor(self, interval_id, max_width, min_diag=0, stream=None):
        """The table of triangle_sums as one torch int64 tensor [max_width, ncols] on the device, filled there by
        the kernels: nothing crosses to the host (the objective or the feature map of a fitting loop).  The words
        hold the uint64 sums bit for bit.  The work is enqueued on `stream` (None: the default stream, on which
        torch orders its own work) and not waited for."""
        import torch

        from . import pixels

        d_band, _, nrows, ncols = self.outputs(interval_id)
        out = torch.empty((int(max_width), ncols), dtype=torch.int64, device=torch.device("cuda", self.device))
        pixels.triangles_into(d_band, nrows, ncols, max_width, min_diag, out.data_ptr(), out.numel(), stream,
                              device=self.device)
        return out

    def call_domains(self, interval_id, max_width, min_diag=0, gamma=None, min_width=None, factor=1, first_bin=0):
        """The domains of the interval, a list of pixels.DomainCall sorted by start (bins [start, end) of `factor`
        times the bin size): pixels.domain_calls of triangle_sums, formed on the device, and of
        pixels.triangle_cells.  None for `gamma`, `min_width`: the defaults of pixels.domain_calls.  ValueError
        when a sum reaches 2^53."""
        from . import pixels

        table = self.triangle_sums(interval_id, max_width, min_diag, factor, first_bin)
        options = {name: v for name, v in (("gamma", gamma), ("min_width", min_width)) if v is not None}
        return pixels.domain_calls(table, pixels.triangle_cells(table.shape[1], max_width, min_diag), **options)


# ---------------------------------------------------------------------------------------------
# device path
# ---------------------------------------------------------------------------------------------
class Simulator(BandAnalyses):
    """One simulation context bound to one GPU (one process per GPU)."""

    def __init__(self, cfg, device=0):
        err = _errbuf()
        self._L = lib()
        self.cfg = cfg
        self.device = int(device)
        self._h = self._L.modle_hip_create(C.byref(cfg), device, err, len(err))
        if not self._h:
            raise ModleHipError(f"modle_hip_create failed: {err.value.decode(errors='replace')}")
        self._n_submitted = {}

    def close(self):
        if self._h:
            self._L.modle_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self._L.modle_hip_reset(self._h)
        self._n_submitted = {}

    def add_interval(self, start, end, bar_pos, bar_dir, stp_active, stp_inactive,
                     d_contacts=None, d_occupancy=None):
        err = _errbuf()
        rc = self._L.modle_hip_add_interval(
            self._h, start, end, np.ascontiguousarray(bar_pos, dtype=np.uint64),
            np.ascontiguousarray(bar_dir, dtype=np.uint8),
            np.ascontiguousarray(stp_active, dtype=np.float64),
            np.ascontiguousarray(stp_inactive, dtype=np.float64), len(bar_pos), d_contacts,
            d_occupancy, err, len(err))
        iv = _check(rc, err)
        self._n_submitted[iv] = 0
        return iv

    def submit(self, interval_id, tasks):
        err = _errbuf()
        _check(self._L.modle_hip_submit_tasks(self._h, interval_id, tasks, len(tasks), err,
                                              len(err)), err)
        self._n_submitted[interval_id] += len(tasks)

    def launch(self, stream=None):
        err = _errbuf()
        _check(self._L.modle_hip_launch(self._h, stream, err, len(err)), err)

    def wait(self):
        """collects the launch; raises ModleHipError with code ERR_TIMEOUT when the launch ran into
        the deadline (set_wait_timeout / MODLE_HIP_WAIT_TIMEOUT_S) and was aborted"""
        err = _errbuf()
        _check(self._L.modle_hip_wait(self._h, err, len(err)), err)

    def set_wait_timeout(self, seconds):
        if self._L.modle_hip_set_wait_timeout(self._h, float(seconds)) < 0:
            raise ModleHipError("modle_hip_set_wait_timeout: the deadline must be positive", ERR_ARG)

    def launch_info(self):
        """layout of the last launch (modle_hip_launch_info) as a dict"""
        info = LaunchInfo()
        if self._L.modle_hip_last_launch_info(self._h, C.byref(info)) < 0:
            raise ModleHipError("modle_hip_last_launch_info failed")
        return {name: int(getattr(info, name)) for name, _ in LaunchInfo._fields_}

    def enable_state_log(self, max_epochs_per_task):
        """--log-model-internal-state: needs the diagnostic build (MODLE_HIP_LIB=
        libmodle_hip_statelog.so); the default build refuses"""
        err = _errbuf()
        _check(self._L.modle_hip_enable_state_log(self._h, int(max_epochs_per_task), err, len(err)), err)
        self._state_log_cap = int(max_epochs_per_task)

    def state_log(self, interval_id, task_index):
        """records of one task of the last launch: uint64 array (n_epochs, 10), see
        MODLE_HIP_STATE_LOG_WORDS in include/modle_hip.h"""
        cap = getattr(self, "_state_log_cap", 0)
        rec = np.zeros((cap, 10), dtype=np.uint64)
        n = C.c_size_t(0)
        err = _errbuf()
        _check(self._L.modle_hip_get_state_log(self._h, interval_id, task_index, rec.ctypes.data, cap,
                                               C.byref(n), err, len(err)), err)
        return rec[:n.value]

    def interval_done(self, interval_id):
        """True when the launch in flight has finished every task of this interval."""
        rc = self._L.modle_hip_interval_done(self._h, interval_id)
        if rc < 0:
            raise ModleHipError(f"modle_hip_interval_done failed: {rc}")
        return rc == 1

    def cancel(self):
        err = _errbuf()
        _check(self._L.modle_hip_cancel(self._h, err, len(err)), err)

    def kernel_ms(self):
        ms = C.c_float(0)
        self._L.modle_hip_last_kernel_ms(self._h, C.byref(ms))
        return ms.value

    def results(self, interval_id):
        n = self._n_submitted[interval_id]
        res = (CellResult * n)()
        rc = self._L.modle_hip_get_results(self._h, interval_id, res, n)
        if rc < 0:
            raise ModleHipError(f"modle_hip_get_results failed: {rc}")
        return res

    def outputs(self, interval_id):
        dc, do = C.c_void_p(), C.c_void_p()
        nr, nc = C.c_uint64(), C.c_uint64()
        self._L.modle_hip_interval_outputs(self._h, interval_id, C.byref(dc), C.byref(do),
                                           C.byref(nr), C.byref(nc))
        return dc.value, do.value, nr.value, nc.value

    def copy_outputs(self, interval_id, want_contacts=True):
        _, d_occ, nrows, ncols = self.outputs(interval_id)
        contacts = np.zeros(nrows * ncols + 1, dtype=np.uint32) if want_contacts else None
        occ = np.zeros(ncols, dtype=np.uint64) if d_occ else None
        missed = C.c_uint64(0)
        err = _errbuf()
        _check(self._L.modle_hip_copy_outputs(
            self._h, interval_id, contacts.ctypes.data if contacts is not None else None,
            C.byref(missed), occ.ctypes.data if occ is not None else None, err, len(err)), err)
        return contacts, missed.value, occ

    def simulate_interval(self, start, end, bar_pos, bar_dir, stp_active, stp_inactive, tasks):
        """One-call seam (modle_hip_simulate_interval): returns contacts, missed, occupancy,
        results."""
        nrows, ncols = matrix_shape(self.cfg, end - start)
        contacts = np.zeros(nrows * ncols + 1, dtype=np.uint32)
        occ = np.zeros(ncols, dtype=np.uint64)
        missed = C.c_uint64(0)
        res = (CellResult * len(tasks))()
        err = _errbuf()
        _check(self._L.modle_hip_simulate_interval(
            self._h, start, end, np.ascontiguousarray(bar_pos, dtype=np.uint64),
            np.ascontiguousarray(bar_dir, dtype=np.uint8),
            np.ascontiguousarray(stp_active, dtype=np.float64),
            np.ascontiguousarray(stp_inactive, dtype=np.float64), len(bar_pos), tasks, len(tasks),
            contacts, nrows, ncols, C.byref(missed), occ.ctypes.data, res, err, len(err)), err)
        return contacts, missed.value, occ, res

    def test_units(self, what, pairs, nrows=0, ncols=0, contacts=None, missed=0, out=None):
        """Unit-level entry point (modle_hip_test_units); returns (out words, contacts, missed).
        `out`: a contiguous uint64 array of 2 n words of the caller's (a window of a larger, guarded one)."""
        pairs = np.ascontiguousarray(pairs, dtype=np.uint64).reshape(-1)
        n = len(pairs) // 2
        if out is None:
            out = np.zeros(2 * n, dtype=np.uint64)
        if out.dtype != np.uint64 or out.shape != (2 * n,) or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous uint64 array of 2 n words")
        m = C.c_uint64(missed)
        err = _errbuf()
        _check(self._L.modle_hip_test_units(
            self._h, what, pairs, n, nrows, ncols,
            contacts.ctypes.data if contacts is not None else None, C.byref(m), out, err,
            len(err)), err)
        return out, contacts, m.value

    def test_phases(self, mask, st, prng_state):
        """Phase-level entry point (mirrors Simulation::test_* hooks) on KatState-like arrays."""
        prng = (C.c_uint64 * 4)(*prng_state)
        consumed = C.c_uint64(0)
        err = _errbuf()
        _check(self._L.modle_hip_test_phases(
            self._h, mask, st.start, st.end, st.n, st.rev_pos, st.fwd_pos, st.epoch, st.rev_rank,
            st.fwd_rank, st.rev_moves, st.fwd_moves, st.rev_coll, st.fwd_coll, len(st.bar_pos),
            st.bar_pos, st.bar_dir, st.bar_active, prng, C.byref(consumed), err, len(err)), err)
        return consumed.value


class LoadedBands(BandAnalyses):
    """Bands that were not simulated: every analysis of BandAnalyses on a band built on the device from a
    pixel list (a cooler's: cooler.CoolerReader.pixels) or on a band that already lies there.  The ids count
    from 0 in the order of loading, so that driver.write_outputs takes this object where it takes a
    Simulator."""

    def __init__(self, device=0):
        self.device = int(device)
        self._bands = []  # (tensor, nrows, ncols)

    def load_pixels(self, bin1, bin2, count, nrows, ncols, bin_offset=0):
        """(id, stats): the band of `nrows` diagonals and `ncols` columns of the host pixels (bin1[t] -
        bin_offset, bin2[t] - bin_offset) with count[t] contacts, a torch int32 tensor of nrows * ncols + 1
        words on the device, filled there by the kernel (pixels.band_from_host): only the pixels cross.  The
        list must be strictly increasing in (bin1, bin2), else pixels.BandListError; the pixels beyond the
        band and outside the matrix are counted in `stats` (pixels.BandStats) and left out.  The band is then
        counted by the extraction's own kernel, which must agree with the statistics of the list."""
        import torch

        from . import pixels

        nrows, ncols = int(nrows), int(ncols)
        band = torch.empty(nrows * ncols + 1, dtype=torch.int32, device=torch.device("cuda", self.device))
        ex = pixels.extractor(self.device)
        stats = ex.band_from_host(bin1, bin2, count, nrows, ncols, bin_offset, band.data_ptr(), band.numel())
        seen = ex.count(band.data_ptr(), nrows, ncols)
        if (seen.nnz, seen.sum, seen.max_count) != (stats.nnz_in, stats.sum_in, stats.max_count):
            raise ModleHipError(f"load_pixels: the band holds {seen.nnz} pixels, {seen.sum} contacts and a maximum of "
                                f"{seen.max_count}; the list has {stats.nnz_in}, {stats.sum_in} and {stats.max_count}")
        return self.add_band(band, nrows, ncols), stats

    def add_band(self, tensor, nrows, ncols):
        """the id of a band that already lies on the device: a contiguous torch int32 tensor of at least
        nrows * ncols + 1 words in the band's layout (sample_tensors' result, for one)"""
        import torch

        if tensor.dtype != torch.int32 or tensor.device != torch.device("cuda", self.device) or \
                not tensor.is_contiguous() or tensor.numel() < int(nrows) * int(ncols) + 1:
            raise ValueError("add_band: the band must be a contiguous int32 tensor of nrows * ncols + 1 words on "
                             "this object's device")
        self._bands.append((tensor, int(nrows), int(ncols)))
        return len(self._bands) - 1

    def band(self, band_id):
        return self._bands[band_id][0]

    def release(self, band_id):
        """lets go of the band; the id is not used again"""
        self._bands[band_id] = None

    def outputs(self, band_id):
        tensor, nrows, ncols = self._bands[band_id]
        return tensor.data_ptr(), None, nrows, ncols

    def copy_outputs(self, band_id, want_contacts=False):
        """(None, 0, None): a loaded band has no dense host copy, no missed updates and no occupancy"""
        if want_contacts:
            raise ModleHipError("copy_outputs: a loaded band is not copied to the host; use pixels()")
        return None, 0, None

    def close(self):
        self._bands = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
