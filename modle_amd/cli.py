"""`modle simulate`-shaped front end over the C ABI.

    python -m modle_amd simulate -c hg38.chrom.sizes -b barriers.bed.xz -o out/prefix [options]

Option names, defaults and the derivation of the dependent parameters follow the reference's
`modle simulate` (reference: src/modle/cli.cpp:53-602 options, :886-1016 transform_args); the
task derivation is `run_simulate`'s (src/libmodle/cpu/scheduler_simulate.cpp:43-170) and the
outputs are the reference's: `<prefix>.cool` (with --mcool-resolutions `<prefix>.mcool`: the same
contacts at several bin sizes, coarsened on the GPU) and, with the 1-D LEF position track on,
`<prefix>_lef_1d_occupancy.bw` (cli.cpp:867-882); with --dense-region also `<prefix>_dense.npz`, the
square matrices of the named regions, unpacked on the GPU; with --expected `<prefix>_expected.tsv`, the
contacts per diagonal, and with --coverage `<prefix>_coverage.bedgraph`, the contacts per bin, both
summed on the GPU; with --insulation-windows `<prefix>_insulation.tsv`, the insulation sums and scores
per bin over sliding diamond windows, summed on the GPU; with --dots `<prefix>_dots.bedpe`, the pixels
enriched over their four HiCCUPS neighbourhoods, found on the GPU; with --pileup-at `<prefix>_pileup.tsv`,
the windows around the dots, the barriers or the pairs of a BEDPE file, summed on the GPU; with
--subsample-frac or --subsample-to `<prefix>_sampled.cool`, the matrix with every contact kept with one
probability, drawn on the GPU (with --subsample-split also `<prefix>_sampled_rest.cool`, the others); with
--compare-to REF.cool (or REF.mcool::/resolutions/R) `<prefix>_stripes.tsv`, every bin's vertical and
horizontal stripe scored against the reference file the way `evaluate` scores them, from integer sums formed
on the GPU: --compare-metrics LIST (pearson, spearman, rmse, eucl_dist; default pearson), --compare-resolution
R (a multiple of -r, the bin size of REF; default -r) and --compare-exclude-zero-pixels (not with spearman);
with --compare-to REF --scc also `<prefix>_scc.tsv`, per interval the stratum-adjusted correlation coefficient
of HiCRep against the reference and the correlation of every diagonal, from integer sums formed on the GPU, at
the bin size of the comparison: --scc-smooth D (the half-width of the smoothing box, a whole number of bins, at
most 20; default 0), --scc-max-distance D (the last diagonal, a whole number of bins; default and at most the
widest the band allows with that smoothing), --scc-ignore-diags N (the first diagonal; default 1, HiCRep's
excluded main diagonal) and --scc-include-zeros (a diagonal counts all its pixels, not only those that are
non-zero in either matrix).  HiCRep compares at equal depth: sample the deeper matrix first (--subsample-to).
The score is the one pixels.scc_scores states, modelled on the Python package `hicrep`, not a run of it.
With --dots --dots-fdr Q (0 < Q < 1) the dots also pass the statistical test of HiCCUPS: every pixel is binned by
its locally adjusted expected count into --dots-lambda-chunks N (1 to 63, default 40) logarithmic chunks, the
counts of every chunk are histogrammed over all intervals on the GPU, a Poisson tail under the Benjamini-Hochberg
rule at the rate Q gives every chunk a count threshold (`<prefix>_dots_thresholds.tsv`), and a dot must clear the
threshold of its chunk for all four neighbourhoods; the fold test of --dots-folds stays on.
With --domains-at FILE.bed (three columns; may be given several times) `<prefix>_domains.tsv`, the average domain:
every domain of the file, padded by --domains-flank-percent P (0 to 200, default 100) of its own bins on either
side, is cut into --domains-size N (1 to 128, default 60) blocks a side, and the blocks of all of them are summed
on the GPU into one N x N pile with the number of source pixels of every cell, at --domains-resolution R (a
multiple of -r, coarsened on the GPU; default -r); the file also holds what the distance-decay curve expects of
every cell and the strength of the average domain (api.domain_strength).  observed / area is the pooled mean of a
cell, in which large domains weigh more: it is not the mean of per-domain interpolations of coolpup.py --rescale.
With --call-stripes `<prefix>_stripe_calls.bedpe`, the architectural stripes of every interval: for every bin the
stripe that runs upstream and the one that runs downstream of it are summed on the GPU at the --call-stripes-lengths
LIST (1 to 4, default 200kb,400kb,800kb) together with their cross-section, the same sums up to --call-stripes-flank
D (at most 8 bins; default 50kb) to either side, and a bin is called at the longest length at which its centre of
--call-stripes-width D (an odd number of bins, default one) holds at least --call-stripes-min-count N contacts
(default 1) and its mean is at least --call-stripes-fold F (default 1.5) times the mean of either shoulder; the
calls of one direction are thinned to the best within --call-stripes-radius D (default: the flank).
--call-stripes-ignore-diags N leaves out the first N diagonals (default and at least the bins of the flank, 2 at
least) and --call-stripes-resolution R (a multiple of -r, coarsened on the GPU; default -r) sets the bin size.  The
fold, the count and the radius are choices, not measured optima; the rule is pixels.stripe_calls', not Stripenn's.
With --call-domains `<prefix>_domain_calls.bed` (chrom, start, end, name, score, strength), the domains of every
interval: the contacts inside every window on the diagonal, of every start and every width up to
--call-domains-max-width D (default 2mb, clamped to the band), are summed on the GPU into one table, and the
disjoint windows of at least --call-domains-min-width D (default 3 bins) are called that maximise the sum of
their contacts less --call-domains-gamma G (default 1) times the mean of the chromosome's windows of their width
(pixels.domain_calls; the strength is the window over that mean).  --call-domains-ignore-diags N leaves out the
first N diagonals (default 2) and --call-domains-resolution R (a multiple of -r, coarsened on the GPU; default -r)
sets the bin size.  With --call-domains, and only then, `--domains-at called` averages the domains just called.
The rule is the project's own, neither Armatus' exponent nor a p-value, and its defaults are choices.
Everything heavy is native: parsing and
task generation in libmodle_hip.so (host), the simulation on the MI355X (one process per GPU;
under torch.distributed.run the cells are sharded over the ranks and the matrices are summed
with RCCL, or with --dist-backend gloo on host copies), the writers in libmodle_cooler.so.  `-t/--threads` is accepted and ignored.

    python -m modle_amd analyze IN.cool | IN.mcool::/resolutions/R -o out/prefix [-w 3mb] [analysis options]

runs the same analyses on the matrix of a file: its pixels are read by libmodle_cooler.so, scattered into band
matrices on the GPU (libmodle_pixels.so) and handed to the output stage of `simulate` as they are."""
import argparse
import collections
import decimal
import json
import os
import sys
import time

from . import api, driver, genome, pixels
from .params import CS_LOOP, CS_NOISIFY, CS_TAD

STRATEGIES = {  # cli.hpp:63-72
    "tad-only": CS_TAD, "loop-only": CS_LOOP, "tad-plus-loop": CS_TAD | CS_LOOP,
    "tad-only-with-noise": CS_TAD | CS_NOISIFY, "loop-only-with-noise": CS_LOOP | CS_NOISIFY,
    "tad-plus-loop-with-noise": CS_TAD | CS_LOOP | CS_NOISIFY,
}


_DISTANCE_UNITS = {"bp": 1, "k": 10**3, "kb": 10**3, "kbp": 10**3, "m": 10**6, "mb": 10**6,
                   "mbp": 10**6, "g": 10**9, "gb": 10**9, "gbp": 10**9}  # cli_utils.hpp:86-96


def genomic_distance(text):
    """`20kb`, `1.5Mbp`, `3000000`: a number of base pairs with an optional unit, the reference's
    AsGenomicDistance transform (src/common/cli_utils_impl.hpp:304-362; the unit is case
    insensitive and the product must be a whole number).  The reference multiplies in double and so
    refuses `1.025mb` (1024999.9999999999); a product that is whole in exact decimal arithmetic is
    accepted here as well."""
    k = len(text)
    while k > 0 and text[k - 1].isalpha():
        k -= 1
    num, unit = text[:k], text[k:].lower()
    if not num:
        raise argparse.ArgumentTypeError(f"value {text} could not be converted")
    if not unit:
        try:
            v = int(num)
        except ValueError:
            raise argparse.ArgumentTypeError(f"unable to convert {text} to a number")
        if v < 0:
            raise argparse.ArgumentTypeError(f"unable to convert {text} to a number")
        return v
    if unit not in _DISTANCE_UNITS:
        raise argparse.ArgumentTypeError(f"{text[k:]} unit not recognized; valid units: "
                                         + ", ".join(sorted(_DISTANCE_UNITS)))
    try:
        m = float(num) * _DISTANCE_UNITS[unit]
    except ValueError:
        raise argparse.ArgumentTypeError(f"unable to convert {num} to a number")
    if m != m or m in (float("inf"), float("-inf")):
        raise argparse.ArgumentTypeError(f"unable to convert {num} to a number")
    if m != int(m):
        try:
            exact = decimal.Decimal(num) * _DISTANCE_UNITS[unit]
        except decimal.InvalidOperation:
            exact = None
        if exact is not None and exact == exact.to_integral_value():
            m = int(exact)
    if m != int(m) or m < 0:
        raise argparse.ArgumentTypeError(f"Unable to convert {text} to a number of base-pairs "
                                         f"({m} is not an integral number)")
    return int(m)


def resolution_list(text):
    """`10kb,25kb,100kb`: comma-separated genomic distances (--mcool-resolutions)"""
    items = [t.strip() for t in text.split(",")]
    if not text.strip() or any(not t for t in items):
        raise argparse.ArgumentTypeError(f"{text!r} is not a comma-separated list of resolutions")
    return [genomic_distance(t) for t in items]


# the limits and defaults of the library, under the names the front end uses (importing pixels loads nothing)
MAX_INSULATION_WINDOWS, MAX_INSULATION_WINDOW_BINS = pixels.MAX_WINDOWS, pixels.MAX_WINDOW
MAX_DOT_WINDOW_BINS, MAX_PILEUP_FLANK_BINS = pixels.MAX_DOT_WINDOW, pixels.MAX_PILEUP_FLANK
MAX_SCC_SMOOTH_BINS = pixels.MAX_SCC_SMOOTH
DOT_FOLDS, COMPARE_METRICS = pixels.DOT_FOLDS, pixels.STRIPE_METRICS


def window_list(text):
    """`100kb,250kb`: comma-separated genomic distances (--insulation-windows), at most 8 of them"""
    items = [t.strip() for t in text.split(",")]
    if not text.strip() or any(not t for t in items):
        raise argparse.ArgumentTypeError(f"{text!r} is not a comma-separated list of window sizes")
    if len(items) > MAX_INSULATION_WINDOWS:
        raise argparse.ArgumentTypeError(f"{text!r} lists {len(items)} windows: at most {MAX_INSULATION_WINDOWS}")
    return [genomic_distance(t) for t in items]


def metric_list(text):
    """`pearson,rmse`: the comma-separated metrics of --compare-metrics, each once"""
    items = [t.strip() for t in text.split(",")]
    if any(t not in COMPARE_METRICS for t in items) or len(set(items)) != len(items):
        raise argparse.ArgumentTypeError(f"{text!r} is not a comma-separated list of distinct metrics of "
                                         f"{', '.join(COMPARE_METRICS)}")
    return items


def fold_list(text):
    """`1.75,1.75,1.5,1.5`: the four thresholds of --dots-folds, finite and not negative"""
    try:
        folds = [float(t) for t in text.split(",")]
    except ValueError:
        folds = []
    if len(folds) != 4 or any(not 0 <= f < float("inf") for f in folds):
        raise argparse.ArgumentTypeError(f"{text!r} is not four comma-separated non-negative numbers")
    return folds


def mcool_bin_sizes(resolutions, base):
    """the bin sizes of the .mcool: the base (-r) and the listed resolutions, sorted, without
    duplicates.  Every listed one must be a multiple of the base and larger than it."""
    base = int(base)
    for r in resolutions:
        if r <= base or r % base != 0:
            raise SystemExit(f"--mcool-resolutions: {r} is not a multiple of the resolution ({base}) "
                             "that is larger than it")
        if r >= 2**32:
            raise SystemExit(f"--mcool-resolutions: {r} does not fit the 32-bit bin size of a cooler")
    return [base] + sorted(set(resolutions))


def dense_region(text):
    """`chrom` or `chrom:start-end` (--dense-region): (chrom, None, None) or (chrom, start, end) in
    base pairs; the positions are genomic distances (`100kb`, `1.5mb`) and may carry commas"""
    if ":" not in text:
        if not text.strip():
            raise argparse.ArgumentTypeError("an empty region")
        return text, None, None
    chrom, _, span = text.rpartition(":")
    ends = span.replace(",", "").split("-")
    if not chrom or len(ends) != 2 or not ends[0] or not ends[1]:
        raise argparse.ArgumentTypeError(f"{text!r} is not chrom or chrom:start-end")
    return chrom, genomic_distance(ends[0]), genomic_distance(ends[1])


def dense_path(prefix):
    return prefix + "_dense.npz"


def expected_path(prefix):
    return prefix + "_expected.tsv"


def coverage_path(prefix):
    return prefix + "_coverage.bedgraph"


def insulation_path(prefix):
    return prefix + "_insulation.tsv"


def dots_path(prefix):
    return prefix + "_dots.bedpe"


def dots_thresholds_path(prefix):
    return prefix + "_dots_thresholds.tsv"


def pileup_path(prefix):
    return prefix + "_pileup.tsv"


def domains_path(prefix):
    return prefix + "_domains.tsv"


def stripes_path(prefix):
    return prefix + "_stripes.tsv"


def scc_path(prefix):
    return prefix + "_scc.tsv"


def stripe_calls_path(prefix):
    return prefix + "_stripe_calls.bedpe"


def domain_calls_path(prefix):
    return prefix + "_domain_calls.bed"


def sampled_paths(prefix, mcool=False):
    """(the file of the kept contacts, the file of the others) of --subsample-frac / --subsample-to"""
    ext = ".mcool" if mcool else ".cool"
    return prefix + "_sampled" + ext, prefix + "_sampled_rest" + ext


def add_analysis_arguments(io):
    """the options of the analyses of a band, which `simulate` and `analyze` share: added to the argument group
    `io` in the order of simulate's help"""
    io.add_argument("--mcool-resolutions", type=resolution_list, default=None, metavar="LIST",
                    help="write <prefix>.mcool instead of <prefix>.cool: the matrix at the resolution "
                         "(-r), which need not be listed, and at every bin size of the comma-separated "
                         "LIST (e.g. 10kb,25kb,100kb; multiples of -r), coarsened on the GPU")
    io.add_argument("--dense-region", type=dense_region, action="append", default=None, metavar="REGION",
                    help="also write <prefix>_dense.npz with the symmetric int32 matrix of REGION (chrom or "
                         "chrom:start-end, snapped outward to whole bins of -r; inside one simulated "
                         "interval), unpacked on the GPU; may be given several times")
    io.add_argument("--expected", action="store_true", default=None,
                    help="also write <prefix>_expected.tsv: the sum and the mean of the contacts per diagonal "
                         "(the distance-decay curve) of every interval, at -r and at every bin size of "
                         "--mcool-resolutions, summed on the GPU")
    io.add_argument("--coverage", action="store_true", default=None,
                    help="also write <prefix>_coverage.bedgraph: the sum of every bin's row of the symmetric "
                         "matrix at -r, summed on the GPU")
    io.add_argument("--coverage-ignore-diags", type=int, default=None, metavar="N",
                    help="with --coverage: leave out the first N diagonals (default 0)")
    io.add_argument("--insulation-windows", type=window_list, default=None, metavar="LIST",
                    help="also write <prefix>_insulation.tsv: for every bin and every window size of the "
                         "comma-separated LIST (e.g. 100kb,250kb; at most 8, multiples of the insulation "
                         "resolution, at most 1024 bins, and the diamond of 2 w - 1 diagonals must fit -w) the "
                         "sum of the contacts that cross the bin inside the sliding diamond window, the number "
                         "of pixels of the diamond and the log2 insulation score, summed on the GPU")
    io.add_argument("--insulation-resolution", type=genomic_distance, default=None, metavar="R",
                    help="with --insulation-windows: the bin size of the insulation track (a multiple of -r, "
                         "coarsened on the GPU; default -r)")
    io.add_argument("--insulation-ignore-diags", type=int, default=None, metavar="N",
                    help="with --insulation-windows: leave out the first N diagonals (default 2)")
    io.add_argument("--dots", action="store_true",
                    help="also write <prefix>_dots.bedpe: the pixels that stand out over their four HiCCUPS "
                         "neighbourhoods (donut, lower-left, horizontal, vertical) against the interval's own "
                         "distance-decay curve, found on the GPU from raw counts and thinned to local maxima")
    io.add_argument("--dots-resolution", type=genomic_distance, default=None, metavar="R",
                    help="with --dots: the bin size dots are called at (a multiple of -r, coarsened on the GPU; "
                         "default -r)")
    io.add_argument("--dots-window", type=genomic_distance, default=None, metavar="SIZE",
                    help="with --dots: the half-width of the neighbourhood window (a multiple of the dots "
                         "resolution, at most 20 bins; 4 w + 1 diagonals and the ignored ones must fit -w; "
                         "default 5 bins)")
    io.add_argument("--dots-peak", type=genomic_distance, default=None, metavar="SIZE",
                    help="with --dots: the half-width of the peak left out of the neighbourhoods (a multiple of "
                         "the dots resolution below the window; default 2 bins)")
    io.add_argument("--dots-min-count", type=int, default=None, metavar="N",
                    help="with --dots: the smallest count of a dot (default 1)")
    io.add_argument("--dots-folds", type=fold_list, default=None, metavar="a,b,c,d",
                    help="with --dots: the enrichment asked for over the donut, lower-left, horizontal and "
                         "vertical neighbourhood (default 1.75,1.75,1.5,1.5)")
    io.add_argument("--dots-ignore-diags", type=int, default=None, metavar="N",
                    help="with --dots: no window may reach below diagonal N (default 2)")
    io.add_argument("--dots-cluster-radius", type=genomic_distance, default=None, metavar="SIZE",
                    help="with --dots: a candidate is dropped when a better one lies within this distance on "
                         "both axes (a multiple of the dots resolution; 0 keeps all; default 20kb, rounded down "
                         "to whole bins, at least one bin)")
    io.add_argument("--pileup-at", action="append", default=None, metavar="WHAT",
                    help="also write <prefix>_pileup.tsv: the windows of the symmetric matrix around a list of "
                         "anchor pairs, summed on the GPU into one observed pile, with the pile the interval's "
                         "distance-decay curve expects and the APA scores.  WHAT is `dots` (the run's own dots: "
                         "needs --dots at the pileup resolution), `barriers` (every barrier, on the diagonal) or "
                         "the path of a BEDPE file (cis pairs, placed by the midpoints of their sides); may be "
                         "given several times")
    io.add_argument("--pileup-flank", type=genomic_distance, default=None, metavar="SIZE",
                    help="with --pileup-at: the window reaches SIZE to every side of an anchor (a positive "
                         "multiple of the pileup resolution, at most 32 bins; 2 f + 1 diagonals must fit -w; "
                         "default 10 bins)")
    io.add_argument("--pileup-resolution", type=genomic_distance, default=None, metavar="R",
                    help="with --pileup-at: the bin size of the pileup (a multiple of -r, coarsened on the GPU; "
                         "default -r)")
    io.add_argument("--pileup-corner", type=genomic_distance, default=None, metavar="SIZE",
                    help="with --pileup-at: the side of the corner blocks of the APA scores (a positive multiple "
                         "of the pileup resolution, at most the flank; default a third of the flank's bins, at "
                         "least one)")
    depth = io.add_mutually_exclusive_group()
    depth.add_argument("--subsample-frac", type=float, default=None, metavar="F",
                       help="also write <prefix>_sampled.cool (.mcool with --mcool-resolutions): the matrix with "
                            "every contact kept with probability F, 0 < F <= 1, independently (binomial thinning, "
                            "the default mode of `cooltools random-sample`: the total is random around F times "
                            "the matrix's, not equal to it), drawn on the GPU at -r by a generator keyed by the "
                            "pixel's bin ids in the file; the other resolutions are coarsened from the sampled one")
    depth.add_argument("--subsample-to", type=int, default=None, metavar="N",
                       help="like --subsample-frac with the fraction that brings the contacts of the whole "
                            "matrix to about N; with N at or above them the unsampled matrix is written, with a "
                            "warning")
    io.add_argument("--subsample-seed", type=int, default=None, metavar="S",
                    help="with --subsample-frac / --subsample-to: the seed of the draw (default --seed); the same "
                         "seed at a larger fraction keeps a superset")
    io.add_argument("--subsample-split", action="store_true",
                    help="with --subsample-frac / --subsample-to: also write <prefix>_sampled_rest.cool, the "
                         "contacts that were not kept: two disjoint pseudo-replicates that add up to the matrix")
    # The comparison with a reference file (<prefix>_stripes.tsv; the module's text describes the four
    # options).  They are parsed like the others and kept out of the generated help: the text of
    # `simulate --help` is held fixed by tests/golden/simulate_help.txt.
    io.add_argument("--compare-to", default=None, metavar="REF", help=argparse.SUPPRESS)
    io.add_argument("--compare-metrics", type=metric_list, default=None, metavar="LIST", help=argparse.SUPPRESS)
    io.add_argument("--compare-resolution", type=genomic_distance, default=None, metavar="R",
                    help=argparse.SUPPRESS)
    io.add_argument("--compare-exclude-zero-pixels", action="store_true", default=None, help=argparse.SUPPRESS)
    # HiCRep's SCC against the same reference (<prefix>_scc.tsv), kept out of the generated help likewise
    io.add_argument("--scc", action="store_true", default=None, help=argparse.SUPPRESS)
    io.add_argument("--scc-smooth", type=genomic_distance, default=None, metavar="D", help=argparse.SUPPRESS)
    io.add_argument("--scc-max-distance", type=genomic_distance, default=None, metavar="D", help=argparse.SUPPRESS)
    io.add_argument("--scc-ignore-diags", type=int, default=None, metavar="N", help=argparse.SUPPRESS)
    io.add_argument("--scc-include-zeros", action="store_true", default=None, help=argparse.SUPPRESS)
    # The statistical test of the dot calling (<prefix>_dots_thresholds.tsv; the module's text describes the
    # two options), kept out of the generated help likewise
    io.add_argument("--dots-fdr", type=float, default=None, metavar="Q", help=argparse.SUPPRESS)
    io.add_argument("--dots-lambda-chunks", type=int, default=None, metavar="N", help=argparse.SUPPRESS)
    # The average domain (<prefix>_domains.tsv; the module's text describes the four options), kept out of the
    # generated help likewise
    io.add_argument("--domains-at", action="append", default=None, metavar="FILE.bed", help=argparse.SUPPRESS)
    io.add_argument("--domains-size", type=int, default=None, metavar="N", help=argparse.SUPPRESS)
    io.add_argument("--domains-flank-percent", type=int, default=None, metavar="P", help=argparse.SUPPRESS)
    io.add_argument("--domains-resolution", type=genomic_distance, default=None, metavar="R", help=argparse.SUPPRESS)
    # Stripe calling (<prefix>_stripe_calls.bedpe; the module's text describes the options), kept out of the
    # generated help likewise
    io.add_argument("--call-stripes", action="store_true", default=None, help=argparse.SUPPRESS)
    io.add_argument("--call-stripes-lengths", type=window_list, default=None, metavar="LIST", help=argparse.SUPPRESS)
    io.add_argument("--call-stripes-flank", type=genomic_distance, default=None, metavar="D", help=argparse.SUPPRESS)
    io.add_argument("--call-stripes-width", type=genomic_distance, default=None, metavar="D", help=argparse.SUPPRESS)
    io.add_argument("--call-stripes-fold", type=float, default=None, metavar="F", help=argparse.SUPPRESS)
    io.add_argument("--call-stripes-min-count", type=int, default=None, metavar="N", help=argparse.SUPPRESS)
    io.add_argument("--call-stripes-ignore-diags", type=int, default=None, metavar="N", help=argparse.SUPPRESS)
    io.add_argument("--call-stripes-radius", type=genomic_distance, default=None, metavar="D", help=argparse.SUPPRESS)
    io.add_argument("--call-stripes-resolution", type=genomic_distance, default=None, metavar="R",
                    help=argparse.SUPPRESS)
    # Domain calling (<prefix>_domain_calls.bed; the module's text describes the options), kept out of the
    # generated help likewise
    io.add_argument("--call-domains", action="store_true", default=None, help=argparse.SUPPRESS)
    io.add_argument("--call-domains-max-width", type=genomic_distance, default=None, metavar="D", help=argparse.SUPPRESS)
    io.add_argument("--call-domains-min-width", type=genomic_distance, default=None, metavar="D", help=argparse.SUPPRESS)
    io.add_argument("--call-domains-gamma", type=float, default=None, metavar="G", help=argparse.SUPPRESS)
    io.add_argument("--call-domains-ignore-diags", type=int, default=None, metavar="N", help=argparse.SUPPRESS)
    io.add_argument("--call-domains-resolution", type=genomic_distance, default=None, metavar="R",
                    help=argparse.SUPPRESS)


def build_parser():
    ap = argparse.ArgumentParser(prog="modle_amd", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="command", required=True)
    p = sub.add_parser("simulate", aliases=["sim"], help="simulate loop extrusion and write a .cool")
    io = p.add_argument_group("input / output")
    io.add_argument("-c", "--chrom-sizes", required=True)
    io.add_argument("-b", "--extrusion-barrier-file", required=True)
    io.add_argument("-g", "--genomic-intervals", "--chrom-subranges", default=None)
    io.add_argument("-f", "--force", action="store_true")
    io.add_argument("-o", "--output-prefix", required=True)
    io.add_argument("--assembly-name", default="unknown")
    io.add_argument("-q", "--quiet", action="store_true")
    io.add_argument("-v", "--verbose", action="store_true", help="accepted (the log is short anyway)")
    io.add_argument("--skip-output", action="store_true")
    add_analysis_arguments(io)
    io.add_argument("--log-model-internal-state", action="store_true",
                    help="write <prefix>_internal_state.log.gz: one line of statistics per task and "
                         "epoch (uses the diagnostic build libmodle_hip_statelog.so)")
    io.add_argument("--internal-state-max-epochs", type=int, default=4096,
                    help="epochs recorded per task with --log-model-internal-state")
    io.add_argument("--simulate-chromosomes-wo-barriers", dest="wo_barriers", action="store_true")
    io.add_argument("--skip-chromosomes-wo-barriers", dest="wo_barriers", action="store_false")
    io.add_argument("-t", "--threads", type=int, default=None, help="ignored (the GPU does the work)")
    io.add_argument("--device", type=int, default=None, help="HIP device (default: LOCAL_RANK or 0)")
    io.add_argument("--dist-backend", choices=["nccl", "gloo"], default="nccl",
                    help="nccl (= RCCL, default): the matrices are reduced on the GPUs over xGMI.  gloo: "
                         "the same per-interval ordering with the reduce done on host copies -- for "
                         "rehearsing the N > 1 path with several ranks on ONE GPU (tests; pass --device)")
    g = p.add_argument_group("model parameters (reference names; omitted => reference default)")
    for flags, dest, typ in [
        (("--lef-density", "--lefs-per-mbp"), "number_of_lefs_per_mbp", float),
        (("--avg-lef-processivity",), "avg_lef_processivity", genomic_distance),
        (("--probability-of-lef-bypass",), "probability_of_extrusion_unit_bypass", float),
        (("--extrusion-barrier-occupancy",), "extrusion_barrier_occupancy", float),
        (("--hard-stall-lef-stability-multiplier",), "hard_stall_lef_stability_multiplier", float),
        (("--soft-stall-lef-stability-multiplier",), "soft_stall_lef_stability_multiplier", float),
        (("--fwd-extrusion-speed",), "fwd_extrusion_speed", genomic_distance),
        (("--rev-extrusion-speed",), "rev_extrusion_speed", genomic_distance),
        (("--fwd-extrusion-speed-std",), "fwd_extrusion_speed_std", float),
        (("--rev-extrusion-speed-std",), "rev_extrusion_speed_std", float),
        (("--lef-bar-major-collision-prob",), "lef_bar_major_collision_pblock", float),
        (("--lef-bar-minor-collision-prob",), "lef_bar_minor_collision_pblock", float),
        (("--extrusion-barrier-bound-stp",), "barrier_occupied_stp", float),
        (("--extrusion-barrier-not-bound-stp",), "barrier_not_occupied_stp", float),
        (("--contact-sampling-interval",), "contact_sampling_interval", genomic_distance),
        (("-r", "--resolution"), "bin_size", genomic_distance),
        (("-w", "--diagonal-width"), "diagonal_width", genomic_distance),
        (("--tad-to-loop-contact-ratio",), "tad_to_loop_contact_ratio", float),
        (("--mu", "--genextr-location"), "genextreme_mu", float),
        (("--sigma", "--genextr-scale"), "genextreme_sigma", float),
        (("--xi", "--genextr-shape"), "genextreme_xi", float),
        (("--target-number-of-epochs",), "target_simulation_epochs", int),
        (("--target-contact-density",), "target_contact_density", float),
        (("--ncells",), "num_cells", int),
        (("--seed",), "seed", int),
        (("--burnin-target-epochs-for-lef-activation",), "burnin_target_epochs_for_lef_activation", int),
        (("--burnin-history-length",), "burnin_history_length", int),
        (("--burnin-smoothing-window-size",), "burnin_smoothing_window_size", int),
        (("--min-burnin-epochs",), "min_burnin_epochs", int),
        (("--max-burnin-epochs",), "max_burnin_epochs", int),
        (("--burnin-extr-speed-coefficient",), "burnin_speed_coefficient", float),
        (("--probability-normalization-factor",), "probability_normalization_factor", genomic_distance),
    ]:
        g.add_argument(*flags, dest=dest, type=typ, default=None)
    g.add_argument("--contact-sampling-strategy", choices=sorted(STRATEGIES), default=None)
    g.add_argument("-s", "--stopping-criterion", choices=["contact-density", "simulation-epochs"],
                   default="contact-density")
    g.add_argument("--track-1d-lef-position", dest="track_1d", action="store_true", default=None)
    g.add_argument("--no-track-1d-lef-position", dest="track_1d", action="store_false")
    g.add_argument("--skip-burnin", action="store_true")
    g.add_argument("--interpret-extrusion-barrier-name-as-not-bound-stp", dest="name_as_stp",
                   action="store_true")
    g.add_argument("--normalize-probabilities", dest="normalize", action="store_true", default=None)
    g.add_argument("--no-normalize-probabilities", dest="normalize", action="store_false")
    p.set_defaults(wo_barriers=False)
    e = sub.add_parser("evaluate", aliases=["eval"],
                       help="compare two .cool files stripe by stripe (modle_tools evaluate)")
    e.add_argument("-i", "--input-cooler", required=True, help="the matrix under test")
    e.add_argument("-r", "--reference-cooler", required=True)
    e.add_argument("-c", "--chrom-sizes", required=True, help="chromosomes to compare")
    e.add_argument("-w", "--diagonal-width", type=int, default=3_000_000)
    e.add_argument("-m", "--metric", choices=["pearson", "spearman", "rmse", "eucl_dist"],
                   default="pearson")
    e.add_argument("--exclude-zero-pixels", action="store_true")
    n = sub.add_parser("analyze", aliases=["an"],
                       help="run the analyses of `simulate` on the matrix of a .cool or of one resolution of an "
                            ".mcool, loaded into band matrices on the GPU")
    nio = n.add_argument_group("input / output")
    nio.add_argument("input", metavar="IN.cool | IN.mcool::/resolutions/R",
                     help="the cooler: the bin size and the chromosomes are the file's; raw counts are read, "
                          "balancing weights are ignored")
    nio.add_argument("-o", "--output-prefix", required=True)
    nio.add_argument("-w", "--diagonal-width", type=genomic_distance, default=None,
                     help="the width of the band that is loaded (default 3mb, as for simulate); the contacts "
                          "of the file beyond it are counted and left out")
    nio.add_argument("--chromosomes", default=None, metavar="LIST",
                     help="comma-separated names of the chromosomes to analyse (default: all of the file)")
    nio.add_argument("--device", type=int, default=None, help="HIP device (default: LOCAL_RANK or 0)")
    nio.add_argument("-f", "--force", action="store_true")
    nio.add_argument("-q", "--quiet", action="store_true")
    nio.add_argument("--assembly-name", default="unknown")
    add_analysis_arguments(nio)
    # (what preflight and write_outputs look at of simulate's other options)
    n.set_defaults(skip_output=False, log_model_internal_state=False)
    return ap


def config_from_args(a):
    """reference defaults, the options given on the command line, then Cli::transform_args"""
    over = {}
    for k, v in vars(a).items():
        if v is not None and hasattr(api.Config, k):
            over[k] = v
    if a.fwd_extrusion_speed is not None:
        over["fwd_extrusion_speed_set"] = 1
    if a.rev_extrusion_speed is not None:
        over["rev_extrusion_speed_set"] = 1
    if a.extrusion_barrier_occupancy is not None:
        if a.barrier_occupied_stp is not None:
            raise SystemExit("--extrusion-barrier-occupancy excludes --extrusion-barrier-bound-stp")
        over["extrusion_barrier_occupancy_set"] = 1
    if a.name_as_stp and a.barrier_not_occupied_stp is not None:
        raise SystemExit("--interpret-extrusion-barrier-name-as-not-bound-stp excludes "
                         "--extrusion-barrier-not-bound-stp")
    if a.contact_sampling_strategy is not None:
        over["contact_sampling_strategy"] = STRATEGIES[a.contact_sampling_strategy]
    if a.track_1d is not None:
        over["track_1d_lef_position"] = int(a.track_1d)
    if a.normalize is not None:
        over["normalize_probabilities"] = int(a.normalize)
    over["skip_burnin"] = int(a.skip_burnin)
    over["simulate_chromosomes_wo_barriers"] = int(a.wo_barriers)
    if a.stopping_criterion == "simulation-epochs":
        # cli.cpp:783-797 + simulation.cpp:1058-1074: epochs mode switches the density target off
        if a.target_simulation_epochs is None:
            raise SystemExit("--stopping-criterion=simulation-epochs requires --target-number-of-epochs")
        if a.target_contact_density is not None:
            raise SystemExit("--target-contact-density excludes --target-number-of-epochs")
        over["target_contact_density"] = -1.0
    elif a.target_simulation_epochs is not None:
        raise SystemExit("--stopping-criterion=contact-density excludes --target-number-of-epochs")
    mn, mx = over.get("min_burnin_epochs"), over.get("max_burnin_epochs")
    if mn is not None and mx is not None and mn > mx:
        raise SystemExit(f"--min-burnin-epochs={mn} cannot be greater than --max-burnin-epochs={mx}.")
    return api.make_config(**over)


def output_paths(prefix, mcool=False):
    return prefix + (".mcool" if mcool else ".cool"), prefix + "_lef_1d_occupancy.bw"


def _file(a, path_of, wanted=True):
    """this run's file by the `*_path` function `path_of`, or None: not `wanted`, or --skip-output"""
    return path_of(a.output_prefix) if wanted and not a.skip_output else None


# The files without options of their own; a path is None for a file the run does not write, `state_log` is
# this rank's.  (The first four fields are also made positionally: `expected` and `coverage` default to None.)
Outputs = collections.namedtuple("Outputs", "cooler bigwig dense state_log expected coverage", defaults=(None, None))
# what --insulation-windows asks for: the file (None with --skip-output), the bin size of the track, the
# windows in base pairs as given and the diagonals left out
Insulation = collections.namedtuple("Insulation", "path resolution windows min_diag")
# what --dots asks for: the file (None with --skip-output), the bin size, window, peak and cluster radius
# in base pairs, the smallest count, the four folds and the diagonals no window may reach below; and of
# --dots-fdr the rate (None: the fold test alone), the number of lambda-chunk edges and the file of the thresholds
Dots = collections.namedtuple("Dots", "path resolution window peak min_count folds min_diag radius fdr chunks "
                                      "thresholds_path", defaults=(None, pixels.DOT_LAMBDA_CHUNKS, None))
# what --pileup-at asks for: the file (None with --skip-output), the bin size, the flank and the corner of
# the APA scores in base pairs, and the sources in the order given (`dots`, `barriers` or a BEDPE path)
Pileup = collections.namedtuple("Pileup", "path resolution flank corner sources")
# what --subsample-frac / --subsample-to ask for: the files of the kept and of the other contacts (None
# with --skip-output, which is refused), the fraction or the target (one of them None), the seed, and
# whether the second file is written
Subsample = collections.namedtuple("Subsample", "path rest_path frac target seed split")
# what --compare-to asks for: the file (None with --skip-output, which is refused), the reference cooler as
# given, the bin size of the comparison, the metrics in the order given, whether zero pixels are left out,
# and what preflight read of the reference: its bin size and its chromosomes
Stripes = collections.namedtuple("Stripes", "path reference resolution metrics exclude_zero ref_bin_size ref_chroms")
# what --scc asks for: the file (None with --skip-output, which --compare-to refuses), the half-width of the
# smoothing box and the last diagonal in base pairs (None: the widest the band allows), the first diagonal, and
# whether a diagonal counts the pixels that are zero in both matrices; the bin size is Stripes.resolution
Scc = collections.namedtuple("Scc", "path smooth max_distance min_diag include_zeros")
# what --domains-at asks for: the file (None with --skip-output), the bin size, the side of the grid in cells, the
# padding of a domain in percent of its bins, and the BED files in the order given
Domains = collections.namedtuple("Domains", "path resolution size flank_percent sources")
# The whole plan of a run, which preflight makes once: the bin sizes of the .mcool (None: a .cool), the
# Outputs, this rank among the ranks and its device, the five records above (None: not asked for), the
# diagonals --coverage leaves out, the Domains and the Scc.  (The first five fields are also made positionally:
# the others default.)
_PreflightFields = collections.namedtuple(
    "Preflight", "bin_sizes outputs rank world device insulation dots pileup subsample stripes coverage_min_diag "
                 "domains scc",
    defaults=(None, None, None, None, None, 0, None, None))
# what --call-stripes asks for: the file (None with --skip-output), the bin size, the lengths, the flank (m bins),
# the width of the centre (2 h + 1 bins) and the thinning radius in base pairs, the fold, the smallest centre sum
# and the diagonals left out
StripeCalls = collections.namedtuple("StripeCalls", "path resolution lengths flank width fold min_count min_diag radius")


# what --call-domains asks for: the file (None with --skip-output), the bin size, the largest and the smallest
# width in base pairs, gamma and the diagonals left out
DomainCalls = collections.namedtuple("DomainCalls", "path resolution max_width min_width gamma min_diag")


class Preflight(_PreflightFields):
    """The 13 fields above, and the StripeCalls and the DomainCalls as the attributes `stripe_calls` and
    `domain_calls` (None: not asked for).  They are no further fields: the tuple is also made positionally and
    unpacked by its length, and a record that is new must not move what those users see.  Keyword-only here,
    kept by _replace."""
    stripe_calls = None  # (of an instance that _make made)
    domain_calls = None

    def __new__(cls, *args, stripe_calls=None, domain_calls=None, **kw):
        self = super().__new__(cls, *args, **kw)
        self.stripe_calls = stripe_calls
        self.domain_calls = domain_calls
        return self

    def _replace(self, **kw):
        stripe_calls = kw.pop("stripe_calls", self.stripe_calls)
        domain_calls = kw.pop("domain_calls", self.domain_calls)
        out = super()._replace(**kw)
        out.stripe_calls = stripe_calls
        out.domain_calls = domain_calls
        return out


def subsample_options(a, cfg):
    """The sampled matrix the arguments ask for, as a Subsample with the files of sampled_paths, or None.
    SystemExit: --subsample-seed or --subsample-split without a depth, both depths (the parser refuses that
    already), a fraction outside (0, 1] or NaN, a negative target, a seed that is no uint64, --skip-output
    (both depths need the cooler: its sums set the target, and the sampled file is a cooler)."""
    frac, target = a.subsample_frac, a.subsample_to
    if frac is None and target is None:
        if a.subsample_seed is not None:
            raise SystemExit("--subsample-seed needs --subsample-frac or --subsample-to")
        if a.subsample_split:
            raise SystemExit("--subsample-split needs --subsample-frac or --subsample-to")
        return None
    if frac is not None and target is not None:
        raise SystemExit("--subsample-frac excludes --subsample-to")
    if frac is not None and not 0.0 < frac <= 1.0:  # (false for NaN)
        raise SystemExit(f"--subsample-frac: {frac} is not in (0, 1]")
    if target is not None and target < 0:
        raise SystemExit(f"--subsample-to: {target} is negative")
    seed = int(cfg.seed) if a.subsample_seed is None else a.subsample_seed
    if not 0 <= seed < 1 << 64:
        raise SystemExit(f"--subsample-seed: {seed} is no unsigned 64-bit number")
    if a.skip_output:
        raise SystemExit(f"--subsample-{'frac' if target is None else 'to'} needs the cooler: it excludes --skip-output")
    kept_path, rest_path = sampled_paths(a.output_prefix, mcool=a.mcool_resolutions is not None)
    return Subsample(kept_path, rest_path, frac, target, seed, bool(a.subsample_split))


def _needs(option, given):
    """SystemExit for the first (name, value) of `given` that is set while `option`, which it needs, is not"""
    for name, v in given:
        if v is not None:
            raise SystemExit(f"{name} needs {option}")


def _analysis_resolution(name, value, cfg):
    """the bin size of an analysis: `value` of the option `name`, None: the resolution; SystemExit unless it is
    a multiple of the resolution"""
    base = int(cfg.bin_size)
    res = base if value is None else int(value)
    if res < base or res % base != 0:
        raise SystemExit(f"{name}: {res} is not a multiple of the resolution ({base})")
    return res


def pileup_options(a, cfg, dots):
    """The pileups the arguments ask for, as a Pileup, or None.  `dots`: what dots_options
    returned.  SystemExit: a --pileup-* option without --pileup-at, a resolution that is no multiple of
    -r, a flank or corner that is no positive multiple of the pileup resolution, a flank above 32 bins, a
    corner above the flank, the source `dots` without --dots or at another resolution than the dots'."""
    if not a.pileup_at:
        _needs("--pileup-at", (("--pileup-flank", a.pileup_flank), ("--pileup-resolution", a.pileup_resolution),
                               ("--pileup-corner", a.pileup_corner)))
        return None
    res = _analysis_resolution("--pileup-resolution", a.pileup_resolution, cfg)
    flank = 10 * res if a.pileup_flank is None else int(a.pileup_flank)
    if flank < res or flank % res != 0:
        raise SystemExit(f"--pileup-flank: {flank} is not a positive multiple of the pileup resolution ({res})")
    if flank // res > MAX_PILEUP_FLANK_BINS:
        raise SystemExit(f"--pileup-flank: {flank} is {flank // res} bins of {res}: at most {MAX_PILEUP_FLANK_BINS}")
    corner = max(1, flank // res // 3) * res if a.pileup_corner is None else int(a.pileup_corner)
    if corner < res or corner % res != 0:
        raise SystemExit(f"--pileup-corner: {corner} is not a positive multiple of the pileup resolution ({res})")
    if corner > flank:
        raise SystemExit(f"--pileup-corner: {corner} is above the flank ({flank})")
    if "dots" in a.pileup_at:
        if dots is None:
            raise SystemExit("--pileup-at dots needs --dots")
        if int(dots.resolution) != res:
            raise SystemExit(f"--pileup-at dots: the pileup resolution ({res}) is not the dots resolution "
                             f"({int(dots.resolution)})")
    return Pileup(_file(a, pileup_path), res, flank, corner, list(a.pileup_at))


MAX_DOMAINS_FLANK_PERCENT = 200


def domains_options(a, cfg):
    """The average domain the arguments ask for, as a Domains, or None.  SystemExit: a --domains-* option without
    --domains-at, a resolution that is no multiple of -r, a size outside 1..128, a flank outside 0..200 percent."""
    if not a.domains_at:
        _needs("--domains-at", (("--domains-size", a.domains_size),
                                ("--domains-flank-percent", a.domains_flank_percent),
                                ("--domains-resolution", a.domains_resolution)))
        return None
    res = _analysis_resolution("--domains-resolution", a.domains_resolution, cfg)
    size = 60 if a.domains_size is None else int(a.domains_size)
    if not 1 <= size <= pixels.MAX_RESCALE:
        raise SystemExit(f"--domains-size: {size} is not in [1, {pixels.MAX_RESCALE}]")
    percent = 100 if a.domains_flank_percent is None else int(a.domains_flank_percent)
    if not 0 <= percent <= MAX_DOMAINS_FLANK_PERCENT:
        raise SystemExit(f"--domains-flank-percent: {percent} is not in [0, {MAX_DOMAINS_FLANK_PERCENT}]")
    return Domains(_file(a, domains_path), res, size, percent, list(a.domains_at))


def dots_options(a, cfg):
    """The dot calling the arguments ask for, as a Dots, or None.  SystemExit: a
    --dots-* option without --dots, a negative number of diagonals, a count below 1, a resolution that is
    no multiple of -r, a window, peak or radius that is no multiple of the dots resolution, a peak that
    is not below the window, a window above 20 bins."""
    given = (("--dots-resolution", a.dots_resolution), ("--dots-window", a.dots_window), ("--dots-peak", a.dots_peak),
             ("--dots-min-count", a.dots_min_count), ("--dots-folds", a.dots_folds),
             ("--dots-ignore-diags", a.dots_ignore_diags), ("--dots-cluster-radius", a.dots_cluster_radius),
             ("--dots-fdr", a.dots_fdr), ("--dots-lambda-chunks", a.dots_lambda_chunks))
    if not a.dots:
        _needs("--dots", given)
        return None
    min_diag = 2 if a.dots_ignore_diags is None else a.dots_ignore_diags
    if min_diag < 0:
        raise SystemExit(f"--dots-ignore-diags: {min_diag} is negative")
    min_count = 1 if a.dots_min_count is None else a.dots_min_count
    if min_count < 1:
        raise SystemExit(f"--dots-min-count: {min_count} is below 1")
    res = _analysis_resolution("--dots-resolution", a.dots_resolution, cfg)
    window = 5 * res if a.dots_window is None else int(a.dots_window)
    peak = min(2 * res, window - res) if a.dots_peak is None else int(a.dots_peak)
    radius = max(1, 20_000 // res) * res if a.dots_cluster_radius is None else int(a.dots_cluster_radius)
    for name, v, least in (("--dots-window", window, res), ("--dots-peak", peak, 0),
                           ("--dots-cluster-radius", radius, 0)):
        if v < least or v % res != 0:
            raise SystemExit(f"{name}: {v} is not a {'positive ' if least else ''}multiple of the dots resolution "
                             f"({res})")
    if peak >= window:
        raise SystemExit(f"--dots-peak: {peak} is not below the window ({window})")
    if window // res > MAX_DOT_WINDOW_BINS:
        raise SystemExit(f"--dots-window: {window} is {window // res} bins of {res}: at most {MAX_DOT_WINDOW_BINS}")
    folds = list(DOT_FOLDS if a.dots_folds is None else a.dots_folds)
    if a.dots_fdr is None:
        _needs("--dots-fdr", (("--dots-lambda-chunks", a.dots_lambda_chunks),))
        return Dots(_file(a, dots_path), res, window, peak, min_count, folds, min_diag, radius)
    if not 0.0 < a.dots_fdr < 1.0:  # (false for NaN)
        raise SystemExit(f"--dots-fdr: {a.dots_fdr} is not in (0, 1)")
    chunks = pixels.DOT_LAMBDA_CHUNKS if a.dots_lambda_chunks is None else a.dots_lambda_chunks
    if not 1 <= chunks <= pixels.MAX_DOT_EDGES:
        raise SystemExit(f"--dots-lambda-chunks: {chunks} is not in [1, {pixels.MAX_DOT_EDGES}]")
    return Dots(_file(a, dots_path), res, window, peak, min_count, folds, min_diag, radius, a.dots_fdr, chunks,
                _file(a, dots_thresholds_path))


def stripes_options(a, cfg):
    """The comparison with a reference cooler the arguments ask for, as a Stripes, or None.
    SystemExit: a --compare-* option without --compare-to, --skip-output (the comparison is a file of the
    output stage, which checks it against the cooler's sums), spearman together with
    --compare-exclude-zero-pixels (its weighted ranks are no integers: `evaluate` has it), a resolution that
    is no multiple of -r, a reference file that is missing or cannot be read as a cooler, or whose bin size is
    not the resolution of the comparison."""
    if a.compare_to is None:
        _needs("--compare-to", (("--compare-metrics", a.compare_metrics),
                                ("--compare-resolution", a.compare_resolution),
                                ("--compare-exclude-zero-pixels", a.compare_exclude_zero_pixels)))
        return None
    if a.skip_output:
        raise SystemExit("--compare-to needs the output stage: it excludes --skip-output")
    metrics = list(a.compare_metrics or ["pearson"])
    exclude_zero = bool(a.compare_exclude_zero_pixels)
    if exclude_zero and "spearman" in metrics:
        raise SystemExit("--compare-exclude-zero-pixels: spearman without the zero pixels has ranks that are no "
                         "integers; the `evaluate` subcommand forms it on the host")
    res = _analysis_resolution("--compare-resolution", a.compare_resolution, cfg)
    path = a.compare_to.split("::", 1)[0]
    if not os.path.isfile(path):
        raise SystemExit(f"--compare-to: {path} is no file")
    from . import cooler

    try:
        with cooler.CoolerReader(a.compare_to) as reader:
            ref_bin_size, ref_chroms = int(reader.bin_size), list(reader.chroms)
    except cooler.CoolerError as e:
        raise SystemExit(f"--compare-to: cannot read {a.compare_to}: {e}")
    if ref_bin_size != res:
        raise SystemExit(f"--compare-to: {a.compare_to} has a bin size of {ref_bin_size}, the comparison runs at "
                         f"{res} (-r, or --compare-resolution)")
    return Stripes(_file(a, stripes_path), a.compare_to, res, metrics, exclude_zero, ref_bin_size, ref_chroms)


def scc_options(a, cfg, stripes):
    """The stratum-adjusted correlation the arguments ask for, as an Scc, or None.  `stripes`: what
    stripes_options returned; the comparison's bin size is its resolution.  SystemExit: a --scc-* option without
    --scc, --scc without --compare-to, a negative number of diagonals, a smoothing or a largest distance that is
    no whole number of bins, a smoothing above 20 bins."""
    if not a.scc:
        _needs("--scc", (("--scc-smooth", a.scc_smooth), ("--scc-max-distance", a.scc_max_distance),
                         ("--scc-ignore-diags", a.scc_ignore_diags), ("--scc-include-zeros", a.scc_include_zeros)))
        return None
    if stripes is None:
        raise SystemExit("--scc needs --compare-to")
    res = int(stripes.resolution)
    min_diag = 1 if a.scc_ignore_diags is None else a.scc_ignore_diags
    if min_diag < 0:
        raise SystemExit(f"--scc-ignore-diags: {min_diag} is negative")
    smooth = 0 if a.scc_smooth is None else int(a.scc_smooth)
    if smooth % res != 0:
        raise SystemExit(f"--scc-smooth: {smooth} is not a multiple of the resolution of the comparison ({res})")
    if smooth // res > MAX_SCC_SMOOTH_BINS:
        raise SystemExit(f"--scc-smooth: {smooth} is {smooth // res} bins of {res}: at most {MAX_SCC_SMOOTH_BINS}")
    far = None if a.scc_max_distance is None else int(a.scc_max_distance)
    if far is not None and far % res != 0:
        raise SystemExit(f"--scc-max-distance: {far} is not a multiple of the resolution of the comparison ({res})")
    return Scc(_file(a, scc_path), smooth, far, min_diag, bool(a.scc_include_zeros))


MAX_STRIPE_FLANK_BINS = pixels.MAX_PROFILE_OFFSET


def stripe_calls_options(a, cfg):
    """The stripe calling the arguments ask for, as a StripeCalls, or None.  SystemExit: a --call-stripes-* option
    without --call-stripes, a resolution that is no multiple of -r, more than 4 lengths, a length, flank, width or
    radius that is no multiple of the resolution of the calls, a width that is no odd number of bins, a flank
    below the width or above 8 bins, ignored diagonals below the flank, a length not above the ignored
    diagonals, lengths that do not increase, a fold that is not positive, a negative count.  The defaults are
    product choices: lengths of 200, 400 and 800 kb, a flank of 50 kb (at most 8 bins, at least the width), a
    centre of one bin, pixels.STRIPE_FOLD and STRIPE_MIN_COUNT, as many diagonals ignored as the flank has bins
    (at least 2), and a thinning radius of the flank."""
    given = (("--call-stripes-lengths", a.call_stripes_lengths), ("--call-stripes-flank", a.call_stripes_flank),
             ("--call-stripes-width", a.call_stripes_width), ("--call-stripes-fold", a.call_stripes_fold),
             ("--call-stripes-min-count", a.call_stripes_min_count),
             ("--call-stripes-ignore-diags", a.call_stripes_ignore_diags),
             ("--call-stripes-radius", a.call_stripes_radius), ("--call-stripes-resolution", a.call_stripes_resolution))
    if not a.call_stripes:
        _needs("--call-stripes", given)
        return None
    res = _analysis_resolution("--call-stripes-resolution", a.call_stripes_resolution, cfg)
    lengths = [200_000, 400_000, 800_000] if a.call_stripes_lengths is None else [int(x) for x in a.call_stripes_lengths]
    if not 1 <= len(lengths) <= pixels.MAX_PROFILE_LENGTHS:
        raise SystemExit(f"--call-stripes-lengths: {len(lengths)} lengths: 1 to {pixels.MAX_PROFILE_LENGTHS}")
    width = res if a.call_stripes_width is None else int(a.call_stripes_width)
    if width < res or width % res != 0 or width // res % 2 != 1:
        raise SystemExit(f"--call-stripes-width: {width} is not an odd number of bins of the resolution of the calls ({res})")
    flank = max(width, min(MAX_STRIPE_FLANK_BINS, max(1, 50_000 // res)) * res) if a.call_stripes_flank is None \
        else int(a.call_stripes_flank)
    radius = flank if a.call_stripes_radius is None else int(a.call_stripes_radius)
    for name, v in [("--call-stripes-lengths", x) for x in lengths] + [("--call-stripes-flank", flank),
                                                                      ("--call-stripes-radius", radius)]:
        if v < 0 or v % res != 0:
            raise SystemExit(f"{name}: {v} is not a multiple of the resolution of the calls ({res})")
    if flank < width:
        raise SystemExit(f"--call-stripes-flank: {flank} is below the width of the centre ({width}): no shoulder is left")
    if flank // res > MAX_STRIPE_FLANK_BINS:
        raise SystemExit(f"--call-stripes-flank: {flank} is {flank // res} bins of {res}: at most {MAX_STRIPE_FLANK_BINS}")
    min_diag = max(flank // res, 2) if a.call_stripes_ignore_diags is None else a.call_stripes_ignore_diags
    if min_diag < flank // res:
        raise SystemExit(f"--call-stripes-ignore-diags: {min_diag} is below the {flank // res} bins of the flank: a "
                         "shoulder would cross the main diagonal")
    for below, length in zip([min_diag * res] + lengths, lengths):
        if length <= below:
            raise SystemExit(f"--call-stripes-lengths: {length} is not above " +
                             (f"the {min_diag} ignored diagonals ({below})" if length is lengths[0] else f"{below}"))
    fold = pixels.STRIPE_FOLD if a.call_stripes_fold is None else a.call_stripes_fold
    if not fold > 0.0 or fold == float("inf"):  # (NaN too)
        raise SystemExit(f"--call-stripes-fold: {fold} is not a positive number")
    min_count = pixels.STRIPE_MIN_COUNT if a.call_stripes_min_count is None else a.call_stripes_min_count
    if min_count < 0:
        raise SystemExit(f"--call-stripes-min-count: {min_count} is negative")
    return StripeCalls(_file(a, stripe_calls_path), res, lengths, flank, width, fold, min_count, min_diag, radius)


def domain_calls_options(a, cfg):
    """The domain calling the arguments ask for, as a DomainCalls, or None.  SystemExit: a --call-domains-* option
    without --call-domains, a resolution that is no multiple of -r, a width that is no positive multiple of the
    resolution of the calls, a largest width below the smallest or above pixels.MAX_TRIANGLE_WIDTH bins, a gamma
    that is negative or not finite, a negative number of diagonals.  The defaults are product choices: 2 Mb (the
    whole bins of it, one at least; every band clamps it to its diagonals), pixels.DOMAIN_MIN_WIDTH bins,
    pixels.DOMAIN_GAMMA, two diagonals ignored."""
    given = (("--call-domains-max-width", a.call_domains_max_width), ("--call-domains-min-width", a.call_domains_min_width),
             ("--call-domains-gamma", a.call_domains_gamma), ("--call-domains-ignore-diags", a.call_domains_ignore_diags),
             ("--call-domains-resolution", a.call_domains_resolution))
    if not a.call_domains:
        _needs("--call-domains", given)
        return None
    res = _analysis_resolution("--call-domains-resolution", a.call_domains_resolution, cfg)
    least = pixels.DOMAIN_MIN_WIDTH * res if a.call_domains_min_width is None else int(a.call_domains_min_width)
    most = max(least, max(1, 2_000_000 // res) * res) if a.call_domains_max_width is None else int(a.call_domains_max_width)
    for name, v in (("--call-domains-min-width", least), ("--call-domains-max-width", most)):
        if v < res or v % res != 0:
            raise SystemExit(f"{name}: {v} is not a positive multiple of the resolution of the calls ({res})")
    if most < least:
        raise SystemExit(f"--call-domains-max-width: {most} is below the smallest width ({least})")
    if most // res > pixels.MAX_TRIANGLE_WIDTH:
        raise SystemExit(f"--call-domains-max-width: {most} is {most // res} bins of {res}: at most "
                         f"{pixels.MAX_TRIANGLE_WIDTH}")
    gamma = pixels.DOMAIN_GAMMA if a.call_domains_gamma is None else a.call_domains_gamma
    if not 0.0 <= gamma < float("inf"):  # (false for NaN)
        raise SystemExit(f"--call-domains-gamma: {gamma} is not a finite number that is not negative")
    min_diag = 2 if a.call_domains_ignore_diags is None else a.call_domains_ignore_diags
    if min_diag < 0:
        raise SystemExit(f"--call-domains-ignore-diags: {min_diag} is negative")
    return DomainCalls(_file(a, domain_calls_path), res, most, least, gamma, min_diag)


def insulation_options(a, cfg):
    """The insulation track the arguments ask for, as an Insulation, or None.
    SystemExit: --insulation-resolution or --insulation-ignore-diags without --insulation-windows, a
    negative number of diagonals, a resolution that is no multiple of -r, a window that is no positive
    multiple of the insulation resolution or has more than 1024 bins."""
    if a.insulation_windows is None:
        _needs("--insulation-windows", (("--insulation-resolution", a.insulation_resolution),
                                        ("--insulation-ignore-diags", a.insulation_ignore_diags)))
        return None
    min_diag = 2 if a.insulation_ignore_diags is None else a.insulation_ignore_diags
    if min_diag < 0:
        raise SystemExit(f"--insulation-ignore-diags: {min_diag} is negative")
    res = _analysis_resolution("--insulation-resolution", a.insulation_resolution, cfg)
    for w in a.insulation_windows:
        if w <= 0 or w % res != 0:
            raise SystemExit(f"--insulation-windows: {w} is not a positive multiple of the insulation "
                             f"resolution ({res})")
        if w // res > MAX_INSULATION_WINDOW_BINS:
            raise SystemExit(f"--insulation-windows: {w} is {w // res} bins of {res}: at most "
                             f"{MAX_INSULATION_WINDOW_BINS}")
    return Insulation(_file(a, insulation_path), res, list(a.insulation_windows), min_diag)


def preflight(a, cfg):
    """The whole plan of the run, a Preflight: what the arguments alone settle and refuse, without a genome or
    a GPU.  Nothing after it derives an analysis from the arguments again.  SystemExit:
    --coverage-ignore-diags without --coverage, or negative; what insulation_options, dots_options,
    pileup_options, domains_options, subsample_options, stripes_options, scc_options, stripe_calls_options and
    domain_calls_options refuse, in that order
    (stripes_options
    opens the reference cooler, the one time it is opened before the launch); a bad --mcool-resolutions list; on
    rank 0, an output that exists without --force (cooler or .mcool, then bigwig, then .npz, then the expected,
    the coverage, the insulation, the dots, the pileup and the domains file, then the sampled files, then the
    stripes, then the SCC, then the stripe calls, then the domain calls).  With
    --skip-output no file is planned and none is looked at."""
    if a.coverage_ignore_diags is not None:
        if not a.coverage:
            raise SystemExit("--coverage-ignore-diags needs --coverage")
        if a.coverage_ignore_diags < 0:
            raise SystemExit(f"--coverage-ignore-diags: {a.coverage_ignore_diags} is negative")
    ins = insulation_options(a, cfg)
    dots = dots_options(a, cfg)
    pile = pileup_options(a, cfg, dots)
    dom = domains_options(a, cfg)
    sub = subsample_options(a, cfg)
    cmp_ = stripes_options(a, cfg)
    scc = scc_options(a, cfg, cmp_)
    calls = stripe_calls_options(a, cfg)
    called = domain_calls_options(a, cfg)
    # (a bad list ends the run here, before anything is imported or simulated)
    bin_sizes = None if a.mcool_resolutions is None else mcool_bin_sizes(a.mcool_resolutions, cfg.bin_size)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    device = a.device if a.device is not None else int(os.environ.get("LOCAL_RANK", "0"))
    analyses = (ins, dots, pile, sub, cmp_, a.coverage_ignore_diags or 0, dom, scc)
    if a.skip_output:
        return Preflight(bin_sizes, Outputs(None, None, None, None), rank, world, device, *analyses, stripe_calls=calls,
                         domain_calls=called)
    cool_path, bw_path = output_paths(a.output_prefix, mcool=bin_sizes is not None)
    # (cli.cpp:871-875; with several ranks every rank writes its own)
    log_path = a.output_prefix + ("_internal_state.log.gz" if world == 1 else f"_internal_state.rank{rank}.log.gz")
    outputs = Outputs(cool_path, bw_path if cfg.track_1d_lef_position else None, _file(a, dense_path, a.dense_region),
                      log_path if a.log_model_internal_state else None, _file(a, expected_path, a.expected),
                      _file(a, coverage_path, a.coverage))
    if rank == 0:
        os.makedirs(os.path.dirname(os.path.abspath(cool_path)), exist_ok=True)
        planned = [outputs.cooler, outputs.bigwig, outputs.dense, outputs.expected, outputs.coverage]
        planned += [r.path for r in (ins, dots, pile, dom, sub) if r is not None]
        planned += [dots.thresholds_path] if dots is not None else []
        planned += [sub.rest_path] if sub is not None and sub.split else []
        planned += [cmp_.path] if cmp_ is not None else []
        planned += [scc.path] if scc is not None else []
        planned += [calls.path] if calls is not None else []
        planned += [called.path] if called is not None else []
        for p in planned:
            if p and os.path.exists(p) and not a.force:
                raise SystemExit(f"refusing to overwrite {p}: pass --force to overwrite")
    return Preflight(bin_sizes, outputs, rank, world, device, *analyses, stripe_calls=calls, domain_calls=called)


def plan_run(a, cfg, pre, log):
    """The chromosomes, this rank's plan and the dense regions; a resolution or region that the plan
    shows to be bad still ends the run before anything is simulated."""
    chroms, intervals, stats = genome.import_genome(cfg, a.chrom_sizes, a.extrusion_barrier_file,
                                                    a.genomic_intervals, a.name_as_stp)
    log(f"imported {len(chroms)} chromosomes, {len(intervals)} intervals, "
        f"{stats['barriers_imported']} barriers ({stats['barriers_without_strand']} without strand dropped)")
    plan = driver.plan_genome(cfg, intervals, pre.rank, pre.world)
    return chroms, plan, check_plan(a, cfg, pre, plan, chroms)


def check_plan(a, cfg, pre, plan, chroms):
    """What a plan shows to be bad of the resolutions, the windows and the regions asked for, as a SystemExit
    before anything is simulated or analysed; returns the dense regions (driver.dense_regions)."""
    if pre.bin_sizes is not None and not a.skip_output:
        hit = driver.mcool_collision(plan, int(cfg.bin_size), pre.bin_sizes)
        if hit is not None:
            raise SystemExit(f"--mcool-resolutions: the intervals {hit[1]} and {hit[2]} share a bin at "
                             f"resolution {hit[0]}: its pixels would not be sorted and unique")
    if pre.insulation is not None and pre.insulation.path is not None:
        bad = driver.insulation_misfit(plan, int(cfg.bin_size), pre.insulation.resolution, pre.insulation.windows)
        if bad is not None:
            raise SystemExit(f"--insulation-windows: the diamond of {bad[1]} ({bad[2]} bins of "
                             f"{pre.insulation.resolution}) does not fit the band of {bad[0]} ({bad[3]} diagonals): "
                             f"the largest window that fits is {bad[4]} ({bad[4] // pre.insulation.resolution} bins)")
    if pre.dots is not None and pre.dots.path is not None:
        bad = driver.dots_misfit(plan, int(cfg.bin_size), pre.dots.resolution, pre.dots.window, pre.dots.min_diag)
        if bad is not None:
            fits = (f"the largest window that fits is {bad[4]} ({bad[4] // pre.dots.resolution} bins)" if bad[4]
                    else "no window fits")
            raise SystemExit(f"--dots-window: the window of {bad[1]} ({bad[2]} bins of {pre.dots.resolution}) with "
                             f"{pre.dots.min_diag} diagonals ignored does not fit the band of {bad[0]} ({bad[3]} "
                             f"diagonals): {fits}")
    if pre.pileup is not None and pre.pileup.path is not None:
        bad = driver.pileup_misfit(plan, int(cfg.bin_size), pre.pileup.resolution, pre.pileup.flank, pre.pileup.sources)
        if bad is not None and bad[0] == "bedpe":
            raise SystemExit(f"--pileup-at {bad[1]}: the file cannot be read as BEDPE: {bad[2]}")
        if bad is not None:
            raise SystemExit(f"--pileup-flank: the flank of {bad[2]} ({bad[3]} bins of {pre.pileup.resolution}) does "
                             f"not fit the band of {bad[1]} ({bad[4]} diagonals): the largest flank that fits is "
                             f"{bad[5]} ({bad[5] // pre.pileup.resolution} bins)")
    if pre.domains is not None and pre.domains.path is not None:
        # (with --call-domains the source `called` is no file: it stands for the domains the run calls)
        sources = [x for x in pre.domains.sources if pre.domain_calls is None or x != driver.CALLED_DOMAINS]
        bad = driver.domains_misfit(plan, int(cfg.bin_size), pre.domains.resolution, pre.domains.size, sources)
        if bad is not None and bad[0] == "bed":
            raise SystemExit(f"--domains-at {bad[1]}: the file cannot be read as BED: {bad[2]}")
        if bad is not None:
            raise SystemExit(f"--domains-size: no window reaches {bad[1]} bins of {pre.domains.resolution}: the "
                             f"deepest band has {bad[2]} diagonals")
    cmp_ = pre.stripes
    if cmp_ is not None:
        bad = driver.stripes_misfit(plan, int(cfg.bin_size), cmp_.resolution, cmp_.metrics, cmp_.ref_bin_size,
                                    cmp_.ref_chroms, chroms)
        if bad is not None:
            raise SystemExit(f"--compare-to {cmp_.reference}: {bad}")
    if pre.scc is not None:
        bad = driver.scc_misfit(plan, int(cfg.bin_size), cmp_.resolution, pre.scc.smooth, pre.scc.max_distance,
                                pre.scc.min_diag)
        if bad is not None:
            raise SystemExit(f"--scc: {bad}")
    calls = pre.stripe_calls
    if calls is not None and calls.path is not None:
        bad = driver.stripe_calls_misfit(plan, int(cfg.bin_size), calls.resolution, calls.lengths, calls.flank)
        if bad is not None:
            raise SystemExit(f"--call-stripes-lengths: {bad}: widen the band with -w")
    return driver.dense_regions(plan, int(cfg.bin_size), chroms, a.dense_region) if a.dense_region else []


def open_simulator(cfg, pre, backend="nccl"):
    """the process group when there are several ranks (`backend`: --dist-backend), and the simulator
    on this rank's device"""
    if pre.world > 1:
        import torch
        import torch.distributed as dist

        torch.cuda.set_device(pre.device)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", pre.device))
        else:
            dist.init_process_group("gloo")
    return api.Simulator(cfg, pre.device)


def run_plan(sim, a, cfg, plan, pre, log):
    """Enqueues the plan, launches it and waits: the interval ids and, with several ranks, the torch
    tensors the kernel accumulated into (else None), for driver.write_outputs"""
    if pre.outputs.state_log is not None:
        # (with --skip-output the log would not be written: nothing is recorded, and the
        # default build of the library serves, like the reference accepts the combination)
        sim.enable_state_log(a.internal_state_max_epochs)
    tensors = None
    if pre.world > 1:
        import torch

        # the matrices are torch tensors the kernel accumulates into: they are reduced in
        # place and rank 0 extracts its pixels from the reduced tensor, without a host copy
        dev = torch.device("cuda", pre.device)
        tensors = [None if e["skipped"] else
                   (torch.zeros(e["nrows"] * e["ncols"] + 1, dtype=torch.int32, device=dev),
                    torch.zeros(e["ncols"], dtype=torch.int64, device=dev)) for e in plan]
        torch.cuda.synchronize(dev)
    ids = driver.enqueue_plan(sim, cfg, plan, device_buffers=None if tensors is None else [
        (None, None) if t is None else (t[0].data_ptr(), t[1].data_ptr()) for t in tensors])
    n_tasks = sum(len(e["tasks"]) for e in plan if not e["skipped"])
    log(f"simulating {n_tasks} (interval, cell) tasks on device {pre.device} (rank {pre.rank} of {pre.world})")
    sim.launch()
    sim.wait()
    log(f"simulation kernel: {sim.kernel_ms() / 1e3:.2f} s")
    return ids, tensors


def output_stage(sim, a, cfg, plan, ids, tensors, pre, regions, chroms, log, generated_by, backend="nccl"):
    """driver.write_outputs for the plan `pre`, with the attributes every cooler of the run carries: the
    arguments that were given as the metadata, --assembly-name, --force and the chromosomes of the genome"""
    meta = json.dumps({k: v for k, v in vars(a).items() if v is not None and k != "command"}, sort_keys=True)
    return driver.write_outputs(sim, cfg, plan, ids, tensors, pre, regions, log, backend, assembly=a.assembly_name,
                                generated_by=generated_by, metadata_json=meta, force_overwrite=a.force, chroms=chroms)


def simulate(a, log=print):
    """preflight (arguments only) -> plan_run -> open_simulator -> run_plan -> output_stage,
    and the bigwig once the simulator is closed"""
    cfg = config_from_args(a)
    pre = preflight(a, cfg)
    t0 = time.time()
    chroms, plan, regions = plan_run(a, cfg, pre, log)
    sim = open_simulator(cfg, pre, a.dist_backend)
    try:
        ids, tensors = run_plan(sim, a, cfg, plan, pre, log)
        # The contact matrices stay on the device: the cooler is written from their non-zero
        # pixels, extracted there (libmodle_pixels.so), and the warning uses the extraction's sum.
        occupancies = output_stage(sim, a, cfg, plan, ids, tensors, pre, regions, chroms, log, "modle_amd (MI355X)",
                                   a.dist_backend)
    finally:
        sim.close()
    if pre.rank == 0 and pre.outputs.bigwig is not None:
        driver.write_bigwig(pre.outputs.bigwig, cfg, plan, occupancies, chroms, force_overwrite=a.force)
        log(f"written {pre.outputs.bigwig}")
    if pre.world > 1:
        import torch.distributed as dist

        dist.destroy_process_group()
    log(f"done in {time.time() - t0:.1f} s")
    return 0


ANALYSIS_SCRATCH_BANDS = 4  # what the analyses hold at once besides the bands: coarse, dot candidates, kept, rest


def analyze_plan(cfg, reader, names):
    """a plan of driver.plan_genome's shape for the chromosomes `names` of the open cooler `reader`, in the
    file's order: every chromosome one interval from 0 with the band api.matrix_shape gives it, no barriers
    and no tasks"""
    plan = []
    for name, size in reader.chroms:
        if name in names:
            nrows, ncols = api.matrix_shape(cfg, int(size))
            iv = {"name": name, "size": int(size), "start": 0, "end": int(size), "bar_pos": [], "bar_dir": []}
            plan.append({"interval": iv, "nrows": nrows, "ncols": ncols, "tasks": None, "skipped": False})
    return plan


def check_band_memory(plan, free_bytes, table_bytes=0):
    """SystemExit when the bands of the plan and the scratch of the analyses, ANALYSIS_SCRATCH_BANDS times the
    largest band and `table_bytes`, the largest triangle table of --call-domains
    (driver.domain_calls_table_bytes), exceed `free_bytes` of device memory"""
    sizes = [(e["nrows"] * e["ncols"] + 1) * 4 for e in plan]
    need = sum(sizes) + ANALYSIS_SCRATCH_BANDS * max(sizes, default=0) + int(table_bytes)
    if table_bytes and need > free_bytes:
        raise SystemExit(f"analyze: the bands of the {len(plan)} chromosomes ({sum(sizes)} bytes), the scratch of "
                         f"the analyses ({ANALYSIS_SCRATCH_BANDS} times the largest band, {max(sizes)} bytes) and the "
                         f"triangle table of --call-domains ({int(table_bytes)} bytes) need {need} bytes; the device has "
                         f"{int(free_bytes)} free: lower --call-domains-max-width, narrow the band with -w or take "
                         "fewer chromosomes with --chromosomes")
    if need > free_bytes:
        raise SystemExit(f"analyze: the bands of the {len(plan)} chromosomes ({sum(sizes)} bytes) and the scratch of "
                         f"the analyses ({ANALYSIS_SCRATCH_BANDS} times the largest band, {max(sizes)} bytes) need "
                         f"{need} bytes; the device has {int(free_bytes)} free: narrow the band with -w or take fewer "
                         "chromosomes with --chromosomes")


def load_bands(bands, reader, plan, log):
    """Loads every chromosome of the plan from `reader` into `bands` (an api.LoadedBands); a chromosome without a
    pixel in its band is marked skipped, as simulate skips one without barriers.  Returns the ids per entry
    (None: skipped).  SystemExit: a pixel list that is out of order or holds a negative count."""
    from . import pixels

    ids = []
    for entry in plan:
        name = entry["interval"]["name"]
        bin1, bin2, count, first = reader.pixels(name)
        try:
            bid, st = bands.load_pixels(bin1, bin2, count, entry["nrows"], entry["ncols"], first)
        except pixels.BandListError as e:
            what = "is not after its predecessor in (bin1, bin2)" if e.code == pixels.ERR_ORDER else \
                "has a negative count"
            raise SystemExit(f"{reader.uri}: chromosome {name}: pixel {e.stats.first_bad} of its {len(bin1)} {what}: "
                             "the file is no valid cooler")
        log(f"{name}: {st.n_in} pixels in the band ({st.sum_in} contacts), beyond the band {st.n_beyond} pixels "
            f"({st.sum_beyond} contacts), outside {st.n_outside} pixels ({st.sum_outside} contacts)")
        if st.n_in == 0:
            bands.release(bid)
            entry["skipped"] = True
            bid = None
        ids.append(bid)
    return ids


def analyze(a, log=print):
    """The analyses of simulate on a file: refusals (arguments, file, outputs) -> the plan -> the bands on the
    device (api.LoadedBands) -> check_plan -> output_stage, which writes what it writes for simulate"""
    from . import cooler

    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("analyze runs on one GPU: WORLD_SIZE is above 1")
    if a.pileup_at and "barriers" in a.pileup_at:
        raise SystemExit("--pileup-at barriers: a file has no barriers; give `dots` or a BEDPE file")
    if a.subsample_seed is None and (a.subsample_frac is not None or a.subsample_to is not None):
        a.subsample_seed = 0
    t0 = time.time()
    try:
        reader = cooler.CoolerReader(a.input)
    except cooler.CoolerError as e:
        raise SystemExit(f"analyze: cannot read {a.input}: {e}")
    with reader:
        names = [n for n, _ in reader.chroms] if a.chromosomes is None else \
            [n for n in a.chromosomes.split(",") if n]
        for name in names:
            if name not in dict(reader.chroms):
                raise SystemExit(f"--chromosomes: {name} is not a chromosome of {a.input} "
                                 f"({', '.join(n for n, _ in reader.chroms)})")
        over = {"bin_size": int(reader.bin_size), "track_1d_lef_position": 0}
        if a.diagonal_width is not None:
            over["diagonal_width"] = int(a.diagonal_width)
        cfg = api.make_config(**over)
        pre = preflight(a, cfg)
        plan = analyze_plan(cfg, reader, set(names))
        import torch

        table = 0 if pre.domain_calls is None else driver.domain_calls_table_bytes(plan, int(cfg.bin_size),
                                                                                    pre.domain_calls)
        check_band_memory(plan, torch.cuda.mem_get_info(pre.device)[0], table)
        bands = api.LoadedBands(pre.device)
        try:
            ids = load_bands(bands, reader, plan, log)
            regions = check_plan(a, cfg, pre, plan, reader.chroms)
            output_stage(bands, a, cfg, plan, ids, None, pre, regions, reader.chroms, log, "modle_amd analyze (MI355X)")
        finally:
            bands.close()
    log(f"done in {time.time() - t0:.1f} s")
    return 0


def evaluate_cmd(a):
    """prints one JSON object: {chromosome: {vertical: summary, horizontal: summary}}"""
    from . import evaluate as ev

    cfg = api.make_config()
    chroms, _, _ = genome.import_genome_text(cfg, genome.read_text(a.chrom_sizes), b"")
    res = ev.compare_coolers(a.reference_cooler, a.input_cooler, [n for n, _ in chroms],
                             a.diagonal_width, a.metric, a.exclude_zero_pixels)
    print(json.dumps({"metric": a.metric, "chromosomes": res}, indent=1))
    return 0


def main(argv=None):
    a = build_parser().parse_args(argv)
    if a.command in ("evaluate", "eval"):
        return evaluate_cmd(a)
    if a.command in ("analyze", "an"):
        return analyze(a, (lambda *x: None) if a.quiet else (lambda *x: print(*x, file=sys.stderr, flush=True)))
    if a.log_model_internal_state and not a.skip_output:
        # the recording code lives in a diagnostic build of the library, chosen at import time
        from . import _lib

        if _lib._lib is not None and "statelog" not in _lib.SO_PATH:
            raise SystemExit("--log-model-internal-state needs MODLE_HIP_LIB=libmodle_hip_statelog.so "
                             "to be set before modle_amd is imported")
        if _lib._lib is None:
            _lib.SO_PATH = os.path.join(os.path.dirname(_lib.SO_PATH), "libmodle_hip_statelog.so")
    log = (lambda *x: None) if a.quiet else (lambda *x: print(*x, file=sys.stderr, flush=True))
    return simulate(a, log)
