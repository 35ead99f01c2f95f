# same-box comparison of builds of the library: ab.sh <rounds> <libA.so> <libB.so> [...]
# (file names inside modle_amd/; one bench.py run per build and round, kernel time from HIP events).
# The order of the builds is reversed in every other round: the second run of a pair tends to be a
# per cent or two slower than the first whatever it runs (clocks), which is more than most of the
# differences this script is asked about.
# Every run is a fresh process under a time limit of its own (AB_STEP_TIMEOUT seconds, default 300), and
# the first run that fails or runs out of time ends the script: nothing more is started on that GPU.
R=$GRAFT_REPO_ROOT; N=$1; shift
T=$(mktemp -d)  # the bench line and the error output of the run in hand
AB_BENCH_ARGS="--full $AB_BENCH_ARGS"  # (the `checked` column: the self-check runs with --full only)
for r in $(seq 1 $N); do
  if [ $((r % 2)) -eq 1 ]; then order="$@"; else order=$(echo "$@" | tr ' ' '\n' | tac | tr '\n' ' '); fi
  for v in $order; do
    MODLE_HIP_LIB=$v timeout -k 10 ${AB_STEP_TIMEOUT:-300} python3 $R/bench.py --steps 1 --warmup 0 --no-cpu-baseline $AB_BENCH_ARGS > $T/ab.json 2> $T/ab.err
    rc=$?
    if [ $rc -ne 0 ]; then echo "$v: bench.py ended with status $rc (round $r): stopping"; tail -5 $T/ab.err; exit $rc; fi
    python3 -c "import json;d=json.load(open('$T/ab.json'));print('$v', round(d['roofline']['kernel_ms'],1), d['checked'], round(d['value'],2))" || exit 1
  done
done
