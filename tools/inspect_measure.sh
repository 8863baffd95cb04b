#!/bin/bash
# The three records of the table walk (bns_table_tally): tools/inspect_measure.sh OUT_DIR "walk cli bench" [PARENT_TREE] [reps of the 10 M-read file = 3]
#   walk   OUT_DIR/inspect.txt           one walk of the benchmark db's table: wall per call, kernel times (a traced run of its own), the numpy model
#   cli    OUT_DIR/inspect_cli.txt       bonsai classify -K -R -u with and without -d on one plain FASTQ file, alternating
#   bench  OUT_DIR/inspect_bench_ab.txt  python bench.py of PARENT_TREE (a built checkout of the parent commit) and of this tree, alternating
# Each step that uses the GPU runs under a time limit of its own and the script stops at the first that fails.
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${1:?output directory}; WHAT=${2:-walk cli bench}; PARENT_TREE=${3:-}; REP=${4:-3}
mkdir -p "$OUT"
D=$(mktemp -d /tmp/inspect_db.XXXXXX)
trap 'rm -rf "$D"' EXIT
die() { echo "step failed: $*" >&2; exit 1; }

if [[ "$WHAT" == *walk* || "$WHAT" == *cli* ]]; then
  timeout -k 10 420 python bench.py --save-db "$D" --save-reads 10000000 --steps 2 --warmup 1 --no-cpu --no-probe --no-text --no-inflate 2>/dev/null > "$D/db.txt" || die "bench.py --save-db"
fi

if [[ "$WHAT" == *walk* ]]; then
  {
    echo "# tools/inspect_bench.py on the benchmark db (bench.py --save-db): wall per call, host clock around bns_table_tally; the numpy model on the same khash arrays"
    timeout -k 10 420 python tools/inspect_bench.py "$D" 5 || die "inspect_bench.py"
    echo "# the same under rocprofv3 --kernel-trace --stats, a run of its own (inspect_minb_kernel<false>: upper half-lines, <true>: whole lines)"
  } > "$OUT/inspect.txt"
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$D/prof" -o walk --output-format csv -- python tools/inspect_bench.py "$D" 5 --no-model > "$D/prof.log" 2>&1 || { tail -5 "$D/prof.log" >&2; die "rocprofv3"; }
  STATS=$(find "$D/prof" -name '*kernel_stats.csv' | head -1)
  [ -n "$STATS" ] || die "no kernel_stats.csv"
  { head -1 "$STATS"; grep -E "inspect_|clade_" "$STATS"; } >> "$OUT/inspect.txt"
fi

if [[ "$WHAT" == *cli* ]]; then
  rm -f "$D/long.fq"; for i in $(seq "$REP"); do cat "$D/reads.fq" >> "$D/long.fq"; done
  cat "$D/long.fq" "$D/bns.db" > /dev/null
  run() {
    local t0 t1; t0=$(date +%s.%N)
    timeout -k 10 300 env BNS_CLI_TIMING=1 bonsai_amd/bin/bonsai classify -K -R "$D/r.report" -u "$@" "$D/bns.db" "$D/nodes.dmp" "$D/long.fq" > /dev/null 2> "$D/err.txt" || { tail -5 "$D/err.txt" >&2; die "bonsai classify $*"; }
    t1=$(date +%s.%N)
    grep -E "process_dataset|report " "$D/err.txt" | tr '\n' ' '
    python3 -c "print('  wall %.3f s  [%s]' % ($t1 - $t0, '-u $*'))"
  }
  {
    echo "# bonsai classify -K -R -u [-d] on $((REP * 10)) M reads of plain FASTQ against the benchmark db, alternating"
    run > /dev/null
    for i in 1 2 3; do run; run -d; done
    echo "# the report's last lines with -d"
    tail -3 "$D/r.report"
  } > "$OUT/inspect_cli.txt"
fi

if [[ "$WHAT" == *bench* ]]; then
  [ -f "$PARENT_TREE/bench.py" ] || die "bench: a built checkout of the parent commit is needed"
  {
    echo "# python bench.py (default) of the parent commit and of this tree, alternating on one box"
    for i in 1 2 3; do
      for which in parent this; do
        tree=.; [ $which = parent ] && tree="$PARENT_TREE"
        line=$(timeout -k 10 400 python "$tree/bench.py" 2> "$D/bench_err.txt" | tail -1) || { tail -5 "$D/bench_err.txt" >&2; die "bench.py ($which)"; }
        echo "$which $(echo "$line" | python3 -c "import json,sys; r=json.loads(sys.stdin.read()); print('value %.5g reads/s  ms_per_step %.4f' % (r['value'], r['ms_per_step']))")"
      done
    done
  } > "$OUT/inspect_bench_ab.txt"
fi
