#!/bin/bash
# End-of-iteration GPU run (bash tools/profiling/run_round.sh [prefix], on the GPU machine): GPU tests, smoke, the separate --pmc
# passes of the bench command, then the full bench line (bench.py --full, which quotes the PMC summary just taken: HBM traffic and
# VALU instructions per berg-step at the population it runs) and the rocprofv3 --stats summary of the same command.  Outputs land
# in $OUT (default out/ in the repository); the ones to keep are copied to profiles/ by tools/profiling/keep_round.sh.
R=$GRAFT_REPO_ROOT
P=${1:-r03}
cd $R
OUT=$(realpath -m "${OUT:-out}"); mkdir -p "$OUT"
python -m pytest tests -m gpu -q > "$OUT/pytest_gpu_round.log" 2>&1; echo "pytest exit=$?" | tee -a "$OUT/pytest_gpu_round.log"; tail -3 "$OUT/pytest_gpu_round.log"
python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke_round.log" 2>&1; tail -1 "$OUT/smoke_round.log"
bash tools/profiling/run_pmc.sh > "$OUT/round_pmc_summary.json" 2> "$OUT/round_pmc.err"
# (on the box: what bench.py reads below) -- only a summary whose five passes all completed replaces the committed one
if python3 -c "import json,sys; sys.exit(0 if json.load(open(sys.argv[1])).get('complete') else 1)" "$OUT/round_pmc_summary.json"; then
  cp "$OUT/round_pmc_summary.json" profiles/${P}_pmc_summary.json
else
  echo "PMC passes incomplete: profiles/${P}_pmc_summary.json left as it is" | tee -a "$OUT/round_pmc.err"
fi
cd $R
python bench.py --full > "$OUT/bench_round.log" 2>&1; tail -1 "$OUT/bench_round.log" | cut -c1-400
cd /tmp; export TMPDIR=/tmp
rm -rf "$OUT/prof_round"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_round" -- python3 $R/bench.py --steps 40 --warmup 5 > "$OUT/prof_round.log" 2>&1
cp "$OUT"/prof_round/*/*kernel_stats.csv "$OUT/round_kernel_stats.csv"
head -c 600 "$OUT/round_kernel_stats.csv"
