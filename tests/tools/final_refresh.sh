# End-of-round refresh on a GPU machine: GPU suite, smoke, the --full bench line of c2 / c3 / c4 / c5, a kernel trace of the default --full command and
# the HBM traffic of the headline's loop kernels (two separate PMC passes, never combined with other trace domains).  Stops at the first failing step.
# Usage: bash tests/tools/final_refresh.sh <output dir>
set -o pipefail
R=$(cd "$(dirname "$0")/../.." && pwd); cd $R || exit 1
mkdir -p "${1:?usage: final_refresh.sh <output dir>}" && O=$(cd "$1" && pwd) || exit 1
step() { # log name, seconds, command...
  n=$1; s=$2; shift 2
  timeout -k 10 $s "$@" > $O/$n.log 2>&1 || { echo "$n failed ($?)"; tail -5 $O/$n.log; exit 1; }
}
step pytest_gpu 900 python -m pytest tests -m gpu -q; tail -2 $O/pytest_gpu.log
step smoke 120 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')"; tail -1 $O/smoke.log
for c in c2 c3 c4 c5; do
  step bench_$c 600 python bench.py --full --config $c; tail -1 $O/bench_$c.log > $O/bench_$c.json; cut -c1-300 $O/bench_$c.json
done
cd /tmp && export TMPDIR=/tmp
step prof 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -o bench -- python3 $R/bench.py --full
cd $R; f=$(find $O/prof -name "*kernel_stats.csv" | head -1); echo stats=$f; python tests/tools/print_stats.py $f 8
cd /tmp
step pmc_f 300 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/pmc_f -o f -- python3 $R/bench.py --steps 4
step pmc_w 300 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $O/pmc_w -o w -- python3 $R/bench.py --steps 4
cd $R; ff=$(find $O/pmc_f -name "*counter_collection.csv" | head -1); fw=$(find $O/pmc_w -name "*counter_collection.csv" | head -1)
python tests/tools/pmc_summary.py $ff $fw $O/pmc_traffic.json > $O/pmc_traffic.txt 2>&1; sed -n 1,6p $O/pmc_traffic.txt
