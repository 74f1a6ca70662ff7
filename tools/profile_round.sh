# Round profile: rocprofv3 kernel-trace summary + the two PMC passes (FETCH_SIZE, WRITE_SIZE: separate runs, no trace domains) of bench.py,
# once per precision.  Run on an MI355X:  GG_GIT_HEAD=<commit> bash tools/profile_round.sh <fp32|bf16> <tag> [out dir, default profile_out]  -> <out dir>/<tag>_*
# (a copy of the tree without .git: pass the commit in; the JSON also records the sha256 of the kernel sources, which bench.py checks)
set -x
P=${1:-fp32}
TAG=${2:-r05_$P}
cd "$(dirname "$0")/.."
O=${3:-profile_out}
mkdir -p "$O" && O=$(cd "$O" && pwd)
export TMPDIR=/tmp
rm -rf $O/${TAG}_trace $O/${TAG}_fetch $O/${TAG}_write
timeout -k 10 500 rocprofv3 --kernel-trace --stats -d $O/${TAG}_trace -o t --output-format csv -- python3 bench.py --full --steps 4 --warmup 2 --no-cpu-baseline --no-secondary --precision $P --dump-launches $O/${TAG}_launches > $O/${TAG}_trace.log 2>&1 || exit 1
tail -1 $O/${TAG}_trace.log | cut -c1-300
timeout -k 10 500 rocprofv3 --pmc FETCH_SIZE -d $O/${TAG}_fetch -o f --output-format csv -- python3 bench.py --steps 2 --warmup 1 --precision $P > $O/${TAG}_fetch.log 2>&1
timeout -k 10 500 rocprofv3 --pmc WRITE_SIZE -d $O/${TAG}_write -o w --output-format csv -- python3 bench.py --steps 2 --warmup 1 --precision $P > $O/${TAG}_write.log 2>&1
F=$(find $O/${TAG}_fetch -name "*counter_collection.csv" | head -1); W=$(find $O/${TAG}_write -name "*counter_collection.csv" | head -1)
GG_PMC_COMMAND="python3 bench.py --steps 2 --warmup 1 --precision $P" python3 tools/pmc_traffic.py $F $W 3 $O/${TAG}_hbm_traffic_pmc.json $O/${TAG}_launches.$P.json $O/${TAG}_gemm_forms_traffic.txt
cp $O/${TAG}_hbm_traffic_pmc.json $O/${TAG%%_*}_hbm_traffic_pmc_$P.json      # the name bench.py's `roofline.traffic` reads under profiles/
S=$(find $O/${TAG}_trace -name "*kernel_stats.csv" | head -1); cp $S $O/${TAG}_kernel_stats.csv
# keep the output small: drop the raw per-dispatch tables
rm -rf $O/${TAG}_trace $O/${TAG}_fetch $O/${TAG}_write
ls -la $O | grep ${TAG}
