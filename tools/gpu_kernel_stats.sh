#!/bin/bash
# rocprofv3 kernel-trace stats of one bench workload; prints the top kernels. usage: tools/gpu_kernel_stats.sh <workload> <tag> [steps]
# Outputs under $OUT/<tag> (default: out/ in the repository).
R=$GRAFT_REPO_ROOT; [ -z "$R" ] && R=$(pwd)
W=${1:-semantic_m}; TAG=${2:-stats}; STEPS=${3:-2}
O=${OUT:-$R/out}; mkdir -p $O
export TMPDIR=/tmp
cd /tmp
rm -rf $O/$TAG
rocprofv3 --kernel-trace --stats --output-format csv -d $O/$TAG -- python3 $R/bench.py --full --full-line --workload $W --steps $STEPS --warmup 1 --no-cpu-baseline > $O/$TAG.json 2> $O/$TAG.err
cd $R
f=$(find $O/$TAG -name "*kernel_stats.csv" | head -1)
cp $f $O/${TAG}_kernel_stats.csv
head -14 $f | cut -c1-150
find $O/$TAG -name "*.csv" -size +1M -delete; find $O/$TAG -name "*.db" -delete
python3 -c "
import json;d=json.load(open('$O/$TAG.json'));print(d['ms_per_step'],d['token_checksum']);[print(k,v['ms_per_step']) for k,v in d['breakdown'].items()]"
