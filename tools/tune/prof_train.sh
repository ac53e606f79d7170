R=$(cd "$(dirname "$0")/../.." && pwd); OUT=${FAC_TUNE_OUT:-$R/tune_out}; mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/tstats -o t -- python $R/tools/train_bench.py --batch 16 --steps 2 --warmup 1 > $OUT/tstats.log 2>&1
tail -1 $OUT/tstats.log | cut -c1-400
