R=$(cd "$(dirname "$0")/../.." && pwd); OUT=${FAC_TUNE_OUT:-$R/tune_out}; mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/pmc_f -o f -- python $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-roofline > $OUT/pmc_f.log 2>&1
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/pmc_w -o w -- python $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-roofline > $OUT/pmc_w.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/kstats -o k -- python $R/bench.py --full --steps 4 --warmup 2 --no-cpu-baseline --no-roofline > $OUT/kstats.log 2>&1
find $OUT/pmc_f $OUT/pmc_w $OUT/kstats -name "*.csv" | head -20
tail -2 $OUT/kstats.log
