# column-split wave layouts of the weight gradient (FAC_WGRAD_NARROW) + the rest of the weight-batch tests: tests, per-shape bench, train A/B
R=$(cd "$(dirname "$0")/../.." && pwd); OUT=${FAC_TUNE_OUT:-$R/tune_out}; mkdir -p $OUT
O=$OUT/${1:-wgn_ab}; mkdir -p $O
cd $R
timeout 1500 python -m pytest tests/test_weight_batch.py tests/test_wgrad_split.py -x -q -m gpu 2>&1 | tail -15 | tee $O/test.log
for nv in 0 1; do
  echo "FAC_WGRAD_NARROW=$nv" | tee -a $O/wgrad_bench.log
  FAC_WGRAD_NARROW=$nv timeout 600 python tools/wgrad_bench.py 2>>$O/err.log | tee -a $O/wgrad_bench.log
done
for i in 1 2 3; do
  for nv in 0 1; do
    FAC_WGRAD_NARROW=$nv python tools/train_bench.py --batch 16 --steps 6 --warmup 3 --predictors 2>>$O/err.log | tail -1 | python -c "
import json,sys; d=json.loads(sys.stdin.readline()); print('train FAC_WGRAD_NARROW=$nv', d.get('ms_per_step'), d.get('loss'))" | tee -a $O/ab.log
  done
done
tail -5 $O/err.log
