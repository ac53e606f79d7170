# forward (configs[1]) A/B on one box, alternating: $2 = environment of the B leg
R=$(cd "$(dirname "$0")/../.." && pwd); OUT=${FAC_TUNE_OUT:-$R/tune_out}; mkdir -p $OUT
O=$OUT/${1:-fwd_ab}; mkdir -p $O
cd $R
for i in 1 2; do
  python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-train --no-streaming 2>>$O/err.log | tail -1 | python -c "
import json,sys; d=json.loads(sys.stdin.readline()); print('baseline', d['value'], d['ms_per_step'], d['roofline']['frac'], d.get('codes_match'))" | tee -a $O/ab.log
  env $2 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-train --no-streaming 2>>$O/err.log | tail -1 | python -c "
import json,sys; d=json.loads(sys.stdin.readline()); print('$2', d['value'], d['ms_per_step'], d['roofline']['frac'], d.get('codes_match'))" | tee -a $O/ab.log
done
