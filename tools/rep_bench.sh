# development: is the short-window bench reproducible?  (driver flags, fresh process each time)  usage: tools/rep_bench.sh [out-dir]
O=${1:-rep_bench_out}
mkdir -p $O; rm -f $O/rep.txt
for i in 1 2 3 4 5 6 7 8; do python3 bench.py --gpus 1 --steps 20 --warmup 5 2>/dev/null | python3 -c "
import json,sys
for l in sys.stdin:
    if l.startswith('{'):
        d=json.loads(l); print('run', round(d['value']), round(d['ms_per_step'],3), round(d['roofline']['kernel_ms'],3), d['host'])
" >> $O/rep.txt; done
python3 bench.py --full --gpus 1 --steps 20 --warmup 5 > $O/rep_full1.json 2>/dev/null
python3 bench.py --full --gpus 1 --steps 100 --warmup 100 > $O/rep_full2.json 2>/dev/null
BENCH_BACKEND=gloo python3 bench.py --gpus 2 --envs 1024 --steps 20 --warmup 5 > $O/rep_2rank.json 2>$O/rep_2rank.err
