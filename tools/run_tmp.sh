for d in "0.06,0.06,0.22" "0.07,0.07,0.25" "0.08,0.08,0.3"; do
  python bench.py --full --no-cpu-baseline --steps 6 --warmup 2 --densities $d 2> /dev/null | python -c "
import json, sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('$d |', round(d['value']/1e6,2), 'M parity', d.get('parity_checked'), 'S', d['config']['streams_per_workgroup'], 'blocks', d['config']['gru_a_blocks'], 'frac', round(d['roofline']['frac'],3))"
done
