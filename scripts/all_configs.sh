# every BASELINE configuration and training mode, one line each (also written, as it runs, to $ALL_CONFIGS_LOG when set)
LOG=${ALL_CONFIGS_LOG:-/dev/null}; : > "$LOG"
for a in "" "--all-reference-calls" "--config 2" "--config 4" "--config 5" "--train-adapters" "--train-adapters --train-encoder" "--operand bf16"; do
  python bench.py $a --steps 8 --warmup 3 --full --no-cpu-baseline --no-secondary 2>/dev/null | python -c "import sys,json; j=json.loads([l for l in sys.stdin if l.startswith('{')][-1]); print('$a', j['value'], j['ms_per_step'], j['roofline']['achieved'], 'precise_level', j['config'].get('precise_level'), 'split_attn_out', j['config'].get('split_attn_out'))" | tee -a "$LOG"
done
