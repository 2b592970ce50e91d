LOG=$(mktemp); timeout -k 10 300 python bench.py --full --no-train-step --no-cpu-baseline --no-parity > $LOG 2>&1; python - $LOG <<PY
import json, sys
for l in open(sys.argv[1]):
    if l.startswith("{"):
        j=json.loads(l); print("BENCH", j["value"], j["ms_per_step"], j["roofline"]["kernel_ms"], j["free_running"]["value"], j["free_running"]["kernel_ms"])
PY
rm -f $LOG
