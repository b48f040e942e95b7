#!/bin/bash
# bench.py through its N > 1 code path on ONE GPU (world-1 RCCL communicators, ISEGMI_BENCH_FORCE_DIST=1), next to the plain N = 1 run: same box
# (JSON lines and logs under $OUT_DIR/fd, default bench_out/fd)
set -e -o pipefail
out=${OUT_DIR:-bench_out}/fd
mkdir -p $out
export HSA_ENABLE_IPC_MODE_LEGACY=0
python bench.py --steps 40 --warmup 10 --full --no-cpu-baseline --no-latency "$@" > $out/plain.json 2> $out/plain.err
ISEGMI_BENCH_FORCE_DIST=1 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29517 bench.py --gpus 1 --steps 40 --warmup 10 --full --no-cpu-baseline --no-latency "$@" > $out/forced.json 2> $out/forced.err
python - "$out" <<'PY'
import json, os, sys
for n in ("plain", "forced"):
    d = json.loads([l for l in open(os.path.join(sys.argv[1], "%s.json" % n)) if l.startswith("{")][0])
    print("%-7s value %.1f resident %.1f e2e %.1f  rccl_ranks %s" % (n, d["value"], d.get("value_resident", 0), d.get("value_e2e", 0), d.get("rccl_ranks")))
PY
