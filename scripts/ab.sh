#!/bin/bash
# A/B of library variants on the default bench inside ONE gpurun call (box-to-box spread is larger than most effects):
#   bash scripts/ab.sh [rounds] item...     item = lib | lib,ENV=VAL[,ENV=VAL...]    ("default" = the in-tree library)
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
R=$1; shift
for i in $(seq 1 $R); do
  for item in "$@"; do
    IFS=',' read -ra parts <<< "$item"
    l=${parts[0]}
    envs=("${parts[@]:1}")
    if [ "$l" = default ]; then libenv=(); else libenv=("CLASSPRO_AMD_LIB=$GRAFT_REPO_ROOT/$l"); fi
    out=$(env "${libenv[@]}" "${envs[@]}" python bench.py --full --no-cpu --no-extras --steps 10 --warmup 3 2>&1)
    python - "$item" "$out" <<'PY'
import json,sys
try:
    j=json.loads([l for l in sys.argv[2].splitlines() if l.startswith("{")][-1]); print("%-44s %9.1f Mbases/s  %7.3f ms/step  scan %.1f us frac %.3f" % (sys.argv[1], j["value"], j["ms_per_step"], j["roofline"]["ms_per_launch"]*1e3, j["roofline"]["frac"]))
except Exception as e:
    print(sys.argv[1], "FAILED", e, sys.argv[2][-400:])
PY
  done
done
