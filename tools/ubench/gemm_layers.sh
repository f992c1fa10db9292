#!/bin/bash
# per-layer table of the fused conv GEMM (tuning aid): tools/ubench/gemm_layers.sh [extra bench args]
LINE=$(mktemp)
PFANN_PROF_LAYERS=1 python bench.py --full --no-cpu-baseline --no-cli --no-alt --steps 3 --filler-db "$@" > $LINE 2>/dev/null
python tools/per_layer_table.py $LINE
rm -f $LINE
