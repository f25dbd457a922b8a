#!/usr/bin/env bash
# A/B of the render MLP dataflows on one box: the weight-streamed kernels of the variant library
# (`make -C articulated-object-nerf_amd/csrc variant-ws`) against the release library's LDS-ring
# kernels -- the bit-equality tests (tests/test_gpu_variants.py) and the interleaved timing of
# both on the bench frame's fine level (tools/prof_mlp_ws.py), vanilla and articulated.
# Stops at the first failing step.  Usage: bash scripts/ws_ab.sh OUTDIR (logs go there)
set -u
OUT=${1:?OUTDIR}
mkdir -p "$OUT"; export TMPDIR=/tmp
timeout -k 10 300 python -u -m pytest -x -q -p no:cacheprovider --timeout 120 --timeout-method thread -m gpu \
  tests/test_gpu_variants.py -k ws_equals_streamed > "$OUT/test.log" 2>&1 || { echo "test failed"; tail -5 "$OUT/test.log"; exit 1; }
timeout -k 10 200 python -u tools/prof_mlp_ws.py > "$OUT/prof.log" 2>&1 || exit 1
timeout -k 10 200 python -u tools/prof_mlp_ws.py --art --rays 76800 > "$OUT/prof_art.log" 2>&1 || exit 1
echo "$(tail -1 "$OUT/test.log")"
echo "  vanilla $(tail -1 "$OUT/prof.log")"
echo "  art     $(tail -1 "$OUT/prof_art.log")"
