#!/bin/bash
# time each ablated conv variant (tools/ablate_conv.py) against the full kernel
set -uo pipefail
OUT=gpurun_out/abl
mkdir -p $OUT
for v in noload nostage nowload noepi; do
  timeout -k 10 120 python -u tools/ab_conv.py --epi fwd --rounds 3 --iters 10 \
      --lib-a build/abl/libfull.so --lib-b build/abl/lib$v.so > $OUT/$v.log 2>&1
  rc=$?; [ $rc -eq 0 ] || { tail -5 $OUT/$v.log; exit $rc; }
  echo "== $v"; grep conv3x3 $OUT/$v.log | sed 's/max rel.*//'
done
