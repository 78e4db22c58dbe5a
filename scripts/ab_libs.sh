#!/bin/bash
# A/B of library builds on the cfg2 render launch: scripts/ab_libs.sh "<channels>" lib1.so lib2.so ...   (paths relative to selfocc_amd/)
# Each run has its own time limit; the first one that fails ends the A/B (nothing more is started on that GPU).
set -o pipefail
R=${GRAFT_REPO_ROOT:-$(pwd)}; ch=$1; shift
mkdir -p $R/gpurun_out
tmp=$(mktemp)
for round in 1 2; do
  for l in "$@"; do
    SELFOCC_HIP_LIB=$R/selfocc_amd/$l timeout -k 10 300 python $R/scripts/ab_render.py $ch > $tmp 2>&1 ||
      { rc=$?; echo "ab_render.py failed (rc=$rc, lib=$l):"; tail -5 $tmp; exit $rc; }
    grep -E "default|no_face_safe |inv_s_200" $tmp | grep -v no_ahead
  done
done | tee $R/gpurun_out/ab_libs.txt
rc=$?; rm -f $tmp; exit $rc
