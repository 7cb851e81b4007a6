#!/bin/bash
L=$GRAFT_REPO_ROOT/bayesfmmm_amd/libbfmmm_hip.so
echo "== config4"; bash tools/kstat.sh $L config4 1
echo "== config4 again"; bash tools/kstat.sh $L config4 1 | grep chi
