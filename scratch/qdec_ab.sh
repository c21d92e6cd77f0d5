#!/bin/bash
# the quality decoder alone under the variant builds scratch/libsfq_qalone_*.so, then the full bench's decode leg with the in-tree library and scratch/libsfq_flat.so
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}; cd $ROOT
cp slimfastq_amd/libslimfastq_amd.so /tmp/lib_keep.so
for f in scratch/libsfq_qalone_*.so; do echo "== $f"; cp $f slimfastq_amd/libslimfastq_amd.so; timeout -k 10 200 python3 scratch/qalone.py 10000000 0 2>&1 | grep "EXP" | tr '\n' ' '; echo; done
cp /tmp/lib_keep.so slimfastq_amd/libslimfastq_amd.so
B="--full --steps 5 --warmup 2 --no-size-sweep --no-cpu-baseline --no-genome-leg --no-format6-leg --no-adaptive-leg --no-host-leg"
show() { python3 -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(d['value'], d['ms_per_step'], d['decode']['ms'], d['decode']['round_trip_identical'], d['decode']['phase_ms'])"; }
for i in 1 2; do
  echo "== in-tree"; cp /tmp/lib_keep.so slimfastq_amd/libslimfastq_amd.so; python3 bench.py $B 2>/dev/null | show
  echo "== flat"; cp scratch/libsfq_flat.so slimfastq_amd/libslimfastq_amd.so; python3 bench.py $B 2>/dev/null | show
done
cp /tmp/lib_keep.so slimfastq_amd/libslimfastq_amd.so
