#!/bin/bash
# tools/ab_build.sh [--csrc DIR] NAME [extra hipcc flags...] : builds nextsimdg_amd/lib/alt/NAME/libnsdg.so for an A/B run
# (tools/ab_bench.py, NSDG_LIB).  Sources and flags are those of the build.py beside the csrc directory, so the library is whole
# and loads.  --csrc DIR takes the sources from another checkout (DIR = <checkout>/nextsimdg_amd/csrc): that is how the parent
# commit is built next to the working tree.
set -e
cd "$(dirname "$0")/.."
csrc=nextsimdg_amd/csrc
if [ "$1" = --csrc ]; then
  csrc=$2; shift 2
fi
name=$1; shift
out=nextsimdg_amd/lib/alt/$name
mkdir -p "$out"
recipe=$(python3 -c 'import runpy, sys; b = runpy.run_path(sys.argv[1]); print(*b["SOURCES"]); print(*b["FLAGS"])' "$(dirname "$csrc")/build.py")
read -r -a SOURCES <<< "$(sed -n 1p <<< "$recipe")"
read -r -a FLAGS <<< "$(sed -n 2p <<< "$recipe")"
objs=(); pids=()
for s in "${SOURCES[@]}"; do
  o=$out/${s%.hip}.o
  hipcc "${FLAGS[@]}" "$@" -c "$csrc/$s" -o "$o" &
  pids+=($!); objs+=("$o")
done
for p in "${pids[@]}"; do wait "$p"; done
hipcc --offload-arch=gfx950 -shared -fPIC -o "$out/libnsdg.so" "${objs[@]}" -ldl -lpthread
echo built "$out/libnsdg.so"
