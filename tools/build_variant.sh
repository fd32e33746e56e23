#!/bin/bash
# build one library variant: tools/build_variant.sh <name> [extra hipcc flags...]  -> htscodecs_amd/variants/lib<name>.so
# (objects are rebuilt from scratch, and a failed compile fails the script: a stale object must never be linked)
set -e
cd "$(dirname "$0")/../htscodecs_amd/csrc"
name=$1; shift
mkdir -p ../variants ../../build/var_$name
rm -f ../../build/var_$name/*.o
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -ffp-contract=off -fno-fast-math -Wno-unused-function -Wno-unused-variable"
# the translation units are the Makefile's: SRC, and SRC_ILP with the Makefile's ILP flags
SRC=$(sed -n 's/^SRC *:= *//p' Makefile); SRC_ILP=$(sed -n 's/^SRC_ILP *:= *//p' Makefile); ILP=$(sed -n 's/^ILP *:= *//p' Makefile)
[ -n "$SRC" ] && [ -n "$SRC_ILP" ] || { echo "build_variant: no SRC / SRC_ILP in the Makefile" >&2; exit 1; }
objs=""; pids=""
for f in $SRC; do
  o=../../build/var_$name/${f%.hip}.o
  /opt/rocm/bin/hipcc $FLAGS "$@" -c $f -o $o & pids="$pids $!"; objs="$objs $o"
done
for f in $SRC_ILP; do
  o=../../build/var_$name/${f%.hip}.o
  /opt/rocm/bin/hipcc $FLAGS $ILP "$@" -c $f -o $o & pids="$pids $!"; objs="$objs $o"
done
for p in $pids; do wait $p || { echo "build_variant: a compile failed" >&2; exit 1; }; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -fPIC -shared -Wl,--version-script=exports.map -o ../variants/lib$name.so $objs
echo built ../variants/lib$name.so
