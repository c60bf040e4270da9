#!/bin/bash
# Compile every translation unit of a source tree by the rules of its own csrc/Makefile (flags, the four tri_inst.hip units) plus
# -save-temps=obj, one output directory per unit (the tri_inst.hip units share temp-file names), for tools/device_code_diff.py.
#   tools/build_units_temps.sh <tree root> <output dir> [jobs]
# also links <output dir>/libcrt1d_hip.so from the objects.
set -e -o pipefail
R=$(cd "$1" && pwd); OUT=$2; JOBS=${3:-8}
C=$R/crt1d_amd/csrc
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)
# the Makefile's own object list ($(OBJ)): printed by a rule read from stdin after it
UNITS=$(printf 'include %s/Makefile\nunits:\n\t@echo $(OBJ:.o=)\n' "$C" | make -s -f - units)
one() {
  mkdir -p "$OUT/$1"
  make -s -C "$OUT/$1" -f "$C/Makefile" VPATH="$C" HIPCC="$HIPCC" EXTRA=-save-temps=obj "$1.o" > "$OUT/$1/build.log" 2>&1 || { cat "$OUT/$1/build.log"; exit 1; }
}
export -f one; export C OUT HIPCC
echo $UNITS | tr ' ' '\n' | xargs -P "$JOBS" -I{} bash -c 'one {}'
OBJS=""; for u in $UNITS; do OBJS="$OBJS $OUT/$u/$u.o"; done
$HIPCC -shared -fPIC --offload-arch=gfx950 $OBJS -o "$OUT/libcrt1d_hip.so" -Wl,-rpath,/opt/rocm/lib
echo "built $OUT/libcrt1d_hip.so"
