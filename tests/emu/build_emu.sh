#!/bin/bash
# TEST INFRASTRUCTURE: compile the *unmodified* product sources against the functional HIP emulation in
# tests/emu/include so that kernel logic can be exercised on a CPU-only box.  Output: tests/emu/libgnark_amd_emu.so
# (never loaded by the gnark_amd package).
# GA_EMU_BUILD_DIR: objects AND the library go to that directory instead (instrumented builds, tools/emu_coverage.sh; the build the
# tests use is never touched); GA_EMU_EXTRA_FLAGS: appended to the compile and link flags of such a build.
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
SRC="$HERE/../../gnark_amd/csrc"
OUT="${GA_EMU_BUILD_DIR:-$HERE/build}"
LIBDIR="$HERE"
[ -n "$GA_EMU_BUILD_DIR" ] && LIBDIR="$OUT"
mkdir -p "$OUT"
# one builder at a time (pytest-xdist workers all ask for the library at session start)
exec 9>"$OUT/.lock"
flock 9
FLAGS="-O2 -g0 -std=c++17 -fPIC -I$HERE/include -I$SRC -I$HERE/../../include -w $GA_EMU_EXTRA_FLAGS"
pids=()
objs=("$OUT/emu_impl.o")
for s in "$SRC"/*.hip; do
  f=$(basename "$s" .hip)
  [ "$f" = microbench ] && continue   # (issue-rate probes of gfx950 instructions: nothing to emulate)
  objs+=("$OUT/$f.o")
  if [ ! -f "$OUT/$f.o" ] || [ -n "$(find "$SRC" "$HERE/include" -newer "$OUT/$f.o" \( -name '*.hip.h' -o -name '*.h' -o -name '*.hpp' -o -name "$f.hip" \) | head -1)" ]; then
    g++ $FLAGS -x c++ -c "$SRC/$f.hip" -o "$OUT/$f.o" &
    pids+=($!)
  fi
done
g++ $FLAGS -c "$HERE/emu_impl.cpp" -o "$OUT/emu_impl.o" &
pids+=($!)
for p in "${pids[@]}"; do wait $p; done
g++ -shared $GA_EMU_EXTRA_FLAGS -o "$LIBDIR/libgnark_amd_emu.so.tmp" "${objs[@]}" -lpthread
mv -f "$LIBDIR/libgnark_amd_emu.so.tmp" "$LIBDIR/libgnark_amd_emu.so"
echo "built $LIBDIR/libgnark_amd_emu.so"
