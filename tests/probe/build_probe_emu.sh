#!/bin/bash
# TEST INFRASTRUCTURE: compile tests/probe/field_probe.hip (the unmodified product headers behind one exported function) against the
# functional HIP emulation in tests/emu/include, for the CPU runs of tests/test_field_boundaries.py.
# Output: tests/probe/libga_probe_emu.so
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
EMU="$HERE/../emu"
SRC="$HERE/../../gnark_amd/csrc"
OUT="$HERE/build"
mkdir -p "$OUT"
# one builder at a time (pytest-xdist workers all ask for the library at session start)
exec 9>"$OUT/.lock"
flock 9
FLAGS="-O2 -g0 -std=c++17 -fPIC -I$EMU/include -I$SRC -I$HERE/../../include -w"
if [ ! -f "$OUT/field_probe.o" ] || [ -n "$(find "$SRC" "$EMU/include" "$HERE/field_probe.hip" -newer "$OUT/field_probe.o" \( -name '*.hip.h' -o -name '*.h' -o -name '*.hpp' -o -name field_probe.hip \) | head -1)" ]; then
  g++ $FLAGS -x c++ -c "$HERE/field_probe.hip" -o "$OUT/field_probe.o" &
fi
if [ ! -f "$OUT/emu_impl.o" ] || [ -n "$(find "$EMU/emu_impl.cpp" "$EMU/include" -newer "$OUT/emu_impl.o" -type f | head -1)" ]; then
  g++ $FLAGS -c "$EMU/emu_impl.cpp" -o "$OUT/emu_impl.o" &
fi
wait
[ -f "$OUT/field_probe.o" ] && [ -f "$OUT/emu_impl.o" ]
g++ -shared -o "$HERE/libga_probe_emu.so.tmp" "$OUT/field_probe.o" "$OUT/emu_impl.o" -lpthread
mv -f "$HERE/libga_probe_emu.so.tmp" "$HERE/libga_probe_emu.so"
echo "built $HERE/libga_probe_emu.so"
