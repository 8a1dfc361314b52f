#!/bin/bash
# Which lines of gnark_amd/csrc does the CPU suite execute?  The unmodified product sources are compiled against the functional HIP
# emulation (tests/emu/build_emu.sh) with gcov instrumentation into a build directory of their own, never tests/emu/build; the CPU suite
# runs on that library (GA_EMU_LIB_PATH, tests/conftest.py); every worker exits normally, which is when the counters are written; gcov's
# output is merged over all objects by tools/emu_coverage_merge.py.  TEST INFRASTRUCTURE, CPU only: nothing is preloaded, nothing of it
# runs on a device.
#   tools/emu_coverage.sh [report, default profiles/emu_coverage.txt] [pytest arguments, default: tests -m "not gpu"]
# GA_COV_WORK: the work directory (default: a fresh one from mktemp, removed at the end).  With GA_COV_KEEP=1 and a work directory that
# already holds an instrumented build, nothing is rebuilt and the counters of the earlier runs stay: the new run ADDS to them (see
# profiles/README.md, which also says how profiles/emu_coverage_parent.txt was made).
# The few tests that load tests/emu/libgnark_amd_emu.so by path (the C ABI clients, the multi-process worker, bench.py --emu) run on
# the plain build and are not counted.
set -e
set -o pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
REPORT=${1:-$ROOT/profiles/emu_coverage.txt}
[ $# -gt 0 ] && shift
if [ -n "$GA_COV_WORK" ]; then
  WORK=$GA_COV_WORK
  mkdir -p "$WORK"
else
  WORK=$(mktemp -d "${TMPDIR:-/tmp}/ga_cov.XXXXXX")
  trap 'rm -rf "$WORK"' EXIT
fi
exec 8>"$WORK/.lock"   # one run per work directory
flock -n 8 || { echo "another run is using $WORK" >&2; exit 1; }
LIB=$WORK/build/libgnark_amd_emu.so
if [ -z "$GA_COV_KEEP" ] || [ ! -f "$LIB" ]; then
  rm -rf "$WORK/build"
  # (plain counter updates: lanes run on host threads and an update may be lost, but a counter that was ever non-zero stays so, and
  # executed or not is all the report asks)
  GA_EMU_BUILD_DIR=$WORK/build GA_EMU_EXTRA_FLAGS="--coverage" "$ROOT/tests/emu/build_emu.sh"
fi
cd "$ROOT"
if [ $# -eq 0 ]; then set -- tests -m "not gpu"; fi
status=0   # (a failing test still leaves its counters: the report is written, and the failure is the script's exit status)
GA_EMU_LIB_PATH=$LIB python -m pytest -q -n ${GA_COV_JOBS:-8} -p no:cacheprovider "$@" | tee "$WORK/pytest.log" || status=$?
tail -1 "$WORK/pytest.log" | sed -E 's/^=+ //; s/ in [0-9.]+s.*$//' >> "$WORK/runs.txt"
# one JSON document per object, named after it
mkdir -p "$WORK/gcov"
rm -f "$WORK"/gcov/*.json
for d in "$WORK"/build/*.gcda; do
  f=$(basename "$d" .gcda)
  [ "$f" = emu_impl ] && continue
  gcov --json-format --stdout -o "$WORK/build" "$d" > "$WORK/gcov/$f.json"
done
python "$ROOT/tools/emu_coverage_merge.py" "$ROOT/gnark_amd/csrc" "$WORK/gcov" "$(paste -sd+ "$WORK/runs.txt" | sed 's/+/ + /g')" > "$REPORT"
echo "wrote $REPORT"
exit $status
