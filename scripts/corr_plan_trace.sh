#!/bin/bash
# Recorded-launch comparison of depthg_amd/csrc/dg_api_corr.hip, a parent revision against the working tree, without a GPU:
# scripts/corr_plan_trace.cpp is built against each tree's unit (host code only, recording stand-ins for the launchers and the HIP
# runtime; the dg_*_supported predicates are lifted as text from each tree's own dg_corr2.hip and dg_small.hip) and run three times in fresh processes - as is, with DG_FOLD_INTRA=0 and with DG_SPLIT_MASKS=0.  The two sides' outputs
# (one digest line per descriptor, the totals, the per-route counts) must be equal; prints the totals and the sha256 of each output.
#   usage: scripts/corr_plan_trace.sh <parent-rev>      SAN=1: build with -fsanitize=address,undefined      (TRACE_WORK: scratch directory)
set -euo pipefail
root=$(git rev-parse --show-toplevel)
rev=$(git -C "$root" rev-parse --short "$1")
work=${TRACE_WORK:-${TMPDIR:-/tmp}/dg_trace}
san=; [ "${SAN:-0}" = 1 ] && san="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
mkdir -p "$work/parent-$rev" "$work/new"
[ -d "$work/parent-$rev/depthg_amd" ] || git -C "$root" archive "$rev" depthg_amd/csrc include | tar -x -C "$work/parent-$rev"

build() {   # build <tree root> <output directory>
    local src=$1/depthg_amd/csrc flags="-O1 -g -std=c++17 --cuda-host-only -Wall -Wno-unused-function $san"
    # the predicates of this tree: dg_corr2_shape_supported and dg_corr2_supported (adjacent, each closed by a "}" in column 1), dg_small_supported
    { awk '/^bool dg_corr2_shape_supported\(/ { on = 1 } on { print } on && /^}/ && ++n == 2 { exit }' "$src/dg_corr2.hip"
      grep '^bool dg_small_supported(' "$src/dg_small.hip"; } > "$2/predicates.inc"
    [ "$(grep -c '^bool dg_' "$2/predicates.inc")" = 3 ] || { echo "could not lift the three predicates from $src" >&2; exit 2; }
    ${HIPCC:-hipcc} $flags -I"$src" -c "$src/dg_api_corr.hip" -o "$2/unit.o"
    ${HIPCC:-hipcc} $flags -I"$src" -I"$2" -x hip -c "$root/scripts/corr_plan_trace.cpp" -o "$2/trace.o"
    ${CXX:-clang++} ${san//-Xarch_host /} "$2/unit.o" "$2/trace.o" -o "$2/corr_plan_trace"      # (no HIP runtime on the link line)
}
run() {     # run <output directory> <UBSAN_OPTIONS>: three fresh processes, the switches are read once
    export UBSAN_OPTIONS=$2
    "$1/corr_plan_trace" > "$1/default.txt"
    DG_FOLD_INTRA=0 "$1/corr_plan_trace" > "$1/fold_off.txt"
    DG_SPLIT_MASKS=0 "$1/corr_plan_trace" > "$1/split_off.txt"
}
build "$work/parent-$rev" "$work/parent-$rev"
build "$root" "$work/new"
run "$work/parent-$rev" halt_on_error=0
run "$work/new" halt_on_error=1          # (SAN=1: the working tree's unit must end clean)

bad=0
echo "| run | descriptors, calls, launches | parent $rev sha256 | working tree sha256 | |"
echo "|---|---|---|---|---|"
for r in default fold_off split_off; do
    a=$(grep -v '^note:' "$work/parent-$rev/$r.txt" | sha256sum | cut -c1-16) b=$(grep -v '^note:' "$work/new/$r.txt" | sha256sum | cut -c1-16)
    if [ "$a" = "$b" ]; then v=identical; else v=DIFFERENT; bad=1; fi
    echo "| $r | $(grep '^descriptors=' "$work/new/$r.txt" | sed 's/ digest=.*//') | $a | $b | $v |"
done
grep -h '^note:' "$work/parent-$rev/default.txt" | sed "s/^note:/parent $rev:/"
grep -h '^note:' "$work/new/default.txt" | sed 's/^note:/working tree:/'
grep -h '^route xop ' "$work/new/default.txt" | sed 's/^route xop \(.*\)/working tree: the intra-feature operand (xop) was reached by \1 launches/'
exit $bad
