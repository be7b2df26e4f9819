#!/bin/bash
# Device code of every unit of depthg_amd/csrc, a parent revision against the working tree: each .hip is compiled to gfx950
# assembly with the Makefile's flags, the lines that carry the path-derived __hip_cuid name are dropped, and the two texts must be
# equal (instruction streams, register counts, LDS and scratch sizes, kernel set).  Prints one markdown table row per unit and
# fails if any differs.      usage: scripts/isa_compare.sh <parent-rev> [unit.hip ...]      (ISA_WORK: where the assembly is kept;
# EXTRA: further flags for both sides, e.g. EXTRA='-DDG_DEVTOOLS -DC2_STAMPS' - the assembly is then kept apart per flag set)
set -euo pipefail
root=$(git rev-parse --show-toplevel)
rev=$(git -C "$root" rev-parse --short "$1"); shift
work=${ISA_WORK:-${TMPDIR:-/tmp}/dg_isa}$(echo "${EXTRA:-}" | tr -c 'A-Za-z0-9_=\n' _)
export EXTRA=${EXTRA:-}
mkdir -p "$work/parent-$rev" "$work/new"
[ -d "$work/parent-$rev/depthg_amd" ] || git -C "$root" archive "$rev" depthg_amd/csrc include | tar -x -C "$work/parent-$rev"
units=${*:-$(cd "$root/depthg_amd/csrc" && ls *.hip)}

asm() {     # asm <tree root> <unit> <output>: nothing to do when the output is newer than every source of the tree
    local src=$1/depthg_amd/csrc extra=
    [ "$2" = dg_corr2.hip ] && extra="-mllvm -disable-machine-licm"
    [ -s "$3" ] && [ -z "$(find "$src" "$1/include" -newer "$3" -type f \( -name '*.h' -o -name "$2" \))" ] && return 0
    (cd "$src" && ${HIPCC:-hipcc} -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S $extra $EXTRA "$2" -o - | grep -v __hip_cuid > "$3.tmp") && mv "$3.tmp" "$3"
}
export -f asm
for u in $units; do
    echo "asm '$work/parent-$rev' $u '$work/parent-$rev/${u%.hip}.s'"
    echo "asm '$root' $u '$work/new/${u%.hip}.s'"
done | xargs -P "${JOBS:-8}" -I{} bash -c {}

bad=0
echo "| unit | kernels | device code |"
echo "|---|---|---|"
for u in $units; do
    a=$work/parent-$rev/${u%.hip}.s b=$work/new/${u%.hip}.s
    n=$(grep -c '^\s*\.amdhsa_kernel ' "$b" || true)
    names=$(grep '^\s*\.amdhsa_kernel ' "$b" | awk '{ s = $2; if (match(s, /^_Z[0-9]+/)) s = substr(s, RLENGTH + 1, substr(s, 3, RLENGTH - 2) + 0); else if (s ~ /^_ZN/) s = "(rocprim)"; print s }' | sort -u | paste -sd' ' - || true)
    if cmp -s "$a" "$b"; then r=identical; else r=DIFFERENT; bad=1; fi
    echo "| $u | $n: ${names:--} | $r |"
done
exit $bad
