#!/bin/bash
# Is the device code of the row kernels the same as at another revision?  (the gate of a refactor of sl_rowlane.hip)
#   tools/isa_same.sh <rev> [extra hipcc flags, e.g. -DSL_TRACE -DSL_DEV_SHAPES]
#   UNITS="sl_episode_log sl_schedule sl_history" tools/isa_same.sh <rev>      other translation units of csrc/
# Exports <rev> with git archive into a temporary directory, compiles the three row-kernel translation units of that
# tree and of this one to listings with the build's flags (six hipcc side by side, a few minutes), and says per file
# whether the listings are identical -- if not, the first kernel whose text differs.  Exit status 0: all identical.
cd "$(dirname "$0")/.."
REV=${1:?usage: tools/isa_same.sh <rev> [extra hipcc flags]}; shift
TMP=$(mktemp -d /tmp/sl_isa_same_XXXX)
trap 'rm -rf $TMP' EXIT
mkdir -p $TMP/old $TMP/s
git archive "$REV" | tar -x -C $TMP/old || exit 2
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-gpu-rdc -ffp-contract=off -mllvm -amdgpu-kernarg-preload-count=8"
UNITS=${UNITS:-sl_rowlane sl_rowlane_b sl_rowlane_c}
for u in $UNITS; do                             # (from each tree's root: the listings name their source by relative path)
    (cd $TMP/old && /opt/rocm/bin/hipcc $FLAGS -S --cuda-device-only -fuse-cuid=none "$@" safelife_amd/csrc/$u.hip -o $TMP/s/$u.old.s) &
    /opt/rocm/bin/hipcc $FLAGS -S --cuda-device-only -fuse-cuid=none "$@" safelife_amd/csrc/$u.hip -o $TMP/s/$u.new.s &
done
wait
rc=0
for u in $UNITS; do
    for t in old new; do
        [ -s $TMP/s/$u.$t.s ] || { echo "$u.hip: the $t tree did not compile"; exit 2; }
        grep -v __hip_cuid_ $TMP/s/$u.$t.s > $TMP/s/$u.$t.f
    done
    n=$(grep -c '^[[:space:]]*\.amdhsa_kernel ' $TMP/s/$u.new.f)
    if cmp -s $TMP/s/$u.old.f $TMP/s/$u.new.f; then
        echo "$u.hip: identical ($n kernels)"
    else
        rc=1
        # the first differing line of the new listing, and the function label (a line "name:") last seen above it
        line=$(cmp $TMP/s/$u.old.f $TMP/s/$u.new.f | sed 's/.* line //')
        kern=$(head -n "$line" $TMP/s/$u.new.f | grep -E '^_Z[A-Za-z0-9_]*:' | tail -n 1 | sed 's/:.*//')
        echo "$u.hip: DIFFERENT from line $line on, first in $(echo "${kern:-the preamble}" | c++filt 2>/dev/null || echo "$kern")"
    fi
done
exit $rc
