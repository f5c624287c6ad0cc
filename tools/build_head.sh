#!/bin/bash
# build a committed revision's library as lib/var_head, for A/B runs against the
# working tree, and its device assembly as lib/var_head/asm/<file>.s (for
# tools/isa_same.py), with that revision's own Makefile, flags and file set:
#   tools/build_head.sh [rev, default HEAD] [EXTRA flags...]
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
REV=${1:-HEAD}
[ $# -gt 0 ] && shift
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
git -C "$R" archive "$REV" include slam-kinectfusion_amd | tar -x -C "$T"
S=$T/slam-kinectfusion_amd
O=$R/slam-kinectfusion_amd/lib/var_head
rm -rf "$O"  # objects of another revision would pass for current (archive files carry the commit's time)
make -C "$S" -j8 OUT="$O" "$O/libkfx.so" EXTRA="$*" > /dev/null
if make -C "$S" -n OUT="$O" EXTRA="$*" asm > /dev/null 2>&1; then
  make -C "$S" -j8 OUT="$O" EXTRA="$*" asm > /dev/null
else  # a revision from before the asm target: this tree's rule, on that revision's HIPCC and HIPFLAGS
  make -C "$S" -j8 OUT="$O" EXTRA="$*" asm --eval='asm: $(patsubst csrc/%.hip,$(OUT)/asm/%.s,$(wildcard csrc/*.hip))
$(OUT)/asm/%.s: csrc/%.hip ; @mkdir -p $(OUT)/asm && $(HIPCC) $(HIPFLAGS) --cuda-device-only -S $< -o $@' > /dev/null
fi
echo "built lib/var_head from $REV"
