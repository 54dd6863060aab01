#!/bin/bash
# usage: bash tools/code_object_compare.sh [REV] > profiles/NAME.txt      (REV: the commit to compare against, default HEAD~1:
#        the parent, once the change is committed; pass HEAD to compare an uncommitted tree with the commit it stands on)
# Do the existing translation units compile to the same gfx950 code as at REV?  REV's wurblpt_amd/csrc and include/ are
# exported into a scratch directory and built there; then this tree's copies replace them IN THE SAME directory and are built
# into the same build directory (hipcc derives a symbol of each unit from its path and command line), and the code objects
# of both builds are hashed with tools/code_object_hashes.sh.  One line per unit: sha256 of the code object and of its
# disassembly for both builds (16 hex digits each), and "same", "DIFFERS" or "new".  Exit status 1 if a unit differs.
set -e
REV=${1:-HEAD~1}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
JOBS=${JOBS:-8}
git -C "$ROOT" archive "$REV" wurblpt_amd/csrc include | tar -x -C "$T"
make -s -j"$JOBS" -C "$T/wurblpt_amd/csrc" ../lib/libwurblpt_hip.so >&2
bash "$ROOT/tools/code_object_hashes.sh" "$T/wurblpt_amd/csrc/build" | sort > "$T/parent.txt"
rm -rf "$T/wurblpt_amd/csrc" "$T/include" "$T/wurblpt_amd/lib"
mkdir -p "$T/wurblpt_amd/csrc" "$T/include"
cp "$ROOT"/wurblpt_amd/csrc/*.h "$ROOT"/wurblpt_amd/csrc/*.hip "$ROOT"/wurblpt_amd/csrc/Makefile "$T/wurblpt_amd/csrc/"
cp -r "$ROOT"/include/. "$T/include/"
make -s -j"$JOBS" -C "$T/wurblpt_amd/csrc" ../lib/libwurblpt_hip.so >&2
bash "$ROOT/tools/code_object_hashes.sh" "$T/wurblpt_amd/csrc/build" | sort > "$T/new.txt"
echo "# bash tools/code_object_compare.sh $REV: gfx950 code objects of $(git -C "$ROOT" rev-parse --short "$REV")'s sources and of this tree's,"
echo "# both compiled from one source directory into one build directory"
echo "# unit : code object, disassembly at $REV : code object, disassembly in this tree : verdict"
join -a 2 -e - -o 0,1.2,1.3,2.2,2.3 "$T/parent.txt" "$T/new.txt" | awk '
  { v = ($2 == "-") ? "new" : (($2 == $4 && $3 == $5) ? "same" : "DIFFERS"); if (v == "DIFFERS") bad = 1;
    printf "%s : %s %s : %s %s : %s\n", $1, $2, $3, $4, $5, v }
  END { exit bad }'
