#!/bin/sh
# Device code of two builds of libdccn.so, unit by unit: the gfx950 code object of every dl_ofdm_amd/lib/obj/<unit>.o of tree A against
# tree B's, as disassembly (kernels, in the order the code object holds them).  Host-only refactors must leave it identical.
# The units are the Makefile's UNITS (tree B's).  A unit that differs as a whole is compared symbol by symbol: which kernels keep
# their instructions under their name, which changed, which exist on one side only (addresses and branch targets move with
# whatever stands in front of a kernel, so instructions are compared without them).
#   tools/device_code_diff.sh <tree A> <tree B> [work dir]        (both trees built with `make -C dl_ofdm_amd/csrc`)
set -eu
A=$1; B=$2; W=${3:-$(mktemp -d)}
LLVM=${LLVM:-/opt/rocm/lib/llvm/bin}
ARCH=${ARCH:-gfx950}
mkdir -p "$W"
status=0
units=$(sed -n 's/^UNITS *:= *//p' "$B/dl_ofdm_amd/csrc/Makefile")
# one file per symbol: its instructions without addresses, encodings and resolved branch targets
split_symbols() {
    rm -rf "$2"; mkdir -p "$2"
    awk -v dir="$2" '
        /^[0-9a-f]+ <.*>:$/ { name = $2; gsub(/[<>:]/, "", name); out = dir "/" name; next }
        out != "" && NF { line = $0; sub(/\/\/.*$/, "", line); sub(/<[^>]*>/, "", line); gsub(/[ \t]+$/, "", line); print line > out }
    ' "$1"
}
for u in $units; do
    for side in A B; do
        eval tree=\$$side
        "$LLVM/llvm-objcopy" -O binary --only-section=.hip_fatbin "$tree/dl_ofdm_amd/lib/obj/$u.o" "$W/$side.$u.fat"
        "$LLVM/clang-offload-bundler" --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--$ARCH --input="$W/$side.$u.fat" --output="$W/$side.$u.co"
        # (the first lines name the file)
        "$LLVM/llvm-objdump" -d "$W/$side.$u.co" | tail -n +3 > "$W/$side.$u.s"
    done
    kernels=$(grep -c '^[0-9a-f]* <.*>:$' "$W/B.$u.s" || true)
    if cmp -s "$W/A.$u.s" "$W/B.$u.s"; then
        echo "$u: identical ($kernels symbols, $(wc -l < "$W/B.$u.s") lines of disassembly)"
    else
        echo "$u: DIFFERENT (diff $W/A.$u.s $W/B.$u.s)"
        status=1
        split_symbols "$W/A.$u.s" "$W/A.$u.sym"
        split_symbols "$W/B.$u.s" "$W/B.$u.sym"
        for f in "$W/A.$u.sym"/*; do
            s=$(basename "$f")
            if [ ! -e "$W/B.$u.sym/$s" ]; then echo "    only in A: $s"
            elif cmp -s "$f" "$W/B.$u.sym/$s"; then echo "    same:      $s"
            else echo "    CHANGED:   $s"; fi
        done
        for f in "$W/B.$u.sym"/*; do
            s=$(basename "$f")
            [ -e "$W/A.$u.sym/$s" ] || echo "    only in B: $s"
        done
    fi
done
exit $status
