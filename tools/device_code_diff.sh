#!/bin/sh
# Device code of two builds of libdccn.so, unit by unit: the gfx950 code object of every dl_ofdm_amd/lib/obj/<unit>.o of tree A against
# tree B's, as disassembly (kernels, in the order the code object holds them).  Host-only refactors must leave it identical.
#   tools/device_code_diff.sh <tree A> <tree B> [work dir]        (both trees built with `make -C dl_ofdm_amd/csrc`)
set -eu
A=$1; B=$2; W=${3:-$(mktemp -d)}
LLVM=${LLVM:-/opt/rocm/lib/llvm/bin}
ARCH=${ARCH:-gfx950}
mkdir -p "$W"
status=0
for u in dccn_abi dccn_abi_eq dccn_abi_gen dccn_abi_conv; do
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
    fi
done
exit $status
