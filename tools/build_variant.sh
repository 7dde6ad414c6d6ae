#!/bin/bash
# Build a variant of libcenternet_amd.so with extra compiler flags (A/B of build-time choices):
#   tools/build_variant.sh <name> "<extra hipcc flags>"   ->  centernet_amd/variants/libcenternet_amd_<name>.so
# Use with CENTERNET_AMD_LIB=<that path>.  Objects go to /tmp; the in-tree build is untouched.
# The csrc Makefile does the compiling, so the per-file flags are the in-tree build's.
set -e
name=$1; extra=$2
root=$(cd "$(dirname "$0")/.." && pwd)
obj=/tmp/cn_variant_$name
out=$root/centernet_amd/variants/libcenternet_amd_$name.so
mkdir -p "$obj" "$root/centernet_amd/variants"
make -C "$root/centernet_amd/csrc" -j16 OBJDIR="$obj" OUT="$out" EXTRA="$extra" >&2
echo "$out"
