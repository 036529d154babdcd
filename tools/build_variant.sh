#!/bin/bash
# Builds the library with extra compiler flags into tools/scratch/lib_<name>.so (git-ignored; travels to the GPU box),
# e.g.  tools/build_variant.sh jump4 -DBROTLI_AMD_PE_JUMP_LOG=4 ; then BROTLI_AMD_LIB=tools/scratch/lib_jump4.so python bench.py ...
# The sources are the Makefile's: objects go to tools/scratch/build_<name>/.
set -eu
REPO=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; shift
D=$REPO/tools/scratch/build_$NAME
mkdir -p "$D"
make -s -C "$REPO/rust-brotli-decompressor_amd" -j8 OBJDIR="$D" OUT="$REPO/tools/scratch/lib_$NAME.so" EXTRA="$*"
echo "built tools/scratch/lib_$NAME.so"
