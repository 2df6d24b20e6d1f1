#!/bin/bash
# Build tools/variants/libabl_<NAME>.so = the product sources + extra compiler flags
# (A/B builds; load one with BB_LIB=$PWD/tools/variants/libabl_<NAME>.so).  The sources and
# the base flags are build.sh's: this only says where the library goes and what is added.
#   usage: tools/build_variant.sh NAME [flags...]
# The flags travel as one string (BB_EXTRA_FLAGS) that build.sh splits at blanks: a flag that
# holds a blank itself, such as -DX="a b", cannot be given this way.
set -euo pipefail
cd "$(dirname "$0")/.."
mkdir -p tools/variants
name=$1; shift
BB_OUT=tools/variants/libabl_$name.so BB_EXTRA_FLAGS="$*" ./build.sh
echo "$*" > tools/variants/libabl_$name.flags
echo "built tools/variants/libabl_$name.so ($*)"
