#!/bin/bash
# Builds an experimental libtrainer variant with extra HIP defines into variants/ (gitignored),
# by the Makefile's own rules; select it with SHREDWORD_LIB=variants/libtrainer_NAME.so:
#   tools/build_variant.sh NAME "-DSHRED_WL_STAMPS ..."
set -e
HERE=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; DEFS=$2
LIB=$HERE/../variants/libtrainer_$NAME.so
make -s -j16 -C "$HERE" HIPDEFS="$DEFS" BUILD="$HERE/../variants/$NAME" LIB="$LIB" "$LIB" >/dev/null
echo "$LIB"
