#!/bin/bash
# usage: build_variant.sh <name> <extra -D flags...>   -> gama_tts_amd/lib_variants/libgama_vtm_<name>.so
# The product's recipe (csrc/Makefile: `variant`) with the extra flags on the six synthesis units, the host side of the C ABI
# and the hooks, compiled into csrc/_obj_<name>/; everything else is linked from csrc/_obj/.  The units are compiled afresh
# every time: the flags of an earlier variant of the same name are not make's to know.
set -e
name=$1; shift
csrc="$(dirname "$(readlink -f "$0")")/../gama_tts_amd/csrc"
rm -rf "$csrc/_obj_$name"
make -j4 -C "$csrc" variant VARIANT="$name" VARIANT_FLAGS="$*"
echo built $name
