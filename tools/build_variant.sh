#!/bin/bash
# usage: tools/build_variant.sh <name> [extra hipcc flags]   -> windgym_amd/variants/lib_<name>.so  (A/B builds; WG_LIB selects one)
# (sources and flags: windgym_amd/build.py)
set -e
cd "$(dirname "$0")/.."
mkdir -p windgym_amd/variants
n=$1; shift
WG_HIPCC_FLAGS="$*" python3 -m windgym_amd.build --out windgym_amd/variants/lib_$n.so
