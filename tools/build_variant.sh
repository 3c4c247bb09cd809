#!/bin/bash
# tools/build_variant.sh <name> [-DFLAG=...]... — an extra build of the library under build_ablate/
# (git-ignored, travels with gpurun) for interleaved A/B runs: tools/ab_engines.py --libs ...
set -e
cd "$(dirname "$0")/.."
name=$1; shift
mkdir -p build_ablate
UNITS=$(python -c "from rtlsdr_amd.build import DEVICE_UNITS; print(' '.join('rtlsdr_amd/csrc/' + u for u in DEVICE_UNITS))")
hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -w -Iinclude "$@" \
  $UNITS -o build_ablate/lib_$name.so
echo build_ablate/lib_$name.so
