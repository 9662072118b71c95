#!/bin/bash
# AddressSanitizer + UBSan over the sparse power-flow plan builder, as a stand-alone host program (no GPU, no Python):
#   tools/plan_sanitize.sh
set -euo pipefail
here="$(cd "$(dirname "$0")/.." && pwd)"
out="$(mktemp -d)"
trap 'rm -rf "$out"' EXIT
${HOSTCXX:-g++} -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    "$here/tools/plan_sanitize.cpp" "$here/poweflownet_amd/csrc/powerflow_plan.cpp" -o "$out/plan_sanitize"
"$out/plan_sanitize"
