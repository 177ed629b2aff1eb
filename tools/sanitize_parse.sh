#!/bin/bash
# The device request parser (csrc/kernels/zk_wire.h) as a stand-alone host
# program under AddressSanitizer + UBSan: tools/fuzz_reqparse.cpp, built
# into a temporary directory and run on two seeds.  No GPU, no Python.
set -eo pipefail
cd "$(dirname "$0")/.."
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
  -Icsrc/kernels tools/fuzz_reqparse.cpp -o "$OUT/fuzz_reqparse"
"$OUT/fuzz_reqparse" --fuzz 200000 1
"$OUT/fuzz_reqparse" --fuzz 200000 2
