#!/bin/bash
# The device request parser (csrc/kernels/zk_wire.h) and the tree image's
# checks (csrc/kernels/zk_snap.h) as stand-alone host programs under
# AddressSanitizer + UBSan: tools/fuzz_reqparse.cpp and tools/fuzz_snap.cpp,
# built into a temporary directory and run on two seeds each.  No GPU, no
# Python.
set -eo pipefail
cd "$(dirname "$0")/.."
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
  -Icsrc/kernels tools/fuzz_reqparse.cpp -o "$OUT/fuzz_reqparse"
"$OUT/fuzz_reqparse" --fuzz 200000 1
"$OUT/fuzz_reqparse" --fuzz 200000 2
# the tree image's structural checks (csrc/kernels/zk_snap.h), likewise
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
  -Icsrc/kernels tools/fuzz_snap.cpp -o "$OUT/fuzz_snap"
"$OUT/fuzz_snap" --fuzz 200000 1
"$OUT/fuzz_snap" --fuzz 200000 2
