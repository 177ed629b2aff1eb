#!/bin/bash
# The device request parser (csrc/kernels/zk_wire.h), the tree image's
# checks (csrc/kernels/zk_snap.h) and the session batches' segment rule
# (csrc/kernels/zk_sess.h) as stand-alone host programs under
# AddressSanitizer + UBSan: tools/fuzz_reqparse.cpp, tools/fuzz_snap.cpp and
# tools/sess_host.cpp, built into a temporary directory and run on two seeds
# each.  No GPU, no Python.
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
# the session batches' segment rule (csrc/kernels/zk_sess.h), likewise
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
  -Icsrc/kernels tools/sess_host.cpp -o "$OUT/sess_host"
"$OUT/sess_host" --self 20000 1
"$OUT/sess_host" --self 20000 2
