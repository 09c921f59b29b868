#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over the owner of the library's streams, events and page-locked memory (csrc/pt_owned.h:
# Owned), in a stand-alone program with its own main: CPU only, nothing loaded into an interpreter, no preloaded runtime.
#   bash tests/run_owned_handles_sanitizer.sh      -> "sanitizer run finished" and exit 0 when clean
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${PT_SAN_DIR:-/tmp/pt_san}
mkdir -p "$OUT"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
# (the sanitizers go to the host compilation alone; the program has no kernel)
"$HIPCC" --offload-arch=gfx950 -O1 -g -std=c++17 -Wall \
    -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -Xarch_host -fno-omit-frame-pointer \
    -o "$OUT/sanitize_owned_handles" "$ROOT/tests/sanitize_owned_handles.hip"
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 "$OUT/sanitize_owned_handles"
