#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over the host code that compares a full pt_init call with the live renderer's own
# (PT_FLAG_KEEP_RENDERER; csrc/pt_scene_plan.h: keep_renderer_mismatch), in a stand-alone program with its own main: CPU only, nothing
# loaded into an interpreter, no preloaded runtime.
#   bash tests/run_keep_renderer_sanitizer.sh      -> "sanitizer run finished" and exit 0 when clean
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${PT_SAN_DIR:-/tmp/pt_san}
mkdir -p "$OUT"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
# (the sanitizers go to the host compilation alone: the headers' kernels are compiled for the device as usual and never launched)
"$HIPCC" --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -fno-fast-math -Wno-unused-function \
    -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -Xarch_host -fno-omit-frame-pointer \
    -o "$OUT/sanitize_keep_renderer" "$ROOT/tests/sanitize_keep_renderer.hip"
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 "$OUT/sanitize_keep_renderer"
