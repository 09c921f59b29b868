#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over the host code that builds the camera rays' work list in two passes
# (csrc/pt_host_scene.h), in a stand-alone program with its own main: CPU only, nothing loaded into an interpreter, no preloaded runtime.
#   bash tests/run_camera_list_sanitizer.sh      -> "sanitizer run finished" and exit 0 when clean
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${PT_SAN_DIR:-/tmp/pt_san}
mkdir -p "$OUT"
python3 "$ROOT/tests/camera_poses.py" "$OUT/camera_poses.bin"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
# (the sanitizers go to the host compilation alone: the headers' kernels are compiled for the device as usual and never launched)
"$HIPCC" --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -fno-fast-math -Wno-unused-function \
    -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -Xarch_host -fno-omit-frame-pointer \
    -o "$OUT/sanitize_camera_list" "$ROOT/tests/sanitize_camera_list.hip"
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 "$OUT/sanitize_camera_list" "$OUT/camera_poses.bin"
