// pt_common.h -- launch geometry shared by the render kernels and the stream-compaction library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ptk {
constexpr int kBlock = 256;          // threads per workgroup = paths per tile (4 wave64)
constexpr int kWaves = kBlock / 64;
constexpr uint32_t kCamPad = 0xffffffffu;   // an entry of the camera rays' work list that holds no pixel (BounceArgs::camPix)
}  // namespace ptk
