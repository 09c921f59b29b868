// pt_noise.h -- how converged is the frame: the error statistics of 16 x 16 pixel tiles, from the accumulator S and the second moments Q
// (PT_FLAG_MOMENTS).  One kernel, outside the render path like the denoiser's (k_bounce, k_mesh_walk, k_commit and their arguments do not
// know of it):
//   k_noise_stats   per tile the mean pixel variance relative to the squared mean luminance; per frame how many tiles lie above a threshold
//                   and the largest ratio.  Reads 16 B per pixel, writes one float per TILE at most.
// Included by pt_api.hip only.
//
// Why tiles: a pixel whose samples all missed the light has variance exactly 0 and looks converged, so the number of pixels above a
// per-pixel threshold GROWS with the sample count (Cornell 64 x 48, relative standard error >= 0.25: 213 pixels at 2 samples, 1794 at 64).
// The sum of a tile's pixel variances is an unbiased estimate of the variance of the tile's summed luminance and follows the 1 / sqrt(n) law.
//
// ---- the statistics, operation by operation (tests/noise_ref.py restates them in numpy, bit for bit: every fp32 operation below is one
// IEEE operation, -ffp-contract=off, in the order written) ----
//   tiles     PT_NOISE_TILE = 16.  Tile (tx, ty) covers x in [16 tx, min(16 tx + 16, W)), y likewise; tiles_x = ceil(W / 16), tiles_y = ceil(H / 16).
//   lanes     256 lanes per tile.  Lane l of wave w is pixel x = 16 tx + (l & 15), y = 16 ty + 4 w + (l >> 4).
//   pixel     (c, v) = meanAndVariance(S, Q, pix, n, n - 1) (pt_denoise.h: the variance of the pixel's mean luminance); L = atrousLum(c).
//             A lane outside the frame holds v = L = +0.
//   sums      V of v and M of L: inside a wave the xor butterfly  for o in 32, 16, 8, 4, 2, 1: a += a[lane ^ o]  (waveSum's order, pt_trace.h;
//             every lane ends with the same bits), then across the waves (w0 + w1) + (w2 + w3).
//   ratio     N = the tile's pixel count as float;  mv = V / N;  ml = M / N;  mf = ml > floor ? ml : floor (a NaN gives the floor);
//             r = mv / (mf * mf).  sqrt(r) is the tile's relative standard error.  v >= +0 and mf > 0, so r >= +0 or NaN (inf / inf).
//   flag      the tile is unconverged iff r > thr2, thr2 = threshold * threshold formed in fp32 on the host.  A NaN compares false.
//   frame     unconverged = the number of flagged tiles (an integer atomic); max_rel_var = the maximum of r over the tiles from 0, a NaN
//             ignored: r >= 0, so an unsigned atomic max on the bits is exact and free of order.
// The result is a function of the frame alone.
#pragma once
#include "pt_denoise.h"

namespace ptk {

constexpr int kNoiseTile = 16;
static_assert(kNoiseTile * kNoiseTile == 4 * 64 && kBlock == 256, "a tile is four row groups of 64 lanes; four waves per workgroup");

constexpr int kNoiseTilesPerWave = 2;    // the library's choice (profiles/noise_cost.txt has 1, 2 and 4 side by side)

// frame[0]: the flagged tiles, frame[1]: the bits of the largest ratio -- both zeroed by the host before the launch; tileMap: tiles_y x tiles_x
// ratios, or NULL.  How the lanes of the text above are laid over the hardware: a tile's four "waves" are ONE hardware wave that holds the
// tile's four row groups in four registers -- the same butterflies over the same 64 values, the same (w0 + w1) + (w2 + w3), no LDS and no
// barrier on the way -- and wave g of the grid takes the tiles g * tilesPerWave .. + tilesPerWave - 1 (row-major, so neighbours in memory).
// A workgroup's four waves pool their counts and maxima in LDS and issue ONE pair of atomics, and none for a zero.  An integer sum and an
// unsigned maximum: the grouping does not enter the result.  (The first form -- one tile per workgroup of four waves, the waves' sums through
// LDS and a barrier, thread 0 alone dividing, a pair of atomics per tile on the same two addresses -- took 46 us at 1280 x 720 and 98 us at
// 1920 x 1080, in step with the tile count; this one 14 and 22 us: DESIGN.md section 4, profiles/noise_cost.txt.)
__global__ __launch_bounds__(kBlock) void k_noise_stats(const float *accum, const float *moments, int W, int H, int tilesX, int tiles, int tilesPerWave,
                                                        float n, float nM1, float lumFloor, float thr2, uint32_t *frame, float *tileMap) {
    __shared__ uint32_t s_cnt[4], s_max[4];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lx = lane & 15, ly = lane >> 4;
    const int first = ((int)blockIdx.x * 4 + wave) * tilesPerWave;
    uint32_t cnt = 0u, mx = 0u;
    for (int t = first; t < first + tilesPerWave && t < tiles; ++t) {
        const int ty = t / tilesX, tx = t - ty * tilesX;
        const int x0 = tx * kNoiseTile, y0 = ty * kNoiseTile, x = x0 + lx;
        float v[4], L[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int y = y0 + 4 * g + ly;
            v[g] = 0.0f;
            L[g] = 0.0f;
            if (x < W && y < H) {
                const float4 cv = meanAndVariance(accum, moments, (size_t)y * (size_t)W + (size_t)x, n, nM1);
                v[g] = cv.w;
                L[g] = atrousLum(cv.x, cv.y, cv.z);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {      // the eight butterflies side by side: eight independent exchanges per round
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                v[g] += __shfl_xor(v[g], o, 64);
                L[g] += __shfl_xor(L[g], o, 64);
            }
        }
        const float V = (v[0] + v[1]) + (v[2] + v[3]);
        const float M = (L[0] + L[1]) + (L[2] + L[3]);
        const int nx = W - x0 < kNoiseTile ? W - x0 : kNoiseTile, ny = H - y0 < kNoiseTile ? H - y0 : kNoiseTile;
        const float N = (float)(nx * ny);
        const float mv = V / N, ml = M / N;
        const float mf = ml > lumFloor ? ml : lumFloor;
        const float r = mv / (mf * mf);          // (every lane holds the same bits)
        if (tileMap && lane == 0) tileMap[t] = r;
        if (r > thr2) cnt += 1u;
        if (r == r && __float_as_uint(r) > mx) mx = __float_as_uint(r);
    }
    if (lane == 0) {
        s_cnt[wave] = cnt;
        s_max[wave] = mx;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    cnt = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
    mx = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
    if (cnt) atomicAdd(&frame[0], cnt);
    if (mx) atomicMax(&frame[1], mx);
}

}  // namespace ptk
