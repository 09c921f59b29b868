// pt_spatial_var.h -- the spatial variance estimate (PT_FLAG_SPATIAL_VARIANCE): SVGF's estimate for pixels of short history (Schied et al.,
// HPG 2017, section 4.2).  A pixel whose effective sample count is below PT_SPATIAL_MIN_COUNT has no variance of its own -- one sample, or a
// disocclusion of a one-sample view under PT_FLAG_TEMPORAL -- so the colour term of the variance-guided filter shuts and the pixel stays a raw
// sample inside a filtered frame.  Such a pixel takes the variance of the luminance over a small guide-weighted window of its neighbours'
// first and second moments instead.  Two launches in front of the filter's levels, outside the render path like the denoiser's; included by
// pt_api.hip only.
//   stage A   k_temporal<kTemporalMoments> (pt_temporal.h): steps 1 - 7 of the blend, then M[p] = (c.r, c.g, c.b, m2) and N[p] = tot, uncapped.
//             Without history that is c = S / n, m2 = Q / n, N = n.
//   stage B   k_spatial_variance_*<R> (here): out[p] = (c_p, v), the (r, g, b, variance) image level 0 of k_atrous_*<AtrousGuided> reads
//             where k_temporal<kTemporalFilter> puts its image.
//
// ---- stage B, operation by operation (tests/spatial_var_ref.py restates it in numpy, bit for bit: every fp32 operation below is one IEEE
// operation, -ffp-contract=off, in the order written; dot = (x + y) + z as ptd::dot) ----
//   inputs      M = (c.r, c.g, c.b, m2) and N per pixel, the guides (P, t) and (N, id) of pt_denoise.h, and the call's invN, invP as
//               atrous_run forms them on the host: 1 / (sigma_normal * sigma_normal), 1 / (sigma_position * sigma_position)
//   every p     L_p = atrousLum(c_p)
//   N_p >= PT_SPATIAL_MIN_COUNT
//               dd = m2_p - L_p * L_p;  dd = dd > 0 ? dd : 0 (a NaN gives 0);  v = dd / (N_p - 1)      -- step 8 of k_temporal, to the bit
//   otherwise   (a NaN count lands here) over the taps q = p + (dx, dy), dy = -R .. R (outer loop), dx = -R .. R (inner loop), in that
//               order; a tap outside the frame is skipped.  The centre tap has w = 1, nothing is evaluated for it.  A tap of which exactly
//               one of p, q is a miss (id < 0) is skipped.  Every other tap:
//                   a = dot(dn, dn) * invN;  a = a + dot(dp, dp) * invP;  w = expNegPoly(a)      dn, dp = q - p of the normal and the position
//               sw += w;  s1 += L_q * w;  s2 += m2_q * w  -- all from 0 (the centre included: L_p * 1)
//               M1 = s1 / sw;  M2 = s2 / sw;  d = M2 - M1 * M1;  d = d > 0 ? d : 0 (a NaN gives 0);  v = d / N_p
//               The divisor is N_p, not N_p - 1: the mean comes from the window, not from the pixel.  The centre alone gives sw >= 1: no guard.
//   out[p] = (c_p.r, c_p.g, c_p.b, v)
// The result of a pixel is a function of the frame alone: neither the kernel form, nor the tile shape, nor the early-out enters.
//
// Two forms, as the filter's levels have them; a workgroup of either computes 64 x 4 neighbouring pixels, one per lane:
//   gather   every tap is a load through L2 (52 bytes from four arrays), taken only by the lanes below the count
//   tiled    the tile and its R-pixel halo go to LDS once -- (64 + 2R) x (4 + 2R) entries of {normal + id; position + L; m2}: two float4
//            images and one float image, 36 bytes per entry, 25,200 bytes at R = 3 -- and the taps read from there.  A wave reads 64
//            consecutive entries of one LDS row per tap: the two 16-byte reads (ds_read_b128) cover, per 16-lane group, the 16 slots of the
//            256-byte bank row exactly once whatever dx and the pitch, the 4-byte read 64 consecutive banks: no bank conflict.  A workgroup
//            none of whose lanes is below the count stages nothing (one __syncthreads_or): with history only disocclusions take the estimate.
// The product launches the tiled form, by measurement (pt_api.hip: kSpatialForm; profiles/spatial_var_cost.txt): at 1280 x 720 stage B takes
// about half of one tiled level of the filter at step 1 and the gather two thirds, stage A a fifth.
#pragma once
#include "pt_temporal.h"

namespace ptk {

struct SpatialArgs {
    const float4 *m4;                 // M: (mean r, g, b, m2)
    const float *cnt;                 // N: the effective sample count
    const float4 *posT, *nrmId;       // the guides
    int W, H;
    float invN, invP;
    float4 *out;                      // (c, variance)
};

// the running sums of a pixel's taps
struct SpatialSums {
    float w, s1, s2;
};

// the variance of a pixel that has its own: step 8 of k_temporal
__device__ __forceinline__ float spatialOwn(float m2, float L, float n) {
    float dd = m2 - L * L;
    dd = dd > 0.0f ? dd : 0.0f;
    return dd / (n - 1.0f);
}

// one tap of the window that lies inside the frame and is not the centre: (normal, id), position, luminance and m2 of the tap
__device__ __forceinline__ void spatialTap(const SpatialArgs &A, float4 nq, float qx, float qy, float qz, float Lq, float m2q, const float4 &np,
                                           const float4 &pp, SpatialSums &S) {
    if ((__float_as_int(nq.w) < 0) != (__float_as_int(np.w) < 0)) return;     // exactly one of the two is a miss
    const F3 dn = f3(nq.x, nq.y, nq.z) - f3(np.x, np.y, np.z);
    const F3 dp = f3(qx, qy, qz) - f3(pp.x, pp.y, pp.z);
    float a = dot(dn, dn) * A.invN;
    a = a + dot(dp, dp) * A.invP;
    const float w = expNegPoly(a);
    S.w += w;
    S.s1 += Lq * w;
    S.s2 += m2q * w;
}

__device__ __forceinline__ float spatialFinish(const SpatialSums &S, float n) {
    const float M1 = S.s1 / S.w, M2 = S.s2 / S.w;
    float d = M2 - M1 * M1;
    d = d > 0.0f ? d : 0.0f;
    return d / n;
}

// The plain gather.
template <int R>
__global__ __launch_bounds__(kBlock) void k_spatial_variance_gather(SpatialArgs A) {
    const int tilesX = (A.W + kAtrousTileW - 1) / kAtrousTileW;
    const int tY = (int)(blockIdx.x / (unsigned)tilesX), tX = (int)(blockIdx.x - (unsigned)tY * (unsigned)tilesX);
    const int x = tX * kAtrousTileW + (int)(threadIdx.x & 63u), y = tY * 4 + (int)(threadIdx.x >> 6);
    if (x >= A.W || y >= A.H) return;
    const size_t pix = (size_t)x + (size_t)y * (size_t)A.W;
    const float4 c = A.m4[pix];
    const float n = A.cnt[pix];
    const float L = atrousLum(c.x, c.y, c.z);
    float v;
    if (n >= PT_SPATIAL_MIN_COUNT) {
        v = spatialOwn(c.w, L, n);
    } else {
        const float4 np = A.nrmId[pix], pp = A.posT[pix];
        SpatialSums S = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int dy = -R; dy <= R; ++dy) {
            const int qy = y + dy;
            if (qy < 0 || qy >= A.H) continue;
#pragma unroll
            for (int dx = -R; dx <= R; ++dx) {
                const int qx = x + dx;
                if (dx == 0 && dy == 0) {
                    S.w += 1.0f;
                    S.s1 += L * 1.0f;
                    S.s2 += c.w * 1.0f;
                } else if (qx >= 0 && qx < A.W) {
                    const size_t q = (size_t)qx + (size_t)qy * (size_t)A.W;
                    const float4 mq = A.m4[q], pq = A.posT[q];
                    spatialTap(A, A.nrmId[q], pq.x, pq.y, pq.z, atrousLum(mq.x, mq.y, mq.z), mq.w, np, pp, S);
                }
            }
        }
        v = spatialFinish(S, n);
    }
    A.out[pix] = make_float4(c.x, c.y, c.z, v);
}

// The LDS-tiled form.
template <int R>
__global__ __launch_bounds__(kBlock) void k_spatial_variance_tiled(SpatialArgs A) {
    constexpr int PITCH = kAtrousTileW + 2 * R, ROWS = 4 + 2 * R, ENTRIES = PITCH * ROWS;
    __shared__ float4 s_n[ENTRIES], s_p[ENTRIES];       // (normal, id) and (position, L)
    __shared__ float s_m[ENTRIES];                      // m2
    const int tilesX = (A.W + kAtrousTileW - 1) / kAtrousTileW;
    const int tY = (int)(blockIdx.x / (unsigned)tilesX), tX = (int)(blockIdx.x - (unsigned)tY * (unsigned)tilesX);
    const int x0 = tX * kAtrousTileW, y0 = tY * 4;
    const int tx = (int)(threadIdx.x & 63u), ty = (int)(threadIdx.x >> 6);
    const int x = x0 + tx, y = y0 + ty;
    const bool inside = x < A.W && y < A.H;
    const size_t pix = (size_t)x + (size_t)y * (size_t)A.W;
    float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float n = PT_SPATIAL_MIN_COUNT;
    if (inside) {
        c = A.m4[pix];
        n = A.cnt[pix];
    }
    const float L = atrousLum(c.x, c.y, c.z);
    const bool estimate = inside && !(n >= PT_SPATIAL_MIN_COUNT);
    if (!__syncthreads_or(estimate ? 1 : 0)) {          // (workgroup-uniform) every pixel of the tile has its own variance
        if (inside) A.out[pix] = make_float4(c.x, c.y, c.z, spatialOwn(c.w, L, n));
        return;
    }
    for (int e = (int)threadIdx.x; e < ENTRIES; e += kBlock) {
        const int ly = e / PITCH, lx = e - ly * PITCH;
        const int gx = x0 + lx - R, gy = y0 + ly - R;
        float4 nn = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(kAtrousOutside)), p = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float m2 = 0.0f;
        if (gx >= 0 && gx < A.W && gy >= 0 && gy < A.H) {
            const size_t q = (size_t)gx + (size_t)gy * (size_t)A.W;
            const float4 mq = A.m4[q], pq = A.posT[q];
            nn = A.nrmId[q];
            p = make_float4(pq.x, pq.y, pq.z, atrousLum(mq.x, mq.y, mq.z));
            m2 = mq.w;
        }
        s_n[e] = nn; s_p[e] = p; s_m[e] = m2;
    }
    __syncthreads();
    if (!inside) return;
    float v;
    if (!estimate) {
        v = spatialOwn(c.w, L, n);
    } else {
        const int e0 = (ty + R) * PITCH + tx + R;
        const float4 np = s_n[e0], pp = s_p[e0];
        SpatialSums S = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
            for (int dx = -R; dx <= R; ++dx) {
                if (dx == 0 && dy == 0) {
                    S.w += 1.0f;
                    S.s1 += L * 1.0f;
                    S.s2 += c.w * 1.0f;
                } else {
                    const int e = e0 + dy * PITCH + dx;
                    const float4 nq = s_n[e];
                    if (__float_as_int(nq.w) != kAtrousOutside) {
                        const float4 pq = s_p[e];
                        spatialTap(A, nq, pq.x, pq.y, pq.z, pq.w, s_m[e], np, pp, S);
                    }
                }
            }
        }
        v = spatialFinish(S, n);
    }
    A.out[pix] = make_float4(c.x, c.y, c.z, v);
}

}  // namespace ptk
