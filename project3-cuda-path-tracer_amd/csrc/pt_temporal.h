// pt_temporal.h -- temporal reprojection (PT_FLAG_TEMPORAL): the temporal half of SVGF (Schied et al., HPG 2017) for a static scene under a
// moving pinhole camera.  One kernel, outside the render path like the denoiser's (k_bounce, k_mesh_walk, k_commit and their arguments do not
// know of it); included by pt_api.hip only.
//   k_temporal<kTemporalFilter>    the FILTER form: per pixel of the new view the count-weighted blend of the reprojected history with the new samples, as
//                                  the (r, g, b, variance) image level 0 of k_atrous_*<AtrousGuided> then reads in place of meanAndVariance(S, Q)
//   k_temporal<kTemporalCapture>   the CAPTURE form: the same blend, stored as the next history (mean colour, mean squared luminance; the capped count)
//   k_temporal<kTemporalMoments>   the MOMENTS form: the same blend, stored with the count uncapped -- what the spatial variance estimate reads
//                                  (PT_FLAG_SPATIAL_VARIANCE: pt_spatial_var.h)
//   k_temporal<FORM, true>         ALBEDO (PT_FLAG_DEMOD_HISTORY): each of the three also blends the history's mean first-hit albedo with the
//                                  renderer's albedo sums and writes it; kTemporalFilterDemod is the filter form with the division by that
//                                  albedo folded into its store.  The ALBEDO = false forms are the kernels they were before.
//
// ---- the kernel, operation by operation (tests/temporal_ref.py restates it in numpy, bit for bit: every fp32 operation below is one IEEE
// operation, -ffp-contract=off, in the order written; dot = (x + y) + z as ptd::dot) ----
//   inputs      the current view: S (packed RGB sums), Q (sums of squared luminance), n = (float)samples, the guides (P, t) and (N, id);
//               the history: Hc = (mean r, g, b, mean squared luminance m2), Hn = effective sample count (0: none), the old view's guides
//               Hpos = (P_q, t_q), Hnrm = (N_q, id_q), and the old camera: eye e, pixLenX, pixLenY, halfW, halfH and the rows r0, r1, r2 of the
//               inverse of [view | -right | -up] (the host inverts in double and rounds once: temporal_camera), the exact inverse of
//               cameraRayAt's pinhole map dir ~ (view - right a) - up b
//   1           id < 0: no history
//   2           d = P - e;  s = dot(r0, d);  !(s > 0): no history (behind the old camera; a NaN lands here)
//   3           a = dot(r1, d) / s;  b = dot(r2, d) / s;  u = (a / pixLenX + halfW) - 0.5f;  v = (b / pixLenY + halfH) - 0.5f;
//               !(u > -1 && u < W && v > -1 && v < H): no history (W, H as floats; a NaN lands here)
//   4           x0 = floor(u), wx = u - x0;  y0 = floor(v), wy = v - y0
//   5           four taps q = (x0 + i, y0 + j), j = 0, 1 outer, i = 0, 1 inner.  A tap counts iff q is inside the frame, Hn[q] > 0, id_q == id
//               (integers), dot(N_q, N) >= c_n and |dot(P_q - P, N)| <= c_p * t.  Then w = (i ? wx : 1 - wx) * (j ? wy : 1 - wy);
//               sumW += w;  sumC.k += Hc[q].k * w (k = r, g, b, m2);  sumN += Hn[q] * w  -- all from 0
//   6           !(sumW > w_min): no history.  Else hc = sumC / sumW, hn = sumN / sumW, Nh = hn < cap ? hn : cap
//   7           no history: hc = 0, Nh = 0.  tot = Nh + n;  c.k = (hc.k * Nh + S.k) / tot;  m2 = (hc.m2 * Nh + Q) / tot
//   8  filter   L = atrousLum(c);  dd = m2 - L * L;  dd = dd > 0 ? dd : 0 (a NaN gives 0);  out = (c, dd / (tot - 1))
//      capture  Hc' = (c, m2);  Hn' = tot < cap ? tot : cap
//      moments  M = (c, m2);  N = tot
// ---- ALBEDO (PT_FLAG_DEMOD_HISTORY: the history also carries the mean first-hit albedo; tests/temporal_demod_ref.py restates it) ----
//   inputs      Ha = (mean first-hit albedo r, g, b; .w is never read) beside Hc, and Asum, the renderer's albedo sums (k_albedo's, pt_albedo.h)
//   5           every tap that counts also adds  sumA.k += Ha[q].k * w  (k = r, g, b) -- from 0; taps, conditions and order as above
//   6           ha.k = sumA.k / sumW
//   7           no history: ha = 0.  Ab.k = (ha.k * Nh + Asum.k) / tot
//   8           outA = (Ab, tot) in every form: the capture's is the next history's Ha', the filter's and the moments form's what k_demodulate
//               divides out (with samples = 1: x / 1 is exact) and, below PT_DEMOD_HISTORY_MIN_OWN samples, what the last level multiplies back
//      fused    kTemporalFilterDemod: the filter form with k_demodulate's operations (pt_albedo.h) applied to its own result before the store:
//               A'.k = Ab.k > eps ? Ab.k : eps;  c'.k = c.k / A'.k;  L' = lum(c');  rho = L > 0 ? L' / L : 1;  out = (c', v * (rho * rho))
//               -- the bits of k_temporal<kTemporalFilter, true> followed by k_demodulate<true>
// Without history Ab = (0 * 0 + Asum) / n = Asum / n: the bits demodAlbedo forms before its floor.
// Without history step 7 is 0 * 0 + S = S over n and step 8 is meanAndVariance(S, Q) to the bit (sums are never -0: they grow from +0).
// ---- MOTION (PT_FLAG_OBJECT_HISTORY: the history follows primitives that moved between the two views; tests/temporal_motion_ref.py restates it) ----
//   inputs      the motion table, one row of 96 bytes per primitive (MotionRow): m[3][4], rows 0..2 of A = T_old Tinv_new -- the new world to the
//               old --, G[3][3], the inverse transpose of A's linear part, and the primitive's state (0 unmoved, 1 moved, 2 no history); the host
//               forms both in double and rounds once (pt_api.hip: motion_table).  capH: the cap step 6 takes in the place of `cap`
//               (PT_OBJECT_HISTORY_MAX for a table that holds a row of another state than 0)
//   1'          st = row[id].state (an id past the table: 0)
//               st == 2: no history
//               st == 1: P'.k = ((m[k][0] * P.x + m[k][1] * P.y) + m[k][2] * P.z) + m[k][3];  g.k = (G[k][0] * N.x + G[k][1] * N.y) + G[k][2] * N.z;
//                        l = (g.x * g.x + g.y * g.y) + g.z * g.z;  !(l > 0): no history (a NaN lands here);  N' = g / sqrtf(l)
//               st == 0: P' = P, N' = N -- the values themselves, not their product with an identity: an unmoved primitive takes the bits above
//   2 .. 5      with P' for P and N' for N: d = P' - e, dot(N_q, N') >= c_n, |dot(P_q - P', N')| <= c_p * t.  t stays the new hit's own distance,
//               id_q == id stays
//   6           Nh = hn < capH ? hn : capH.  Steps 7, 8 and all of ALBEDO as above (the capture's and the moments form's counts keep `cap`)
// The MOTION = false forms are the kernels they were before.
// cap, c_n, c_p, w_min: PT_TEMPORAL_MAX_HISTORY, _NORMAL_DOT, _PLANE_FRACTION, _MIN_WEIGHT of include/pt_amd.h.
//
// Cost: a gather.  A pixel reads its own 60 bytes (S 12, Q 4, two guide float4s 32, and 12 of padding it does not use), up to four taps of
// 52 bytes from four arrays -- neighbouring pixels project to neighbouring old pixels, so a wave's taps fall into the cache lines its
// neighbours fetch -- and writes 16 (filter) or 20 bytes (capture).  ALBEDO: a tap reads 68 bytes from five arrays, a pixel 16 more of its own
// (Asum) and writes 16 more (outA).  MOTION: a pixel reads 16 bytes of its primitive's row for the state, and 80 more where it moved -- per
// lane, but a wave shows few primitives: the rows are cache lines its lanes share.
#pragma once
#include "pt_denoise.h"

namespace ptk {

// the old view's camera as the kernel needs it: plain fp32 constants
struct TemporalCam {
    float e[3];
    float pixLenX, pixLenY, halfW, halfH;
    float r0[3], r1[3], r2[3];
};

struct TemporalArgs {
    const float *accum, *moments;     // S, Q of the current view
    const float4 *posT, *nrmId;       // its guides
    const float4 *hc;                 // history: (mean r, g, b, m2) ...
    const float *hn;                  // ... the effective sample count (NULL: the context holds no history -- every pixel takes step 7 without) ...
    const float4 *hpos, *hnrm;        // ... and the old view's guides
    TemporalCam cam;
    int W, H;
    float samples;
    float4 *out;                      // filter: (c, variance); capture: Hc'; moments: M
    float *outN;                      // capture: Hn'; moments: N
    // ALBEDO alone reads what follows (behind the members every form reads: their places in the kernel's arguments are the unflagged build's)
    const float4 *ha;                 // history: the mean first-hit albedo (NULL with hn)
    const float4 *asum;               // the current view's albedo sums
    float4 *outA;                     // (Ab, tot)
    float eps;                        // kTemporalFilterDemod: PT_DEMOD_MIN_ALBEDO
    // MOTION alone reads what follows
    const float4 *motion;             // MotionRow[motionN] as six float4 per primitive
    int motionN;
    float histCap;                    // step 6's cap
};

// a primitive's row of the motion table (PT_FLAG_OBJECT_HISTORY): six float4, so that a lane fetches it in 16-byte loads -- g0 first, for the state
struct MotionRow {
    float m[3][4];                    // rows 0..2 of A: new world -> old world
    float g0[3]; int state;           // row 0 of G, the inverse transpose of A's linear part; 0 unmoved, 1 moved, 2 no history
    float g1[3], pad1;
    float g2[3], pad2;
};
static_assert(sizeof(MotionRow) == 96, "six float4 per primitive");
enum { kMotionRowVec = 6 };

enum { kTemporalFilter = 0, kTemporalCapture = 1, kTemporalMoments = 2, kTemporalFilterDemod = 3 };

template <int FORM, bool ALBEDO = false, bool MOTION = false>
__global__ __launch_bounds__(kBlock) void k_temporal(TemporalArgs A) {
    static_assert(FORM != kTemporalFilterDemod || ALBEDO, "the fused front divides by the blended albedo");
    const int npix = A.W * A.H;
    const int pix = blockIdx.x * kBlock + threadIdx.x;
    if (pix >= npix) return;
    const float cap = PT_TEMPORAL_MAX_HISTORY;
    float4 pp = A.posT[pix], np = A.nrmId[pix];
    const int id = __float_as_int(np.w);
    const float capH = MOTION ? A.histCap : cap;
    bool follow = true;               // MOTION, step 1': false where the primitive's row says there is no history to follow
    if (MOTION && A.hn != nullptr && id >= 0 && id < A.motionN) {
        const float4 *row = A.motion + (size_t)id * kMotionRowVec;
        const float4 g0 = row[3];
        const int st = __float_as_int(g0.w);
        if (st == 1) {
            const float4 m0 = row[0], m1 = row[1], m2r = row[2], g1 = row[4], g2 = row[5];
            const float px = ((m0.x * pp.x + m0.y * pp.y) + m0.z * pp.z) + m0.w;
            const float py = ((m1.x * pp.x + m1.y * pp.y) + m1.z * pp.z) + m1.w;
            const float pz = ((m2r.x * pp.x + m2r.y * pp.y) + m2r.z * pp.z) + m2r.w;
            const float gx = (g0.x * np.x + g0.y * np.y) + g0.z * np.z;
            const float gy = (g1.x * np.x + g1.y * np.y) + g1.z * np.z;
            const float gz = (g2.x * np.x + g2.y * np.y) + g2.z * np.z;
            const float l = (gx * gx + gy * gy) + gz * gz;
            if (l > 0.0f) {
                const float len = __builtin_sqrtf(l);
                pp.x = px; pp.y = py; pp.z = pz;
                np.x = gx / len; np.y = gy / len; np.z = gz / len;
            } else {
                follow = false;
            }
        } else if (st != 0) {
            follow = false;
        }
    }
    float hcx = 0.0f, hcy = 0.0f, hcz = 0.0f, hcw = 0.0f, Nh = 0.0f;
    float hax = 0.0f, hay = 0.0f, haz = 0.0f;
    if (A.hn != nullptr && id >= 0 && (!MOTION || follow)) {
        const TemporalCam &c = A.cam;
        const float dx = pp.x - c.e[0], dy = pp.y - c.e[1], dz = pp.z - c.e[2];
        const float s = (c.r0[0] * dx + c.r0[1] * dy) + c.r0[2] * dz;
        if (s > 0.0f) {
            const float a = ((c.r1[0] * dx + c.r1[1] * dy) + c.r1[2] * dz) / s;
            const float b = ((c.r2[0] * dx + c.r2[1] * dy) + c.r2[2] * dz) / s;
            const float u = (a / c.pixLenX + c.halfW) - 0.5f;
            const float v = (b / c.pixLenY + c.halfH) - 0.5f;
            if (u > -1.0f && u < (float)A.W && v > -1.0f && v < (float)A.H) {
                const float fx = __builtin_floorf(u), fy = __builtin_floorf(v);
                const float wx = u - fx, wy = v - fy;
                const int x0 = (int)fx, y0 = (int)fy;
                const float lim = PT_TEMPORAL_PLANE_FRACTION * pp.w;
                float sumW = 0.0f, sumN = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sw = 0.0f;
                float ax = 0.0f, ay = 0.0f, az = 0.0f;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int qy = y0 + j;
                    if (qy < 0 || qy >= A.H) continue;
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int qx = x0 + i;
                        if (qx < 0 || qx >= A.W) continue;
                        const int q = qx + qy * A.W;
                        const float nq = A.hn[q];
                        if (!(nq > 0.0f)) continue;
                        const float4 hn4 = A.hnrm[q];
                        if (__float_as_int(hn4.w) != id) continue;
                        if (!((hn4.x * np.x + hn4.y * np.y) + hn4.z * np.z >= PT_TEMPORAL_NORMAL_DOT)) continue;
                        const float4 hp = A.hpos[q];
                        const float off = ((hp.x - pp.x) * np.x + (hp.y - pp.y) * np.y) + (hp.z - pp.z) * np.z;
                        if (!(__builtin_fabsf(off) <= lim)) continue;
                        const float w = (i ? wx : 1.0f - wx) * (j ? wy : 1.0f - wy);
                        const float4 h = A.hc[q];
                        sumW += w;
                        sx += h.x * w;
                        sy += h.y * w;
                        sz += h.z * w;
                        sw += h.w * w;
                        sumN += nq * w;
                        if (ALBEDO) {
                            const float4 a = A.ha[q];
                            ax += a.x * w;
                            ay += a.y * w;
                            az += a.z * w;
                        }
                    }
                }
                if (sumW > PT_TEMPORAL_MIN_WEIGHT) {
                    hcx = sx / sumW; hcy = sy / sumW; hcz = sz / sumW; hcw = sw / sumW;
                    const float hn = sumN / sumW;
                    Nh = hn < capH ? hn : capH;
                    if (ALBEDO) { hax = ax / sumW; hay = ay / sumW; haz = az / sumW; }
                }
            }
        }
    }
    const float *S = A.accum + 3 * (size_t)pix;
    const float tot = Nh + A.samples;
    const float r = (hcx * Nh + S[0]) / tot, g = (hcy * Nh + S[1]) / tot, b = (hcz * Nh + S[2]) / tot;
    const float m2 = (hcw * Nh + A.moments[pix]) / tot;
    float abx = 0.0f, aby = 0.0f, abz = 0.0f;
    if (ALBEDO) {
        const float4 as = A.asum[pix];
        abx = (hax * Nh + as.x) / tot; aby = (hay * Nh + as.y) / tot; abz = (haz * Nh + as.z) / tot;
        A.outA[pix] = make_float4(abx, aby, abz, tot);
    }
    if (FORM == kTemporalCapture) {
        A.out[pix] = make_float4(r, g, b, m2);
        A.outN[pix] = tot < cap ? tot : cap;
    } else if (FORM == kTemporalMoments) {
        A.out[pix] = make_float4(r, g, b, m2);
        A.outN[pix] = tot;
    } else {
        const float L = atrousLum(r, g, b);
        float dd = m2 - L * L;
        dd = dd > 0.0f ? dd : 0.0f;
        const float var = dd / (tot - 1.0f);
        if (FORM == kTemporalFilterDemod) {
            const float alx = abx > A.eps ? abx : A.eps, aly = aby > A.eps ? aby : A.eps, alz = abz > A.eps ? abz : A.eps;
            const float rd = r / alx, gd = g / aly, bd = b / alz;
            const float Ld = atrousLum(rd, gd, bd);
            const float rho = L > 0.0f ? Ld / L : 1.0f;
            A.out[pix] = make_float4(rd, gd, bd, var * (rho * rho));
        } else {
            A.out[pix] = make_float4(r, g, b, var);
        }
    }
}

}  // namespace ptk
