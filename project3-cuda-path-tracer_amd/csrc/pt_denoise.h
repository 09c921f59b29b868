// pt_denoise.h -- the edge-avoiding a-trous wavelet filter over the renderer's image, guided by first-hit position and normal
// (Dammertz, Sewtz, Hanika, Lensch: "Edge-Avoiding A-Trous Wavelet Transform for fast Global Illumination Filtering", HPG 2010), and its
// variance-guided variant (SVGF's spatial filter: Schied et al., "Spatiotemporal Variance-Guided Filtering", HPG 2017).
// Its kernels, all outside the render path (k_bounce, k_mesh_walk, k_commit and their arguments do not know of them):
//   k_gbuffer     the guide buffers: the nearest hit of the camera rays of ONE iteration, brute force over the scene's primitives
//   k_variance    the variance of every pixel's mean luminance, from the accumulator and the second moments (PT_FLAG_MOMENTS)
//   k_atrous_*    one level of a filter (the hot path): a 5 x 5 stencil with holes, LDS-tiled per residue class or a plain gather.  One skeleton
//                 each; a filter -- AtrousPlain, AtrousGuided -- is a description of its four differences (below).  (A third description,
//                 AtrousDemod, is AtrousGuided with another last store: pt_albedo.h.)
// Included by pt_api.hip only.
//
// ---- the filters, operation by operation (tests/denoise_ref.py restates the plain one in numpy, tests/denoise_var_ref.py the guided one,
// bit for bit: every fp32 operation below is one IEEE operation, -ffp-contract=off, in the order written) ----
// Common to both:
//   guides      pos_t[p] = (P.x, P.y, P.z, t), nrm_id[p] = (N.x, N.y, N.z, bits of the int32 geom index); a miss is (0, 0, 0, -1) and
//               (0, 0, 0, id = -1).  N is the un-bumped shading normal (hitNormal; a mesh with `vn`: the blended vertex normal).
//   colour      a float4 per pixel: level 0 forms it from the accumulators (difference 1); levels 1 .. levels - 1 read the float4 image
//               the level before wrote; the last level writes packed RGB (difference 4).
//   taps        level i has step s = 2^i.  For the output pixel p the taps are q = p + s (dx, dy), dy = -2 .. 2 (outer loop), dx = -2 .. 2
//               (inner loop), in that order; a tap outside the frame is skipped.
//   weights     h = [1/16, 1/4, 3/8, 1/4, 1/16], hw = h[dy + 2] * h[dx + 2] (exact).  The centre tap has w = hw, nothing is evaluated for
//               it.  A tap of which exactly one of p, q is a miss (id < 0) has weight 0: it is skipped like a tap outside the frame.
//               Every other tap:  a = the filter's colour term (difference 2);  a = a + dot(dn, dn) * invN;  a = a + dot(dp, dp) * invP;
//               w = hw * expNegPoly(a)  with dn, dp = q - p of the normal and the position, dot = ptd::dot ((x + y) + z).
//   sums        sumW += w;  sumC.k += c_q.k * w  (a multiplication and an addition), from sumW = sumC.k = 0;  out.k = sumC.k / sumW.
//               The centre tap alone gives sumW >= 9 / 64: no guard.
//   expNegPoly  ptd::expNegPoly (pt_device.h): t = a * (-1.44269504088896341f); !(t >= -126) -> 0 (NaN lands there); else exp2Poly(t),
//               the exponential half of powPoly.
//   sigmas      on the host, fp32: invN = 1 / (sigma_normal * sigma_normal), invP = 1 / (sigma_position * sigma_position); a sigma of
//               +inf gives 0: term off.
// The result of a pixel is a function of the frame alone: neither kernel form, nor the tile shape, nor the order of the workgroups enters.
//
// AtrousPlain (pt_denoise: one global sigma_color):
//   1 level 0      reads the accumulator: c0.k = sum.k / (float)samples, one correctly rounded division per channel; .w = 0
//   2 colour term  a = dot(dc, dc) * invC_i, dc = q - p of the level's input colour; on the host, fp32:
//                  invC_i = (1 / (sigma_color * sigma_color)) * 4^i (Dammertz halves the colour sigma per level)
//   3 variance     none: no prefilter, the .w of every image is 0
//   4 store        the last level writes packed RGB
// AtrousGuided (pt_denoise_var: the colour term weighted by each pixel's own measured standard error; the variance of the pixel's mean luminance
// rides in the colour float4's .w, so a level stages and moves what the plain filter's does).  lum(c) = (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z
//   1 level 0      reads the accumulator S and the second moments Q (PT_FLAG_MOMENTS: k_commit<true>, k_commit_one<true>), n = (float)samples:
//                  c.k = S.k / n;  L = lum(c);  d = Q / n - L * L;  d = d > 0 ? d : 0 (a NaN gives 0);  v = d / (float)(samples - 1)
//   2 colour term  dl = lum(c_q) - lum(c_p);  a = (dl * dl) * invL, with the
//     scale        invL = 1.0f / (sl2 * g + 1e-8f), sl2 = sigma_lum * sigma_lum (host, fp32); sl2 = +inf: invL = 0, the term is off whatever g
//                  is (inf * 0 would be a NaN).  NOT halved per level: the variance shrinks by itself.
//   3 variance     the prefilter in front of the taps: g = gv / gw over the 3 x 3 taps q = p + s (dx, dy), dy = -1 .. 1 (outer loop),
//                  dx = -1 .. 1 (inner loop), centre included, k = k3[dy + 1] * k3[dx + 1], k3 = [1/4, 1/2, 1/4]:  gw += k;  gv += v_q * k
//                  from 0; a tap outside the frame or across the hit / miss border is skipped.  With the sums:
//                  sumV += v_q * (w * w), behind sumC's;   c' = sumC / sumW;  v' = sumV / (sumW * sumW)
//   4 store        (c', v') between the levels.  The last level writes packed RGB and, where asked for, the filtered variance -- or, in its
//                  BYTES form (PT_FLAG_DISPLAY_FILTER: the level that ends the display path), sendImageToPBO's bytes of the filtered colour
//                  and nothing else: k_to_rgba8's conversion of a mean of one sample, (int)(x * 255.0) formed in double, clamped to
//                  0 .. 255, .w = 0, one uchar4 store per lane -- the bytes k_to_rgba8 makes of the packed RGB, without the 12 B per pixel
//                  written and read back in between.
#pragma once
#include "pt_trace.h"

namespace ptk {

// ---- guide buffers ---------------------------------------------------------------------------------------------------------------
// One thread per pixel of the FULL frame (blocks of kBlock; dynamic LDS = the lanes' mesh traversal stacks, [levels][kBlock] words, as
// k_test_mesh has them).  The camera ray is the one iteration `guideIter` traces for the pixel (cameraRayAt: jitter, and the lens when the
// camera has one); it is tested against EVERY primitive in index order with the renderer's exact tests -- no culling table, no certificate --
// and the nearest hit is chosen as the oracle's nearest_hit does: t > 0, smallest t, an equal t keeps the lower index.  The primitive index is
// wave-uniform: its record arrives through the scalar path.
__global__ __launch_bounds__(kBlock) void k_gbuffer(KParams prm, const GeomDev *ggeoms, const float4 *meshRecs, int guideIter, float4 *posT,
                                                    float4 *nrmId) {
    extern __shared__ uint32_t s_gbufStack[];
    const int npix = prm.W * prm.H;
    const int pix = blockIdx.x * kBlock + threadIdx.x;
    const int pc = pix < npix ? pix : npix - 1;       // (lanes beyond the frame trace its last pixel and store nothing)
    const int y = (int)fastDiv((uint32_t)pc, prm.magicW, prm.shiftW);
    const int x = pc - y * prm.W;
    F3 org, dir;
    cameraRayAt(prm, iterationHash(guideIter, 0), pc, x, y, org, dir);
    const GeomPtr geoms = (GeomPtr)ggeoms;
    int hit = -1;
    float tMin = 0.0f;
    F3 P = f3(0.0f, 0.0f, 0.0f), nsrc = f3(0.0f, 0.0f, 0.0f);
    bool outside = false;
    for (int g = 0; g < prm.ngeoms; ++g) {
        const PT_CAS GeomDev &G = *(launder(geoms) + g);
        F3 tp = f3(0.0f, 0.0f, 0.0f), tn = f3(0.0f, 0.0f, 0.0f);
        bool to = false;
        float t;
        if ((G.flags & 32) != 0) t = meshIntersectionTest<false, kBlock>(G, meshRecs, G.meshRoot, G.meshStride, s_gbufStack + threadIdx.x, org, dir, tp, tn, to);
        else if ((G.flags & 1) == 0) t = sphereIntersectionTest(G, org, dir, tp, tn, to);
        else t = boxIntersectionTest<false>(G, org, dir, tp, tn, to);
        if (t > 0.0f && (hit < 0 || t < tMin)) {
            tMin = t;
            hit = g;
            P = tp;
            nsrc = tn;
            outside = to;
        }
    }
    if (pix >= npix) return;
    float4 a = make_float4(0.0f, 0.0f, 0.0f, -1.0f), b = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
    if (hit >= 0) {
        const F3 N = hitNormal(ggeoms[hit], nsrc, outside);       // (per lane: the winner's record through the vector path, once)
        a = make_float4(P.x, P.y, P.z, tMin);
        b = make_float4(N.x, N.y, N.z, __int_as_float(hit));
    }
    posT[pix] = a;
    nrmId[pix] = b;
}

// ---- the variance of the mean ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float atrousLum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// the mean colour and the variance of its luminance from the two accumulators (k_variance, and level 0 of the guided filter)
__device__ __forceinline__ float4 meanAndVariance(const float *accum, const float *moments, size_t pix, float n, float nM1) {
    const float *s = accum + 3 * pix;
    const float r = s[0] / n, g = s[1] / n, b = s[2] / n;
    const float L = atrousLum(r, g, b);
    float d = moments[pix] / n - L * L;
    d = d > 0.0f ? d : 0.0f;
    return make_float4(r, g, b, d / nM1);
}

// pt_variance: the variance of every pixel's mean luminance
__global__ __launch_bounds__(kBlock) void k_variance(const float *accum, const float *moments, int npix, float n, float nM1, float *var) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= npix) return;
    var[i] = meanAndVariance(accum, moments, (size_t)i, n, nM1).w;
}

// k_to_rgba8's conversion of one channel of a mean (pt_trace.h)
__device__ __forceinline__ unsigned char atrousByte(float x) {
    const int i = (int)(x * 255.0);
    return (unsigned char)(i < 0 ? 0 : (i > 255 ? 255 : i));
}

// ---- one level of a filter ----------------------------------------------------------------------------------------------------------
constexpr int kAtrousOutside = (int)0x80000000;      // LDS halo: the id of an entry outside the frame (ids of the frame are >= -1)
constexpr int kAtrousTileW = 64;                     // a wave filters 64 consecutive pixels of one row of its residue class
constexpr int kAtrousPitch = kAtrousTileW + 4;       // ... whose LDS rows carry the two-pixel halo on either side
constexpr int kAtrousTiledMaxStep = 4;               // levels of a larger step take the plain gather (pt_api.hip: atrous_run); a choice by reasoning, unmeasured
constexpr int kAtrousVarTiledMaxStep = 8;            // ... of the variance-guided filter: measured -- at step 8 the 64 x 8 tiles beat the gather by a sixth at
                                                     // 1280 x 720, at step 16 by less than two spreads, beyond nothing is measured (profiles/denoise_var_cost.txt)

// the output pixel of a stencil: its colour, normal + id and position, and what the guided filter forms of them once (lum(c); invL)
struct AtrousCentre {
    float4 c, n, p;
    float lum, invL;
};

// the running sums of a pixel's taps: weight, colour, variance (dead code in a filter without the variance channel)
struct AtrousSums {
    float w;
    F3 c;
    float v;
};

// A filter description: the kernel argument struct (the skeleton uses the names both have), whether the colour's .w carries a variance, the
// level-0 colour load, the colour term of a tap, the store of (r, g, b, variance), the largest step the product path tiles, and -- on the
// host -- the colour term's scale at a level.
struct AtrousArgs {
    const float *accum;       // FIRST: the accumulator, packed RGB sums
    const float4 *cin;        // later levels: the level before
    float4 *cout;             // every level but the last
    float *out3;              // LAST: packed RGB
    const float4 *posT, *nrmId;
    int W, H, step;
    float samples;            // FIRST: (float)samples
    float invC, invN, invP;
};

struct AtrousPlain {
    using Args = AtrousArgs;
    static constexpr bool kVariance = false;
    static constexpr int kTiledMaxStep = kAtrousTiledMaxStep;
    static void hostColourScale(Args &A, float sigma, int level) { A.invC = (1.0f / (sigma * sigma)) * (float)(1 << (2 * level)); }
    template <bool FIRST>
    static __device__ __forceinline__ float4 colour(const Args &A, size_t pix) {
        if (!FIRST) return A.cin[pix];
        const float *s = A.accum + 3 * pix;
        return make_float4(s[0] / A.samples, s[1] / A.samples, s[2] / A.samples, 0.0f);
    }
    static __device__ __forceinline__ float colourTerm(const Args &A, float4 cq, const AtrousCentre &P) {
        const F3 dc = f3(cq.x, cq.y, cq.z) - f3(P.c.x, P.c.y, P.c.z);
        return dot(dc, dc) * A.invC;
    }
    template <bool LAST, bool BYTES>
    static __device__ __forceinline__ void store(const Args &A, size_t pix, float4 o) {
        static_assert(!BYTES, "the plain filter has no BYTES form");
        if (LAST) {
            float *d = A.out3 + 3 * pix;
            d[0] = o.x; d[1] = o.y; d[2] = o.z;
        } else {
            A.cout[pix] = make_float4(o.x, o.y, o.z, 0.0f);
        }
    }
};

struct AtrousVarArgs {
    const float *accum, *moments;   // FIRST: the accumulator's packed RGB sums and the sums of squared luminance
    const float4 *cin;              // later levels: the level before, (r, g, b, variance)
    float4 *cout;                   // every level but the last
    union {
        float *out3;                // LAST: packed RGB ...
        uchar4 *out8;               // ... or, BYTES: the display's bytes (the same kernel argument: the other forms keep their layout)
    };
    float *outVar;                  // LAST: the variance (or NULL); BYTES: unused
    const float4 *posT, *nrmId;
    int W, H, step;
    float samples, samplesM1;       // FIRST: (float)samples, (float)(samples - 1)
    float sl2, invN, invP;
};

struct AtrousGuided {
    using Args = AtrousVarArgs;
    static constexpr bool kVariance = true;
    static constexpr int kTiledMaxStep = kAtrousVarTiledMaxStep;
    static void hostColourScale(Args &A, float sigma, int) { A.sl2 = sigma * sigma; }
    template <bool FIRST>
    static __device__ __forceinline__ float4 colour(const Args &A, size_t pix) {
        if (!FIRST) return A.cin[pix];
        return meanAndVariance(A.accum, A.moments, pix, A.samples, A.samplesM1);
    }
    static __device__ __forceinline__ float colourTerm(const Args &, float4 cq, const AtrousCentre &P) {
        const float dl = atrousLum(cq.x, cq.y, cq.z) - P.lum;
        return (dl * dl) * P.invL;
    }
    template <bool LAST, bool BYTES>
    static __device__ __forceinline__ void store(const Args &A, size_t pix, float4 o) {
        if (BYTES) {
            uchar4 b;
            b.w = 0; b.x = atrousByte(o.x); b.y = atrousByte(o.y); b.z = atrousByte(o.z);
            A.out8[pix] = b;
        } else if (LAST) {
            float *d = A.out3 + 3 * pix;
            d[0] = o.x; d[1] = o.y; d[2] = o.z;
            if (A.outVar) A.outVar[pix] = o.w;
        } else {
            A.cout[pix] = o;
        }
    }
};

__device__ __forceinline__ float atrousH(int i) { return i == 2 ? 0.375f : ((i == 1 || i == 3) ? 0.25f : 0.0625f); }
__device__ __forceinline__ float atrousK3(int i) { return i == 1 ? 0.5f : 0.25f; }

// one tap of the 3 x 3 variance prefilter that lies inside the frame: (variance, bits of the id) of the tap, the id's bits of the centre
__device__ __forceinline__ void atrousPreTap(float k, float vq, float idq, float idp, float &gw, float &gv) {
    if ((__float_as_int(idq) < 0) != (__float_as_int(idp) < 0)) return;
    gw += k;
    gv += vq * k;
}

// what the guided filter's taps need of the centre, behind the prefilter
__device__ __forceinline__ void atrousScale(AtrousCentre &P, float sl2, float gw, float gv) {
    const float g = gv / gw;
    P.invL = sl2 <= 3.402823466e38f ? 1.0f / (sl2 * g + 1e-8f) : 0.0f;      // (uniform: +inf switches the term off)
    P.lum = atrousLum(P.c.x, P.c.y, P.c.z);
}

// one tap of the 5 x 5 stencil that lies inside the frame
template <class Filter, bool CENTRE>
__device__ __forceinline__ void atrousTap(const typename Filter::Args &A, float hw, float4 cq, float4 nq, float4 pq, const AtrousCentre &P, AtrousSums &S) {
    float w = hw;
    if (!CENTRE) {
        if ((__float_as_int(nq.w) < 0) != (__float_as_int(P.n.w) < 0)) return;     // exactly one of the two is a miss
        float a = Filter::colourTerm(A, cq, P);
        const F3 dn = f3(nq.x, nq.y, nq.z) - f3(P.n.x, P.n.y, P.n.z);
        const F3 dp = f3(pq.x, pq.y, pq.z) - f3(P.p.x, P.p.y, P.p.z);
        a = a + dot(dn, dn) * A.invN;
        a = a + dot(dp, dp) * A.invP;
        w = hw * expNegPoly(a);
    }
    S.w += w;
    S.c.x += cq.x * w;
    S.c.y += cq.y * w;
    S.c.z += cq.z * w;
    S.v += cq.w * (w * w);
}

template <class Filter, bool LAST, bool BYTES>
__device__ __forceinline__ void atrousStore(const typename Filter::Args &A, size_t pix, const AtrousSums &S) {
    Filter::template store<LAST, BYTES>(A, pix, make_float4(S.c.x / S.w, S.c.y / S.w, S.c.z / S.w, S.v / (S.w * S.w)));
}

// The plain gather: a workgroup filters 64 x 4 neighbouring pixels, every tap is a load through L2.
template <class Filter, bool FIRST, bool LAST, bool BYTES = false>
__global__ __launch_bounds__(kBlock) void k_atrous_gather(typename Filter::Args A) {
    static_assert(LAST || !BYTES, "only a last level writes the bytes");
    static_assert(Filter::kVariance || !BYTES, "only the variance-guided filter ends the display path");
    const int tilesX = (A.W + kAtrousTileW - 1) / kAtrousTileW;
    const int tY = (int)(blockIdx.x / (unsigned)tilesX), tX = (int)(blockIdx.x - (unsigned)tY * (unsigned)tilesX);
    const int x = tX * kAtrousTileW + (int)(threadIdx.x & 63u), y = tY * 4 + (int)(threadIdx.x >> 6);
    if (x >= A.W || y >= A.H) return;
    const size_t pix = (size_t)x + (size_t)y * (size_t)A.W;
    AtrousCentre P = {Filter::template colour<FIRST>(A, pix), A.nrmId[pix], A.posT[pix], 0.0f, 0.0f};
    if constexpr (Filter::kVariance) {
        float gw = 0.0f, gv = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int qy = y + dy * A.step;
            if (qy < 0 || qy >= A.H) continue;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int qx = x + dx * A.step;
                const float k = atrousK3(dy + 1) * atrousK3(dx + 1);
                if (dx == 0 && dy == 0) {
                    atrousPreTap(k, P.c.w, P.n.w, P.n.w, gw, gv);
                } else if (qx >= 0 && qx < A.W) {
                    const size_t q = (size_t)qx + (size_t)qy * (size_t)A.W;
                    atrousPreTap(k, Filter::template colour<FIRST>(A, q).w, A.nrmId[q].w, P.n.w, gw, gv);
                }
            }
        }
        atrousScale(P, A.sl2, gw, gv);
    }
    AtrousSums S = {0.0f, f3(0.0f, 0.0f, 0.0f), 0.0f};
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * A.step;
        if (qy < 0 || qy >= A.H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * A.step;
            const float hw = atrousH(dy + 2) * atrousH(dx + 2);
            if (dx == 0 && dy == 0) {
                atrousTap<Filter, true>(A, hw, P.c, P.n, P.p, P, S);
            } else if (qx >= 0 && qx < A.W) {
                const size_t q = (size_t)qx + (size_t)qy * (size_t)A.W;
                const float4 nq = A.nrmId[q];
                atrousTap<Filter, false>(A, hw, Filter::template colour<FIRST>(A, q), nq, A.posT[q], P, S);
            }
        }
    }
    atrousStore<Filter, LAST, BYTES>(A, pix, S);
}

// The LDS-tiled form.  The taps of a level stay inside one residue class (x mod s, y mod s), in which they are a DENSE 5 x 5 stencil: a
// workgroup owns a tile of 64 x (4 RPT) pixels of one class, stages the tile and its two-pixel halo -- colour, normal + id, position: three
// float4 images of kAtrousPitch x (4 RPT + 4) entries -- in LDS once and filters from there, RPT rows per wave.  A wave reads 64 consecutive
// 16-byte entries of one LDS row per tap (ds_read_b128: each of its 16-lane groups covers the 16 slots of the 256-byte bank row exactly
// once, whatever dx and the row pitch: no bank conflict); the staging writes are 16-byte stores of consecutive entries.
// Grid: classes x tiles of the largest class; a tile beyond its class's extent returns before the barrier.
// The 3 x 3 prefilter reads the .w of the eight inner taps' colour and normal + id entries once more: 16 ds_read_b32 per row next to the taps'
// 16-byte reads, each striding 16 bytes across the wave (four lanes per bank).  The levels are bound by vector issue, not by LDS
// (profiles/denoise_var_cost.txt: a tiled level costs 1.00 - 1.12 x the plain filter's), so the entries are not kept in registers for them.
template <class Filter, bool FIRST, bool LAST, int RPT, bool BYTES = false>
__global__ __launch_bounds__(kBlock) void k_atrous_tiled(typename Filter::Args A) {
    static_assert(LAST || !BYTES, "only a last level writes the bytes");
    static_assert(Filter::kVariance || !BYTES, "only the variance-guided filter ends the display path");
    constexpr int TH = 4 * RPT, ROWS = TH + 4, ENTRIES = kAtrousPitch * ROWS;
    __shared__ float4 s_c[ENTRIES], s_n[ENTRIES], s_p[ENTRIES];
    const int s = A.step;
    const int cw = (A.W + s - 1) / s, ch = (A.H + s - 1) / s;          // extent of the largest class
    const int tilesX = (cw + kAtrousTileW - 1) / kAtrousTileW, tilesY = (ch + TH - 1) / TH;
    const unsigned perClass = (unsigned)tilesX * (unsigned)tilesY;
    const int cls = (int)(blockIdx.x / perClass), tile = (int)(blockIdx.x - (unsigned)cls * perClass);
    const int ry = cls / s, rx = cls - ry * s;
    const int tY = tile / tilesX, tX = tile - tY * tilesX;
    const int cx0 = tX * kAtrousTileW, cy0 = tY * TH;                   // the tile's first pixel, in class coordinates
    if (rx + s * cx0 >= A.W || ry + s * cy0 >= A.H) return;             // (workgroup-uniform)
    for (int e = (int)threadIdx.x; e < ENTRIES; e += kBlock) {
        const int ly = e / kAtrousPitch, lx = e - ly * kAtrousPitch;
        const int x = rx + s * (cx0 + lx - 2), y = ry + s * (cy0 + ly - 2);
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), n = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(kAtrousOutside)), p = c;
        if (x >= 0 && x < A.W && y >= 0 && y < A.H) {
            const size_t q = (size_t)x + (size_t)y * (size_t)A.W;
            c = Filter::template colour<FIRST>(A, q);
            n = A.nrmId[q];
            p = A.posT[q];
        }
        s_c[e] = c; s_n[e] = n; s_p[e] = p;
    }
    __syncthreads();
    const int tx = (int)(threadIdx.x & 63u), wy = (int)(threadIdx.x >> 6);
    const int x = rx + s * (cx0 + tx);
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int ly = wy + 4 * r;
        const int y = ry + s * (cy0 + ly);
        if (x >= A.W || y >= A.H) continue;
        const int e0 = (ly + 2) * kAtrousPitch + tx + 2;
        AtrousCentre P = {s_c[e0], s_n[e0], s_p[e0], 0.0f, 0.0f};
        if constexpr (Filter::kVariance) {
            float gw = 0.0f, gv = 0.0f;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const float k = atrousK3(dy + 1) * atrousK3(dx + 1);
                    if (dx == 0 && dy == 0) {
                        atrousPreTap(k, P.c.w, P.n.w, P.n.w, gw, gv);
                    } else {
                        const int e = e0 + dy * kAtrousPitch + dx;
                        const float idq = s_n[e].w;
                        if (__float_as_int(idq) != kAtrousOutside) atrousPreTap(k, s_c[e].w, idq, P.n.w, gw, gv);
                    }
                }
            }
            atrousScale(P, A.sl2, gw, gv);
        }
        AtrousSums S = {0.0f, f3(0.0f, 0.0f, 0.0f), 0.0f};
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const float hw = atrousH(dy + 2) * atrousH(dx + 2);
                if (dx == 0 && dy == 0) {
                    atrousTap<Filter, true>(A, hw, P.c, P.n, P.p, P, S);
                } else {
                    const int e = e0 + dy * kAtrousPitch + dx;
                    const float4 nq = s_n[e];
                    if (__float_as_int(nq.w) != kAtrousOutside) atrousTap<Filter, false>(A, hw, s_c[e], nq, s_p[e], P, S);
                }
            }
        }
        atrousStore<Filter, LAST, BYTES>(A, (size_t)x + (size_t)y * (size_t)A.W, S);
    }
}

// workgroups of a level's launch
inline unsigned atrousGridGather(int W, int H) {
    return (unsigned)((W + kAtrousTileW - 1) / kAtrousTileW) * (unsigned)((H + 3) / 4);
}
inline unsigned long long atrousGridTiled(int W, int H, int s, int rpt) {
    const int cw = (W + s - 1) / s, ch = (H + s - 1) / s, th = 4 * rpt;
    return (unsigned long long)((cw + kAtrousTileW - 1) / kAtrousTileW) * (unsigned long long)((ch + th - 1) / th) * (unsigned long long)s * (unsigned long long)s;
}

}  // namespace ptk
