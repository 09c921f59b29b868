// pt_albedo.h -- albedo demodulation (PT_FLAG_DEMODULATE): the variance-guided filter runs on the light that reaches a surface, not on the
// light it reflects, so that a texture under the filter's stencil is divided out before the levels and multiplied back behind them (SVGF
// filters demodulated illumination the same way: Schied et al., "Spatiotemporal Variance-Guided Filtering", HPG 2017).  Two kernels, both outside the render path like the
// denoiser's (k_bounce, k_mesh_walk, k_commit and their arguments do not know of them); the remodulating store is the third filter description of
// pt_denoise.h, AtrousDemod.  Included by pt_api.hip only.
//   k_albedo      the accumulator: per pixel the SUM of the first-hit albedo of every committed iteration's own camera ray, and their count
//   k_demodulate  between the filter's front and level 0: (c, v) -> (c / A', v rho^2) with A' the pixel's mean albedo
// Why the mean over the committed iterations and not one iteration's albedo ("Demodulation"): the other samples of a pixel on a texel
// border hit other texels, so c / A_one is an outlier of up to the texture's contrast, while c / mean(A) = sum A_i e_i / sum A_i is an
// albedo-weighted mean of the irradiance samples e_i.
//
// ---- operation by operation (tests/demod_ref.py restates it in numpy, bit for bit: every fp32 operation below is one IEEE operation,
// -ffp-contract=off, in the order written) ----
//   A_i         of iteration i at a pixel: the camera ray is cameraRayAt(prm, iterationHash(i, 0), ..) -- the jitter and lens sample the renderer
//               traces --, its nearest hit k_gbuffer's (every primitive in index order, the renderer's exact tests, t > 0, smallest t, an equal t
//               keeps the lower index).
//                 a miss                                                               (1, 1, 1)
//                 a hit whose material emits, reflects or refracts (emittance > 0,
//                 hasReflective > 0 or hasRefractive > 0; a mesh face's own material
//                 where it has one, else the object's)                                 (1, 1, 1)
//                 otherwise   the mcol k_bounce forms there: the material's colour, times textureSample at the hit's texture coordinates
//                             where a texture is bound (sphereUV of the object-space hit point, cubeUV of inverseTransform * (P, 1) and the hit
//                             face, meshUV of the winning triangle's corner UVs and barycentrics): colour.k * texel.k, one multiplication
//   accumulate  iterations in ascending order:  Asum.k = Asum.k + A_i.k;  Asum.w = Asum.w + 1  -- so a batch equals its single calls to the bit
//   A'          n = (float)samples, eps = PT_DEMOD_MIN_ALBEDO:  a.k = Asum.k / n;  A'.k = a.k > eps ? a.k : eps  (a NaN gives eps)
//   demodulate  c'.k = c.k / A'.k;  L = lum(c);  L' = lum(c');  rho = L > 0 ? L' / L : 1;  v' = v * (rho * rho)
//               -- the relative standard error of the luminance is kept; (c, v) is meanAndVariance of the accumulators, or the image
//               k_spatial_variance_* left (one sample under PT_FLAG_SPATIAL_VARIANCE), which is then rewritten in place
//   remodulate  AtrousDemod::store (pt_denoise.h), with (co, vo) the last level's filtered colour and variance and A' formed again from the sums:
//               out.k = co.k * A'.k;  rho' = lum(co) > 0 ? lum(out) / lum(co) : 1;  var = vo * (rho' * rho')
#pragma once
#include "pt_denoise.h"

namespace ptk {

struct AlbedoArgs {
    KParams prm;
    const GeomDev *ggeoms;
    const MaterialDev *gmats;
    const float4 *meshRecs;
    const TexGeom *texGeom;         // NULL: no texture is bound in this scene
    const int4 *texDesc;
    const float4 *texels, *texUV;
    int firstIter, count;           // iterations firstIter .. firstIter + count - 1
    float4 *asum;                   // (sum of A_i, number of iterations added)
};

// One thread per pixel of the full frame (blocks of kBlock; dynamic LDS = the lanes' mesh traversal stacks, as k_gbuffer has them), which
// loops over the batch's iterations.  The primitive index is wave-uniform: its record arrives through the scalar path, the tests' matrix
// operands are SGPRs.  What a winner needs beyond t -- the hit point, the object-space vector, the face's material, the triangle and its
// barycentrics -- stays in registers until the loop over the primitives ends; the material and the texel are read once per iteration, for the
// winner alone, through the vector path.
__global__ __launch_bounds__(kBlock) void k_albedo(AlbedoArgs A) {
    extern __shared__ uint32_t s_albedoStack[];
    const int npix = A.prm.W * A.prm.H;
    const int pix = blockIdx.x * kBlock + threadIdx.x;
    const int pc = pix < npix ? pix : npix - 1;       // (lanes beyond the frame trace its last pixel and store nothing)
    const int y = (int)fastDiv((uint32_t)pc, A.prm.magicW, A.prm.shiftW);
    const int x = pc - y * A.prm.W;
    const GeomPtr geoms = (GeomPtr)A.ggeoms;
    float4 sum = A.asum[pc];
    for (int it = A.firstIter; it < A.firstIter + A.count; ++it) {
        F3 org, dir;
        cameraRayAt(A.prm, iterationHash(it, 0), pc, x, y, org, dir);
        int hit = -1, faceMat = 0;
        float tMin = 0.0f;
        F3 P = f3(0.0f, 0.0f, 0.0f), nsrc = f3(0.0f, 0.0f, 0.0f);
        uint32_t unit = 0u;
        float2 bary = make_float2(0.0f, 0.0f);
        for (int g = 0; g < A.prm.ngeoms; ++g) {
            const PT_CAS GeomDev &G = *(launder(geoms) + g);
            F3 tp = f3(0.0f, 0.0f, 0.0f), tn = f3(0.0f, 0.0f, 0.0f);
            bool to = false;
            int fm = 0;
            uint32_t tu = 0u;
            float2 tb = make_float2(0.0f, 0.0f);
            float t;
            if ((G.flags & 32) != 0)
                t = meshIntersectionTest<false, kBlock>(G, A.meshRecs, G.meshRoot, G.meshStride, s_albedoStack + threadIdx.x, org, dir, tp, tn, to, fm, tu, tb);
            else if ((G.flags & 1) == 0) t = sphereIntersectionTest(G, org, dir, tp, tn, to);
            else t = boxIntersectionTest<false>(G, org, dir, tp, tn, to);
            if (t > 0.0f && (hit < 0 || t < tMin)) {
                tMin = t;
                hit = g;
                P = tp;
                nsrc = tn;
                faceMat = fm;
                unit = tu;
                bary = tb;
            }
        }
        F3 a = f3(1.0f, 1.0f, 1.0f);
        if (hit >= 0) {
            const GeomDev &W = A.ggeoms[hit];          // (per lane: the winner's record through the vector path)
            const MaterialDev &M = A.gmats[faceMat != 0 ? faceMat - 1 : W.material];
            if (!(M.emittance > 0.0f || M.hasReflective > 0.0f || M.hasRefractive > 0.0f)) {
                a = f3(M.color[0], M.color[1], M.color[2]);
                if (A.texGeom) {
                    const int4 tg = *reinterpret_cast<const int4 *>(A.texGeom + hit);     // TexGeom {tex, kind, uvBase, triBase}
                    if (tg.x >= 0) {
                        float u, v;
                        if (tg.y == 2) {
                            const size_t row = (size_t)tg.z + (unit - (uint32_t)tg.w) / (uint32_t)kMeshTriUnits;
                            const float4 c01 = A.texUV[2 * row], c2 = A.texUV[2 * row + 1];
                            meshUV(c01, make_float2(c2.x, c2.y), bary.x, bary.y, u, v);
                        } else if (tg.y == 1) {
                            bool faceOk = true;
                            const int face = cubeFace(nsrc, faceOk);
                            cubeUV(mulMV(W.inv, P, 1.0f), faceOk ? face : 0, u, v);
                        } else {
                            sphereUV(nsrc, u, v);
                        }
                        const int4 td = A.texDesc[tg.x];                                  // {first texel, W, H, 0}
                        a = a * textureSample(A.texels, td.x, td.y, td.z, u, v);
                    }
                }
            }
        }
        sum.x = sum.x + a.x;
        sum.y = sum.y + a.y;
        sum.z = sum.z + a.z;
        sum.w = sum.w + 1.0f;
    }
    if (pix < npix) A.asum[pix] = sum;
}

// the pixel's mean albedo, floored: A' of the header (k_demodulate, and AtrousDemod::store once more: same expression, same bits)
__device__ __forceinline__ F3 demodAlbedo(const float4 *asum, size_t pix, float n, float eps) {
    const float4 s = asum[pix];
    const float ax = s.x / n, ay = s.y / n, az = s.z / n;
    return f3(ax > eps ? ax : eps, ay > eps ? ay : eps, az > eps ? az : eps);
}

struct DemodArgs {
    const float *accum, *moments;   // !INPLACE: the accumulators
    float4 *img;                    // level 0's input, (r, g, b, variance): written; INPLACE: read first
    const float4 *asum;
    int npix;
    float samples, samplesM1, eps;
};

template <bool INPLACE>
__global__ __launch_bounds__(kBlock) void k_demodulate(DemodArgs A) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= A.npix) return;
    const float4 c = INPLACE ? A.img[i] : meanAndVariance(A.accum, A.moments, (size_t)i, A.samples, A.samplesM1);
    const F3 al = demodAlbedo(A.asum, (size_t)i, A.samples, A.eps);
    const float r = c.x / al.x, g = c.y / al.y, b = c.z / al.z;
    const float L = atrousLum(c.x, c.y, c.z);
    const float Ld = atrousLum(r, g, b);
    const float rho = L > 0.0f ? Ld / L : 1.0f;
    A.img[i] = make_float4(r, g, b, c.w * (rho * rho));
}

// ---- the third filter description: AtrousGuided whose last level multiplies the pixel's mean albedo back ------------------------------------
struct AtrousDemodArgs : AtrousVarArgs {
    const float4 *asum;             // LAST: the albedo sums ...
    float demodN, demodEps;         // ... (float)samples and PT_DEMOD_MIN_ALBEDO
};

struct AtrousDemod : AtrousGuided {
    using Args = AtrousDemodArgs;
    template <bool LAST, bool BYTES>
    static __device__ __forceinline__ void store(const Args &A, size_t pix, float4 o) {
        static_assert(LAST, "the levels below the last are AtrousGuided's");
        const F3 al = demodAlbedo(A.asum, pix, A.demodN, A.demodEps);
        const float r = o.x * al.x, g = o.y * al.y, b = o.z * al.z;
        if (BYTES) {
            uchar4 q;
            q.w = 0; q.x = atrousByte(r); q.y = atrousByte(g); q.z = atrousByte(b);
            A.out8[pix] = q;
        } else {
            float *d = A.out3 + 3 * pix;
            d[0] = r; d[1] = g; d[2] = b;
            if (A.outVar) {
                const float Lc = atrousLum(o.x, o.y, o.z);
                const float rho = Lc > 0.0f ? atrousLum(r, g, b) / Lc : 1.0f;
                A.outVar[pix] = o.w * (rho * rho);
            }
        }
    }
};

}  // namespace ptk
