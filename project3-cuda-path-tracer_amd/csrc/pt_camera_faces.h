// pt_camera_faces.h -- THE FACE CERTIFICATE of a camera pixel (pt_host_scene.h: "THE FACE CERTIFICATE", where the argument is written out),
// as one body for the host and the device, and k_camera_faces, which evaluates it for the pixels of one one-cube signature group.
// Header-only part of the single translation unit pt_api.hip (namespace ptk).
//
// pt_init evaluates the certificate on the host (build_camera_list); the camera move (pt_api.hip), which moves the camera of a live renderer, evaluates it
// here: per-pixel float64 arithmetic with no dependence between pixels.  The two must agree on EVERY pixel -- the split of the work list by
// face is part of what the frames are compared on, bit for bit -- so there is one definition: face_certificate below, compiled for both
// sides with -ffp-contract=off (no fused multiply-add on either), IEEE double division and square root (correctly rounded on gfx950 without
// fast-math: the division is the div_scale / div_fmas / div_fixup sequence, the root v_sqrt_f64 with its correction step).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace ptk {

// what the certificate reads of a cube (CubeCert, pt_host_scene.h) ...
struct FaceCube {
    double o[3], L[3][3], inset[3];     // the object-space eye, inverseTransform's linear part, the per-axis insets
    double clear = 0;                   // the least s o_K - 1/2 - inset_K: (ii)'s room and (i)'s distance
};
// ... and of the camera (CameraResolve): view, right * pixLenX, up * pixLenY
struct FaceBasis {
    double view[3], rx[3], uy[3];
    double halfW = 0, halfH = 0;
};
constexpr double kFaceFootprint = 2.0, kFaceRho = 1.0 / 4096, kFaceClear = 1e-2, kFaceInsetAbs = 1e-4, kFaceInsetD = 8.0, kFaceMinSlope = 1e-3;

__host__ __device__ inline bool faceFinite(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }      // (NaN fails)

// the face (2 K + (s > 0)) pixel (x, y) is resolved to on the cube, or -1.  Every loop has a constant bound, so the device form unrolls
// them all: q stays in registers, and an axis or a corner that fails early is a lane's branch around the rest.
__host__ __device__ inline int face_certificate(const FaceCube &c, const FaceBasis &b, int x, int y) {
    // the four corner directions of the footprint, object space
    double q[4][3], qn[4];
#pragma unroll
    for (int corner = 0; corner < 4; ++corner) {
        const double cx = (corner & 1) ? (double)x + 1.0 + kFaceFootprint : (double)x - kFaceFootprint;
        const double cy = (corner & 2) ? (double)y + 1.0 + kFaceFootprint : (double)y - kFaceFootprint;
        const double sx = cx - b.halfW, sy = cy - b.halfH;
        double d[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) d[a] = b.view[a] - b.rx[a] * sx - b.uy[a] * sy;
#pragma unroll
        for (int r = 0; r < 3; ++r) q[corner][r] = c.L[r][0] * d[0] + c.L[r][1] * d[1] + c.L[r][2] * d[2];
        qn[corner] = __builtin_sqrt(q[corner][0] * q[corner][0] + q[corner][1] * q[corner][1] + q[corner][2] * q[corner][2]);
        if (!faceFinite(qn[corner]) || !(qn[corner] > 0)) return -1;
    }
#pragma unroll
    for (int K = 0; K < 3; ++K) {
        const double s = c.o[K] > 0 ? 1.0 : -1.0;
        if (!(s * c.o[K] >= 0.5 + c.clear + c.inset[K])) continue;           // (ii), and (i)'s distance
        const double a = 0.5 * s - c.o[K];                                  // (sign -s)
        bool ok = true;
#pragma unroll
        for (int corner = 0; corner < 4; ++corner) {
            if (!ok) break;
            const double qK = q[corner][K];
            ok = s * qK < 0 && __builtin_fabs(qK) >= kFaceMinSlope * qn[corner];
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                if (!ok) break;
                const double lam = a * (side ? 1.0 + kFaceRho : 1.0 - kFaceRho) / qK;
                ok = faceFinite(lam) && lam > 0;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    if (j == K || !ok) continue;
                    const double pj = c.o[j] + lam * q[corner][j];
                    ok = __builtin_fabs(pj) <= 0.5 - c.inset[j];             // (NaN fails)
                }
            }
        }
        if (ok) return 2 * K + (s > 0 ? 1 : 0);
    }
    return -1;
}

// One launch per one-cube signature group: lane i takes pixel pix[i] (x | y << 16) and writes its face, -1 .. 5, as one signed byte.
// The cube and the basis are kernel arguments -- uniform, so their 27 doubles come through scalar loads of the kernarg segment and cost no
// vector register; 256-thread workgroups, no LDS, no scratch (profiles/set_camera_resource_usage.txt).
struct CameraFacesArgs {
    FaceCube cube;
    FaceBasis basis;
    const uint32_t *pix;
    signed char *face;
    int n;
};
__global__ void __launch_bounds__(256) k_camera_faces(const CameraFacesArgs A) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= A.n) return;
    const uint32_t w = A.pix[i];
    A.face[i] = (signed char)face_certificate(A.cube, A.basis, (int)(w & 0xffffu), (int)(w >> 16));
}

}  // namespace ptk
