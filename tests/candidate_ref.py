"""The scatter's two candidacy certificates for a binned primitive (k_bounce, class bit 3; KParams::binCull / binBox), restated in numpy
float32 for the tests -- operation for operation as csrc/pt_device.h writes them (certainMiss, certainMissClamped, wallCertainMissByAxis)
and as the host prepares their constants (pt_host_scene.h: pack_geom's bounding ball, wall_box).  A fused multiply-add is evaluated in
float64 and rounded once; v_rcp_f32 is taken as the correctly rounded quotient (it is within one ulp of it)."""
import numpy as np

F = np.float32


def _fma(a, b, c):
    return F(np.float64(a) * np.float64(b) + np.float64(c))


def ball_of(g):
    """(centre[3], cullR2, cullK) of a sphere or a cube, as pack_geom computes them (float32); cullR2 = inf: never culled"""
    m = np.asarray(g["transform"], np.float64).reshape(-1)
    mi = np.asarray(g["inverseTransform"], np.float64).reshape(-1)
    A = np.array([[m[c * 4 + r] for r in range(3)] for c in range(3)])          # A[c] = column c
    Ai = np.array([[mi[c * 4 + r] for r in range(3)] for c in range(3)])
    ln = np.sqrt((A * A).sum(1))
    orth = all(abs(A[a] @ A[b]) <= 1e-5 * ln[a] * ln[b] for a in range(3) for b in range(a + 1, 3))
    if orth:
        smax, smin = ln.max() * (1 + 1e-5), ln.min() * (1 - 1e-5)
    else:
        smax = np.sqrt((A * A).sum())
        froi = (Ai * Ai).sum()
        smin = 1.0 / np.sqrt(froi) if froi > 0 else 0.0
    rho2 = 0.25 if int(np.asarray(g["type"]).reshape(-1)[0]) == 0 else 0.75
    r2 = rho2 * smax * smax * (1 + 1e-3)
    kk = 1e-4 * (smax / smin) ** 2 if smin > 0 else np.inf
    ok = np.isfinite(r2) and np.isfinite(kk) and kk < 0.5 and smin > 0
    centre = np.array([m[12], m[13], m[14]], F)
    return centre, (F(r2) if ok else F(np.inf)), (F(kk) if ok else F(0))


def wall_box(g):
    """(lo[3], hi[3], omax) of a cube: wall_box's inflated world box, rounded outwards, and the bound on |x| + |y| + |z| of the ray origins
    its certificate is issued for, as the plan stores it (rounded towards zero)"""
    m = np.asarray(g["transform"], np.float64).reshape(-1)
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for corner in range(8):
        o = [0.5 if corner & 1 else -0.5, 0.5 if corner & 2 else -0.5, 0.5 if corner & 4 else -0.5]
        q = np.array([m[0 + r] * o[0] + m[4 + r] * o[1] + m[8 + r] * o[2] + m[12 + r] for r in range(3)])
        lo, hi = np.minimum(lo, q), np.maximum(hi, q)
    big = max(np.abs(lo).max(), np.abs(hi).max())
    S = max(np.sqrt(((hi - lo) ** 2).sum()), big)
    delta = 4e-5 * S
    lo32 = np.nextafter((lo - delta).astype(F), F(-np.inf))
    hi32 = np.nextafter((hi + delta).astype(F), F(np.inf))
    return lo32, hi32, np.nextafter(F(5.0 * S - big), F(0))


def ball_miss(ball, org, d, half_line):
    """certainMissClamped(g, org, dir, dot(dir, dir), halfLine); half_line = False is certainMiss, the parent's rule"""
    centre, r2, kk = ball
    with np.errstate(all="ignore"):
        org, d = np.asarray(org, F), np.asarray(d, F)
        dd = F(F(F(d[0] * d[0]) + F(d[1] * d[1])) + F(d[2] * d[2]))               # dot(): (x x + y y) + z z
        oc = (org - centre).astype(F)
        oo = _fma(oc[2], oc[2], _fma(oc[1], oc[1], F(oc[0] * oc[0])))
        od = _fma(oc[2], d[2], _fma(oc[1], d[1], F(oc[0] * d[0])))
        if half_line:
            od = F(0) if np.isnan(od) else min(od, F(0))                           # (v_min_f32 keeps the operand that is not NaN)
        return bool(_fma(oo, dd, -F(od * od)) > F(_fma(kk, oo, r2) * dd))


def box_miss(box, org, d):
    """the slab certificate under its guard: l1(org) <= omax and wallCertainMissByAxis(box, org, dir)"""
    lo, hi, omax = box
    with np.errstate(all="ignore"):
        org, d = np.asarray(org, F), np.asarray(d, F)
        l1 = F(F(abs(org[0]) + abs(org[1])) + abs(org[2]))
        tmin, tmax = F(-np.inf), F(np.inf)
        for a in range(3):
            inv = F(1) / d[a]
            t1, t2 = F(F(lo[a] - org[a]) * inv), F(F(hi[a] - org[a]) * inv)
            tmin = np.fmax(tmin, np.fmin(t1, t2))                                  # (fmax / fmin drop a NaN, as v_max_f32 / v_min_f32 do)
            tmax = np.fmin(tmax, np.fmax(t1, t2))
        slab = bool(F(tmin - tmax) > F(F(1e-5) * F(abs(tmin) + abs(tmax)))) or bool(tmax < 0)
        return slab and bool(l1 <= omax)


def certified(g, org, d, tight=True):
    """Does the scatter certify that the ray misses binned primitive g?  tight = False: the bounding ball alone, the parent's rule."""
    sphere = int(np.asarray(g["type"]).reshape(-1)[0]) == 0
    ball = ball_of(g)
    if not tight:
        return ball_miss(ball, org, d, False)
    if sphere:
        return ball_miss(ball, org, d, True)
    return ball_miss(ball, org, d, False) or box_miss(wall_box(g), org, d)
