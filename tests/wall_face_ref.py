"""The later bounces' wall-face certificate (csrc/pt_device.h: wallFaceCertificate) and the reference's slab loop (src/intersections.h:51-77),
restated in numpy float32, with the scenes and the ray families tests/test_wall_face_cpu.py sweeps them on.

Every array operation below is ONE float32 operation per element, in the order the device code and the reference write them; the fused
multiply-adds of the certificate's four crossing points go through float64 (the product of two float32 is exact there).  The certificate's
v_rcp_f32 is the correctly rounded reciprocal here: the two differ by an ulp, against margins of 2^-12 and 2^-16."""
import os
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

RHO = f32(2.0 ** -12)          # kWallFaceRho
INSET = f32(2.0 ** -16)        # kWallFaceInset
OTHER_MAX = f32(8.0)           # kWallFaceOtherMax
ORIGIN_MAX = f32(2.0 ** 19)    # kWallFaceOriginMax
MIN_SHARE = f32(2.0 ** -39)    # kWallFaceMinShare

# Cornell's walls (objects 1 .. 5 of scenes/cornell.txt) and, one scene each, a wall of the same place and size turned by 90 degrees about
# x, y and z: (object, its replacement lines ROTAT / SCALE)
ROTATED = [(4, "ROTAT 90 0 0", "SCALE .01 10 10"), (1, "ROTAT 0 90 0", "SCALE 10 .01 10"), (3, "ROTAT 0 0 90", "SCALE 10 10 .01")]


def rotated_scene_text(obj, rotat, scale):
    """scenes/cornell.txt with object `obj`'s ROTAT and SCALE lines replaced."""
    lines = open(os.path.join(ROOT, "scenes", "cornell.txt")).read().split("\n")
    at = lines.index("OBJECT %d" % obj)
    for k in range(at, at + 8):
        if lines[k].startswith("ROTAT"):
            lines[k] = rotat
        elif lines[k].startswith("SCALE"):
            lines[k] = scale
    return "\n".join(lines)


def load_scenes(pt):
    """[(name, Scene, wall objects to sweep)]: Cornell with its five walls, then the three scenes with one turned wall each."""
    out = [("cornell", pt.Scene(os.path.join(ROOT, "scenes", "cornell.txt")), [1, 2, 3, 4, 5])]
    for obj, rotat, scale in ROTATED:
        with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as fh:
            fh.write(rotated_scene_text(obj, rotat, scale))
        try:
            out.append(("cornell, object %d %s" % (obj, rotat), pt.Scene(fh.name), [obj]))
        finally:
            os.unlink(fh.name)
    return out


def matrices(geom):
    """(inverseTransform, transform) of a PtGeom as float32 4x4 arrays M[row, column] (the file is column-major)."""
    return (np.asarray(geom["inverseTransform"], f32).reshape(4, 4).T.copy(), np.asarray(geom["transform"], f32).reshape(4, 4).T.copy())


def to_object_space(inv, org, dirs):
    """qo = mulMV(inv, org, 1), qdu = mulMV0(inv, inv[:, 3] * 0, dir): ptd's sums, (a + b) + (c + d)."""
    org, dirs = np.asarray(org, f32), np.asarray(dirs, f32)
    with np.errstate(all="ignore"):
        qo = np.stack([(inv[r, 0] * org[:, 0] + inv[r, 1] * org[:, 1]) + (inv[r, 2] * org[:, 2] + inv[r, 3] * f32(1)) for r in range(3)], axis=1)
        qdu = np.stack([(inv[r, 0] * dirs[:, 0] + inv[r, 1] * dirs[:, 1]) + (inv[r, 2] * dirs[:, 2] + inv[r, 3] * f32(0)) for r in range(3)], axis=1)
    assert qo.dtype == f32 and qdu.dtype == f32
    return qo, qdu


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def certificate(qo, qdu, face, beyond):
    """wallFaceCertificate(qo, qdu, face, beyond), per ray."""
    K, s = face >> 1, f32(1.0 if face & 1 else -1.0)
    I, J = [a for a in range(3) if a != K]
    beyond = f32(beyond)
    with np.errstate(all="ignore"):
        u = qdu
        x = (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]
        ok = (x.view(np.uint32) - np.uint32(0x17800000)) < np.uint32(0x50000000)          # 2^-80 <= x < 2^80 (wraps like the device's)
        au = np.abs(u)
        ok &= np.minimum(np.minimum(au[:, 0], au[:, 1]), au[:, 2]) >= MIN_SHARE * ((au[:, 0] + au[:, 1]) + au[:, 2])
        ok &= np.abs(qo[:, I]) + np.abs(qo[:, J]) <= OTHER_MAX
        ok &= np.abs(qo[:, K]) <= ORIGIN_MAX
        ok &= s * qo[:, K] >= beyond
        ok &= s * u[:, K] < 0
        a = f32(0.5) * s - qo[:, K]
        t = a * (f32(1) / u[:, K])
        tm, tp = t * (f32(1) - RHO), t * (f32(1) + RHO)
        m = np.zeros(len(qo), f32)
        bad = np.zeros(len(qo), bool)
        for ax in (I, J):
            for tt in (tm, tp):
                p = np.abs(_fma(tt, u[:, ax], qo[:, ax]))
                bad |= ~(p <= f32(0.5) - INSET)                                            # (NaN fails)
        ok &= ~bad
    return ok


def slab_loop(qo, qdu):
    """src/intersections.h:51-77 on object-space rays: (hit, outside, face = 2 axis + (n > 0) or -1, tmin)."""
    n = len(qo)
    with np.errstate(all="ignore"):
        x = (qdu[:, 0] * qdu[:, 0] + qdu[:, 1] * qdu[:, 1]) + qdu[:, 2] * qdu[:, 2]
        qd = qdu * (f32(1) / np.sqrt(x))[:, None]
        tmin, tmax = np.full(n, -1e38, f32), np.full(n, 1e38, f32)
        fmin, fmax = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
        for xyz in range(3):
            t1 = (f32(-0.5) - qo[:, xyz]) / qd[:, xyz]
            t2 = (f32(0.5) - qo[:, xyz]) / qd[:, xyz]
            ta = np.where(t2 < t1, t2, t1)                 # glm::min(t1, t2) = (t2 < t1) ? t2 : t1
            tb = np.where(t1 < t2, t2, t1)                 # glm::max(t1, t2) = (t1 < t2) ? t2 : t1
            nf = (2 * xyz + (t2 < t1)).astype(np.int32)
            up = (ta > 0) & (ta > tmin)
            tmin, fmin = np.where(up, ta, tmin), np.where(up, nf, fmin)
            up = tb < tmax
            tmax, fmax = np.where(up, tb, tmax), np.where(up, nf, fmax)
        hit = (tmax >= tmin) & (tmax > 0)
        inside = tmin <= 0
        return hit, hit & ~inside, np.where(inside, fmax, fmin), np.where(inside, tmax, tmin)


def room_box(geoms, walls):
    """The room in world space, float64: per axis the innermost planes of the walls' boxes that lie on either side of the room's middle."""
    lo, hi = np.full(3, -np.inf), np.full(3, np.inf)
    boxes = []
    for g in walls:
        _, xf = matrices(geoms[g])
        c = np.array([[sx, sy, sz, 1.0] for sx in (-.5, .5) for sy in (-.5, .5) for sz in (-.5, .5)]) @ xf.astype(np.float64).T
        boxes.append((c[:, :3].min(axis=0), c[:, :3].max(axis=0)))
    allLo, allHi = np.min([b[0] for b in boxes], axis=0), np.max([b[1] for b in boxes], axis=0)
    mid = 0.5 * (allLo + allHi)
    for blo, bhi in boxes:
        for a in range(3):
            if bhi[a] < mid[a]:
                lo[a] = max(lo[a], bhi[a])
            if blo[a] > mid[a]:
                hi[a] = min(hi[a], blo[a])
    lo = np.where(np.isfinite(lo), lo, allLo)
    hi = np.where(np.isfinite(hi), hi, allHi)
    return lo, hi


def rays_for_wall(geom, face, room, n, seed):
    """n seeded world-space rays (float32 origins, directions) aimed at face `face` of cube `geom` from the room `room` = (lo, hi).
    Origins: uniform in the room shrunk by 1e-3 on every side -- a scattered ray starts 1e-3 off the surface it leaves --, a third of them ON
    the shrunk room's border: 1e-3 off a neighbouring wall's inner face (or this wall's own).
    Directions, by family: at a uniform point of the face widened by 5 % (hits, near misses); at a point within 1e-3 .. 1e-7 of one of its
    edges; of a corner; grazing, the component along the face's normal scaled down to 2^-45 of the others; uniform on the sphere; and a few
    with NaN, inf and exact-zero components."""
    rng = np.random.default_rng(seed)
    lo, hi = room[0] + 1e-3, room[1] - 1e-3
    org = lo + rng.random((n, 3)) * (hi - lo)
    snap = rng.random(n) < 1.0 / 3.0
    ax = rng.integers(0, 3, n)
    side = rng.random(n) < 0.5
    rows = np.nonzero(snap)[0]
    org[rows, ax[rows]] = np.where(side[rows], hi[ax[rows]], lo[ax[rows]])
    org = org.astype(f32)
    inv, xf = matrices(geom)
    xf64 = xf.astype(np.float64)
    K, s = face >> 1, (1.0 if face & 1 else -1.0)
    I, J = [a for a in range(3) if a != K]
    fam = rng.integers(0, 16, n)
    q = np.zeros((n, 3))
    q[:, K] = 0.5 * s
    a, b = rng.random(n) * 1.05 - 0.525, rng.random(n) * 1.05 - 0.525
    eps = 10.0 ** -(3 + 4 * rng.random(n)) * np.where(rng.random(n) < 0.5, 1.0, -1.0)
    sa, sb = np.where(rng.random(n) < 0.5, 0.5, -0.5), np.where(rng.random(n) < 0.5, 0.5, -0.5)
    edge = (fam >= 6) & (fam < 10)
    corner = (fam >= 10) & (fam < 12)
    a = np.where(edge | corner, sa * (1.0 + eps), a)
    b = np.where(corner, sb * (1.0 + eps * rng.random(n)), b)
    swap = edge & (rng.random(n) < 0.5)
    a, b = np.where(swap, b, a), np.where(swap, a, b)
    q[:, I], q[:, J] = a, b
    target = q @ xf64[:3, :3].T + xf64[:3, 3]
    d = target - org.astype(np.float64)
    graze = fam == 12
    if graze.any():
        # object-space direction with the normal component scaled down, back to world space
        L = inv.astype(np.float64)[:3, :3]
        qd = d[graze] @ L.T
        qd[:, K] = -s * np.abs(qd[:, K]) * 2.0 ** -(45.0 * rng.random(int(graze.sum())))
        d[graze] = qd @ xf64[:3, :3].T
    uni = fam == 13
    d[uni] = rng.normal(size=(int(uni.sum()), 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    d = d.astype(f32)
    odd = np.nonzero(fam >= 14)[0]                           # NaN / inf / exact zeros, in a direction or an origin
    kind = rng.integers(0, 5, len(odd))
    comp = rng.integers(0, 3, len(odd))
    d[odd[kind == 0], comp[kind == 0]] = np.nan
    d[odd[kind == 1], comp[kind == 1]] = np.inf
    d[odd[kind == 2], comp[kind == 2]] = 0.0
    org[odd[kind == 3], comp[kind == 3]] = np.nan
    d[odd[kind == 4]] = 0.0
    special = np.zeros(n, bool)
    special[odd] = True
    return org, d, special


def hit_inside_shrunk_face(geom, face, org, dirs, shrink=0.01):
    """float64: the ray starts beyond the face's plane, moves towards it and crosses it at a point whose two other object-space coordinates lie inside
    the face shrunk by `shrink` of its side on every edge."""
    inv, _ = matrices(geom)
    M = inv.astype(np.float64)
    K, s = face >> 1, (1.0 if face & 1 else -1.0)
    I, J = [a for a in range(3) if a != K]
    with np.errstate(all="ignore"):
        o = org.astype(np.float64) @ M[:3, :3].T + M[:3, 3]
        u = dirs.astype(np.float64) @ M[:3, :3].T
        t = (0.5 * s - o[:, K]) / u[:, K]
        pi, pj = o[:, I] + t * u[:, I], o[:, J] + t * u[:, J]
        return (s * o[:, K] > 0.5) & (s * u[:, K] < 0) & (t > 0) & (np.abs(pi) <= 0.5 - shrink) & (np.abs(pj) <= 0.5 - shrink)
