"""numpy float32 restatement of the kernels' bump mapping (csrc/pt_device.h, "bump mapping"), operation for operation: the project compiles
with -ffp-contract=off and correctly rounded division and square root, so these match the device bit for bit.  Vectors are (n, 3) arrays."""
import numpy as np

import texture_ref as tr

F = np.float32
PI = tr.PI
HALF_PI = tr.HALF_PI


def _f(a):
    return np.asarray(a, np.float32)


def dot(a, b):
    t = a * b
    return (t[:, 0] + t[:, 1]) + t[:, 2]


def cross(x, y):
    return np.stack([x[:, 1] * y[:, 2] - y[:, 1] * x[:, 2], x[:, 2] * y[:, 0] - y[:, 2] * x[:, 0], x[:, 0] * y[:, 1] - y[:, 0] * x[:, 1]], 1)


def normalize(a):
    with np.errstate(all="ignore"):
        return a * (F(1) / np.sqrt(dot(a, a)))[:, None]


def gradient(height, s, uv):
    """(hu, hv) of a height map (H, W) float32 (row 0 = top) with scale s (n,) at uv (n, 2)"""
    height = _f(height)
    Hh, Ww = height.shape
    tex = np.repeat(height[:, :, None], 3, 2)
    uv = _f(uv).reshape(-1, 2)
    fw, fh = F(Ww), F(Hh)
    du, dv = F(1) / fw, F(1) / fh
    u, v = uv[:, 0], uv[:, 1]
    h = lambda a, b: tr.sample(tex, np.stack([a, b], 1))[:, 0]
    hr, hl, ht, hb = h(u + du, v), h(u - du, v), h(u, v + dv), h(u, v - dv)
    s = _f(s)
    return (s * (hr - hl)) * (fw * F(0.5)), (s * (ht - hb)) * (fh * F(0.5))


def mul_l(xf, t):
    """the linear part of column-major transforms xf (n, 12) times t (n, 3)"""
    m = _f(xf).reshape(-1, 12)
    return np.stack([(m[:, 0] * t[:, 0] + m[:, 3] * t[:, 1]) + m[:, 6] * t[:, 2], (m[:, 1] * t[:, 0] + m[:, 4] * t[:, 1]) + m[:, 7] * t[:, 2],
                     (m[:, 2] * t[:, 0] + m[:, 5] * t[:, 1]) + m[:, 8] * t[:, 2]], 1)


def sphere_tangents(q):
    """(Tu, Tv, ok) at object-space sphere hits q; ok = False at the poles"""
    d = normalize(_f(q).reshape(-1, 3))
    with np.errstate(all="ignore"):
        rho = np.sqrt(d[:, 0] * d[:, 0] + d[:, 2] * d[:, 2])
        tu = np.stack([PI * -d[:, 2], np.zeros(len(d), np.float32), PI * d[:, 0]], 1)
        tv = np.stack([HALF_PI * ((-d[:, 1] * d[:, 0]) / rho), HALF_PI * rho, HALF_PI * ((-d[:, 1] * d[:, 2]) / rho)], 1)
    return tu, tv, rho != F(0)


def cube_tangents(xf, face):
    """(Pu, Pv): columns (a + 1) % 3 and (a + 2) % 3 of each transform, a = face >> 1"""
    m = _f(xf).reshape(-1, 12)
    a = np.asarray(face, np.int64) >> 1
    i = np.arange(len(m))[:, None]
    cu, cv = (a + 1) % 3, (a + 2) % 3
    return m[i, 3 * cu[:, None] + np.arange(3)], m[i, 3 * cv[:, None] + np.arange(3)]


def mesh_tangents(tri, uv):
    """(Tu, Tv, ok) of triangles tri (n, 9) object-space corners with corner UVs uv (n, 6); ok = det != 0"""
    tri, uv = _f(tri).reshape(-1, 9), _f(uv).reshape(-1, 6)
    e1, e2 = tri[:, 3:6] - tri[:, 0:3], tri[:, 6:9] - tri[:, 0:3]
    du1, dv1, du2, dv2 = uv[:, 2] - uv[:, 0], uv[:, 3] - uv[:, 1], uv[:, 4] - uv[:, 0], uv[:, 5] - uv[:, 1]
    det = du1 * dv2 - du2 * dv1
    with np.errstate(all="ignore"):
        tu = (e1 * dv2[:, None] - e2 * dv1[:, None]) / det[:, None]
        tv = (e2 * du1[:, None] - e1 * du2[:, None]) / det[:, None]
    return tu, tv, det != F(0)


def bump_normal(N, Pu, Pv, hu, hv, outside, d):
    """(Ns, bumped): the shading normal, N itself where the hit stays unbumped"""
    N, Pu, Pv, d = (_f(x).reshape(-1, 3) for x in (N, Pu, Pv, d))
    hu, hv = _f(hu), _f(hv)
    outside = np.asarray(outside, bool)
    with np.errstate(all="ignore"):
        J = dot(N, cross(Pu, Pv))
        a = cross(Pv, N) * hu[:, None] + cross(N, Pu) * hv[:, None]
        g = a / J[:, None]
        n = normalize(np.where(outside[:, None], N - g, N + g))
        ok = ~((hu == 0) & (hv == 0)) & (J != 0) & np.isfinite(g).all(1) & np.isfinite(n).all(1) & (dot(n, d) < 0)
    return np.where(ok[:, None], n, N).astype(np.float32), ok


def evaluate(height, kind, inp):
    """what pt_test_bump_normal returns: kind (n,), inp (n, 40) -> (n, 16) {hu, hv, Pu, Pv, Ns, bumped, u, v, 0, 0}"""
    kind = np.asarray(kind).reshape(-1)
    e = _f(inp).reshape(len(kind), 40)
    n = len(kind)
    xf = e[:, 8:20]
    uv = np.zeros((n, 2), np.float32)
    Pu, Pv = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    tok = np.ones(n, bool)
    for k in (0, 1, 2):
        m = kind == k
        if not m.any():
            continue
        if k == 2:
            uv[m] = tr.mesh_uv(np.c_[e[m, 20:22], e[m, 22:28]])
            tu, tv, ok = mesh_tangents(e[m, 28:37], e[m, 22:28])
            Pu[m], Pv[m], tok[m] = mul_l(xf[m], tu), mul_l(xf[m], tv), ok
        elif k == 1:
            face = e[m, 23].astype(np.int64)
            uv[m] = tr.cube_uv(e[m, 20:23], face)
            Pu[m], Pv[m] = cube_tangents(xf[m], face)
        else:
            uv[m] = tr.sphere_uv(e[m, 20:23])
            tu, tv, ok = sphere_tangents(e[m, 20:23])
            Pu[m], Pv[m], tok[m] = mul_l(xf[m], tu), mul_l(xf[m], tv), ok
    hu, hv = gradient(height, e[:, 0], uv)
    N = e[:, 2:5]
    Ns, ok = bump_normal(N, Pu, Pv, hu, hv, e[:, 1] != 0, e[:, 5:8])
    ok &= tok
    Ns = np.where(ok[:, None], Ns, N)
    return np.c_[hu, hv, Pu, Pv, Ns, ok.astype(np.float32), uv, np.zeros((n, 2), np.float32)].astype(np.float32)
