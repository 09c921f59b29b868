"""numpy float32 restatement of the kernels' texture mapping (csrc/pt_device.h, "texture mapping"), operation for operation: the
project compiles with -ffp-contract=off and correctly rounded division and square root, so these match the device bit for bit."""
import numpy as np

F = np.float32
HALF_PI = F(1.57079637050628662109375)
QUARTER_PI = F(0.785398185253143310546875)
PI = F(3.1415927410125732421875)
INV_TWO_PI = F(0.15915493667125701904296875)
INV_PI = F(0.3183098733425140380859375)


def _f(a):
    return np.asarray(a, np.float32)


def atan01(t):
    t = _f(t)
    big = t > F(0.4142135623730950)
    with np.errstate(all="ignore"):
        x = np.where(big, (t - F(1)) / (t + F(1)), t).astype(np.float32)
    z = x * x
    p = F(8.05374449538e-2)
    p = p * z - F(1.38776856032e-1)
    p = p * z + F(1.99777106478e-1)
    p = p * z - F(3.33329491539e-1)
    r = (p * z) * x + x
    return np.where(big, QUARTER_PI + r, r).astype(np.float32)


def atan2(y, x):
    y, x = _f(y), _f(x)
    ax, ay = np.abs(x), np.abs(y)
    steep = ay > ax
    mx, mn = np.where(steep, ay, ax), np.where(steep, ax, ay)
    with np.errstate(all="ignore"):
        t = np.where(mx > F(0), mn / mx, F(0)).astype(np.float32)
    r = atan01(t)
    r = np.where(steep, HALF_PI - r, r).astype(np.float32)
    r = np.where(x < F(0), PI - r, r).astype(np.float32)
    return np.where(y < F(0), -r, r).astype(np.float32)


def asin(x):
    x = _f(x)
    a = np.abs(x)
    a = np.where(a > F(1), F(1), a).astype(np.float32)
    big = a > F(0.5)
    z = np.where(big, F(0.5) * (F(1) - a), a * a).astype(np.float32)
    with np.errstate(all="ignore"):
        s = np.where(big, np.sqrt(z), a).astype(np.float32)
    p = F(4.2163199048e-2)
    p = p * z + F(2.4181311049e-2)
    p = p * z + F(4.5470025998e-2)
    p = p * z + F(7.4953002686e-2)
    p = p * z + F(1.6666752422e-1)
    r0 = (p * z) * s + s
    r = np.where(big, HALF_PI - F(2) * r0, r0).astype(np.float32)
    return np.where(x < F(0), -r, r).astype(np.float32)


def sphere_uv(q):
    q = _f(q).reshape(-1, 3)
    with np.errstate(all="ignore"):
        dd = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
        inv = F(1) / np.sqrt(dd)
        d = q * inv[:, None]
    u = F(0.5) + atan2(d[:, 2], d[:, 0]) * INV_TWO_PI
    v = F(0.5) + asin(d[:, 1]) * INV_PI
    return np.stack([u, v], 1).astype(np.float32)


def cube_uv(q, face):
    q = _f(q).reshape(-1, 3)
    a = np.asarray(face, np.int64) >> 1
    i = np.arange(len(q))
    u = q[i, (a + 1) % 3] + F(0.5)
    v = q[i, (a + 2) % 3] + F(0.5)
    return np.stack([u, v], 1).astype(np.float32)


def mesh_uv(e):
    """e: (n, 8) = barycentric u, v and the corner UVs u0 v0 u1 v1 u2 v2"""
    e = _f(e).reshape(-1, 8)
    bu, bv = e[:, 0], e[:, 1]
    w = (F(1) - bu) - bv
    u = (e[:, 2] * w + e[:, 4] * bu) + e[:, 6] * bv
    v = (e[:, 3] * w + e[:, 5] * bu) + e[:, 7] * bv
    return np.stack([u, v], 1).astype(np.float32)


def sample(tex, uv):
    """bilinear, repeat-wrapped lookup of tex (H, W, 3) float32 (row 0 = top) at uv (n, 2)"""
    tex = _f(tex)
    H, W = tex.shape[:2]
    uv = _f(uv).reshape(-1, 2)
    u, v = uv[:, 0], uv[:, 1]
    u = np.where(np.isfinite(u), u, F(0)).astype(np.float32)
    v = np.where(np.isfinite(v), v, F(0)).astype(np.float32)
    u = u - np.floor(u)
    v = v - np.floor(v)
    x = u * F(W) - F(0.5)
    y = (F(1) - v) * F(H) - F(0.5)
    xf0, yf0 = np.floor(x), np.floor(y)
    fx, fy = (x - xf0)[:, None], (y - yf0)[:, None]
    x0, y0 = xf0.astype(np.int64), yf0.astype(np.int64)
    x0 = np.where(x0 < 0, x0 + W, np.where(x0 >= W, W - 1, x0))
    y0 = np.where(y0 < 0, y0 + H, np.where(y0 >= H, H - 1, y0))
    x0, y0 = np.maximum(x0, 0), np.maximum(y0, 0)
    x1 = np.where(x0 + 1 == W, 0, x0 + 1)
    y1 = np.where(y0 + 1 == H, 0, y0 + 1)
    a, b, c, d = tex[y0, x0], tex[y0, x1], tex[y1, x0], tex[y1, x1]
    top = a + (b - a) * fx
    bot = c + (d - c) * fx
    return (top + (bot - top) * fy).astype(np.float32)
