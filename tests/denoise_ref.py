"""numpy float32 restatement of the denoiser (csrc/pt_denoise.h gives every operation; ptd::expNegPoly / exp2Poly in csrc/pt_device.h):
vectorised over the pixels, a loop over the levels and the 25 taps.  Every operation is one fp32 operation in the kernels' order, so the
GPU's result equals this one bit for bit.  Also the guide buffers from the CPU oracle (camera_ray + intersect, the nearest_hit rule)."""
import numpy as np

F = np.float32
H5 = (F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625))
OUTSIDE_T = F(-1.0)


def exp2_poly(t):
    """ptd::exp2Poly: 2^t for -126 <= t <= 0."""
    t = np.asarray(t, F)
    nf = np.rint(t)
    g = t - nf
    q = np.full(t.shape, F(1.535336188319500e-4), F)
    for c in (1.339887440266574e-3, 9.618437357674640e-3, 5.550332471162809e-2, 2.402264791363012e-1, 6.931472028550421e-1):
        q = q * g + F(c)
    r = q * g + F(1.0)
    bits = r.view(np.uint32) + (nf.astype(np.int32) << 23).view(np.uint32)
    return bits.view(F)


def exp_neg_poly(a):
    """ptd::expNegPoly: exp(-a); 0 below 2^-126 and for a NaN."""
    a = np.atleast_1d(np.asarray(a, F))
    with np.errstate(all="ignore"):
        t = a * F(-1.44269504088896341)
        ok = t >= F(-126.0)
        return np.where(ok, exp2_poly(np.where(ok, t, F(0.0))), F(0.0)).astype(F)


def _dot(d):
    t = d * d
    return (t[..., 0] + t[..., 1]) + t[..., 2]


def inverse_sigmas(levels, sigma_color, sigma_normal, sigma_position):
    """The host's fp32 constants: ([invC_i], invN, invP)."""
    with np.errstate(all="ignore"):
        sc, sn, sp = F(sigma_color), F(sigma_normal), F(sigma_position)
        inv_c0 = F(1.0) / (sc * sc)
        return [inv_c0 * F(4 ** i) for i in range(levels)], F(1.0) / (sn * sn), F(1.0) / (sp * sp)


def atrous(mean, pos, nrm, geom, levels, sigma_color, sigma_normal, sigma_position):
    """mean (H, W, 3): the filter's input colour; pos, nrm (H, W, 3) and geom (H, W) int32: the guides.  Returns (H, W, 3)."""
    c = np.ascontiguousarray(mean, F).copy()
    pos, nrm = np.asarray(pos, F), np.asarray(nrm, F)
    miss = np.asarray(geom) < 0
    Hh, Ww = c.shape[:2]
    inv_c, inv_n, inv_p = inverse_sigmas(levels, sigma_color, sigma_normal, sigma_position)
    with np.errstate(all="ignore"):
        for i in range(levels):
            s = 1 << i
            sum_w = np.zeros((Hh, Ww), F)
            sum_c = np.zeros((Hh, Ww, 3), F)
            for dy in range(-2, 3):
                y0, y1 = max(0, -dy * s), min(Hh, Hh - dy * s)
                if y0 >= y1:
                    continue
                for dx in range(-2, 3):
                    x0, x1 = max(0, -dx * s), min(Ww, Ww - dx * s)
                    if x0 >= x1:
                        continue
                    ps = (slice(y0, y1), slice(x0, x1))
                    qs = (slice(y0 + dy * s, y1 + dy * s), slice(x0 + dx * s, x1 + dx * s))
                    hw = H5[dy + 2] * H5[dx + 2]
                    cq = c[qs]
                    if dx == 0 and dy == 0:
                        sum_w[ps] = sum_w[ps] + hw
                        sum_c[ps] = sum_c[ps] + cq * hw
                        continue
                    use = miss[qs] == miss[ps]
                    a = _dot(cq - c[ps]) * inv_c[i]
                    a = a + _dot(nrm[qs] - nrm[ps]) * inv_n
                    a = a + _dot(pos[qs] - pos[ps]) * inv_p
                    w = hw * exp_neg_poly(a)
                    sum_w[ps] = np.where(use, sum_w[ps] + w, sum_w[ps])
                    sum_c[ps] = np.where(use[..., None], sum_c[ps] + cq * w[..., None], sum_c[ps])
            c = sum_c / sum_w[..., None]
    return c


def denoise(rgb_sum, samples, pos, nrm, geom, levels, sigma_color, sigma_normal, sigma_position):
    """pt_denoise: the accumulator's sum (H, W, 3) -> the filtered mean."""
    return atrous(np.asarray(rgb_sum, F) / F(samples), pos, nrm, geom, levels, sigma_color, sigma_normal, sigma_position)


def to_rgba8(mean):
    """pt_denoise_rgba8's conversion of the filtered mean (finite values): (N, 4) bytes, alpha 0."""
    m = np.asarray(mean, F).reshape(-1, 3)
    v = np.clip((m.astype(np.float64) * 255.0).astype(np.int64), 0, 255).astype(np.uint8)
    return np.concatenate([v, np.zeros((len(v), 1), np.uint8)], axis=1)


def oracle_guides(orc, ref, guide_iter, meshes=None, mesh_normals=None):
    """The guide buffers as the CPU oracle gives them: for every pixel the ray ref.camera_ray(guide_iter, pixel) against every geom in index
    order (orc.intersect / orc.mesh_intersect), nearest = t > 0, smallest t, an equal t keeps the lower index.
    Returns (pos_t (N, 4), nrm (N, 3), geom (N,) int32)."""
    n = ref.W * ref.H
    pos_t = np.zeros((n, 4), F)
    pos_t[:, 3] = OUTSIDE_T
    nrm = np.zeros((n, 3), F)
    geom = np.full(n, -1, np.int32)
    for pix in range(n):
        ray = ref.camera_ray(guide_iter, pix)
        t_min = F(0.0)
        for g in range(len(ref.geoms)):
            G = ref.geoms[g:g + 1]
            if int(G["type"][0]) == 2:
                t, p, nn = orc.mesh_intersect(G, meshes[g], ray, normals=(mesh_normals or {}).get(g))[:3]
            else:
                t, p, nn = orc.intersect(G, ray)[:3]
            if t > 0 and (geom[pix] < 0 or t < t_min):
                t_min = t
                geom[pix] = g
                pos_t[pix, :3], pos_t[pix, 3], nrm[pix] = p, t, nn
    return pos_t, nrm, geom
