"""numpy float32 restatement of the second moments, the variance of the mean and the variance-guided a-trous filter (csrc/pt_denoise.h gives
every operation: k_commit<true>, k_variance, k_atrous_*<AtrousGuided>), vectorised over the pixels like denoise_ref.py: every operation is one fp32
operation in the kernels' order, so the GPU's result equals this one bit for bit."""
import numpy as np

from denoise_ref import F, H5, _dot, exp_neg_poly

K3 = (F(0.25), F(0.5), F(0.25))


def lum(c):
    """lum(c) = (0.2126f * r + 0.7152f * g) + 0.0722f * b"""
    c = np.asarray(c, F)
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def moments(samples):
    """Q after committing `samples` -- an iterable of single iterations' radiance, (..., 3) each, in iteration order: Q = Q + l * l from 0.
    (A pixel an iteration left untouched holds 0 there: adding +0.)"""
    q = None
    for s in samples:
        l = lum(s)
        q = (np.zeros(l.shape, F) if q is None else q) + l * l
    return q


def mean_and_variance(S, Q, n):
    """(c, v): c.k = S.k / n;  L = lum(c);  d = Q / n - L * L;  d = d > 0 ? d : 0 (a NaN gives 0);  v = d / (n - 1)"""
    S, Q = np.asarray(S, F), np.asarray(Q, F)
    with np.errstate(all="ignore"):
        c = S / F(n)
        L = lum(c)
        d = Q / F(n) - L * L
        d = np.where(d > 0, d, F(0.0)).astype(F)
        return c, d / F(n - 1)


def variance(S, Q, n):
    """pt_variance: the variance of the mean luminance; S (..., 3), Q (...)."""
    return mean_and_variance(S, Q, n)[1]


def atrous_var(mean, var, pos, nrm, geom, levels, sigma_lum, sigma_normal, sigma_position):
    """mean (H, W, 3), var (H, W): the filter's input colour and the variance of its luminance; pos, nrm (H, W, 3), geom (H, W) int32: the guides.
    Returns (colour (H, W, 3), variance (H, W))."""
    c = np.ascontiguousarray(mean, F).copy()
    v = np.ascontiguousarray(var, F).copy()
    pos, nrm = np.asarray(pos, F), np.asarray(nrm, F)
    miss = np.asarray(geom) < 0
    Hh, Ww = c.shape[:2]
    with np.errstate(all="ignore"):
        sl = F(sigma_lum)
        sl2 = sl * sl
        sn, sp = F(sigma_normal), F(sigma_position)
        inv_n, inv_p = F(1.0) / (sn * sn), F(1.0) / (sp * sp)
        for i in range(levels):
            s = 1 << i
            # the 3 x 3 prefilter of the variance
            gw = np.zeros((Hh, Ww), F)
            gv = np.zeros((Hh, Ww), F)
            for dy in range(-1, 2):
                y0, y1 = max(0, -dy * s), min(Hh, Hh - dy * s)
                if y0 >= y1:
                    continue
                for dx in range(-1, 2):
                    x0, x1 = max(0, -dx * s), min(Ww, Ww - dx * s)
                    if x0 >= x1:
                        continue
                    ps = (slice(y0, y1), slice(x0, x1))
                    qs = (slice(y0 + dy * s, y1 + dy * s), slice(x0 + dx * s, x1 + dx * s))
                    k = K3[dy + 1] * K3[dx + 1]
                    use = miss[qs] == miss[ps]
                    gw[ps] = np.where(use, gw[ps] + k, gw[ps])
                    gv[ps] = np.where(use, gv[ps] + v[qs] * k, gv[ps])
            g = gv / gw
            inv_l = F(1.0) / (sl2 * g + F(1e-8)) if np.isfinite(sl2) else np.zeros((Hh, Ww), F)
            l = lum(c)
            sum_w = np.zeros((Hh, Ww), F)
            sum_v = np.zeros((Hh, Ww), F)
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
                    cq, vq = c[qs], v[qs]
                    if dx == 0 and dy == 0:
                        sum_w[ps] = sum_w[ps] + hw
                        sum_c[ps] = sum_c[ps] + cq * hw
                        sum_v[ps] = sum_v[ps] + vq * (hw * hw)
                        continue
                    use = miss[qs] == miss[ps]
                    dl = l[qs] - l[ps]
                    a = (dl * dl) * inv_l[ps]
                    a = a + _dot(nrm[qs] - nrm[ps]) * inv_n
                    a = a + _dot(pos[qs] - pos[ps]) * inv_p
                    w = hw * exp_neg_poly(a)
                    sum_w[ps] = np.where(use, sum_w[ps] + w, sum_w[ps])
                    sum_c[ps] = np.where(use[..., None], sum_c[ps] + cq * w[..., None], sum_c[ps])
                    sum_v[ps] = np.where(use, sum_v[ps] + vq * (w * w), sum_v[ps])
            c = sum_c / sum_w[..., None]
            v = sum_v / (sum_w * sum_w)
    return c, v


def denoise_var(rgb_sum, lum_sq_sum, samples, pos, nrm, geom, levels, sigma_lum, sigma_normal, sigma_position):
    """pt_denoise_var: the two accumulators (H, W, 3) and (H, W) -> (the filtered mean, its filtered variance)."""
    c, v = mean_and_variance(rgb_sum, lum_sq_sum, samples)
    return atrous_var(c, v, pos, nrm, geom, levels, sigma_lum, sigma_normal, sigma_position)
