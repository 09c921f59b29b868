"""numpy float32 restatement of the spatial variance estimate (csrc/pt_spatial_var.h gives every operation: k_temporal<kTemporalMoments>, then
k_spatial_variance_*<R>), vectorised over the pixels like denoise_var_ref.py: every operation is one fp32 operation in the kernels' order, so
the GPU's result equals this one bit for bit."""
import os
import re

import numpy as np

import temporal_ref as tr
from denoise_ref import F, _dot, exp_neg_poly, to_rgba8
from denoise_var_ref import atrous_var, lum


def constants(header=None):
    """(min_count, radius): PT_SPATIAL_MIN_COUNT and PT_SPATIAL_RADIUS as include/pt_amd.h defines them"""
    header = header or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "pt_amd.h")
    text = open(header).read()
    return (F(re.search(r"#define PT_SPATIAL_MIN_COUNT ([0-9.eE+-]+)f\b", text).group(1)),
            int(re.search(r"#define PT_SPATIAL_RADIUS ([0-9]+)\b", text).group(1)))


def moments_form(S, Q, n, pos_t=None, nrm_id=None, history=None, consts=None):
    """Stage A, k_temporal<kTemporalMoments>: (M (h, w, 4) = (c, m2), N (h, w)) -- the count uncapped.  history None: c = S / n, m2 = Q / n,
    N = n (steps 1 - 7 without history: 0 * 0 + S over 0 + n)."""
    S, Q = np.asarray(S, F), np.asarray(Q, F)
    if history is None:
        hc, Nh = np.zeros(S.shape[:2] + (4,), F), np.zeros(S.shape[:2], F)
    else:
        hc, Nh = tr.reproject(pos_t, nrm_id, *history, consts=consts)
    c, m2, tot = tr.blend(S, Q, n, hc, Nh)
    return np.concatenate([c, m2[..., None]], axis=2).astype(F), tot.astype(F)


def spatial_variance(M, N, pos, nrm, geom, radius, sigma_normal, sigma_position, min_count=None):
    """Stage B, k_spatial_variance_*<radius>: M (h, w, 4), N (h, w); pos, nrm (h, w, 3) and geom (h, w) int32: the guides.
    Returns (c (h, w, 3), v (h, w), estimated (h, w) bool: the pixels that took the window)."""
    min_count = constants()[0] if min_count is None else F(min_count)
    M, N = np.asarray(M, F), np.asarray(N, F)
    pos, nrm = np.asarray(pos, F), np.asarray(nrm, F)
    miss = np.asarray(geom) < 0
    h, w = N.shape
    c, m2 = M[..., :3], M[..., 3]
    with np.errstate(all="ignore"):
        L = lum(c)
        dd = m2 - L * L
        dd = np.where(dd > 0, dd, F(0.0)).astype(F)
        own = dd / (N - F(1.0))
        sn, sp = F(sigma_normal), F(sigma_position)
        inv_n, inv_p = F(1.0) / (sn * sn), F(1.0) / (sp * sp)
        sw, s1, s2 = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), F)
        for dy in range(-radius, radius + 1):
            y0, y1 = max(0, -dy), min(h, h - dy)
            if y0 >= y1:
                continue
            for dx in range(-radius, radius + 1):
                x0, x1 = max(0, -dx), min(w, w - dx)
                if x0 >= x1:
                    continue
                ps = (slice(y0, y1), slice(x0, x1))
                qs = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                if dx == 0 and dy == 0:
                    one = F(1.0)
                    sw[ps] = sw[ps] + one
                    s1[ps] = s1[ps] + L[qs] * one
                    s2[ps] = s2[ps] + m2[qs] * one
                    continue
                use = miss[qs] == miss[ps]
                a = _dot(nrm[qs] - nrm[ps]) * inv_n
                a = a + _dot(pos[qs] - pos[ps]) * inv_p
                wt = exp_neg_poly(a)
                sw[ps] = np.where(use, sw[ps] + wt, sw[ps])
                s1[ps] = np.where(use, s1[ps] + L[qs] * wt, s1[ps])
                s2[ps] = np.where(use, s2[ps] + m2[qs] * wt, s2[ps])
        M1, M2 = s1 / sw, s2 / sw
        d = M2 - M1 * M1
        d = np.where(d > 0, d, F(0.0)).astype(F)
        est = d / N
        has_own = N >= min_count
        return c.copy(), np.where(has_own, own, est).astype(F), ~has_own


def denoise_var_spatial(S, Q, n, pos_t, nrm_id, levels, sigma_lum, sigma_normal, sigma_position, history=None, radius=None, min_count=None,
                        consts=None):
    """pt_denoise_var of a PT_FLAG_SPATIAL_VARIANCE renderer at a count below two: stage A, stage B, then the filter's levels (level 0 reads
    stage B's image, at step 1).  pos_t, nrm_id: the guide buffers as the device holds them, (h, w, 4) each; history: temporal_ref's
    (hc, hn, hpos_t, hnrm_id, cam16) or None.  Returns (colour (h, w, 3), variance (h, w))."""
    radius = constants()[1] if radius is None else radius
    pos_t, nrm_id = np.asarray(pos_t, F), np.asarray(nrm_id, F)
    geom = np.ascontiguousarray(nrm_id[..., 3]).view(np.int32)
    M, N = moments_form(S, Q, n, pos_t, nrm_id, history, consts)
    c, v, _ = spatial_variance(M, N, pos_t[..., :3], nrm_id[..., :3], geom, radius, sigma_normal, sigma_position, min_count)
    return atrous_var(c, v, pos_t[..., :3], nrm_id[..., :3], geom, levels, sigma_lum, sigma_normal, sigma_position)


def display_bytes(S, Q, n, pos_t, nrm_id, levels, sigma_lum, sigma_normal, sigma_position, history=None):
    """the display path's bytes of such a frame: (h * w, 4)"""
    return to_rgba8(denoise_var_spatial(S, Q, n, pos_t, nrm_id, levels, sigma_lum, sigma_normal, sigma_position, history)[0])
