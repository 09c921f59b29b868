"""numpy float32 restatement of temporal reprojection (csrc/pt_temporal.h gives every operation: k_temporal<CAPTURE>), vectorised over the
pixels like denoise_var_ref.py: every operation is one fp32 operation in the kernel's order, so the GPU's result equals this one bit for bit.
The camera rows come from temporal_camera (float64, rounded once, as the host computes them); everything else is float32."""
import re
import os

import numpy as np

from denoise_var_ref import atrous_var, lum

F = np.float32


def constants(header=None):
    """(cap, c_n, c_p, w_min): PT_TEMPORAL_MAX_HISTORY, _NORMAL_DOT, _PLANE_FRACTION, _MIN_WEIGHT as include/pt_amd.h defines them"""
    header = header or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "pt_amd.h")
    text = open(header).read()
    return tuple(F(re.search(r"#define PT_TEMPORAL_%s ([0-9.eE+-]+)f\b" % n, text).group(1))
                 for n in ("MAX_HISTORY", "NORMAL_DOT", "PLANE_FRACTION", "MIN_WEIGHT"))


def camera_constants(camera):
    """(view, up, right, eye, pixLenX, pixLenY, halfW, halfH) as camera_params derives them in fp32 from a camera record (position, view, up,
    fov, resolution): right = normalize(cross(view, up)) with s = 1 / sqrt(d), pixLen = 2 tan(fovy) [* W / H] / size.  (tan is the C library's
    in the renderer and numpy's here: the last bit may differ, so a test that needs the renderer's own bits takes pt_test_temporal_camera.)"""
    cam = np.asarray(camera).reshape(-1)[0]
    W, H = int(cam["resolution"][0]), int(cam["resolution"][1])
    view, up, eye = np.asarray(cam["view"], F), np.asarray(cam["up"], F), np.asarray(cam["position"], F)
    cr = np.array([view[1] * up[2] - view[2] * up[1], view[2] * up[0] - view[0] * up[2], view[0] * up[1] - view[1] * up[0]], F)
    d = (cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2]
    s = F(1.0) / np.sqrt(d)
    right = cr * s
    pi = F(3.1415926535897932384626422832795028841971)
    ys = np.tan(F(cam["fov"][1]) * (pi / F(180)))
    xs = (ys * F(W)) / F(H)
    return view, up, right, eye, (F(2.0) * xs) / F(W), (F(2.0) * ys) / F(H), F(W) * F(0.5), F(H) * F(0.5)


def temporal_camera(view, up, right, eye, pix_len_x, pix_len_y, half_w, half_h):
    """The 16 floats k_temporal takes for the old view: eye (3), pixLenX, pixLenY, halfW, halfH, and the rows r0, r1, r2 of the inverse of
    [view | -right | -up] -- by cofactors in float64, each entry divided by the determinant and rounded to fp32 once."""
    m = np.stack([np.asarray(view, F).astype(np.float64), -np.asarray(right, F).astype(np.float64), -np.asarray(up, F).astype(np.float64)], axis=1)
    c00 = m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]
    c01 = m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2]
    c02 = m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]
    det = m[0, 0] * c00 + m[0, 1] * c01 + m[0, 2] * c02
    with np.errstate(all="ignore"):
        inv = np.array([[c00 / det, (m[0, 2] * m[2, 1] - m[0, 1] * m[2, 2]) / det, (m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]) / det],
                        [c01 / det, (m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0]) / det, (m[0, 2] * m[1, 0] - m[0, 0] * m[1, 2]) / det],
                        [c02 / det, (m[0, 1] * m[2, 0] - m[0, 0] * m[2, 1]) / det, (m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]) / det]])
        return np.concatenate([np.asarray(eye, F), [F(pix_len_x), F(pix_len_y), F(half_w), F(half_h)], inv.astype(F).reshape(-1)]).astype(F)


def camera16(camera):
    """temporal_camera of a camera record"""
    return temporal_camera(*camera_constants(camera))


def pack_guides(pos_t, nrm, geom, h, w):
    """the two float4 guide images as the device holds them, from pt_gbuffer's three arrays: (pos_t (h, w, 4), nrm_id (h, w, 4))"""
    nrm_id = np.empty((h, w, 4), F)
    nrm_id[..., :3] = np.asarray(nrm, F).reshape(h, w, 3)
    nrm_id[..., 3] = np.ascontiguousarray(geom, np.int32).reshape(h, w).view(F)
    return np.ascontiguousarray(pos_t, F).reshape(h, w, 4).copy(), nrm_id


def empty_history(h, w):
    """a history that holds nothing: (hc, hn, hpos_t, hnrm_id, cam16) with hn = 0 everywhere"""
    z4 = np.zeros((h, w, 4), F)
    nid = z4.copy()
    nid[..., 3] = np.full((h, w), -1, np.int32).view(F)
    return z4.copy(), np.zeros((h, w), F), z4.copy(), nid, np.zeros(16, F)


def _dot3(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def project(pos, cam16):
    """steps 2 - 3: (s, u, v) of world points pos (..., 3) in the old camera"""
    cam = np.asarray(cam16, F)
    e, plx, ply, hw, hh, r0, r1, r2 = cam[0:3], cam[3], cam[4], cam[5], cam[6], cam[7:10], cam[10:13], cam[13:16]
    pos = np.asarray(pos, F)
    with np.errstate(all="ignore"):
        dx, dy, dz = pos[..., 0] - e[0], pos[..., 1] - e[1], pos[..., 2] - e[2]
        s = _dot3(r0[0], r0[1], r0[2], dx, dy, dz)
        a = _dot3(r1[0], r1[1], r1[2], dx, dy, dz) / s
        b = _dot3(r2[0], r2[1], r2[2], dx, dy, dz) / s
        u = (a / plx + hw) - F(0.5)
        v = (b / ply + hh) - F(0.5)
    return s, u, v


def reproject(pos_t, nrm_id, hc, hn, hpos_t, hnrm_id, cam16, consts=None):
    """steps 1 - 6: (hc (h, w, 4), Nh (h, w)) -- zeros where a pixel has no history"""
    cap, c_n, c_p, w_min = consts or constants()
    pos_t, nrm_id = np.asarray(pos_t, F), np.asarray(nrm_id, F)
    hc, hn, hpos_t, hnrm_id = np.asarray(hc, F), np.asarray(hn, F), np.asarray(hpos_t, F), np.asarray(hnrm_id, F)
    h, w = hn.shape
    ids = np.ascontiguousarray(nrm_id[..., 3]).view(np.int32)
    hids = np.ascontiguousarray(hnrm_id[..., 3]).view(np.int32)
    with np.errstate(all="ignore"):
        s, u, v = project(pos_t[..., :3], cam16)
        ok = (ids >= 0) & (s > 0) & (u > F(-1.0)) & (u < F(w)) & (v > F(-1.0)) & (v < F(h))
        fx, fy = np.floor(u), np.floor(v)
        wx, wy = u - fx, v - fy
        x0 = np.where(ok, fx, 0).astype(np.int64)
        y0 = np.where(ok, fy, 0).astype(np.int64)
        lim = c_p * pos_t[..., 3]
        N, P = nrm_id[..., :3], pos_t[..., :3]
        sum_w, sum_n, sum_c = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w, 4), F)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + i, y0 + j
                inside = ok & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                nq, Nq, Pq, Cq = hn[cy, cx], hnrm_id[cy, cx, :3], hpos_t[cy, cx, :3], hc[cy, cx]
                use = inside & (nq > 0) & (hids[cy, cx] == ids)
                use &= _dot3(Nq[..., 0], Nq[..., 1], Nq[..., 2], N[..., 0], N[..., 1], N[..., 2]) >= c_n
                off = _dot3(Pq[..., 0] - P[..., 0], Pq[..., 1] - P[..., 1], Pq[..., 2] - P[..., 2], N[..., 0], N[..., 1], N[..., 2])
                use &= np.abs(off) <= lim
                wt = (wx if i else F(1.0) - wx) * (wy if j else F(1.0) - wy)
                sum_w = np.where(use, sum_w + wt, sum_w)
                sum_c = np.where(use[..., None], sum_c + Cq * wt[..., None], sum_c)
                sum_n = np.where(use, sum_n + nq * wt, sum_n)
        has = ok & (sum_w > w_min)
        hcv = sum_c / sum_w[..., None]
        hnv = sum_n / sum_w
        Nh = np.where(hnv < cap, hnv, cap)
        return np.where(has[..., None], hcv, F(0.0)).astype(F), np.where(has, Nh, F(0.0)).astype(F)


def blend(S, Q, n, hc, Nh):
    """step 7: (c (h, w, 3), m2 (h, w), tot (h, w))"""
    S, Q = np.asarray(S, F), np.asarray(Q, F)
    with np.errstate(all="ignore"):
        tot = Nh + F(n)
        c = (hc[..., :3] * Nh[..., None] + S) / tot[..., None]
        m2 = (hc[..., 3] * Nh + Q) / tot
    return c, m2, tot


def filter_form(S, Q, n, pos_t, nrm_id, hc, hn, hpos_t, hnrm_id, cam16, consts=None):
    """k_temporal<false>: (c (h, w, 3), variance (h, w)) -- what level 0 of the filter reads"""
    c, m2, tot = blend(S, Q, n, *reproject(pos_t, nrm_id, hc, hn, hpos_t, hnrm_id, cam16, consts))
    with np.errstate(all="ignore"):
        L = lum(c)
        dd = m2 - L * L
        dd = np.where(dd > 0, dd, F(0.0)).astype(F)
        return c, dd / (tot - F(1.0))


def capture_form(S, Q, n, pos_t, nrm_id, hc, hn, hpos_t, hnrm_id, cam16, consts=None):
    """k_temporal<true>: (Hc' (h, w, 4), Hn' (h, w))"""
    cap = (consts or constants())[0]
    c, m2, tot = blend(S, Q, n, *reproject(pos_t, nrm_id, hc, hn, hpos_t, hnrm_id, cam16, consts))
    with np.errstate(all="ignore"):
        return np.concatenate([c, m2[..., None]], axis=2).astype(F), np.where(tot < cap, tot, cap).astype(F)


def denoise_var_temporal(S, Q, n, pos_t, nrm_id, history, levels, sigma_lum, sigma_normal, sigma_position, consts=None):
    """pt_denoise_var of a renderer whose context holds `history` = (hc, hn, hpos_t, hnrm_id, cam16): the blend, then the filter's levels
    (level 0 reads the blend, at step 1).  Returns (colour (h, w, 3), variance (h, w))."""
    c, v = filter_form(S, Q, n, pos_t, nrm_id, *history, consts=consts)
    geom = np.ascontiguousarray(np.asarray(nrm_id, F)[..., 3]).view(np.int32)
    return atrous_var(c, v, np.asarray(pos_t, F)[..., :3], np.asarray(nrm_id, F)[..., :3], geom, levels, sigma_lum, sigma_normal, sigma_position)
