"""numpy float32 restatement of demodulated history (PT_FLAG_DEMOD_HISTORY; csrc/pt_temporal.h gives every operation under "ALBEDO"): the
history also carries the mean first-hit albedo, the blend of the reprojected history with the new samples is divided by the BLENDED albedo, and
the last level multiplies an albedo back.  A composition of temporal_ref, demod_ref, spatial_var_ref and denoise_var_ref, none of them edited:
every operation is one fp32 operation in the kernels' order, so the GPU's result equals this one bit for bit.

A history here is temporal_ref's five and the albedo image behind them: (hc, hn, hpos_t, hnrm_id, cam16, ha), ha (h, w, 4) = (Ab, tot)."""
import os
import re

import numpy as np

import demod_ref as dm
import denoise_var_ref as dv
import spatial_var_ref as sv
import temporal_ref as tr

F = np.float32
NEVER = float("inf")          # a PT_DEMOD_HISTORY_MIN_OWN no sample count reaches: always the blended albedo


def min_own(header=None):
    """PT_DEMOD_HISTORY_MIN_OWN as include/pt_amd.h defines it"""
    header = header or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "pt_amd.h")
    return int(re.search(r"^#define PT_DEMOD_HISTORY_MIN_OWN ([0-9]+)$", open(header).read(), re.M).group(1))


def empty_history(h, w):
    """a history that holds nothing"""
    return tr.empty_history(h, w) + (np.zeros((h, w, 4), F),)


def reproject_albedo(pos_t, nrm_id, history, consts=None):
    """steps 1 - 6 over the albedo: temporal_ref.reproject over (ha, 0) -- the same taps, conditions and order, sumA from 0.
    Returns (ha (h, w, 3), Nh (h, w)), zeros where a pixel has no history."""
    hc, hn, hpos_t, hnrm_id, cam16, ha = history
    ha0 = np.concatenate([np.asarray(ha, F)[..., :3], np.zeros(np.asarray(ha).shape[:2] + (1,), F)], axis=2)
    hav, Nh = tr.reproject(pos_t, nrm_id, ha0, hn, hpos_t, hnrm_id, cam16, consts)
    return hav[..., :3], Nh


def blend_albedo(asum, n, hav, Nh):
    """step 7: (Ab, tot) (h, w, 4):  tot = Nh + n;  Ab.k = (ha.k * Nh + Asum.k) / tot"""
    asum = np.asarray(asum, F)
    with np.errstate(all="ignore"):
        tot = Nh + F(n)
        ab = (hav * Nh[..., None] + asum[..., :3]) / tot[..., None]
    return np.concatenate([ab, tot[..., None]], axis=2).astype(F)


def albedo_form(asum, n, pos_t, nrm_id, history, consts=None):
    """outA of every ALBEDO form of k_temporal: (Ab, tot) (h, w, 4)"""
    return blend_albedo(asum, n, *reproject_albedo(pos_t, nrm_id, history, consts))


def capture_form(S, Q, asum, n, pos_t, nrm_id, history, consts=None):
    """k_temporal<kTemporalCapture, true>: the next history's (Hc', Hn', Ha')"""
    hc, hn = tr.capture_form(S, Q, n, pos_t, nrm_id, *history[:5], consts=consts)
    return hc, hn, albedo_form(asum, n, pos_t, nrm_id, history, consts)


def capture(S, Q, asum, n, pos_t, nrm_id, cam16, history, consts=None):
    """what pt_init over a live flagged renderer leaves as the context's history: the capture, the view's guides and its camera"""
    hc, hn, ha = capture_form(S, Q, asum, n, pos_t, nrm_id, history, consts)
    return hc, hn, np.asarray(pos_t, F), np.asarray(nrm_id, F), np.asarray(cam16, F), ha


def front(S, Q, asum, n, pos_t, nrm_id, history, sigma_normal, sigma_position, consts=None):
    """What stands in front of the division: (c (h, w, 3), v (h, w), (Ab, tot) (h, w, 4)) -- from two samples on k_temporal's filter form, at
    one sample (PT_FLAG_SPATIAL_VARIANCE) its moments form and the spatial estimate."""
    pos_t, nrm_id = np.asarray(pos_t, F), np.asarray(nrm_id, F)
    if n >= 2:
        c, v = tr.filter_form(S, Q, n, pos_t, nrm_id, *history[:5], consts=consts)
    else:
        geom = np.ascontiguousarray(nrm_id[..., 3]).view(np.int32)
        M, N = sv.moments_form(S, Q, n, pos_t, nrm_id, history[:5], consts)
        c, v, _ = sv.spatial_variance(M, N, pos_t[..., :3], nrm_id[..., :3], geom, sv.constants()[1], sigma_normal, sigma_position)
    return c, v, albedo_form(asum, n, pos_t, nrm_id, history, consts)


def demodulated_front(S, Q, asum, n, pos_t, nrm_id, history, sigma_normal, sigma_position, consts=None, eps=dm.MIN_ALBEDO):
    """the image level 0 reads, (h, w, 4), and (Ab, tot): k_demodulate over the front with (asum = Ab, samples = 1) -- x / 1 is exact -- which is
    also the fused front's result"""
    c, v, ab = front(S, Q, asum, n, pos_t, nrm_id, history, sigma_normal, sigma_position, consts)
    cd, vd = dm.demodulate(c, v, ab, 1, eps)
    return np.concatenate([cd, vd[..., None]], axis=2).astype(F), ab


def filtered(S, Q, asum, n, pos_t, nrm_id, history, levels, sigma_lum, sigma_normal, sigma_position, consts=None, eps=dm.MIN_ALBEDO):
    """the levels' result BEFORE an albedo is multiplied back: (co (h, w, 3), vo (h, w), (Ab, tot))"""
    pos_t, nrm_id = np.asarray(pos_t, F), np.asarray(nrm_id, F)
    img, ab = demodulated_front(S, Q, asum, n, pos_t, nrm_id, history, sigma_normal, sigma_position, consts, eps)
    geom = np.ascontiguousarray(nrm_id[..., 3]).view(np.int32)
    co, vo = dv.atrous_var(img[..., :3], img[..., 3], pos_t[..., :3], nrm_id[..., :3], geom, levels, sigma_lum, sigma_normal, sigma_position)
    return co, vo, ab


def remodulate(co, vo, ab, asum, n, own_from, eps=dm.MIN_ALBEDO):
    """AtrousDemod's store under the host's choice of (asum, demodN): below `own_from` samples (Ab, 1), from there on the renderer's own sums
    and n"""
    return dm.remodulate(co, vo, ab, 1, eps) if n < own_from else dm.remodulate(co, vo, asum, n, eps)


def denoise_var_demod_history(S, Q, asum, n, pos_t, nrm_id, history, levels, sigma_lum, sigma_normal, sigma_position, own_from=None, consts=None,
                              eps=dm.MIN_ALBEDO):
    """pt_denoise_var of a PT_FLAG_DEMOD_HISTORY renderer whose context holds `history`: (colour (h, w, 3), variance (h, w))"""
    own_from = min_own() if own_from is None else own_from
    co, vo, ab = filtered(S, Q, asum, n, pos_t, nrm_id, history, levels, sigma_lum, sigma_normal, sigma_position, consts, eps)
    return remodulate(co, vo, ab, asum, n, own_from, eps)


def denoise_var_naive(S, Q, asum, n, pos_t, nrm_id, history, levels, sigma_lum, sigma_normal, sigma_position, consts=None, eps=dm.MIN_ALBEDO):
    """What lifting the refusal alone would compute, for the study: the BLENDED colour divided and multiplied by the new samples' mean albedo,
    a history without albedo."""
    pos_t, nrm_id = np.asarray(pos_t, F), np.asarray(nrm_id, F)
    c, v, _ = front(S, Q, asum, n, pos_t, nrm_id, history, sigma_normal, sigma_position, consts)
    geom = np.ascontiguousarray(nrm_id[..., 3]).view(np.int32)
    return dm.atrous_demod(c, v, asum, n, pos_t[..., :3], nrm_id[..., :3], geom, levels, sigma_lum, sigma_normal, sigma_position, eps)
