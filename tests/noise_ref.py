"""numpy float32 restatement of the noise statistics (csrc/pt_noise.h gives every operation: k_noise_stats) and of pt_iterate_until's stopping
rule (include/pt_amd.h): every operation is one fp32 operation in the kernel's order, so the GPU's result equals this one bit for bit."""
import math

import numpy as np

from denoise_var_ref import lum, mean_and_variance

F = np.float32
TILE = 16


def tiles_of(w, h):
    return (w + TILE - 1) // TILE, (h + TILE - 1) // TILE


def butterfly(a):
    """The xor butterfly over the last axis, 64 lanes: for o in 32, 16, 8, 4, 2, 1: a[l] = a[l] + a[l ^ o].  Every lane ends with the same bits."""
    a = np.asarray(a, F)
    lane = np.arange(64)
    with np.errstate(all="ignore"):
        for o in (32, 16, 8, 4, 2, 1):
            a = a + a[..., lane ^ o]
    return a[..., 0]


def tile_sum(a):
    """a (tiles_y, tiles_x, 16, 16), [row][column] of each tile with +0 outside the frame: wave w holds rows 4 w .. 4 w + 3, lane = 16 * (row & 3)
    + column; the waves' butterflies, then (w0 + w1) + (w2 + w3)."""
    w = butterfly(np.asarray(a, F).reshape(a.shape[:-2] + (4, 64)))
    with np.errstate(all="ignore"):
        return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def tile_rel_var(S, Q, n, lum_floor):
    """S (H, W, 3), Q (H, W) -> r (tiles_y, tiles_x): mv = V / N, ml = M / N, mf = ml > floor ? ml : floor, r = mv / (mf * mf)."""
    S, Q = np.asarray(S, F), np.asarray(Q, F)
    h, w = Q.shape
    tx, ty = tiles_of(w, h)
    c, v = mean_and_variance(S, Q, n)
    with np.errstate(all="ignore"):
        L = lum(c)
        pv = np.zeros((ty * TILE, tx * TILE), F)
        pl = np.zeros((ty * TILE, tx * TILE), F)
        pv[:h, :w] = v
        pl[:h, :w] = L
        split = lambda a: a.reshape(ty, TILE, tx, TILE).transpose(0, 2, 1, 3)
        V, M = tile_sum(split(pv)), tile_sum(split(pl))
        nx = np.minimum(TILE, w - TILE * np.arange(tx))
        ny = np.minimum(TILE, h - TILE * np.arange(ty))
        N = (ny[:, None] * nx[None, :]).astype(F)
        mv, ml = V / N, M / N
        fl = F(lum_floor)
        mf = np.where(ml > fl, ml, fl).astype(F)
        return (mv / (mf * mf)).astype(F)


def stats(S, Q, n, threshold, lum_floor, fraction=0.0):
    """pt_noise_stats: a dict of PtNoiseStats' fields and "tile_rel_var".  `converged` is judged with `fraction` (pt_noise_stats itself: 0)."""
    r = tile_rel_var(S, Q, n, lum_floor)
    thr2 = F(threshold) * F(threshold)
    with np.errstate(all="ignore"):
        unconverged = int(np.count_nonzero(r > thr2))
        mx = F(0.0)
        for x in r.reshape(-1):          # the maximum from 0, a NaN ignored
            if x > mx:
                mx = x
    ty, tx = r.shape
    return {"samples": n, "tiles_x": tx, "tiles_y": ty, "tiles": tx * ty, "unconverged": unconverged, "max_rel_var": F(mx), "thr2": thr2,
            "converged": is_converged(unconverged, tx * ty, fraction), "tile_rel_var": r}


def is_converged(unconverged, tiles, fraction):
    return unconverged <= math.floor(float(F(fraction)) * tiles)


def samples_done(converged_at, first_iter, min_samples, max_samples, check_every, lookahead):
    """pt_iterate_until's stopping rule: converged_at(s) -> bool judges the accumulator of s samples.  Rounds of check_every from first_iter - 1,
    the last cut at max_samples; a check after every round that ends with s >= min_samples; s* = the first checked count that is converged.
    lookahead 0: s*; lookahead 1: min(s* + check_every, max_samples); never converged: max_samples.  Returns (samples_done, converged)."""
    s = first_iter - 1
    while s < max_samples:
        s = min(s + check_every, max_samples)
        if s >= min_samples and converged_at(s):
            return (s if lookahead == 0 else min(s + check_every, max_samples)), True
    return max_samples, False
