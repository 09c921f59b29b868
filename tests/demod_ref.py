"""numpy float32 restatement of albedo demodulation (csrc/pt_albedo.h gives every operation: k_albedo's A_i rule and accumulation,
k_demodulate, AtrousDemod's remodulating store), vectorised over the pixels like denoise_var_ref.py: every operation is one fp32 operation in
the kernels' order, so the GPU's result equals this one bit for bit.  The levels between k_demodulate and the store are denoise_var_ref's."""
import numpy as np

import denoise_var_ref as dv

F = np.float32
MIN_ALBEDO = F(0.015625)          # PT_DEMOD_MIN_ALBEDO (include/pt_amd.h; tests/test_demod_cpu.py holds the two together)
CANDIDATES = (F(1.0 / 256.0), F(1.0 / 64.0), F(1.0 / 16.0))


def albedo_of_hit(hit, emittance, has_reflective, has_refractive, color, texel=None):
    """A_i per pixel: hit (...) bool; the hit material's emittance, hasReflective, hasRefractive (...) and colour (..., 3); texel (..., 3) the
    bound texture's sample at the hit, or None where no texture is bound.  (1, 1, 1) for a miss and for a material that emits, reflects or
    refracts; else colour.k * texel.k (one multiplication), or the colour itself."""
    color = np.asarray(color, F)
    a = color if texel is None else color * np.asarray(texel, F)
    plain = np.asarray(hit, bool) & ~((np.asarray(emittance, F) > 0) | (np.asarray(has_reflective, F) > 0) | (np.asarray(has_refractive, F) > 0))
    return np.where(plain[..., None], a, F(1.0)).astype(F)


def accumulate(albedos, asum=None):
    """the sums after the iterations of `albedos` -- an iterable of A_i (..., 3) in ascending iteration order -- were added to asum (..., 4), or
    to zeros: Asum.k = Asum.k + A_i.k;  Asum.w = Asum.w + 1"""
    for a in albedos:
        a = np.asarray(a, F)
        if asum is None:
            asum = np.zeros(a.shape[:-1] + (4,), F)
        asum = np.concatenate([asum[..., :3] + a, asum[..., 3:] + F(1.0)], axis=-1).astype(F)
    return asum


def floored_albedo(asum, n, eps=MIN_ALBEDO):
    """A': a.k = Asum.k / n;  A'.k = a.k > eps ? a.k : eps (a NaN gives eps)"""
    with np.errstate(all="ignore"):
        a = np.asarray(asum, F)[..., :3] / F(n)
        return np.where(a > F(eps), a, F(eps)).astype(F)


def demodulate(c, v, asum, n, eps=MIN_ALBEDO):
    """k_demodulate: (c (..., 3), v (...)) -> (c', v'):  c'.k = c.k / A'.k;  L = lum(c);  L' = lum(c');  rho = L > 0 ? L' / L : 1;
    v' = v * (rho * rho)"""
    c, v = np.asarray(c, F), np.asarray(v, F)
    al = floored_albedo(asum, n, eps)
    with np.errstate(all="ignore"):
        cd = c / al
        L = dv.lum(c)
        Ld = dv.lum(cd)
        rho = np.where(L > 0, Ld / L, F(1.0)).astype(F)
        return cd, v * (rho * rho)


def remodulate(co, vo, asum, n, eps=MIN_ALBEDO):
    """AtrousDemod's last store: (the filtered demodulated colour co, its variance vo) -> (out, var):  out.k = co.k * A'.k;
    rho' = lum(co) > 0 ? lum(out) / lum(co) : 1;  var = vo * (rho' * rho')"""
    co, vo = np.asarray(co, F), np.asarray(vo, F)
    al = floored_albedo(asum, n, eps)
    with np.errstate(all="ignore"):
        out = co * al
        Lc = dv.lum(co)
        rho = np.where(Lc > 0, dv.lum(out) / Lc, F(1.0)).astype(F)
        return out, vo * (rho * rho)


def atrous_demod(mean, var, asum, n, pos, nrm, geom, levels, sigma_lum, sigma_normal, sigma_position, eps=MIN_ALBEDO):
    """the demodulated filter over an (H, W, 3) colour and its (H, W) variance: k_demodulate, denoise_var_ref.atrous_var's levels, the
    remodulating store -> (colour (H, W, 3), variance (H, W))"""
    cd, vd = demodulate(mean, var, asum, n, eps)
    co, vo = dv.atrous_var(cd, vd, pos, nrm, geom, levels, sigma_lum, sigma_normal, sigma_position)
    return remodulate(co, vo, asum, n, eps)


def denoise_var_demod(rgb_sum, lum_sq_sum, asum, samples, pos, nrm, geom, levels, sigma_lum, sigma_normal, sigma_position, eps=MIN_ALBEDO):
    """pt_denoise_var under PT_FLAG_DEMODULATE at samples >= 2: the two accumulators and the albedo sums -> (the filtered mean, its variance)"""
    c, v = dv.mean_and_variance(rgb_sum, lum_sq_sum, samples)
    return atrous_demod(c, v, asum, samples, pos, nrm, geom, levels, sigma_lum, sigma_normal, sigma_position, eps)
