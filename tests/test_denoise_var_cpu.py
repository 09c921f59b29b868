"""Per-pixel variance and the variance-guided a-trous filter on the host (no GPU): the C ABI's new symbols and their refusal before pt_init,
the exact properties of the numpy float32 restatement (tests/denoise_var_ref.py), that the variance estimate is calibrated, and what the
filter is for: ONE setting that helps at every sample count and keeps converged detail, where pt_denoise's global sigma_color does not."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_ref as dr
import denoise_var_ref as dv
from conftest import ROOT, SCENES

F = np.float32
# the filter's setting in every quality test, unchanged between sample counts, and pt_denoise's at the README's
LEVELS, SIGMA_LUM, SIGMA_NORMAL, SIGMA_POSITION = 5, 4.0, 0.35, 2.0
PLAIN = (2.0, 0.35, 2.0)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_struct_and_refusal_before_init(pt):
    hdr = open(os.path.join(ROOT, "include", "pt_amd.h")).read()
    thdr = open(os.path.join(ROOT, "include", "pt_amd_test.h")).read()
    for s in ("pt_readback_moments", "pt_variance", "pt_denoise_var", "pt_denoise_var_rgba8"):
        assert re.search(r"\bint %s\(" % s, hdr), s
        assert s in pt.ABI_SYMBOLS and hasattr(pt.lib(), s)
    assert re.search(r"\bint pt_test_denoise_var\(", thdr)
    assert "pt_test_denoise_var" in pt.TEST_ABI_SYMBOLS and hasattr(pt.test_lib(), "pt_test_denoise_var") and not hasattr(pt.lib(), "pt_test_denoise_var")
    assert re.search(r"PT_FLAG_MOMENTS = 32\b", hdr) and pt.PT_FLAG_MOMENTS == 32
    assert C.sizeof(pt.PtDenoiseVarParams) == 20
    m = re.search(r"typedef struct PtDenoiseVarParams \{(.*?)\} PtDenoiseVarParams;", hdr, re.S)
    names = ["levels", "guide_iter", "sigma_lum", "sigma_normal", "sigma_position"]
    assert m and re.findall(r"\b(levels|guide_iter|sigma_lum|sigma_normal|sigma_position)\b[,;]", m.group(1)) == names
    assert [f[0] for f in pt.PtDenoiseVarParams._fields_] == names
    assert pt.lib().pt_abi_version() == 7                   # additive: the version stays
    L, T = pt.lib(), pt.test_lib()
    L.pt_free()
    T.pt_free()
    prm = pt.PtDenoiseVarParams(5, 1, 4.0, 1.0, 1.0)
    out = np.zeros(12, F)
    assert L.pt_readback_moments(_vp(out)) == -2            # PT_ERR_NOT_INIT
    assert b"before pt_init" in L.pt_last_error()
    assert L.pt_variance(4, _vp(out)) == -2
    assert L.pt_denoise_var(4, C.byref(prm), C.sizeof(prm), _vp(out), _vp(out)) == -2
    assert L.pt_denoise_var_rgba8(4, C.byref(prm), C.sizeof(prm), _vp(out)) == -2
    assert T.pt_test_denoise_var(4, C.byref(prm), C.sizeof(prm), 0, _vp(out), _vp(out), None) == -2
    assert not out.any()


# ---- exact properties of the restatement ---------------------------------------------------------------------------------------------
def _random_guides(rng, h, w, misses=True):
    pos = rng.normal(0, 3, (h, w, 3)).astype(F)
    nrm = rng.normal(0, 1, (h, w, 3)).astype(F)
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True).astype(F)
    geom = rng.integers(-1 if misses else 0, 4, (h, w)).astype(np.int32)
    pos[geom < 0] = 0
    nrm[geom < 0] = 0
    return pos, nrm, geom


def test_moments_and_variance_by_hand():
    s = [np.array([[1.0, 0.5, 0.25]], F), np.array([[0.0, 0.0, 0.0]], F), np.array([[2.0, 2.0, 2.0]], F)]
    l = [(F(0.2126) * x[:, 0] + F(0.7152) * x[:, 1]) + F(0.0722) * x[:, 2] for x in s]
    q = (l[0] * l[0] + F(0)) + l[2] * l[2]
    assert np.array_equal(_bits(dv.moments(s)), _bits(q))
    S = (s[0] + s[1]) + s[2]
    c = S / F(3)
    L = (F(0.2126) * c[:, 0] + F(0.7152) * c[:, 1]) + F(0.0722) * c[:, 2]
    assert np.array_equal(_bits(dv.variance(S, q, 3)), _bits((q / F(3) - L * L) / F(2)))
    # equal samples: no spread -- rounding may leave Q / n a hair below L * L, which the clamp takes; a NaN gives 0 too
    assert dv.variance(np.array([[3.0, 3.0, 3.0]], F), dv.moments([np.ones((1, 3), F)] * 3), 3)[0] <= 2e-7
    assert _bits(dv.variance(np.array([[np.nan, 1.0, 1.0]], F), np.array([1.0], F), 2))[0] == 0


@pytest.mark.parametrize("value", [(0.25, 0.5, 2.0), (1.0, 0.0, 2.0 ** -20), (4.0, 4.0, 4.0)])
def test_constant_image_is_a_fixed_point_bit_for_bit(value):
    """Equal colours give dl = 0, so a pixel's weights do not depend on the channel -- nor on the variance image, whatever it holds -- and a
    channel whose value is a power of two (or 0) comes back exactly (tests/test_denoise_cpu.py has the argument)."""
    rng = np.random.default_rng(1)
    for h, w, levels in ((23, 41, 5), (9, 257, 3), (5, 5, 4), (1, 1, 2)):
        pos, nrm, geom = _random_guides(rng, h, w)
        img = np.broadcast_to(np.array(value, F), (h, w, 3)).copy()
        var = rng.uniform(0, 3, (h, w)).astype(F) * (rng.uniform(0, 1, (h, w)) < 0.8)          # (some exact zeros among them)
        for sigmas in ((4.0, 0.5, 2.0), (np.inf, 0.1, 0.1), (0.01, np.inf, 0.3)):
            out, v = dv.atrous_var(img, var, pos, nrm, geom, levels, *sigmas)
            assert np.array_equal(_bits(out), _bits(img))
            assert np.isfinite(v).all() and (v >= 0).all()


def test_infinite_sigmas_give_the_b3_spline_blur_and_its_variance():
    """All three terms off: every tap's w is hw itself (expNegPoly(0) = 1), the colours are the renormalised B3 blur (denoise_ref's bound), and
    v' = sum hw^2 v / (sum hw)^2.  There hw * hw, the sum of the hw and its square are exact (dyadic fractions of at most 17 bits), so a level
    rounds each of the at most 25 products v * hw^2, each of the 25 additions of non-negative terms, and the division: a relative error of at
    most 51 * 2^-24 per level to first order; 52 to cover the second."""
    rng = np.random.default_rng(3)
    h, w, levels = 19, 30, 3
    img = rng.uniform(0, 4, (h, w, 3)).astype(F)
    var = rng.uniform(0, 2, (h, w)).astype(F)
    pos, nrm, geom = _random_guides(rng, h, w, misses=False)
    got, gotv = dv.atrous_var(img, var, pos, nrm, geom, levels, np.inf, np.inf, np.inf)
    want, wantv = img.astype(np.float64), var.astype(np.float64)
    k = np.array([1, 4, 6, 4, 1], np.float64) / 16
    for i in range(levels):
        s = 1 << i
        num, numv, den = np.zeros_like(want), np.zeros((h, w)), np.zeros((h, w))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                kk = k[dy + 2] * k[dx + 2]
                y0, y1 = max(0, -dy * s), min(h, h - dy * s)
                x0, x1 = max(0, -dx * s), min(w, w - dx * s)
                if y0 < y1 and x0 < x1:
                    num[y0:y1, x0:x1] += kk * want[y0 + dy * s:y1 + dy * s, x0 + dx * s:x1 + dx * s]
                    numv[y0:y1, x0:x1] += kk * kk * wantv[y0 + dy * s:y1 + dy * s, x0 + dx * s:x1 + dx * s]
                    den[y0:y1, x0:x1] += kk
        want, wantv = num / den[..., None], numv / (den * den)
    assert np.max(np.abs(got - want)) < 4 * 25 * levels * 2.0 ** -24        # fp32 sums of 25 terms in [0, 4), `levels` times
    assert np.max(np.abs(gotv / wantv - 1)) <= levels * 52 * 2.0 ** -24
    # the same colours as the plain filter's blur, bit for bit: the colour sums are the same operations
    assert np.array_equal(_bits(got), _bits(dr.atrous(img, pos, nrm, geom, levels, np.inf, np.inf, np.inf)))
    # sigma_lum = +inf switches the term off wherever the variance is 0 as well (inf * 0 is never formed)
    got0, _ = dv.atrous_var(img, np.zeros((h, w), F), pos, nrm, geom, levels, np.inf, np.inf, np.inf)
    assert np.array_equal(_bits(got0), _bits(got))


def test_hit_and_miss_never_mix():
    h, w = 12, 16
    geom = np.zeros((h, w), np.int32)
    geom[:, 8:] = -1
    img = np.zeros((h, w, 3), F)
    img[:, 8:] = 1.0
    var = np.zeros((h, w), F)
    var[:, 8:] = 1.0
    z = np.zeros((h, w, 3), F)
    out, v = dv.atrous_var(img, var, z, z, geom, 3, np.inf, np.inf, np.inf)
    assert np.array_equal(_bits(out), _bits(img))
    assert (v[:, :8] == 0).all() and (v[:, 8:] > 0).all()     # no variance crosses the border, neither in the prefilter nor in the taps
    # ... with a finite sigma_lum too: a hit's scale never sees the misses' variance (g stays 0: only equal colours pass)
    out, v = dv.atrous_var(img, var, z, z, geom, 3, 4.0, np.inf, np.inf)
    assert np.array_equal(_bits(out), _bits(img)) and (v[:, :8] == 0).all() and (v[:, 8:] > 0).all()


# ---- calibration and quality: Cornell on the CPU oracle ---------------------------------------------------------------------------------
W, H = 64, 48


def _rmse(a, ref):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - ref) ** 2)))


@pytest.fixture(scope="module")
def cornell(oracle):
    """Cornell 64 x 48, depth 8: iterations 1..64 taken singly (each into a zeroed accumulator), the accumulators S and Q after 4, 16 and 64
    of them, the mean of iterations 1..512 as the reference, and iteration 1's guides."""
    sc = oracle.Scene(os.path.join(SCENES, "cornell.txt"))
    sc.set_resolution(W, H)
    ref = oracle.Renderer(sc.camera, sc.geoms, sc.materials, 8)
    acc = np.zeros(W * H * 3, F)
    singles, at = [], {}
    for it in range(1, 65):
        one = np.zeros(W * H * 3, F)
        ref.iterate(it, one)
        singles.append(one.reshape(H, W, 3))
        ref.iterate(it, acc)
        if it in (4, 16, 64):
            at[it] = (acc.reshape(H, W, 3).copy(), dv.moments(singles))
    for it in range(65, 513):
        ref.iterate(it, acc)
    converged = (acc / F(512)).reshape(H, W, 3).astype(np.float64)
    pos_t, nrm, geom = dr.oracle_guides(oracle, ref, 1)
    guides = (pos_t[:, :3].reshape(H, W, 3), nrm.reshape(H, W, 3), geom.reshape(H, W))
    return at, converged, guides


def test_the_variance_estimate_is_calibrated(cornell):
    """16 iterations: the frame mean of variance() against the mean squared luminance error of the 16-sample mean (reference: iterations
    1..512) -- 0.02023 against 0.01893, a ratio of 1.069.  A wrong divisor (n, n - 1, a missing square) is off by a factor of 4 or more."""
    at, converged, _ = cornell
    S, Q = at[16]
    v = dv.variance(S, Q, 16).astype(np.float64)
    err = dv.lum(S / F(16)).astype(np.float64) - ((0.2126 * converged[..., 0] + 0.7152 * converged[..., 1]) + 0.0722 * converged[..., 2])
    est, mse = float(v.mean()), float((err ** 2).mean())
    print("mean estimated variance of the mean luminance %.5f, mean squared luminance error %.5f, ratio %.3f" % (est, mse, est / mse))
    assert 0.5 <= est / mse <= 2.0


@pytest.mark.parametrize("n", [4, 64])
def test_guided_cornell_beats_the_unfiltered_and_the_plain_filter(cornell, n):
    """RMSE against the mean of iterations 1..512, one setting (sigma_lum 4, sigma_normal 0.35, sigma_position 2.0, 5 levels) for both counts:
        n = 4:   unfiltered 0.28806, pt_denoise at the README's (2.0, 0.35, 2.0) 0.15602, guided 0.11816
        n = 64:  unfiltered 0.06506, pt_denoise 0.04044, guided 0.03479"""
    at, converged, (pos, nrm, geom) = cornell
    S, Q = at[n]
    raw = _rmse(S / F(n), converged)
    plain = _rmse(dr.denoise(S, n, pos, nrm, geom, LEVELS, *PLAIN), converged)
    guided = _rmse(dv.denoise_var(S, Q, n, pos, nrm, geom, LEVELS, SIGMA_LUM, SIGMA_NORMAL, SIGMA_POSITION)[0], converged)
    print("n = %d: RMSE unfiltered %.5f, plain %.5f, guided %.5f" % (n, raw, plain, guided))
    assert guided < raw
    assert guided < plain


# ---- quality: converged detail survives -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 16, 64])
def test_guided_checkerboard_keeps_the_pattern_the_plain_filter_wipes_out(n):
    """A flat 0.25 / 0.75 checkerboard albedo in 8-pixel cells, RGB = (a, a / 2, 1 - a), samples = albedo x uniform(0, 2), planar guides; RMSE
    against the albedo, the same settings as on Cornell:
        n = 4:   unfiltered 0.14060, plain 0.20697, guided 0.08527
        n = 16:  unfiltered 0.07072, plain 0.20726, guided 0.02957
        n = 64:  unfiltered 0.03434, plain 0.20757, guided 0.00394
    The plain filter is WORSE than no filter at every count: the reason the variance-guided one exists."""
    yy, xx = np.mgrid[0:H, 0:W]
    a = np.where(((xx // 8) + (yy // 8)) % 2 == 0, 0.25, 0.75)
    albedo = np.stack([a, a / 2, 1 - a], axis=2).astype(F)
    rng = np.random.default_rng(7)
    samples = [albedo * rng.uniform(0, 2, (H, W, 1)).astype(F) for _ in range(n)]
    S = np.zeros((H, W, 3), F)
    for s in samples:
        S = S + s
    Q = dv.moments(samples)
    pos = np.stack([xx * 0.05, yy * 0.05, np.zeros((H, W))], axis=2).astype(F)
    nrm = np.broadcast_to(np.array([0, 0, 1], F), (H, W, 3)).copy()
    geom = np.zeros((H, W), np.int32)
    ref = albedo.astype(np.float64)
    raw = _rmse(S / F(n), ref)
    plain = _rmse(dr.denoise(S, n, pos, nrm, geom, LEVELS, *PLAIN), ref)
    guided = _rmse(dv.denoise_var(S, Q, n, pos, nrm, geom, LEVELS, SIGMA_LUM, SIGMA_NORMAL, SIGMA_POSITION)[0], ref)
    print("checkerboard n = %d: RMSE unfiltered %.5f, plain %.5f, guided %.5f" % (n, raw, plain, guided))
    assert guided < raw
    assert plain > raw
