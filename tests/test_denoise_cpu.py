"""The denoiser on the host (no GPU): the C ABI's new symbols and struct, the refusal before pt_init, and the numpy float32 restatement of
the filter (tests/denoise_ref.py) -- its range weight against the CPU oracle's pow_poly bit for bit, its exact properties, and what it is
for: a filtered 4-iteration Cornell frame is closer to the converged frame than the unfiltered one."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_ref as dr
from conftest import ROOT, SCENES

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_denoise_symbols_and_struct(pt):
    hdr = open(os.path.join(ROOT, "include", "pt_amd.h")).read()
    mp = open(os.path.join(ROOT, "project3-cuda-path-tracer_amd", "csrc", "pt_amd.map")).read()
    assert re.search(r"global:\s*pt_\*;", mp)             # the version script exports the header's pt_* names
    for s in ("pt_denoise", "pt_denoise_rgba8", "pt_gbuffer"):
        assert re.search(r"\bint %s\(" % s, hdr), s
        assert s in pt.ABI_SYMBOLS and hasattr(pt.lib(), s)
    for s in ("pt_test_denoise", "pt_test_exp_neg_poly"):
        assert s in pt.TEST_ABI_SYMBOLS and hasattr(pt.test_lib(), s) and not hasattr(pt.lib(), s)
    assert C.sizeof(pt.PtDenoiseParams) == 20
    assert [f[0] for f in pt.PtDenoiseParams._fields_] == ["levels", "guide_iter", "sigma_color", "sigma_normal", "sigma_position"]
    m = re.search(r"typedef struct PtDenoiseParams \{(.*?)\} PtDenoiseParams;", hdr, re.S)
    assert m and re.findall(r"\b(levels|guide_iter|sigma_color|sigma_normal|sigma_position)\b[,;]", m.group(1)) == \
        ["levels", "guide_iter", "sigma_color", "sigma_normal", "sigma_position"]
    assert pt.lib().pt_abi_version() == 7                   # additive: the version stays


def test_denoise_before_init_is_refused(pt):
    L = pt.lib()
    L.pt_free()
    prm = pt.PtDenoiseParams(5, 1, 1.0, 1.0, 1.0)
    out = np.zeros(12, F)
    assert L.pt_denoise(1, C.byref(prm), C.sizeof(prm), out.ctypes.data_as(C.c_void_p)) == -2          # PT_ERR_NOT_INIT
    assert b"before pt_init" in L.pt_last_error()
    assert L.pt_denoise_rgba8(1, C.byref(prm), C.sizeof(prm), out.ctypes.data_as(C.c_void_p)) == -2
    assert L.pt_gbuffer(1, out.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == -2
    assert not out.any()


# ---- expNegPoly ------------------------------------------------------------------------------------------------------------------------
def test_exp_neg_poly_equals_the_oracles_pow_poly(oracle):
    """For x = 0.5 pow_poly's logarithm is exactly -1: expNegPoly(a) == orc_pow(0.5, fl(a * 1.44269504)), bit for bit."""
    L = oracle.lib()
    rng = np.random.default_rng(20)
    a = np.concatenate([rng.uniform(0, 100, 3000), rng.uniform(0, 2, 1000), np.arange(0, 100, 0.5),
                        [0.0, 87.3, 87.4, 126 / 1.44269504, 1e-30, 1e-8]]).astype(F)
    e = a * F(1.44269504)
    want = np.array([L.orc_pow(0.5, float(v)) for v in e], F)
    got = dr.exp_neg_poly(a)
    assert got.dtype == F and np.array_equal(_bits(got), _bits(want))
    # ... and close to exp(-a) where the result is a normal number: the rounding of t = a * log2(e), |t| <= 126, moves the result by at most
    # 126 * 2^-24 * ln 2 = 5.2e-6 relative, the polynomial (pow_poly's own) by 2e-6
    big = want > 1e-37
    assert np.max(np.abs(got[big] / np.exp(-a[big].astype(np.float64)) - 1)) < 7.2e-6
    assert _bits(dr.exp_neg_poly(F(0.0)))[0] == _bits(F(1.0))[0]
    for huge in (1e3, 3e38, np.inf):
        assert _bits(dr.exp_neg_poly(F(huge)))[0] == 0
    assert _bits(dr.exp_neg_poly(F(np.nan)))[0] == 0


# ---- exact properties of the restatement ---------------------------------------------------------------------------------------------
def _random_guides(rng, h, w, misses=True):
    pos = rng.normal(0, 3, (h, w, 3)).astype(F)
    nrm = rng.normal(0, 1, (h, w, 3)).astype(F)
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True).astype(F)
    geom = rng.integers(-1 if misses else 0, 4, (h, w)).astype(np.int32)
    pos[geom < 0] = 0
    nrm[geom < 0] = 0
    return pos, nrm, geom


@pytest.mark.parametrize("value", [(0.25, 0.5, 2.0), (1.0, 0.0, 2.0 ** -20), (4.0, 4.0, 4.0)])
def test_constant_image_is_a_fixed_point_bit_for_bit(value):
    """Equal colours give dc = 0, so a pixel's weights are the same for every channel.  A channel whose value c is a power of two (or 0) makes
    every product c * w and every partial sum of them the exact c-fold of the weights' partial sum (scaling by a power of two commutes with
    rounding), so sumC / sumW returns c itself: a fixed point under ANY guides, frame shape and number of levels."""
    rng = np.random.default_rng(1)
    for h, w, levels in ((23, 41, 5), (9, 257, 3), (37, 70, 5), (5, 5, 4), (1, 1, 2)):
        pos, nrm, geom = _random_guides(rng, h, w)
        img = np.broadcast_to(np.array(value, F), (h, w, 3)).copy()
        out = dr.atrous(img, pos, nrm, geom, levels, 0.7, 0.5, 2.0)
        assert np.array_equal(_bits(out), _bits(img))
        out = dr.atrous(img, pos, nrm, geom, levels, np.inf, 0.1, 0.1)
        assert np.array_equal(_bits(out), _bits(img))


def test_constant_image_of_any_colour_stays_within_rounding():
    """A channel that is no power of two rounds in each of its (at most 25) products and sums: per level a relative error of at most
    (25 + 25 + 25 + 1) 2^-24 -- products, their sum, the weights' sum, the division."""
    rng = np.random.default_rng(2)
    h, w, levels = 23, 41, 5
    pos, nrm, geom = _random_guides(rng, h, w)
    img = np.broadcast_to(np.array([0.3, 0.75, 3.1], F), (h, w, 3)).copy()
    out = dr.atrous(img, pos, nrm, geom, levels, 0.7, 0.5, 2.0)
    assert np.max(np.abs(out.astype(np.float64) / img - 1)) <= levels * 76 * 2.0 ** -24


def test_infinite_sigmas_give_the_b3_spline_blur():
    """All three terms off: a = 0 for every tap, expNegPoly(0) = 1, and a level is the separable B3 kernel with holes, renormalised by the
    weight of the taps inside the frame."""
    rng = np.random.default_rng(3)
    h, w, levels = 19, 30, 3
    img = rng.uniform(0, 4, (h, w, 3)).astype(F)
    pos, nrm, geom = _random_guides(rng, h, w, misses=False)
    got = dr.atrous(img, pos, nrm, geom, levels, np.inf, np.inf, np.inf)
    want = img.astype(np.float64)
    k = np.array([1, 4, 6, 4, 1], np.float64) / 16
    for i in range(levels):
        s = 1 << i
        num, den = np.zeros_like(want), np.zeros((h, w))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                for y in range(h):
                    yy = y + dy * s
                    if not 0 <= yy < h:
                        continue
                    x0, x1 = max(0, -dx * s), min(w, w - dx * s)
                    if x0 < x1:
                        num[y, x0:x1] += k[dy + 2] * k[dx + 2] * want[yy, x0 + dx * s:x1 + dx * s]
                        den[y, x0:x1] += k[dy + 2] * k[dx + 2]
        want = num / den[..., None]
    assert np.max(np.abs(got - want)) < 4 * 25 * levels * 2.0 ** -24        # fp32 sums of 25 terms in [0, 4), `levels` times
    # a guide tensor that differs changes nothing while its sigma is infinite
    pos2, nrm2, _ = _random_guides(rng, h, w, misses=False)
    assert np.array_equal(_bits(dr.atrous(img, pos2, nrm2, geom, levels, np.inf, np.inf, np.inf)), _bits(got))


def test_hit_and_miss_never_mix():
    h, w = 12, 16
    geom = np.zeros((h, w), np.int32)
    geom[:, 8:] = -1
    img = np.zeros((h, w, 3), F)
    img[:, 8:] = 1.0
    z = np.zeros((h, w, 3), F)
    out = dr.atrous(img, z, z, geom, 3, np.inf, np.inf, np.inf)
    assert np.array_equal(_bits(out), _bits(img))


# ---- what it is for ----------------------------------------------------------------------------------------------------------------------
def test_filtered_cornell_is_closer_to_the_converged_frame(oracle):
    """Cornell 64 x 48, depth 8, all on the CPU oracle: the 4-iteration mean filtered by the restatement (guides from camera_ray + intersect
    of iteration 1; levels 5, sigma_color 2.0, sigma_normal 0.35, sigma_position 2.0 -- chosen by trying sigma_color 0.3 .. inf and
    sigma_position 0.5 .. 2 on this frame; every one of them lowers the error) against the 256-iteration mean:
        RMSE unfiltered 0.28699, filtered 0.15661."""
    W, H = 64, 48
    sc = oracle.Scene(os.path.join(SCENES, "cornell.txt"))
    sc.set_resolution(W, H)
    ref = oracle.Renderer(sc.camera, sc.geoms, sc.materials, 8)
    acc = np.zeros(W * H * 3, F)
    for it in range(1, 5):
        ref.iterate(it, acc)
    acc4 = acc.copy()
    for it in range(5, 257):
        ref.iterate(it, acc)
    converged = (acc / F(256)).reshape(H, W, 3).astype(np.float64)
    pos_t, nrm, geom = dr.oracle_guides(oracle, ref, 1)
    assert (geom >= 0).any() and (geom < 0).any()
    out = dr.denoise(acc4.reshape(H, W, 3), 4, pos_t[:, :3].reshape(H, W, 3), nrm.reshape(H, W, 3), geom.reshape(H, W), 5, 2.0, 0.35, 2.0)

    def rmse(a):
        return float(np.sqrt(np.mean((a.astype(np.float64) - converged) ** 2)))

    raw, filtered = rmse(acc4.reshape(H, W, 3) / F(4)), rmse(out)
    print("RMSE against 256 iterations: unfiltered %.5f, filtered %.5f" % (raw, filtered))
    assert filtered < raw
