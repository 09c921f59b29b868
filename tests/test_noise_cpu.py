"""The noise statistics of 16 x 16 tiles and the rule pt_iterate_until stops by, on the host (no GPU): the C ABI's new symbols, struct sizes
and refusal before pt_init, the exact properties of the numpy float32 restatement (tests/noise_ref.py), and -- on the CPU oracle's Cornell
-- that the tile criterion follows the 1 / sqrt(n) law, is calibrated and never goes backwards, where a per-pixel criterion does."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_var_ref as dv
import noise_ref as nr
from conftest import ROOT, SCENES

F = np.float32
FLOOR = 0.05


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_struct_sizes_and_refusal_before_init(pt):
    hdr = open(os.path.join(ROOT, "include", "pt_amd.h")).read()
    thdr = open(os.path.join(ROOT, "include", "pt_amd_test.h")).read()
    for s in ("pt_noise_stats", "pt_iterate_until"):
        assert re.search(r"\bint %s\(" % s, hdr), s
        assert s in pt.ABI_SYMBOLS and hasattr(pt.lib(), s)
    assert len(pt.ABI_SYMBOLS) == 47 and len(set(pt.ABI_SYMBOLS)) == 47
    assert re.search(r"\bint pt_test_noise_stats\(", thdr)
    assert "pt_test_noise_stats" in pt.TEST_ABI_SYMBOLS and hasattr(pt.test_lib(), "pt_test_noise_stats") and not hasattr(pt.lib(), "pt_test_noise_stats")
    assert re.search(r"#define PT_NOISE_TILE 16\b", hdr) and pt.PT_NOISE_TILE == 16 == nr.TILE
    assert C.sizeof(pt.PtNoiseStats) == 40 and C.sizeof(pt.PtNoiseTarget) == 28
    for name, cls in (("PtNoiseStats", pt.PtNoiseStats), ("PtNoiseTarget", pt.PtNoiseTarget)):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S)
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert re.findall(r"\b(\w+)\s*[,;]", body) == [f[0] for f in cls._fields_]
    assert pt.lib().pt_abi_version() == 7                   # additive: the version stays
    L, T = pt.lib(), pt.test_lib()
    L.pt_free()
    T.pt_free()
    st, done = pt.PtNoiseStats(), C.c_int32(-5)
    tgt = pt.PtNoiseTarget(1.0, FLOOR, 0.0, 2, 16, 8, 1)
    tm = np.zeros(12, F)
    assert L.pt_noise_stats(4, 1.0, FLOOR, C.byref(st), C.sizeof(st), tm.ctypes.data_as(C.c_void_p)) == -2            # PT_ERR_NOT_INIT
    assert b"before pt_init" in L.pt_last_error()
    assert L.pt_iterate_until(0, 1, C.byref(tgt), C.sizeof(tgt), C.byref(st), C.byref(done)) == -2
    assert b"before pt_init" in L.pt_last_error()
    assert not tm.any() and done.value == -5 and st.tiles == 0


# ---- exact properties of the restatement ---------------------------------------------------------------------------------------------
def test_one_tile_by_hand_in_float64():
    """16 x 16 pixels of n = 4 samples each whose values are small dyadic fractions, so that every fp32 operation up to the tile sums is exact
    and float64 arithmetic gives the same V and M; the quotients then round once each."""
    rng = np.random.default_rng(11)
    n = 4
    samples = [np.repeat(rng.integers(0, 9, (16, 16, 1)), 3, axis=2).astype(F) / F(4) for _ in range(n)]     # grey: lum(c) = c to rounding
    S = np.zeros((16, 16, 3), F)
    for s in samples:
        S = S + s
    Q = dv.moments(samples)
    r = nr.tile_rel_var(S, Q, n, FLOOR)
    assert r.shape == (1, 1)
    # float64, the textbook way: per pixel the unbiased variance of the mean of the samples' luminance
    l = np.stack([dv.lum(s).astype(np.float64) for s in samples])
    v = l.var(axis=0, ddof=0) / (n - 1)
    want = v.mean() / max(l.mean(), FLOOR) ** 2
    assert abs(float(r[0, 0]) / want - 1) < 1e-5
    st = nr.stats(S, Q, n, np.sqrt(want) * 1.01, FLOOR)
    assert st["unconverged"] == 0 and st["converged"] and st["tiles"] == 1 and _bits(st["max_rel_var"]) == _bits(r[0, 0])
    st = nr.stats(S, Q, n, np.sqrt(want) * 0.99, FLOOR)
    assert st["unconverged"] == 1 and not st["converged"]
    assert nr.stats(S, Q, n, np.sqrt(want) * 0.99, FLOOR, fraction=1.0)["converged"]


def test_the_butterfly_is_not_a_row_major_sum():
    """Values spread over 24 binary orders of magnitude: the order of the additions shows in the bits.  The butterfly written out by hand --
    six rounds of pairwise sums, partners 32, 16, 8, 4, 2, 1 lanes apart, then (w0 + w1) + (w2 + w3) -- against noise_ref, and both against the
    row-major sum, which must differ."""
    rng = np.random.default_rng(5)
    a = (rng.uniform(1, 2, (16, 16)) * 2.0 ** rng.integers(-12, 12, (16, 16))).astype(F)
    waves = []
    for w in range(4):
        lanes = [a[4 * w + (l >> 4), l & 15] for l in range(64)]
        for o in (32, 16, 8, 4, 2, 1):
            lanes = [F(lanes[l] + lanes[l ^ o]) for l in range(64)]
        assert len({_bits(x).item() for x in lanes}) == 1          # every lane holds the same bits
        waves.append(lanes[0])
    want = F(F(waves[0] + waves[1]) + F(waves[2] + waves[3]))
    got = nr.tile_sum(a.reshape(1, 1, 16, 16))[0, 0]
    assert _bits(got) == _bits(want)
    row_major = F(0)
    for x in a.reshape(-1):
        row_major = F(row_major + x)
    assert _bits(row_major) != _bits(want)
    # ... and through tile_rel_var: Q chosen so that v = a exactly (S = 0: L = 0, d = Q / n, v = d / (n - 1) with n = 2)
    r = nr.tile_rel_var(np.zeros((16, 16, 3), F), a * F(2), 2, 1.0)
    assert _bits(r[0, 0]) == _bits(F(want / F(256)) / F(1.0))


@pytest.mark.parametrize("w,h", [(72, 40), (33, 17), (1, 1)])
def test_partial_tiles_count_their_own_pixels_and_padding_adds_nothing(w, h):
    """A frame of equal pixels: every tile's r is the pixel's own v / max(L, floor)^2 up to the rounding of the sums, whatever part of the tile
    lies inside the frame (N = its pixel count); and a tile's r equals the r of the same pixels embedded alone in a frame of their own."""
    tx, ty = nr.tiles_of(w, h)
    assert (tx, ty) == (-(-w // 16), -(-h // 16))
    S = np.full((h, w, 3), 6.0, F)          # n = 4: c = 1.5, L = 1.5 (the weights sum to 1 within rounding)
    Q = np.full((h, w), 4 * 2.5, F)         # Q / n = 2.5
    r = nr.tile_rel_var(S, Q, 4, FLOOR)
    assert r.shape == (ty, tx)
    _, v = dv.mean_and_variance(S[:1, :1], Q[:1, :1], 4)
    L = dv.lum(S[:1, :1] / F(4))
    one = float(v[0, 0]) / float(L[0, 0]) ** 2
    assert np.max(np.abs(r.astype(np.float64) / one - 1)) < 1e-5          # N is the tile's own count: no tile is diluted by its padding
    rng = np.random.default_rng(w * 100 + h)
    S = rng.uniform(0, 8, (h, w, 3)).astype(F)
    Q = rng.uniform(0, 40, (h, w)).astype(F)
    r = nr.tile_rel_var(S, Q, 4, FLOOR)
    for j in range(ty):
        for i in range(tx):
            ys, xs = slice(16 * j, min(16 * j + 16, h)), slice(16 * i, min(16 * i + 16, w))
            alone = nr.tile_rel_var(S[ys, xs], Q[ys, xs], 4, FLOOR)
            assert alone.shape == (1, 1) and _bits(alone[0, 0]) == _bits(r[j, i])
    # the padding holds +0: a tile of negative zeros sums to -0 only without it
    assert _bits(nr.tile_sum(np.zeros((1, 1, 16, 16), F)))[0, 0] == 0


def special_frame():
    """48 x 16, n = 2, floor 0.05: tile 0 NaN and inf in S (L = NaN: the floor takes over; d = NaN: 0) beside ordinary pixels, tile 1 an
    infinite Q (v = inf: r = inf, flagged, the maximum) , tile 2 denormal S and Q."""
    rng = np.random.default_rng(2)
    S = rng.uniform(0, 2, (16, 48, 3)).astype(F)
    Q = rng.uniform(2, 6, (16, 48)).astype(F)
    S[3, 5] = (np.nan, 1.0, 1.0)
    S[4, 6] = (np.inf, 1.0, 1.0)
    S[5, 7] = (-np.inf, 0.0, 0.0)
    Q[6, 8] = np.nan
    Q[2, 20] = np.inf
    S[:, 32:] = rng.uniform(1, 100, (16, 16, 3)).astype(F) * F(1e-42)
    Q[:, 32:] = rng.uniform(1, 100, (16, 16)).astype(F) * F(1e-42)
    return S, Q


def test_nan_inf_and_denormal_inputs():
    S, Q = special_frame()
    r = nr.tile_rel_var(S, Q, 2, FLOOR)
    # tile 0: the luminance sum holds inf + -inf and a NaN: ml is NaN, the floor is taken; the variances are finite (a NaN d gives 0)
    assert np.isfinite(r[0, 0]) and r[0, 0] > 0
    _, v = dv.mean_and_variance(S[:, :16], Q[:, :16], 2)
    assert np.isfinite(v).all() and v[3, 5] == 0 and v[6, 8] == 0
    assert _bits(r[0, 0]) == _bits(F(nr.tile_sum(v.reshape(1, 1, 16, 16))[0, 0] / F(256)) / (F(FLOOR) * F(FLOOR)))
    # tile 1: one infinite variance makes the tile's ratio infinite
    assert np.isposinf(r[0, 1])
    # tile 2: denormal inputs are not flushed: the sums and the quotient by N stay denormal and non-zero, the floor is the divisor
    assert 0 < r[0, 2] < 1e-35
    st = nr.stats(S, Q, 2, 1.0, FLOOR)
    assert st["unconverged"] == 2 and np.isposinf(st["max_rel_var"])          # tile 0 (r ~ 500) and tile 1; tile 2 passes
    # a NaN ratio (inf / inf: an infinite variance in a tile of infinite mean luminance) is neither flagged nor the maximum
    S2, Q2 = S.copy(), Q.copy()
    S2[:, 16:32] = 0
    S2[3, 21] = (np.inf, np.inf, np.inf)          # (pixel (2, 20) keeps its infinite Q: V = inf, and now M = inf)
    r2 = nr.tile_rel_var(S2, Q2, 2, FLOOR)
    assert np.isnan(r2[0, 1])
    st2 = nr.stats(S2, Q2, 2, 1.0, FLOOR)
    assert st2["unconverged"] == 1 and _bits(st2["max_rel_var"]) == _bits(r2[0, 0])


def test_the_stopping_rule():
    conv = lambda at: (lambda s: s >= at)
    assert nr.samples_done(conv(20), 1, 2, 96, 8, 0) == (24, True)
    assert nr.samples_done(conv(20), 1, 2, 96, 8, 1) == (32, True)
    assert nr.samples_done(conv(20), 1, 40, 96, 8, 0) == (40, True)          # min_samples delays the first check
    assert nr.samples_done(conv(90), 1, 2, 92, 8, 0) == (92, True)           # the last round is cut at the cap, and checked
    assert nr.samples_done(conv(90), 1, 2, 92, 8, 1) == (92, True)
    assert nr.samples_done(conv(100), 1, 2, 92, 8, 1) == (92, False)
    assert nr.samples_done(conv(0), 17, 2, 96, 8, 0) == (24, True)           # rounds start at first_iter - 1 = 16
    assert nr.samples_done(conv(0), 1, 50, 40, 8, 1) == (40, False)          # never checked: never converged
    assert nr.is_converged(3, 15, 0.2) and not nr.is_converged(4, 15, 0.2) and nr.is_converged(0, 15, 0.0) and not nr.is_converged(1, 15, 0.0)


# ---- the criterion on the CPU oracle's Cornell --------------------------------------------------------------------------------------
W, H, CAP, STEP, LONG = 72, 40, 192, 8, 2048


def _lum64(c):
    return (0.2126 * c[..., 0] + 0.7152 * c[..., 1]) + 0.0722 * c[..., 2]


@pytest.fixture(scope="module")
def cornell(oracle):
    """Cornell 72 x 40, depth 8: the accumulators S and Q after 8, 16, ..., 192 iterations (Q from every iteration taken singly into a zeroed
    accumulator), and the mean of iterations 1..2048 as the reference."""
    sc = oracle.Scene(os.path.join(SCENES, "cornell.txt"))
    sc.set_resolution(W, H)
    ref = oracle.Renderer(sc.camera, sc.geoms, sc.materials, 8)
    acc = np.zeros(W * H * 3, F)
    Q = np.zeros((H, W), F)
    at = {}
    for it in range(1, CAP + 1):
        one = np.zeros(W * H * 3, F)
        ref.iterate(it, one)
        l = dv.lum(one.reshape(H, W, 3))
        Q = Q + l * l
        ref.iterate(it, acc)
        if it % STEP == 0:
            at[it] = (acc.reshape(H, W, 3).copy(), Q.copy())
    for it in range(CAP + 1, LONG + 1):
        ref.iterate(it, acc)
    return at, (acc.astype(np.float64) / LONG).reshape(H, W, 3)


def _lit(cornell):
    """the tiles whose converged mean luminance lies above the floor: where r is relative to the tile's own light"""
    _, ref = cornell
    L = _lum64(ref)
    tx, ty = nr.tiles_of(W, H)
    out = np.zeros((ty, tx), bool)
    for j in range(ty):
        for i in range(tx):
            out[j, i] = L[16 * j:16 * j + 16, 16 * i:16 * i + 16].mean() > FLOOR
    return out


def test_the_tile_error_follows_one_over_sqrt_n(cornell):
    """The median lit tile's sqrt(r) at 64 samples over that at 16: 1 / sqrt(4) = 0.5 by the law; measured 0.495 (1.25 -> 0.62 over the six tiles whose converged mean luminance lies above the floor)."""
    at, _ = cornell
    lit = _lit(cornell)
    assert lit.sum() >= 4
    m16 = float(np.median(np.sqrt(nr.tile_rel_var(*at[16], 16, FLOOR)[lit])))
    m64 = float(np.median(np.sqrt(nr.tile_rel_var(*at[64], 64, FLOOR)[lit])))
    print("median lit-tile relative standard error: %.3f at 16 samples, %.3f at 64, ratio %.3f" % (m16, m64, m64 / m16))
    assert 0.4 <= m64 / m16 <= 0.6


def test_the_tile_estimate_is_calibrated(cornell):
    """16 samples, every lit tile: the estimated variance of the tile's luminance SUM, the sum of its pixels' v, against the sum of its pixels'
    squared luminance error (reference: the mean of iterations 1..2048) -- both sides of r's numerator times N.  Measured 0.84 .. 1.33."""
    at, ref = cornell
    S, Q = at[16]
    _, v = dv.mean_and_variance(S, Q, 16)
    err2 = (dv.lum(S / F(16)).astype(np.float64) - _lum64(ref)) ** 2
    lit = _lit(cornell)
    ratios = []
    for j, i in zip(*np.nonzero(lit)):
        ys, xs = slice(16 * j, 16 * j + 16), slice(16 * i, 16 * i + 16)
        ratios.append(float(v[ys, xs].astype(np.float64).sum() / err2[ys, xs].sum()))
    print("estimate / true squared error over %d lit tiles: %.3f .. %.3f" % (len(ratios), min(ratios), max(ratios)))
    assert 0.5 <= min(ratios) and max(ratios) <= 2.0


THRESHOLDS = (2.0, 1.5, 1.0, 0.75)


def test_the_unconverged_count_never_rises_and_where_it_reaches_zero(cornell):
    """Checks every 8 samples up to 192, floor 0.05: at thresholds 2.0, 1.5, 1.0 and 0.75 the count of unconverged tiles never rises from one
    check to the next, and the first converged checks (no tile above) are 16, 24, 40 and 64 samples."""
    at, _ = cornell
    first = []
    for thr in THRESHOLDS:
        counts = [nr.stats(*at[s], s, thr, FLOOR)["unconverged"] for s in range(STEP, CAP + 1, STEP)]
        print("threshold %.2f: unconverged tiles per check %s" % (thr, counts))
        assert all(b <= a for a, b in zip(counts, counts[1:])), thr
        done, ok = nr.samples_done(lambda s: nr.stats(*at[s], s, thr, FLOOR)["converged"], 1, 2, CAP, STEP, 0)
        assert ok
        first.append(done)
    print("first converged checks:", first)
    assert first == [16, 24, 40, 64]


def test_a_per_pixel_criterion_goes_backwards(oracle):
    """Why tiles.  Cornell 64 x 48, depth 8, pixels whose relative standard error sqrt(v) / max(L, 0.05) is at or above 0.25: 213 at 2 samples,
    420 at 4, 1121 at 16, 1794 at 64 of 3072 -- the count GROWS with the sample count, because a pixel whose samples all missed the small light
    has variance exactly 0 and looks converged (2855 pixels at 2 samples) until a sample finds the light.  A loop that stops when few pixels
    are flagged would stop at once.  A tile's summed variance is an unbiased estimate of the variance of its summed luminance, however few of
    its pixels have seen the light, and falls as 1 / n (the tests above)."""
    w, h = 64, 48
    sc = oracle.Scene(os.path.join(SCENES, "cornell.txt"))
    sc.set_resolution(w, h)
    ref = oracle.Renderer(sc.camera, sc.geoms, sc.materials, 8)
    acc = np.zeros(w * h * 3, F)
    Q = np.zeros((h, w), F)
    over, zero = {}, {}
    for it in range(1, 65):
        one = np.zeros(w * h * 3, F)
        ref.iterate(it, one)
        l = dv.lum(one.reshape(h, w, 3))
        Q = Q + l * l
        ref.iterate(it, acc)
        if it in (2, 4, 16, 64):
            c, v = dv.mean_and_variance(acc.reshape(h, w, 3), Q, it)
            rse = np.sqrt(v.astype(np.float64)) / np.maximum(dv.lum(c).astype(np.float64), FLOOR)
            over[it] = int((rse >= 0.25).sum())
            zero[it] = int((v == 0).sum())
    print("pixels at or above 0.25:", over, " pixels of variance 0:", zero)
    assert over[2] < over[4] < over[16] < over[64]
    assert zero[2] > (w * h) // 2
