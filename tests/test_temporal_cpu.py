"""Temporal reprojection on the host (no GPU): the flag, the test entry points and pt_init's refusals; the exact properties of the numpy
float32 restatement (tests/temporal_ref.py) -- the projection inverts the camera rays, no history is meanAndVariance to the bit, a constant is a
fixed point, every tap condition rejects alone, the cap holds --; and the study on the CPU oracle that chooses the constants of
include/pt_amd.h and gives the README's numbers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_ref as dr
import denoise_var_ref as dv
import temporal_ref as tr
from conftest import ROOT, SCENES

F = np.float32
EPS = 2.0 ** -24
LEVELS, SIGMA_LUM, SIGMA_NORMAL, SIGMA_POSITION = 5, 4.0, 0.35, 2.0


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_flag_constants_entry_points_and_refusals(pt):
    hdr = open(os.path.join(ROOT, "include", "pt_amd.h")).read()
    thdr = open(os.path.join(ROOT, "include", "pt_amd_test.h")).read()
    assert re.search(r"PT_FLAG_TEMPORAL = 64\b", hdr) and pt.PT_FLAG_TEMPORAL == 64
    assert tuple(float(c) for c in tr.constants()) == tuple(float(F(c)) for c in (pt.PT_TEMPORAL_MAX_HISTORY, pt.PT_TEMPORAL_NORMAL_DOT,
                                                                                   pt.PT_TEMPORAL_PLANE_FRACTION, pt.PT_TEMPORAL_MIN_WEIGHT))
    for s in ("pt_test_temporal", "pt_test_temporal_camera", "pt_test_history"):
        assert re.search(r"\bint %s\(" % s, thdr) and s in pt.TEST_ABI_SYMBOLS and hasattr(pt.test_lib(), s) and not hasattr(pt.lib(), s)
    assert pt.lib().pt_abi_version() == 7                   # a flag and documented behaviour: no function, no struct, the version stays
    assert len(pt.ABI_SYMBOLS) == 47
    # pt_init's refusals, as the planner gives them without a device; every other combination is planned as before
    sc = pt.Scene(os.path.join(SCENES, "cornell.txt"))
    sc.set_resolution(32, 24)
    T, M = pt.PT_FLAG_TEMPORAL, pt.PT_FLAG_MOMENTS
    for bad in (dict(flags=T), dict(flags=T | M | pt.PT_FLAG_TRACE_AHEAD, max_batch=4), dict(flags=T | M | pt.PT_FLAG_TRACE_AHEAD),
                dict(flags=T | M, lens_radius=0.1, focal_distance=5.0), dict(flags=T | M, shard_count=2), dict(flags=T | M | pt.PT_FLAG_ACCUM_SHARD_ROWS)):
        with pytest.raises(pt.PtError, match="pt_amd error -1"):
            pt.scene_plan(sc, **bad)
    for bad in (dict(flags=T), dict(flags=T | M | pt.PT_FLAG_TRACE_AHEAD, max_batch=4), dict(flags=T | M, lens_radius=0.1, focal_distance=5.0)):
        with pytest.raises(pt.PtError, match="PT_FLAG_TEMPORAL"):
            pt.scene_plan(sc, **bad)
    a, b = pt.scene_plan(sc, flags=T | M), pt.scene_plan(sc, flags=M)
    assert bytes(a) == bytes(b)                             # the plan itself does not know of the flag
    # before pt_init the context holds no history
    pt.test_lib().pt_free()
    assert pt.test_history() is None


# ---- the projection ------------------------------------------------------------------------------------------------------------------------
CAMERAS = [((0.0, 5.0, 10.5), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 45.0),                      # axis-aligned (Cornell's)
           ((3.0, 2.0, 7.0), (1.5, 0.0, -2.0), (0.0, 1.0, 0.0), 30.0),                       # rotated, a view vector of length 2.5
           ((-2.0, 6.0, 4.0), (0.3, -0.2, -1.0), (0.1, 1.0, -0.3), 50.0)]                     # up neither unit nor orthogonal to view


def _camera(pt, eye, view, up, fovy, w, h):
    sc = pt.Scene(os.path.join(SCENES, "cornell.txt"))
    sc.set_resolution(w, h)
    cam = sc.camera.copy()
    cam["position"][0], cam["view"][0], cam["up"][0] = eye, view, up
    cam["fov"][0][1] = fovy
    return cam


@pytest.mark.parametrize("eye,view,up,fovy", CAMERAS)
@pytest.mark.parametrize("w,h", [(256, 144), (37, 23)])
def test_projection_inverts_the_camera_rays(pt, eye, view, up, fovy, w, h):
    """The float64 ray through (x + jx, y + jy) -- dir = (view - right a) - up b of the camera's fp32 constants -- and a point on it at a random
    distance, rounded to fp32: steps 2 - 3 give (u + 0.5, v + 0.5) within 1 / 64 px.  (fp32 epsilon times coordinates of at most 256 over a
    dozen operations is three orders of magnitude below that.)  The rows the library computes are the restatement's, bit for bit."""
    cam = _camera(pt, eye, view, up, fovy, w, h)
    lib16 = pt.test_temporal_camera(cam)
    vw, upv, right, e, plx, ply, hw, hh = tr.camera_constants(cam)
    mine = tr.temporal_camera(vw, upv, right, e, lib16[3], lib16[4], hw, hh)       # (pixLen: the library's own tan)
    assert _same(mine, lib16)
    rng = np.random.default_rng(w)
    n = 4000
    px = rng.integers(0, w, n) + rng.uniform(0, 1, n)
    py = rng.integers(0, h, n) + rng.uniform(0, 1, n)
    a = float(lib16[3]) * (px - float(hw))
    b = float(lib16[4]) * (py - float(hh))
    d = vw.astype(np.float64)[None] - right.astype(np.float64)[None] * a[:, None] - upv.astype(np.float64)[None] * b[:, None]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    P = (e.astype(np.float64)[None] + d * rng.uniform(0.5, 30.0, (n, 1))).astype(F)
    s, u, v = tr.project(P, lib16)
    assert (s > 0).all()
    err = np.maximum(np.abs(u.astype(np.float64) + 0.5 - px), np.abs(v.astype(np.float64) + 0.5 - py))
    print("%d x %d: largest projection error %.3g px" % (w, h, err.max()))
    assert err.max() < 1.0 / 64
    s, _, _ = tr.project((e.astype(np.float64)[None] - d).astype(F), lib16)      # points behind the eye
    assert (s < 0).all()


# ---- a wall, two cameras, every number dyadic -----------------------------------------------------------------------------------------------
def _wall_view(eye, w, h, pixlen=0.125, jitter=0.5):
    """The guides of a camera at `eye` looking down -z (up +y, right +x) at the wall z = 0, and its 16 constants.  With pixlen a power of two
    and eye coordinates dyadic everything below is exact in fp32."""
    yy, xx = np.mgrid[0:h, 0:w]
    a = pixlen * (xx + jitter - w / 2)
    b = pixlen * (yy + jitter - h / 2)
    pos_t = np.zeros((h, w, 4), F)
    pos_t[..., 0] = eye[0] - a * eye[2]
    pos_t[..., 1] = eye[1] - b * eye[2]
    pos_t[..., 3] = eye[2] * np.sqrt(a * a + b * b + 1)
    nrm = np.zeros((h, w, 3), F)
    nrm[..., 2] = 1
    _, nrm_id = tr.pack_guides(pos_t, nrm, np.zeros((h, w), np.int32), h, w)
    return pos_t, nrm_id, tr.temporal_camera((0, 0, -1), (0, 1, 0), (1, 0, 0), eye, pixlen, pixlen, F(w) * F(0.5), F(h) * F(0.5))


def test_without_history_the_filter_form_is_mean_and_variance_to_the_bit():
    rng = np.random.default_rng(5)
    h, w, n = 23, 37, 3
    S = rng.uniform(0, 12, (h, w, 3)).astype(F)
    S[rng.uniform(0, 1, (h, w)) < 0.2] = 0                  # (pixels no sample reached: sums of +0)
    Q = rng.uniform(0, 40, (h, w)).astype(F)
    pos_t, nrm_id, cam = _wall_view((0.25, 0.0, 4.0), w, h)
    want_c, want_v = dv.mean_and_variance(S, Q, n)
    for hist in (tr.empty_history(h, w),                                                    # nothing stored
                 (np.full((h, w, 4), 7, F), np.full((h, w), 9, F), pos_t, nrm_id, _wall_view((0.0, 0.0, -4.0), w, h)[2])):    # all of it behind the old camera
        c, v = tr.filter_form(S, Q, n, pos_t, nrm_id, *hist)
        assert _same(c, want_c) and _same(v, want_v)
        hc, hn = tr.capture_form(S, Q, n, pos_t, nrm_id, *hist)
        assert _same(hc[..., :3], want_c) and _same(hc[..., 3], Q / F(n)) and (hn == n).all()


def test_a_constant_is_a_fixed_point_within_the_operation_count():
    """A constant history k (colour and m2) of any counts over a flat wall, a current frame of S = n k, Q = n k: exactly, (hc Nh + n k) / (Nh + n) = k
    whatever Nh is.  In fp32, for a pixel with history: each of the <= 4 products Hc w rounds (the terms are positive, so a relative error
    eps = 2^-24 of a term is at most eps of the sum), each of the <= 3 inexact additions of sumC and of sumW rounds, the division rounds:
    hc = k (1 + 8 eps) to first order.  The blend weighs hc with Nh / (Nh + n) < 1 and rounds hc * Nh, the sum, tot = Nh + n and the
    division: 12 eps in all; 13 to cover the second order.  n = 4 makes S and Q exact."""
    w, h, n = 72, 40, 4
    old = _wall_view((0.0, 0.0, 4.0), w, h)
    new = _wall_view((-0.171875, 0.09375, 4.5), w, h)             # moved sideways, up and back: every fractional position occurs
    rng = np.random.default_rng(2)
    hn = rng.uniform(0.5, 40, (h, w)).astype(F)
    for k in (0.3, 1.0, 5.75):
        hc = np.full((h, w, 4), k, F)
        S, Q = np.full((h, w, 3), F(k) * F(n), F), np.full((h, w), F(k) * F(n), F)
        _, Nh = tr.reproject(new[0], new[1], hc, hn, old[0], old[1], old[2])
        assert 0.6 < (Nh > 0).mean() < 1.0
        c, m2, _ = tr.blend(S, Q, n, *tr.reproject(new[0], new[1], hc, hn, old[0], old[1], old[2]))
        err = max(np.abs(c.astype(np.float64) / float(F(k)) - 1).max(), np.abs(m2.astype(np.float64) / float(F(k)) - 1).max())
        print("k = %g: largest relative deviation %.3g = %.2f eps" % (k, err, err / EPS))
        assert err <= 13 * EPS
        hc2, hn2 = tr.capture_form(S, Q, n, new[0], new[1], hc, hn, old[0], old[1], old[2])
        assert np.abs(hc2.astype(np.float64) / float(F(k)) - 1).max() <= 13 * EPS and hn2.max() <= tr.constants()[0]


def test_every_tap_condition_rejects_alone():
    """Old camera at (0, 0, 4), new one 0.25 to the left: u = x + 0.5, v = y exactly, so pixel (x, y) takes the taps (x, y) and (x + 1, y) with
    weight 1 / 2 each and (., y + 1) with weight 0.  One tap's history holds 1000, the other 1: a pixel whose result stays near 1 has rejected
    the tap.  With both taps of weight rejected sumW = 0 fails w_min: exactly the no-history result."""
    w, h, n = 8, 8, 2
    cap, c_n, c_p, w_min = tr.constants()
    old = _wall_view((0.0, 0.0, 4.0), w, h)
    new = _wall_view((-0.25, 0.0, 4.0), w, h)
    s, u, v = tr.project(new[0][..., :3], old[2])
    yy, xx = np.mgrid[0:h, 0:w]
    assert np.array_equal(u, (xx + 0.5).astype(F)) and np.array_equal(v, yy.astype(F)) and (s == 4).all()
    S, Q = np.full((h, w, 3), 2, F), np.full((h, w), 2, F)
    none_c, none_v = dv.mean_and_variance(S, Q, n)
    y, x = 3, 3

    def run(hpos=None, hnrm_id=None, hn=None, cam=None, poison=(x,)):
        hc = np.ones((h, w, 4), F)
        for px in poison:
            hc[y, px] = 1000
        hnn = np.full((h, w), 4, F) if hn is None else hn
        return tr.filter_form(S, Q, n, new[0], new[1], hc, hnn, old[0] if hpos is None else hpos, old[1] if hnrm_id is None else hnrm_id,
                              old[2] if cam is None else cam)

    c, _ = run()
    assert c[y, x, 0] > 300 and c[y, x - 1, 0] > 300 and c[y, x + 1, 0] < 2          # control: the poisoned tap counts where it is a tap
    t = float(new[0][y, x, 3])
    other_id, turned, off_plane, empty = old[1].copy(), old[1].copy(), old[0].copy(), np.full((h, w), 4, F)
    other_id[y, x, 3] = np.array([1], np.int32).view(F)[0]
    turned[y, x, :3] = (np.sqrt(1 - 0.89 ** 2), 0, 0.89)                               # dot 0.89 < c_n
    off_plane[y, x, 2] = 1.5 * float(c_p) * t                                          # past c_p t ...
    near_plane = old[0].copy()
    near_plane[y, x, 2] = 0.5 * float(c_p) * t                                         # ... and within it
    empty[y, x] = 0
    for name, kw in (("id", dict(hnrm_id=other_id)), ("normal", dict(hnrm_id=turned)), ("plane", dict(hpos=off_plane)), ("Hn", dict(hn=empty))):
        c, _ = run(**kw)
        assert abs(c[y, x, 0] - 1) < 1e-6 and abs(c[y, x - 1, 0] - 1) < 1e-6, name     # rejected by both pixels that take it
        # the tap carried half the weight: sumW = 1 / 2 is not > w_min = 1 / 2, and the pixel has no history at all
        assert float(w_min) == 0.5 and _same(c[y, x], none_c[y, x]) and _same(c[y, x + 1, 0], F((1 * 4 + 2) / 6))
    c, _ = run(hpos=near_plane)
    assert c[y, x, 0] > 300
    # off the frame: the last column's second tap; its first carries 1 / 2 -- not enough
    c, v_ = run(poison=())
    assert _same(c[:, w - 1], none_c[:, w - 1]) and _same(v_[:, w - 1], none_v[:, w - 1]) and _same(c[y, w - 2, 0], F(1.0))
    # behind the old camera (s < 0), and on its plane (s = 0)
    for ez in (-4.0, 0.0):
        c, v_ = run(cam=_wall_view((0.0, 0.0, ez), w, h)[2])
        assert _same(c, none_c) and _same(v_, none_v)
    # every tap rejected: exactly the no-history result, frame-wide
    c, v_ = run(hn=np.zeros((h, w), F))
    assert _same(c, none_c) and _same(v_, none_v)
    c, v_ = run(hnrm_id=np.broadcast_to(other_id[y, x], (h, w, 4)).copy())
    assert _same(c, none_c) and _same(v_, none_v)


def test_a_chain_of_captures_never_stores_more_than_the_cap():
    w, h, n = 24, 16, 7
    cap = float(tr.constants()[0])
    rng = np.random.default_rng(9)
    hist = tr.empty_history(h, w)
    seen = []
    for k in range(8):
        g = _wall_view((0.0625 * k, -0.03125 * k, 4.0), w, h)
        S, Q = rng.uniform(0, 4, (h, w, 3)).astype(F), rng.uniform(0, 9, (h, w)).astype(F)
        hc, hn = tr.capture_form(S, Q, n, g[0], g[1], *hist)
        assert hn.max() <= cap and hn.min() >= n
        seen.append(float(hn.max()))
        hist = (hc, hn, g[0], g[1], g[2])
    assert seen[0] == n and seen[-1] == cap and seen == sorted(seen)        # 7, 14, 21, 28, then the cap


# ---- the study: the CPU oracle chooses the constants ----------------------------------------------------------------------------------------
W, H = 72, 40
OLD, NEW = 16, (2, 4)
# candidates: the cap never binds in one step from 16 samples, so it is varied at the shipped setting only (the README's long chain decides it)
CANDIDATES = [(32, 0.9, cp, wm) for cp in (0.01, 0.02, 0.05) for wm in (0.01, 0.25, 0.5, 0.75)] + \
             [(16, 0.9, 0.01, 0.5), (64, 0.9, 0.01, 0.5), (32, 0.8, 0.01, 0.5), (32, 0.98, 0.01, 0.5)]
CANDIDATES = [tuple(float(F(c)) for c in cd) for cd in CANDIDATES]          # (as fp32 holds them: what tr.constants() reads from the header)


def _rmse(a, ref, mask=None):
    d = (np.asarray(a, np.float64) - ref) ** 2
    return float(np.sqrt((d if mask is None else d[mask]).mean()))


def _edge_band(ids, r=3):
    """pixels within r px (Chebyshev) of a pixel whose 4-neighbour shows another primitive"""
    e = np.zeros(ids.shape, bool)
    dx, dy = ids[:, 1:] != ids[:, :-1], ids[1:, :] != ids[:-1, :]
    e[:, 1:] |= dx
    e[:, :-1] |= dx
    e[1:, :] |= dy
    e[:-1, :] |= dy
    b = np.zeros_like(e)
    hh, ww = ids.shape
    for oy in range(-r, r + 1):
        for ox in range(-r, r + 1):
            b[max(0, -oy):hh + min(0, -oy), max(0, -ox):ww + min(0, -ox)] |= e[max(0, oy):hh + min(0, oy), max(0, ox):ww + min(0, ox)]
    return b


def _view(oracle, cam, geoms, mats, eye, first, counts, nref=0, guides=True):
    """iterations first, first + 1, ... from `eye`: {n: (S, Q)} for n in counts, the mean of the first nref as float64 (or None), the guides
    of iteration 1 (or None) and the camera's 16 constants"""
    cam = cam.copy()
    cam["position"][0] = eye
    ref = oracle.Renderer(cam, geoms, mats, 8)
    acc, singles, at = np.zeros(W * H * 3, F), [], {}
    for k in range(1, max(max(counts), nref) + 1):
        if k <= max(counts):
            one = np.zeros(W * H * 3, F)
            ref.iterate(first + k - 1, one)
            singles.append(one.reshape(H, W, 3))
        ref.iterate(first + k - 1, acc)
        if k in counts:
            at[k] = (acc.reshape(H, W, 3).copy(), dv.moments(singles))
    conv = (acc / F(nref)).reshape(H, W, 3).astype(np.float64) if nref else None
    guides = tr.pack_guides(*dr.oracle_guides(oracle, ref, 1), H, W) if guides else None
    return at, conv, guides, tr.camera16(cam)


def _cornell(oracle):
    sc = oracle.Scene(os.path.join(SCENES, "cornell.txt"))
    sc.set_resolution(W, H)
    return sc.camera, sc.geoms, sc.materials, (0.0, 5.0, 10.5), (0.3, 5.0, 10.5)


def _sphere_before_a_wall(oracle):
    """a red sphere of radius 1.5 three units in front of a white wall, a floor, a light above: the sidestep of 1.5 moves the sphere 7 px and
    the wall 5, and uncovers the strip of wall between"""
    cam = _cornell(oracle)[0].copy()
    cam["view"][0], cam["up"][0] = (0, 0, -1), (0, 1, 0)
    cam["fov"][0][1] = 30
    mats = np.zeros(3, oracle.MATERIAL_DTYPE)
    mats["color"] = [(1, 1, 1), (0.85, 0.85, 0.85), (0.8, 0.2, 0.2)]
    mats["emittance"] = [5, 0, 0]
    geoms = np.concatenate([oracle.make_geom(1, 0, (0, 8, 3), (0, 0, 0), (6, 0.3, 6)), oracle.make_geom(1, 1, (0, 0, -3), (0, 0, 0), (20, 20, 0.2)),
                            oracle.make_geom(1, 1, (0, -3, 0), (0, 0, 0), (20, 0.2, 20)), oracle.make_geom(0, 2, (0, 0, 1), (0, 0, 0), (3, 3, 3))])
    return cam, geoms, mats, (0.0, 0.5, 8.0), (1.5, 0.5, 8.0)


@pytest.fixture(scope="module")
def study(oracle):
    """Per scene: 16 iterations of the old view captured as history; iterations 17 .. of the new view (the numbering goes on, so the new
    samples' random numbers are fresh) after 2 and 4 of them, their mean over 2048 as the reference; the old view's edge band.  Then per
    candidate and count the RMSE of blend -> filter over the frame and over the band, next to the filter alone."""
    out = {}
    for name, make in (("cornell", _cornell), ("sphere", _sphere_before_a_wall)):
        cam, geoms, mats, e0, e1 = make(oracle)
        at0, _, g0, cam0 = _view(oracle, cam, geoms, mats, e0, 1, (OLD,))
        at1, conv, g1, _ = _view(oracle, cam, geoms, mats, e1, OLD + 1, NEW, nref=2048)
        hc, hn = tr.capture_form(*at0[OLD], OLD, *g0, *tr.empty_history(H, W))
        hist = (hc, hn, g0[0], g0[1], cam0)
        band = _edge_band(np.ascontiguousarray(g0[1][..., 3]).view(np.int32))
        ids1 = np.ascontiguousarray(g1[1][..., 3]).view(np.int32)
        for n in NEW:
            S, Q = at1[n]
            alone = dv.denoise_var(S, Q, n, g1[0][..., :3], g1[1][..., :3], ids1, LEVELS, SIGMA_LUM, SIGMA_NORMAL, SIGMA_POSITION)[0]
            out[(name, n, "alone")] = (_rmse(alone, conv), _rmse(alone, conv, band))
            for cd in CANDIDATES + [tuple(float(c) for c in tr.constants())]:
                got = tr.denoise_var_temporal(S, Q, n, *g1, hist, LEVELS, SIGMA_LUM, SIGMA_NORMAL, SIGMA_POSITION, consts=tuple(F(c) for c in cd))[0]
                out[(name, n, cd)] = (_rmse(got, conv), _rmse(got, conv, band))
    return out


# The scores are RMSEs against a reference of 2048 samples, whose own error is 1 / sqrt(2048 / n) = 3 - 4 % of an n-sample frame's for n = 2, 4:
# it does not resolve score differences of a fraction of a percent, and any change to the oracle's sampling moves them.  "The lowest" is
# therefore held within 1 % of the best passing candidate's score.  (Measured: the shipped c_p 0.01 scores 0.046425, c_p 0.02 and 0.05
# 0.046435 -- 0.02 % apart, a tie the margin covers either way --, w_min 0.75 0.04980, 7 % behind.)
BAND_MARGIN = 0.01


def _passes(study, cd):
    return all(study[(s, n, cd)][0] < study[(s, n, "alone")][0] for s in ("cornell", "sphere") for n in NEW) and \
        all(study[("sphere", n, cd)][1] < study[("sphere", n, "alone")][1] for n in NEW)


def _band_score(study, cd):
    return sum(study[("sphere", n, cd)][1] for n in NEW) / len(NEW)


def test_study_history_helps_on_both_scenes_and_does_not_smear_the_silhouette(study):
    """RMSE against 2048 samples of the new view, filter at (5 levels, sigma_lum 4, 0.35, 2.0); 16 old samples, 2 and 4 new ones.  The shipped
    constants (cap 32, c_n 0.9, c_p 0.01, w_min 0.5):
        Cornell 72 x 40, sidestep 0.3:   n = 2: filter alone 0.11197, blend -> filter 0.07401 (0.66 x);  n = 4: 0.08298 -> 0.07033 (0.85 x)
        sphere before a wall, sidestep 1.5:  n = 2: 0.17461 -> 0.04961 (0.28 x);  n = 4: 0.09424 -> 0.04653 (0.49 x)
        ... its edge band (3 px around the old view's primitive-id edges):  n = 2: 0.14391 -> 0.04787 (0.33 x);  n = 4: 0.08383 -> 0.04498 (0.54 x)"""
    shipped = tuple(float(c) for c in tr.constants())
    for s in ("cornell", "sphere"):
        for n in NEW:
            a, g = study[(s, n, "alone")], study[(s, n, shipped)]
            print("%s n = %d: filter alone %.5f, blend -> filter %.5f (%.2f x); edge band %.5f -> %.5f (%.2f x)" % (s, n, a[0], g[0], g[0] / a[0], a[1], g[1], g[1] / a[1]))
            assert g[0] < a[0]
    for n in NEW:
        assert study[("sphere", n, shipped)][1] < study[("sphere", n, "alone")][1]


def test_study_the_shipped_constants_are_the_candidates_best(study):
    """Among the candidates that meet every condition of the test above, the one with the lowest edge-band RMSE on the sphere scene (the mean of
    the two counts; ties within BAND_MARGIN) ships.  The table (frame RMSE Cornell n = 2, 4; sphere n = 2, 4; sphere's edge band n = 2, 4), cap 32 and c_n 0.9 unless named:
        c_p 0.01 w_min 0.01   0.11201 0.10227 | 0.04692 0.04537 | 0.04463 0.04233   fails: Cornell n = 2, 4 are no better than the filter alone
        c_p 0.01 w_min 0.25   0.09548 0.08376 | 0.04859 0.04479 | 0.04602 0.04196   fails: Cornell n = 4
        c_p 0.01 w_min 0.5    0.07401 0.07033 | 0.04961 0.04653 | 0.04787 0.04498   <- shipped
        c_p 0.01 w_min 0.75   0.08708 0.06623 | 0.08727 0.04935 | 0.05196 0.04764
        c_p 0.02 w_min 0.01   0.11196 0.10225 | 0.04690 0.04536 | 0.04459 0.04230   fails
        c_p 0.02 w_min 0.25   0.09542 0.08373 | 0.04860 0.04481 | 0.04603 0.04198   fails
        c_p 0.02 w_min 0.5    0.07391 0.06970 | 0.04962 0.04656 | 0.04786 0.04501
        c_p 0.02 w_min 0.75   0.08705 0.06619 | 0.08729 0.04938 | 0.05199 0.04768
        c_p 0.05              the rows of c_p 0.02 to the digits shown
        cap 16, cap 64        the shipped row (the cap does not bind one step after 16 samples)
        c_n 0.8               the shipped row;   c_n 0.98   0.07509 0.07228 | 0.05029 0.04689 | 0.04919 0.04565
    (filter alone: 0.11197 0.08298 | 0.17461 0.09424 | 0.14391 0.08383.)  A small w_min fails on Cornell: the pixels at the corners of its
    light -- emittance 5 against a ceiling of 0.4, the guide's primitive one jittered sample's -- take a single neighbour's history at a bilinear
    weight of a few percent, and 16 confident samples of the wrong side of the edge keep the filter from repairing them."""
    shipped = tuple(float(c) for c in tr.constants())
    rows = []
    for cd in CANDIDATES:
        r = [study[(s, n, cd)][0] for s in ("cornell", "sphere") for n in NEW] + [study[("sphere", n, cd)][1] for n in NEW]
        rows.append((cd, _passes(study, cd), _band_score(study, cd)))
        print("cap %g c_n %g c_p %g w_min %g:  %.5f %.5f | %.5f %.5f | %.5f %.5f  %s" % (cd + tuple(r) + ("passes" if rows[-1][1] else "fails",)))
    assert shipped in [cd for cd, _, _ in rows]
    assert _passes(study, shipped)
    best = min(score for _, ok, score in rows if ok)
    print("edge-band score: shipped %.6f, the passing candidates' best %.6f" % (_band_score(study, shipped), best))
    assert _band_score(study, shipped) <= best * (1 + BAND_MARGIN)


def test_study_a_chain_of_four_views_keeps_improving(oracle):
    """The sphere scene, the camera stepping 0.5 sideways per view, 2 samples per view (iterations numbered on), each view's history the view
    before's capture; RMSE of blend -> filter against 2048 other samples of the same view (iterations 1001 ..).  A view of 2 samples is one
    draw of heavy noise, so the chain is run three times, from iterations 1, 101 and 201, and judged on the three chains' mean:
        chain from   1:  0.16716, 0.07955, 0.06975, 0.06203   (before the filter 0.62619, 0.38266, 0.28190, 0.23819)
        chain from 101:  0.20837, 0.09747, 0.05878, 0.05174   (0.67690, 0.39570, 0.30122, 0.24239)
        chain from 201:  0.19033, 0.07007, 0.08105, 0.05891   (0.63417, 0.39246, 0.30280, 0.23652)
        mean:            0.18862, 0.08236, 0.06986, 0.05756
    The mean falls view over view; so does the blend before the filter in every single chain; a single chain's filtered RMSE need not (the
    one from iteration 201 rises once).  Every view with history beats the filter alone on its own 2 samples, in every chain."""
    cam, geoms, mats, e0, _ = _sphere_before_a_wall(oracle)
    eyes = [(e0[0] + 0.5 * k, e0[1], e0[2]) for k in range(4)]
    refs = [_view(oracle, cam, geoms, mats, eye, 1001, (1,), nref=2048) for eye in eyes]
    chains = []
    for first in (1, 101, 201):
        hist, errs, pre = tr.empty_history(H, W), [], []
        for k, eye in enumerate(eyes):
            _, conv, g, cam16 = refs[k]
            (S, Q) = _view(oracle, cam, geoms, mats, eye, first + 2 * k, (2,), guides=False)[0][2]
            got = tr.denoise_var_temporal(S, Q, 2, *g, hist, LEVELS, SIGMA_LUM, SIGMA_NORMAL, SIGMA_POSITION)[0]
            alone = dv.denoise_var(S, Q, 2, g[0][..., :3], g[1][..., :3], np.ascontiguousarray(g[1][..., 3]).view(np.int32), LEVELS, SIGMA_LUM,
                                   SIGMA_NORMAL, SIGMA_POSITION)[0]
            errs.append(_rmse(got, conv))
            pre.append(_rmse(tr.blend(S, Q, 2, *tr.reproject(*g, *hist))[0], conv))
            assert k == 0 or errs[-1] < _rmse(alone, conv)
            hc, hn = tr.capture_form(S, Q, 2, *g, *hist)
            hist = (hc, hn, g[0], g[1], cam16)
        print("chain from iteration %d: RMSE %s (before the filter %s)" % (first, ", ".join("%.5f" % e for e in errs), ", ".join("%.5f" % e for e in pre)))
        assert pre[0] > pre[1] > pre[2] > pre[3]
        chains.append(errs)
    mean = np.mean(chains, axis=0)
    print("mean of the three chains: " + ", ".join("%.5f" % e for e in mean))
    assert mean[0] > mean[1] > mean[2] > mean[3]


def test_study_a_long_walk_sets_the_cap(oracle):
    """One step after 16 samples no cap of 16 or more binds, so the cap is chosen on a walk that outlasts it: the sphere scene, 24 views 0.25
    apart, 4 samples each (iterations numbered on), every view's history the capture of the view before under the candidate cap; RMSE of the
    LAST view's blend -> filter against 2048 other samples of it.  The shipped cap is the best of the three candidates: a history that never
    forgets keeps the bilinear taps' blur and every rejected tap's bias of 23 views, a short one throws samples away.
        cap 16: 0.03684   cap 32: 0.03547   cap 64: 0.03569"""
    cam, geoms, mats, e0, _ = _sphere_before_a_wall(oracle)
    eyes = [(e0[0] - 3.0 + 0.25 * k, e0[1], e0[2]) for k in range(24)]
    views = [_view(oracle, cam, geoms, mats, eye, 1 + 4 * k, (4,)) for k, eye in enumerate(eyes)]
    conv = _view(oracle, cam, geoms, mats, eyes[-1], 1001, (1,), nref=2048, guides=False)[1]
    shipped = tuple(tr.constants())
    errs = {}
    for cap in (16.0, 32.0, 64.0):
        consts = (F(cap),) + shipped[1:]
        hist = tr.empty_history(H, W)
        for k, (at, _, g, cam16) in enumerate(views):
            S, Q = at[4]
            if k == len(views) - 1:
                errs[cap] = _rmse(tr.denoise_var_temporal(S, Q, 4, *g, hist, LEVELS, SIGMA_LUM, SIGMA_NORMAL, SIGMA_POSITION, consts=consts)[0], conv)
            hc, hn = tr.capture_form(S, Q, 4, *g, *hist, consts=consts)
            hist = (hc, hn, g[0], g[1], cam16)
    print("the last of 24 views, RMSE by cap: " + ", ".join("%g: %.5f" % kv for kv in sorted(errs.items())))
    assert float(shipped[0]) in errs and errs[float(shipped[0])] == min(errs.values())
