"""Temporal reprojection (PT_FLAG_TEMPORAL) on the MI355X, every comparison bit for bit against the numpy restatement (tests/temporal_ref.py):
k_temporal in both forms over synthetic arrays that take every branch of its steps 1 - 6 and over rendered frames; the chain init -> render ->
re-init with a moved camera -> render -> pt_denoise_var -> re-init again, with the context's history read back after every capture; that the
flag changes nothing else; the history's lifetime and pt_init's refusals; a caller-owned accumulator on a stream of the caller's.
Frames: 72 x 40, 64 x 48 and 37 x 23 (a partial workgroup and an odd pitch).  A NaN's sign and payload are the processor's own, so arrays that
may hold one are compared as: NaN in the same places, the same bits everywhere else."""
import os

import numpy as np
import pytest

import denoise_ref as dr
import denoise_var_ref as dv
import temporal_ref as tr
from conftest import SCENES

pytestmark = pytest.mark.gpu
F = np.float32
SIGMAS = (4.0, 0.35, 2.0)
FRAMES = [("cornell.txt", 72, 40, 5), ("mesh_small.txt", 64, 48, 2), ("cornell.txt", 37, 23, 1)]
EYES = {"cornell.txt": [(0.0, 5.0, 10.5), (0.4, 5.1, 10.3), (0.9, 4.8, 10.0)]}


@pytest.fixture(scope="module")
def gpu(pt):
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return pt


def _bits(a):
    return np.ascontiguousarray(a, F).reshape(-1).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _same_but_nans(a, b):
    a, b = np.ascontiguousarray(a, F).reshape(-1), np.ascontiguousarray(b, F).reshape(-1)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(_bits(a[~na]), _bits(b[~nb]))


def _eyes(sc, scene):
    """three eyes a few pixels of parallax apart: the scene's own, then two moved ones"""
    if scene in EYES:
        return EYES[scene]
    e = np.array(sc.camera["position"][0], np.float64)
    return [tuple(e), tuple(e + (0.15, 0.05, -0.1)), tuple(e + (0.3, -0.05, -0.2))]


def _scene(pt, scene, w, h):
    sc = pt.Scene(os.path.join(SCENES, scene))
    sc.set_resolution(w, h)
    return sc


def _init(pt, sc, eye, temporal=True, free=False, **opts):
    sc.camera["position"][0] = eye
    if free:
        pt.pathtraceFree()
    pt.pathtraceInit(sc, traceDepth=4, moments=True, temporal=temporal, **opts)


def _render(pt, first, n):
    for it in range(first, first + n):
        pt.pathtrace(None, 0, it, readback=False)


def _sums(pt, w, h):
    return pt.readback(w * h).reshape(h, w, 3), pt.readback_moments().reshape(h, w)


def _guides(pt, w, h, guide_iter=1):
    return tr.pack_guides(*pt.gbuffer(guide_iter), h, w)


# ---- 1: the kernel over host arrays ---------------------------------------------------------------------------------------------------
def _synthetic(w, h, seed):
    """A wall z = 0 seen by an old camera at (0, 0, 4) looking down -z with pixLen 1 / 8: every number dyadic, so the projection of a point
    (px, py, 0) is u = (halfW - 0.5) - 2 px EXACTLY and a pixel's target (u, v) can be put on -1, 0, W - 1, W.  The new view's guides are
    made per pixel from such targets (the kernel does not ask whether a camera could have seen them)."""
    rng = np.random.default_rng(seed)
    hw, hh = F(w) * F(0.5), F(h) * F(0.5)
    cam = tr.temporal_camera((0, 0, -1), (0, 1, 0), (1, 0, 0), (0, 0, 4), 0.125, 0.125, hw, hh)
    # targets: pixel grid plus an offset from a set that holds the edges' exact values, halves, eighths and far outside
    yy, xx = np.mgrid[0:h, 0:w]
    off = np.array([0, 0, 0.5, 0.5, 0.125, 0.875, 0.375, -1, 1, 0.25, 2.5, -3, 40, -40], np.float64)
    u = xx + rng.choice(off, (h, w))
    v = yy + rng.choice(off, (h, w))
    edge = rng.uniform(0, 1, (h, w))
    u = np.where(edge < 0.04, -1.0, np.where(edge < 0.08, w, np.where(edge < 0.12, w - 1.0, np.where(edge < 0.16, 0.0, u))))
    edge = rng.uniform(0, 1, (h, w))
    v = np.where(edge < 0.04, -1.0, np.where(edge < 0.08, h, np.where(edge < 0.12, h - 1.0, np.where(edge < 0.16, 0.0, v))))
    pos_t = np.zeros((h, w, 4), F)
    pos_t[..., 0] = ((float(hw) - 0.5) - u) / 2
    pos_t[..., 1] = ((float(hh) - 0.5) - v) / 2
    z = rng.choice(np.array([0, 0, 0, 0, 0.03125, -0.0625, 0.25, 4.0, 5.0, np.nan, np.inf]), (h, w), p=[.4, .2, .1, .1, .05, .03, .02, .03, .03, .02, .02])
    pos_t[..., 2] = z                                   # (4: s = 0 exactly; 5: behind the old camera; NaN, inf: fail step 2 or 3)
    pos_t[..., 3] = rng.choice(np.array([4.0, 2.0, 8.0, 0.5, np.nan, -1.0]), (h, w), p=[.5, .2, .2, .04, .03, .03])
    ids = rng.choice(np.array([-1, 0, 1, 2], np.int32), (h, w), p=[.05, .8, .1, .05])
    nrm = np.zeros((h, w, 3), F)
    nrm[..., 2] = 1
    tilt = rng.uniform(0, 1, (h, w)) < 0.1
    nrm[tilt] = np.array([0.6, 0, 0.8], F)              # dot with (0, 0, 1): 0.8 < c_n
    _, nrm_id = tr.pack_guides(pos_t, nrm, ids, h, w)
    # the history: the wall under the old pixels' centres, some taps off the plane, tilted, of another primitive, empty or not finite
    hpos = np.zeros((h, w, 4), F)
    hpos[..., 0] = ((float(hw) - 0.5) - xx) / 2
    hpos[..., 1] = ((float(hh) - 0.5) - yy) / 2
    hpos[..., 2] = rng.choice(np.array([0, 0.03125, -0.0625, 0.125, -0.5]), (h, w), p=[.85, .05, .05, .03, .02])
    hpos[..., 3] = 4
    hn3 = np.zeros((h, w, 3), F)
    hn3[..., 2] = 1
    ht = rng.uniform(0, 1, (h, w))
    hn3[ht < 0.05] = np.array([0.6, 0, 0.8], F)
    hn3[(ht >= 0.05) & (ht < 0.1)] = np.array([0, 0.4375, 0.899], F)      # dot 0.899 and 0.9 -- one ulp matters -- against (0, 0, 1)
    hn3[(ht >= 0.1) & (ht < 0.2)] = np.array([0, 0.4375, 0.9], F)
    hids = rng.choice(np.array([-1, 0, 1, 2], np.int32), (h, w), p=[.03, .85, .07, .05])
    _, hnrm_id = tr.pack_guides(hpos, hn3, hids, h, w)
    hn = rng.choice(np.array([0, 1, 2.5, 16, 31.5, 32, 64, -1, np.nan, np.inf, -0.0], F), (h, w), p=[.05, .1, .25, .25, .1, .1, .05, .03, .03, .02, .02])
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-40, 3e38], F)
    hc = rng.uniform(0, 4, (h, w, 4)).astype(F)
    m = rng.uniform(0, 1, hc.shape) < 0.05
    hc[m] = rng.choice(special, int(m.sum()))
    S = rng.uniform(0, 9, (h, w, 3)).astype(F)
    m = rng.uniform(0, 1, S.shape) < 0.05
    S[m] = rng.choice(special, int(m.sum()))
    Q = rng.uniform(0, 30, (h, w)).astype(F)
    m = rng.uniform(0, 1, Q.shape) < 0.05
    Q[m] = rng.choice(special, int(m.sum()))
    return S, Q, pos_t, nrm_id, hc, hn, hpos, hnrm_id, cam


@pytest.mark.parametrize("w,h", [(72, 40), (64, 48), (37, 23)])
def test_kernel_on_synthetic_arrays_takes_every_branch(gpu, w, h):
    args = _synthetic(w, h, 11 * w + h)
    S, Q, pos_t, nrm_id, hc, hn, hpos, hnrm_id, cam = args
    # the inputs do take the branches: pixels on every exact edge value, both sides of every tap condition, pixels with and without history
    s, u, v = tr.project(pos_t[..., :3], cam)
    for val in (-1.0, 0.0, w - 1.0, float(w)):
        assert (u == F(val)).any(), val
    for val in (-1.0, 0.0, h - 1.0, float(h)):
        assert (v == F(val)).any(), val
    assert (s == 0).any() and (s < 0).any() and np.isnan(s).any()
    _, Nh = tr.reproject(pos_t, nrm_id, hc, hn, hpos, hnrm_id, cam)
    cap = tr.constants()[0]
    assert (Nh == 0).sum() > w * h // 8 and (Nh > 0).sum() > w * h // 8 and (np.ascontiguousarray(nrm_id[..., 3]).view(np.int32) < 0).any() and (Nh == cap).any() and ((Nh > 0) & (Nh < cap)).any()
    want_c, want_v = tr.filter_form(S, Q, 3, *args[2:])
    got = gpu.test_temporal(False, w, h, 3, *args)
    assert np.isnan(want_c).any() and np.isfinite(want_c).sum() > want_c.size // 2
    assert _same_but_nans(got[:, :3], want_c) and _same_but_nans(got[:, 3], want_v)
    want_hc, want_hn = tr.capture_form(S, Q, 3, *args[2:])
    got_hc, got_hn = gpu.test_temporal(True, w, h, 3, *args)
    assert _same_but_nans(got_hc, want_hc) and _same_but_nans(got_hn, want_hn)
    assert not (want_hn[~np.isnan(want_hn)] > cap).any()


@pytest.mark.parametrize("scene,w,h,levels", FRAMES)
def test_kernel_on_rendered_frames(gpu, scene, w, h, levels):
    sc = _scene(gpu, scene, w, h)
    e0, e1, _ = _eyes(sc, scene)
    try:
        _init(gpu, sc, e0, temporal=False, free=True)
        cam0 = gpu.test_temporal_camera(sc.camera)
        _render(gpu, 1, 3)
        S0, Q0 = _sums(gpu, w, h)
        g0 = _guides(gpu, w, h)
        _init(gpu, sc, e1, temporal=False, free=True)
        _render(gpu, 4, 2)
        S1, Q1 = _sums(gpu, w, h)
        g1 = _guides(gpu, w, h)
    finally:
        gpu.pathtraceFree()
    hc, hn = tr.capture_form(S0, Q0, 3, *g0, *tr.empty_history(h, w))
    got_hc, got_hn = gpu.test_temporal(True, w, h, 3, S0, Q0, *g0, *tr.empty_history(h, w))
    assert _same(got_hc, hc) and _same(got_hn, hn) and (hn == 3).all()
    hist = (hc, hn, g0[0], g0[1], cam0)
    _, Nh = tr.reproject(*g1, *hist)
    hit = np.ascontiguousarray(g1[1][..., 3]).view(np.int32) >= 0
    assert 0.5 < (Nh[hit] > 0).mean() and (Nh[hit] == 0).any()  # most pixels that hit something find their surface again, some do not
    want_c, want_v = tr.filter_form(S1, Q1, 2, *g1, *hist)
    got = gpu.test_temporal(False, w, h, 2, S1, Q1, *g1, *hist)
    assert _same(got[:, :3], want_c) and _same(got[:, 3], want_v)
    want = tr.capture_form(S1, Q1, 2, *g1, *hist)
    got = gpu.test_temporal(True, w, h, 2, S1, Q1, *g1, *hist)
    assert _same(got[0], want[0]) and _same(got[1], want[1]) and abs(want[1].max() - 5) < 1e-5


# ---- 2: end to end ------------------------------------------------------------------------------------------------------------------------
def _history_equals(got, want):
    return got is not None and all(_same(got[k], want[i]) for i, k in enumerate(("hc", "hn", "hpos_t", "hnrm_id", "cam")))


@pytest.mark.parametrize("scene,w,h,levels", FRAMES)
def test_chain_of_three_views(gpu, scene, w, h, levels):
    """init (moments + temporal), render 8; re-init with a moved camera: the history is the restatement's capture; render 2: pt_denoise_var and
    _rgba8 are the restatement's blend-then-filter, in every form of k_atrous_*<AtrousGuided>; re-init again: the recursive capture.  The 64 x 48 case makes
    the capture run k_gbuffer itself (the cached guides are another iteration's); the others hand over the cached ones."""
    sc = _scene(gpu, scene, w, h)
    e0, e1, e2 = _eyes(sc, scene)
    cached = w != 64
    with gpu.renderer_from_test_library():
        _init(gpu, sc, e0, free=True)
        cam0 = gpu.test_temporal_camera(sc.camera)
        g0 = _guides(gpu, w, h)
        if not cached:
            gpu.gbuffer(2)
        assert gpu.test_history() is None
        _render(gpu, 1, 8)
        S0, Q0 = _sums(gpu, w, h)
        plain = gpu.denoise_var(8, levels, *SIGMAS)
        _init(gpu, sc, e1)                                       # over the live renderer: the capture
        cam1 = gpu.test_temporal_camera(sc.camera)
        hist0 = tr.capture_form(S0, Q0, 8, *g0, *tr.empty_history(h, w)) + (g0[0], g0[1], cam0)
        assert _history_equals(gpu.test_history(), hist0)
        assert not gpu.readback(w * h).any() and not gpu.readback_moments().any()
        _render(gpu, 9, 2)
        S1, Q1 = _sums(gpu, w, h)
        g1 = _guides(gpu, w, h)
        want, wantv = tr.denoise_var_temporal(S1, Q1, 2, *g1, hist0, levels, *SIGMAS)
        alone, _ = dv.denoise_var(S1, Q1, 2, g1[0][..., :3], g1[1][..., :3], np.ascontiguousarray(g1[1][..., 3]).view(np.int32), levels, *SIGMAS)
        assert np.isfinite(want).all() and not _same(want, alone)
        got, gotv = gpu.denoise_var(2, levels, *SIGMAS, with_variance=True)
        assert _same(got, want) and _same(gotv, wantv)
        assert _same(gpu.denoise_var(2, levels, *SIGMAS), want)
        assert np.array_equal(gpu.denoise_var_rgba8(2, levels, *SIGMAS), dr.to_rgba8(want))
        for form in (0, 1, 2, 3):
            o, v = gpu.test_denoise_var(2, form, levels, *SIGMAS)
            assert _same(o, want) and _same(v, wantv), form
        assert _history_equals(gpu.test_history(), hist0)       # reading it does not change it
        _init(gpu, sc, e2)                                       # the recursive capture: view 1's blend of ITS history with ITS samples
        hist1 = tr.capture_form(S1, Q1, 2, *g1, *hist0) + (g1[0], g1[1], cam1)
        assert _history_equals(gpu.test_history(), hist1) and abs(hist1[1].max() - 10) < 1e-5
        _render(gpu, 11, 2)
        S2, Q2 = _sums(gpu, w, h)
        g2 = _guides(gpu, w, h)
        want, wantv = tr.denoise_var_temporal(S2, Q2, 2, *g2, hist1, levels, *SIGMAS)
        got, gotv = gpu.denoise_var(2, levels, *SIGMAS, with_variance=True)
        assert _same(got, want) and _same(gotv, wantv)
    assert not _same(plain, want)


def test_counters_reset_and_iterate_until_between_views(gpu):
    """The capture's n is the number of iterations committed into the accumulators since pt_init, whatever was done to the diagnostic
    counters in between: pt_counters_reset in the middle of a view and right before the re-initialisation (PtCounters::iterations then says
    2 and 0), and a view rendered by pt_iterate_until."""
    W, H = 37, 23
    sc = _scene(gpu, "cornell.txt", W, H)
    e0, e1, e2 = EYES["cornell.txt"]
    with gpu.renderer_from_test_library():
        _init(gpu, sc, e0, free=True)
        cam0 = gpu.test_temporal_camera(sc.camera)
        g0 = _guides(gpu, W, H)
        _render(gpu, 1, 8)
        gpu.counters_reset()
        _render(gpu, 9, 2)
        assert gpu.counters().iterations == 2
        S0, Q0 = _sums(gpu, W, H)
        _init(gpu, sc, e1)
        cam1 = gpu.test_temporal_camera(sc.camera)
        hist0 = tr.capture_form(S0, Q0, 10, *g0, *tr.empty_history(H, W)) + (g0[0], g0[1], cam0)
        assert _history_equals(gpu.test_history(), hist0) and (hist0[1] == 10).all()
        _render(gpu, 11, 3)
        S1, Q1 = _sums(gpu, W, H)
        g1 = _guides(gpu, W, H)
        gpu.counters_reset()                                     # right before the re-initialisation: the view still committed 3
        assert gpu.counters().iterations == 0
        _init(gpu, sc, e2)
        cam2 = gpu.test_temporal_camera(sc.camera)
        hist1 = tr.capture_form(S1, Q1, 3, *g1, *hist0) + (g1[0], g1[1], cam1)
        assert _history_equals(gpu.test_history(), hist1) and abs(hist1[1].max() - 13) < 1e-5
        _, done = gpu.iterate_until(1, 1e-4, 6, check_every=2)   # a threshold out of reach: the cap's 6 iterations
        assert done == 6
        S2, Q2 = _sums(gpu, W, H)
        g2 = _guides(gpu, W, H)
        want, _ = tr.denoise_var_temporal(S2, Q2, 6, *g2, hist1, 3, *SIGMAS)
        assert _same(gpu.denoise_var(6, 3, *SIGMAS), want)
        _init(gpu, sc, e0)
        hist2 = tr.capture_form(S2, Q2, 6, *g2, *hist1) + (g2[0], g2[1], cam2)
        assert _history_equals(gpu.test_history(), hist2)


# ---- 3: the flag changes nothing else -------------------------------------------------------------------------------------------------------
def _everything(gpu, w, h, n, levels=4):
    return dict(acc=gpu.readback(w * h), q=gpu.readback_moments(), var=gpu.variance(n), dn=gpu.denoise(n, levels), dv=gpu.denoise_var(n, levels, *SIGMAS),
                stats=gpu.noise_stats(n, 0.1, tile_map=True)["tile_rel_var"])


def test_the_flag_changes_nothing_else(gpu):
    W, H = 72, 40
    sc = _scene(gpu, "cornell.txt", W, H)
    e0, e1, _ = EYES["cornell.txt"]
    try:
        _init(gpu, sc, e0, temporal=False, free=True)
        _render(gpu, 1, 3)
        plain0 = _everything(gpu, W, H, 3)
        _init(gpu, sc, e1, temporal=False, free=True)
        _render(gpu, 4, 2)
        plain1 = _everything(gpu, W, H, 2)
        # the flag, before any re-initialisation: no history, everything the unflagged renderer's bits -- the filter included
        _init(gpu, sc, e0, free=True)
        _render(gpu, 1, 3)
        flagged0 = _everything(gpu, W, H, 3)
        assert all(_same(flagged0[k], plain0[k]) for k in plain0), [k for k in plain0 if not _same(flagged0[k], plain0[k])]
        # after a re-initialisation: both accumulators, the variance, the noise statistics and pt_denoise still; pt_denoise_var is the consumer
        _init(gpu, sc, e1)
        _render(gpu, 4, 2)
        flagged1 = _everything(gpu, W, H, 2)
        assert all(_same(flagged1[k], plain1[k]) for k in plain1 if k != "dv")
        assert not _same(flagged1["dv"], plain1["dv"])
        assert _same(gpu.readback(W * H), plain1["acc"]) and _same(gpu.readback_moments(), plain1["q"])     # ... and leaves them untouched
    finally:
        gpu.pathtraceFree()


# ---- 4: lifetime and refusals -----------------------------------------------------------------------------------------------------------------
def test_history_lifetime_and_refusals(gpu):
    W, H = 37, 23
    sc = _scene(gpu, "cornell.txt", W, H)
    e0, e1, e2 = EYES["cornell.txt"]
    live = gpu.test_lib().pt_test_live_device_buffers
    with gpu.renderer_from_test_library():
        def capture():
            """a context with history of view e0, its renderer at e1 with nothing committed"""
            _init(gpu, sc, e0, free=True)
            assert gpu.test_history() is None
            _render(gpu, 1, 2)
            _init(gpu, sc, e1)
            h = gpu.test_history()
            assert h is not None and (h["hn"] == 2).all()
            return h

        capture()
        gpu.pathtraceFree()                                      # pt_free drops it, and nothing stays allocated
        assert gpu.test_history() is None and live() == 0
        capture()
        _init(gpu, sc, e2, temporal=False)                       # a re-initialisation without the flag
        assert gpu.test_history() is None
        _init(gpu, sc, e2)                                       # ... after which a flagged one has nothing to capture from (the old one had no flag)
        assert gpu.test_history() is None
        capture()
        _render(gpu, 3, 1)
        sc2 = _scene(gpu, "cornell.txt", W + 3, H)
        gpu.pathtraceInit(sc2, traceDepth=4, moments=True, temporal=True)     # another resolution
        assert gpu.test_history() is None
        # refused pt_inits leave the history and the renderer as they were
        h = capture()
        _render(gpu, 3, 2)
        before = gpu.readback(W * H)
        for bad in (dict(moments=False), dict(trace_ahead=True, max_batch=4), dict(lens_radius=0.1, focal_distance=5.0)):
            kw = dict(traceDepth=4, moments=True, temporal=True)
            kw.update(bad)
            with pytest.raises(gpu.PtError, match="pt_amd error -1.*PT_FLAG_TEMPORAL"):
                gpu.pathtraceInit(sc, **kw)
            assert _history_equals(gpu.test_history(), [h[k] for k in ("hc", "hn", "hpos_t", "hnrm_id", "cam")])
            assert _same(gpu.readback(W * H), before)
        _render(gpu, 5, 1)                                       # the old renderer is usable
        assert not _same(gpu.readback(W * H), before)
        assert gpu.denoise_var(3, 2, *SIGMAS).shape == (W * H * 3,)
        # a re-initialisation over a renderer that committed nothing keeps the history there was, with its camera
        h = capture()
        _init(gpu, sc, e2)
        assert _history_equals(gpu.test_history(), [h[k] for k in ("hc", "hn", "hpos_t", "hnrm_id", "cam")])
        _render(gpu, 3, 2)
        S, Q = _sums(gpu, W, H)
        g = _guides(gpu, W, H)
        want, _ = tr.denoise_var_temporal(S, Q, 2, *g, (h["hc"], h["hn"], h["hpos_t"], h["hnrm_id"], h["cam"]), 3, *SIGMAS)
        assert _same(gpu.denoise_var(2, 3, *SIGMAS), want)
        gpu.pathtraceFree()
        assert live() == 0
    assert live() == 0


def test_refusals_on_a_fresh_context_leave_nothing(gpu):
    sc = _scene(gpu, "cornell.txt", 16, 16)
    gpu.pathtraceFree()
    for bad in (dict(moments=False), dict(trace_ahead=True, max_batch=4), dict(lens_radius=0.1, focal_distance=5.0)):
        kw = dict(traceDepth=4, moments=True, temporal=True)
        kw.update(bad)
        with pytest.raises(gpu.PtError, match="pt_amd error -1"):
            gpu.pathtraceInit(sc, **kw)
        assert gpu.lib().pt_readback(None) == -2                  # PT_ERR_NOT_INIT: nothing was initialised
    gpu.pathtraceFree()


# ---- 5: a caller-owned accumulator on the caller's stream -----------------------------------------------------------------------------------
def test_caller_owned_accumulator_and_stream(gpu):
    import torch
    W, H = 72, 40
    sc = _scene(gpu, "cornell.txt", W, H)
    e0, e1, _ = EYES["cornell.txt"]
    try:
        _init(gpu, sc, e0, free=True)
        _render(gpu, 1, 4)
        _init(gpu, sc, e1)
        _render(gpu, 5, 2)
        want = gpu.denoise_var(2, 4, *SIGMAS, with_variance=True)
        gpu.pathtraceFree()
        stream = torch.cuda.Stream()
        acc = [torch.zeros(W * H * 3, dtype=torch.float32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        _init(gpu, sc, e0, accum_dev=acc[0].data_ptr(), stream=stream.cuda_stream)
        _render(gpu, 1, 4)
        _init(gpu, sc, e1, accum_dev=acc[1].data_ptr(), stream=stream.cuda_stream)
        _render(gpu, 5, 2)
        got = gpu.denoise_var(2, 4, *SIGMAS, with_variance=True)
        gpu.sync()
        assert _same(got[0], want[0]) and _same(got[1], want[1])
        assert _same(acc[1].cpu().numpy(), gpu.readback(W * H)) and acc[0].cpu().numpy().any()
    finally:
        gpu.pathtraceFree()


# ---- 6: the headless driver ------------------------------------------------------------------------------------------------------------------
def test_pt_render_history_from(gpu, tmp_path):
    import subprocess
    from conftest import ROOT
    from test_host import _decode_png
    exe = os.path.join(ROOT, "project3-cuda-path-tracer_amd", "host", "pt_render")
    args = [exe, os.path.join(SCENES, "cornell.txt"), "--res", "64", "48", "--iterations", "2", "--depth", "4"]
    bad = subprocess.run(args + ["--out", str(tmp_path / "no"), "--history-from", "0.4", "5.1", "10.3", "6"], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "--denoise-var" in bad.stderr and os.listdir(tmp_path) == []
    r = subprocess.run(args + ["--out", str(tmp_path / "h"), "--denoise-var", "5", "4.0", "0.35", "2.0", "--history-from", "0.4", "5.1", "10.3", "6"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["h.denoised.png", "h.png"]
    sc = _scene(gpu, "cornell.txt", 64, 48)
    home = tuple(float(v) for v in sc.camera["position"][0])
    try:
        _init(gpu, sc, (0.4, 5.1, 10.3), free=True)
        _render(gpu, 1, 6)
        _init(gpu, sc, home)
        _render(gpu, 7, 2)
        frame = gpu.readback(64 * 48).reshape(48, 64, 3) / F(2)
        mean = gpu.denoise_var(2, 5, 4.0, 0.35, 2.0).reshape(48, 64, 3)
        _init(gpu, sc, home, temporal=False, free=True)
        _render(gpu, 7, 2)
        alone = gpu.denoise_var(2, 5, 4.0, 0.35, 2.0).reshape(48, 64, 3)
    finally:
        gpu.pathtraceFree()
    conv = lambda m: (np.clip(m, 0, 1) * F(255)).astype(np.uint8)[:, ::-1]          # the driver's PNG conversion, X mirrored
    assert np.array_equal(_decode_png(str(tmp_path / "h.png")), conv(frame))         # the second view's own samples
    got = _decode_png(str(tmp_path / "h.denoised.png"))
    assert np.array_equal(got, conv(mean)) and not np.array_equal(got, conv(alone))  # the filter of the blend, not of those samples alone
