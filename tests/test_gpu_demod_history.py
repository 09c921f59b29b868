"""Demodulated history (PT_FLAG_DEMOD_HISTORY) on the MI355X, every comparison bit for bit against the numpy restatement
(tests/temporal_demod_ref.py): the ALBEDO forms of k_temporal and the fused front over synthetic arrays that take every branch; rendered frames
of textured scenes through a camera move at 1, 2 and 4 new samples; a chain of three views; the display path; that nothing else moves; the
quality on the device's own frames of the textured wall; pt_render --history-albedo."""
import os
import subprocess

import numpy as np
import pytest

import demod_ref as dm
import denoise_ref as dr
import spatial_var_ref as sv
import temporal_demod_ref as td
import temporal_ref as tr
import textured_scenes as ts
from conftest import ROOT, SCENES
from test_gpu_demod import build as wall_scene
from test_gpu_temporal import _same_but_nans, _synthetic

pytestmark = pytest.mark.gpu
F = np.float32
SIGMAS = (4.0, 0.35, 2.0)
DEPTH = 4
E0, E1, E2 = (0.0, 5.0, 10.5), (0.4, 5.1, 10.3), (0.9, 4.8, 10.0)
EXE = os.path.join(ROOT, "project3-cuda-path-tracer_amd", "host", "pt_render")
KINDS = {"flagged": dict(temporal=True, demodulate=True, demod_history=True), "temporal": dict(temporal=True), "demod": dict(demodulate=True)}


@pytest.fixture(scope="module")
def gpu(pt):
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return pt


def _bits(a):
    return np.ascontiguousarray(a, F).reshape(-1).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _rmse(a, ref):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - ref) ** 2)))


# ---- 1: the kernel forms over host arrays ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(37, 23), (70, 5)])
def test_kernel_forms_on_synthetic_arrays_take_every_branch(gpu, w, h):
    """test_gpu_temporal's generator -- taps outside the frame, Hn = 0, another primitive, normal and plane rejections, NaN guides, counts on
    the cap -- with an albedo history and albedo sums that hold zeros, NaNs and infinities.  37 x 23 and 70 x 5: 851 and 350 pixels, no
    multiple of a wave or of a block of 256, so the last block is partial."""
    n = 3
    args = _synthetic(w, h, 11 * w + h)
    S, Q, pos_t, nrm_id, hc, hn, hpos, hnrm_id, cam = args
    rng = np.random.default_rng(w)
    special = np.array([np.nan, np.inf, 0.0, -0.0, 1e-40, 3e38], F)
    ha = rng.uniform(0, 1, (h, w, 4)).astype(F)
    m = rng.uniform(0, 1, ha.shape) < 0.05
    ha[m] = rng.choice(special, int(m.sum()))
    ha[..., 3] = np.nan                                      # (.w is never read)
    asum = (rng.uniform(0, 1, (h, w, 4)) * n).astype(F)
    m = rng.uniform(0, 1, asum.shape) < 0.08
    asum[m] = rng.choice(np.array([0.0, np.nan, 1e-3, np.inf], F), int(m.sum()))
    hist = (hc, hn, hpos, hnrm_id, cam, ha)
    # the inputs take the branches: pixels with and without history, counts on the cap, and bilinear weights on both sides of w_min
    cap, c_n, c_p, w_min = tr.constants()
    _, Nh = tr.reproject(pos_t, nrm_id, *hist[:5])
    assert (Nh == 0).sum() > w * h // 8 and (Nh > 0).sum() > w * h // 8 and (Nh == cap).any()
    has = lambda wm: tr.reproject(pos_t, nrm_id, *hist[:5], consts=(cap, c_n, c_p, F(wm)))[1] > 0
    assert (has(0.375) & ~(Nh > 0)).any() and ((Nh > 0) & ~has(0.625)).any()
    want_a = td.albedo_form(asum, n, pos_t, nrm_id, hist)
    assert np.isnan(want_a).any() and np.isfinite(want_a).sum() > want_a.size // 2 and (want_a[..., :3] == 0).any()
    common = (w, h, n, S, Q, pos_t, nrm_id, asum, hc, hn, ha, hpos, hnrm_id, cam)
    # the filter form
    want_c, want_v = tr.filter_form(S, Q, n, pos_t, nrm_id, *hist[:5])
    out, _, out_a = gpu.test_temporal_albedo(0, *common)
    assert _same_but_nans(out[:, :3], want_c) and _same_but_nans(out[:, 3], want_v) and _same_but_nans(out_a, want_a)
    # the ALBEDO = false form gives the same colour and variance
    assert _same_but_nans(gpu.test_temporal(False, w, h, n, *args), out)
    # the capture form
    want_hc, want_hn, want_ha = td.capture_form(S, Q, asum, n, pos_t, nrm_id, hist)
    out, out_n, out_a = gpu.test_temporal_albedo(1, *common)
    assert _same_but_nans(out, want_hc) and _same_but_nans(out_n, want_hn) and _same_but_nans(out_a, want_ha)
    assert _same_but_nans(want_ha, want_a)
    # the moments form
    want_m, want_n = sv.moments_form(S, Q, n, pos_t, nrm_id, hist[:5])
    out, out_n, out_a = gpu.test_temporal_albedo(2, *common)
    assert _same_but_nans(out, want_m) and _same_but_nans(out_n, want_n) and _same_but_nans(out_a, want_a)
    assert _same_but_nans(want_a[..., 3], want_n)           # .w is the uncapped tot
    # the fused front equals the two launches, and both the restatement
    want_img, _ = td.demodulated_front(S, Q, asum, n, pos_t, nrm_id, hist, SIGMAS[1], SIGMAS[2])
    fused, _, fused_a = gpu.test_temporal_albedo(0, *common, front=1)
    two, _, two_a = gpu.test_temporal_albedo(0, *common, front=2)
    assert _same_but_nans(fused, two) and _same_but_nans(fused_a, two_a)
    assert _same_but_nans(fused, want_img) and _same_but_nans(fused_a, want_a)
    assert (np.asarray(want_img)[..., :3] != np.asarray(want_c)).any()


# ---- the scenes and a camera move ---------------------------------------------------------------------------------------------------------
def _textured_small(pt, orc):
    """tests/textured_scenes.py's `mesh` scene -- every wall, a sphere, two cubes and two UV-mapped meshes textured -- at 48 x 32"""
    w, h = 48, 32
    cam = pt.Scene(os.path.join(SCENES, "cornell.txt"))
    cam.set_resolution(w, h)
    sc = ts.build(pt, orc, "mesh", False)
    sc.camera = cam.camera.copy()
    sc.traceDepth = DEPTH
    sc.image = np.zeros((h, w, 3), F)
    return sc


@pytest.fixture(scope="module")
def scenes(gpu, oracle):
    return {(48, 32): _textured_small(gpu, oracle), (130, 70): wall_scene(gpu, oracle, 130, 70)}


def _init(pt, sc, eye, kind="flagged", free=False, **opts):
    sc.camera["position"][0] = eye
    if free:
        pt.pathtraceFree()
    opts.setdefault("max_batch", 8)
    opts.setdefault("spatial_variance", True)
    pt.pathtraceInit(sc, traceDepth=DEPTH, moments=True, **KINDS[kind], **opts)


def _state(pt, w, h):
    """(S, Q, pos_t, nrm_id) of the current renderer, the guides of iteration 1 as the device holds them"""
    return (pt.readback(w * h).reshape(h, w, 3), pt.readback_moments().reshape(h, w)) + tr.pack_guides(*pt.gbuffer(1), h, w)


def _moved(gpu, sc, w, h, old=8, **opts):
    """inside renderer_from_test_library: `old` iterations at E0, then the re-initialisation at E1 with no free.  Returns the restatement's
    history of it."""
    _init(gpu, sc, E0, free=True, **opts)
    cam0 = gpu.test_temporal_camera(sc.camera)
    assert gpu.test_history() is None and gpu.test_history_albedo() is None
    gpu.pathtrace_batch(None, 0, 1, old)
    S0, Q0, p0, n0 = _state(gpu, w, h)
    a0 = gpu.test_albedo().reshape(h, w, 4)
    _init(gpu, sc, E1, **opts)
    return td.capture(S0, Q0, a0, old, p0, n0, cam0, td.empty_history(h, w))


@pytest.fixture(scope="module")
def moved(gpu, scenes):
    """Per frame, by the test library's renderer (the product's kernels, its own instance): 8 iterations at E0, the re-initialisation at E1,
    then 1, 2 and 4 iterations there -- the history as the context holds it and as the restatement captures it, and per count the sums, the
    albedo sums and pt_denoise_var's result.  Computed once; the tests below read it."""
    out = {}
    with gpu.renderer_from_test_library():
        for (w, h), sc in scenes.items():
            hist = _moved(gpu, sc, w, h)
            rec = dict(hist=hist, got_hist=gpu.test_history(), got_ha=gpu.test_history_albedo(), at={})
            done = 8
            for n in (1, 2, 4):
                gpu.pathtrace_batch(None, 0, done + 1, 8 + n - done)
                done = 8 + n
                S, Q, pos_t, nrm_id = _state(gpu, w, h)
                rec["at"][n] = dict(S=S, Q=Q, asum=gpu.test_albedo().reshape(h, w, 4), g=(pos_t, nrm_id), dv=gpu.denoise_var(n, 5, *SIGMAS, with_variance=True),
                                    forms=[gpu.test_denoise_var(n, form, 5, *SIGMAS) for form in (0, 1, 2, 3)] if (w, h) == (48, 32) or n == 2 else [],
                                    rgba=gpu.denoise_var_rgba8(n, 5, *SIGMAS))
            rec["cam1"] = gpu.test_temporal_camera(sc.camera)
            out[(w, h)] = rec
        gpu.pathtraceFree()
    return out


# ---- 2: rendered frames ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(48, 32), (130, 70)])
def test_the_capture_carries_the_albedo(gpu, moved, w, h):
    rec = moved[(w, h)]
    hist, got = rec["hist"], rec["got_hist"]
    assert got is not None and all(_same(got[k], hist[i]) for i, k in enumerate(("hc", "hn", "hpos_t", "hnrm_id", "cam")))
    assert rec["got_ha"] is not None and _same(rec["got_ha"], hist[5])
    ha = hist[5]
    assert (ha[..., 3] == 8).all() and (ha[..., :3] < 0.9).any() and (ha[..., :3] == 1).any()         # textures, and lights or misses


@pytest.mark.parametrize("n", [1, 2, 4])
@pytest.mark.parametrize("w,h", [(48, 32), (130, 70)])
def test_denoise_var_after_a_camera_move_is_the_restatement(gpu, moved, w, h, n):
    rec = moved[(w, h)]
    at = rec["at"][n]
    want, wantv = td.denoise_var_demod_history(at["S"], at["Q"], at["asum"], n, *at["g"], rec["hist"], 5, *SIGMAS)
    assert np.isfinite(want).all()
    got, gotv = at["dv"]
    assert _same(got, want) and _same(gotv, wantv)
    assert np.array_equal(at["rgba"], dr.to_rgba8(want))
    for form, (o, v) in enumerate(at["forms"]):
        assert _same(o, want) and _same(v, wantv), form
    # it is neither the temporal-only filter nor the other albedo multiplied back
    other = td.denoise_var_demod_history(at["S"], at["Q"], at["asum"], n, *at["g"], rec["hist"], 5, *SIGMAS,
                                         own_from=td.NEVER if n >= gpu.PT_DEMOD_HISTORY_MIN_OWN else 1)[0]
    assert not _same(want, other)
    plain = tr.denoise_var_temporal(at["S"], at["Q"], n, *at["g"], rec["hist"][:5], 5, *SIGMAS)[0] if n >= 2 else \
        sv.denoise_var_spatial(at["S"], at["Q"], n, *at["g"], 5, *SIGMAS, history=rec["hist"][:5])[0]
    assert not _same(want, plain)


def test_the_product_library_gives_the_same_frames(gpu, scenes, moved):
    """the same sequence through libpt_amd.so, other levels and sigmas included"""
    w, h = 48, 32
    sc, rec = scenes[(w, h)], moved[(w, h)]
    try:
        _init(gpu, sc, E0, free=True)
        gpu.pathtrace_batch(None, 0, 1, 8)
        _init(gpu, sc, E1)
        done = 8
        for n in (1, 2, 4):
            gpu.pathtrace_batch(None, 0, done + 1, 8 + n - done)
            done = 8 + n
            got, gotv = gpu.denoise_var(n, 5, *SIGMAS, with_variance=True)
            assert _same(got, rec["at"][n]["dv"][0]) and _same(gotv, rec["at"][n]["dv"][1]), n
        at = rec["at"][4]
        want, wantv = td.denoise_var_demod_history(at["S"], at["Q"], at["asum"], 4, *at["g"], rec["hist"], 2, 2.0, 0.5, 1.0)
        got, gotv = gpu.denoise_var(4, levels=2, sigma_lum=2.0, sigma_normal=0.5, sigma_position=1.0, with_variance=True)
        assert _same(got, want) and _same(gotv, wantv)
    finally:
        gpu.pathtraceFree()


# ---- 3: a chain of three views ----------------------------------------------------------------------------------------------------------------
def test_a_chain_of_three_views_is_recursive_and_the_counts_cap(gpu, scenes):
    """E0: 20 iterations, E1: 20, E2: 2.  The second capture is view 1's blend of ITS albedo history with ITS sums (Ha' = Ab), its colour count
    is capped at PT_TEMPORAL_MAX_HISTORY while .w of the albedo keeps the uncapped tot."""
    w, h = 48, 32
    sc = scenes[(w, h)]
    with gpu.renderer_from_test_library():
        hist0 = _moved(gpu, sc, w, h, old=20, max_batch=32)
        cam1 = gpu.test_temporal_camera(sc.camera)
        gpu.pathtrace_batch(None, 0, 21, 20)
        S1, Q1, p1, n1 = _state(gpu, w, h)
        a1 = gpu.test_albedo().reshape(h, w, 4)
        _init(gpu, sc, E2, max_batch=32)
        hist1 = td.capture(S1, Q1, a1, 20, p1, n1, cam1, hist0)
        got, ha = gpu.test_history(), gpu.test_history_albedo()
        assert all(_same(got[k], hist1[i]) for i, k in enumerate(("hc", "hn", "hpos_t", "hnrm_id", "cam"))) and _same(ha, hist1[5])
        cap = tr.constants()[0]
        assert hist1[1].max() == cap and hist1[5][..., 3].max() > cap and not _same(hist1[5][..., :3], a1[..., :3] / F(20))
        gpu.pathtrace_batch(None, 0, 41, 2)
        S2, Q2, p2, n2 = _state(gpu, w, h)
        a2 = gpu.test_albedo().reshape(h, w, 4)
        want, wantv = td.denoise_var_demod_history(S2, Q2, a2, 2, p2, n2, hist1, 5, *SIGMAS)
        got, gotv = gpu.denoise_var(2, 5, *SIGMAS, with_variance=True)
        assert _same(got, want) and _same(gotv, wantv)
        gpu.pathtraceFree()


# ---- 4: the display path ----------------------------------------------------------------------------------------------------------------------
def _pbo(w, h):
    import torch
    t = torch.full((w * h, 4), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def test_the_display_path_shows_the_flagged_filter(gpu, scenes, moved):
    """The count the bytes are made with is the one pt_iterate divides by -- its `iter` -- so the new view's iterations are numbered 1, 2, ...
    (by the test library's renderer, whose albedo sums can be read)."""
    w, h = 48, 32
    sc, hist = scenes[(w, h)], moved[(w, h)]["hist"]
    assert (gpu.PT_DISPLAY_LEVELS, gpu.PT_DISPLAY_GUIDE_ITER, gpu.PT_DISPLAY_SIGMA_LUM, gpu.PT_DISPLAY_SIGMA_NORMAL, gpu.PT_DISPLAY_SIGMA_POSITION) == (5, 1) + SIGMAS
    counts = sorted({1, 2, gpu.PT_DEMOD_HISTORY_MIN_OWN})
    pbo = _pbo(w, h)
    try:
        with gpu.renderer_from_test_library():
            _init(gpu, sc, E0, free=True, display_filter=True)
            gpu.pathtrace_batch(None, 0, 1, 8)
            _init(gpu, sc, E1, display_filter=True)
            for n in range(1, counts[-1] + 1):
                gpu.pathtrace(pbo.data_ptr(), 0, n, readback=False)
                if n not in counts:
                    continue
                gpu.sync()
                shown = pbo.cpu().numpy()
                S, Q, pos_t, nrm_id = _state(gpu, w, h)
                asum = gpu.test_albedo().reshape(h, w, 4)
                want = dr.to_rgba8(td.denoise_var_demod_history(S, Q, asum, n, pos_t, nrm_id, hist, 5, *SIGMAS)[0])
                assert np.array_equal(shown, want), n
                assert np.array_equal(gpu.readback_rgba8(n, w * h), want) and np.array_equal(gpu.denoise_var_rgba8(n), want), n
                plain = tr.denoise_var_temporal(S, Q, n, pos_t, nrm_id, hist[:5], 5, *SIGMAS)[0] if n >= 2 else \
                    sv.denoise_var_spatial(S, Q, n, pos_t, nrm_id, 5, *SIGMAS, history=hist[:5])[0]
                assert not np.array_equal(want, dr.to_rgba8(plain)), n
            gpu.pathtraceFree()
    finally:
        del pbo


def test_no_allocation_after_pt_init(gpu, scenes):
    w, h = 48, 32
    sc = scenes[(w, h)]
    pbo = _pbo(w, h)
    live = gpu.test_lib().pt_test_live_device_buffers
    with gpu.renderer_from_test_library():
        _init(gpu, sc, E0, free=True, display_filter=True, max_batch=2)
        gpu.pathtrace_batch(None, 0, 1, 2)
        _init(gpu, sc, E1, display_filter=True, max_batch=2)           # a context with history
        before = live()
        gpu.pathtrace(pbo.data_ptr(), 0, 1, readback=False)            # one sample: the moments form and the spatial estimate
        gpu.sync()
        first = live()
        gpu.pathtrace_batch(pbo.data_ptr(), 0, 2, 2)
        gpu.sync()
        assert before > 0 and (first, live()) == (before, before)
        assert np.array_equal(gpu.readback_rgba8(3, w * h), pbo.cpu().numpy()) and live() == before
        gpu.pathtraceFree()
        assert live() == 0
    del pbo


# ---- 5: nothing else moves --------------------------------------------------------------------------------------------------------------------
def _everything(gpu, w, h, n):
    """(one sample has no variance: pt_variance and pt_noise_stats refuse it for every renderer)"""
    out = dict(S=gpu.readback(w * h), Q=gpu.readback_moments(), asum=gpu.test_albedo(), plain=gpu.denoise(n), pos=gpu.gbuffer(2)[0], nrm=gpu.gbuffer(2)[1],
               geom=gpu.gbuffer(2)[2].view(F), dvar=gpu.denoise_var(n, 5, *SIGMAS), dvar1=gpu.denoise_var(n, 1, *SIGMAS))
    if n >= 2:
        st = gpu.noise_stats(n, 0.05, tile_map=True)
        out.update(var=gpu.variance(n), tile=st.pop("tile_rel_var"))
    return out


@pytest.mark.parametrize("n", [1, 3])
def test_without_history_the_renderer_is_the_demodulating_one(gpu, scenes, n):
    w, h = 48, 32
    sc = scenes[(w, h)]
    res = {}
    with gpu.renderer_from_test_library():
        for kind in ("demod", "flagged"):
            _init(gpu, sc, E0, kind=kind, free=True, max_batch=4)
            gpu.pathtrace_batch(None, 0, 1, n)
            res[kind] = _everything(gpu, w, h, n)
        gpu.pathtraceFree()
    diff = [k for k in res["demod"] if not _same(res["demod"][k], res["flagged"][k])]
    assert not diff, diff


def test_history_lifetime(gpu, scenes):
    w, h = 48, 32
    sc = scenes[(w, h)]
    live = gpu.test_lib().pt_test_live_device_buffers
    with gpu.renderer_from_test_library():
        _moved(gpu, sc, w, h, old=2)
        assert gpu.test_history_albedo() is not None
        gpu.pathtraceFree()                                      # pt_free drops it, and nothing stays allocated
        assert gpu.test_history() is None and gpu.test_history_albedo() is None and live() == 0
        # flagged -> unflagged temporal: the history is dropped, and so is what the unflagged one then captures for a flagged one
        _moved(gpu, sc, w, h, old=2)
        gpu.pathtrace_batch(None, 0, 3, 2)
        _init(gpu, sc, E2, kind="temporal")
        assert gpu.test_history() is None and gpu.test_history_albedo() is None
        gpu.pathtrace_batch(None, 0, 5, 2)
        S, Q, pos_t, nrm_id = _state(gpu, w, h)
        geom = np.ascontiguousarray(nrm_id[..., 3]).view(np.int32)
        import denoise_var_ref as dv
        assert _same(gpu.denoise_var(2, 5, *SIGMAS), dv.denoise_var(S, Q, 2, pos_t[..., :3], nrm_id[..., :3], geom, 5, *SIGMAS)[0])
        _init(gpu, sc, E1, kind="temporal")                      # unflagged -> unflagged: a history without albedo
        assert gpu.test_history() is not None and gpu.test_history_albedo() is None
        _init(gpu, sc, E0, kind="flagged")                       # unflagged temporal -> flagged: dropped
        assert gpu.test_history() is None and gpu.test_history_albedo() is None
        gpu.pathtrace_batch(None, 0, 7, 2)
        S, Q, pos_t, nrm_id = _state(gpu, w, h)
        a = gpu.test_albedo().reshape(h, w, 4)
        geom = np.ascontiguousarray(nrm_id[..., 3]).view(np.int32)
        assert _same(gpu.denoise_var(2, 5, *SIGMAS), dm.denoise_var_demod(S, Q, a, 2, pos_t[..., :3], nrm_id[..., :3], geom, 5, *SIGMAS)[0])
        # refused: the two flags without the new one, over a live flagged renderer -- which stays
        with pytest.raises(gpu.PtError, match="pt_amd error -1.*PT_FLAG_DEMODULATE is not for PT_FLAG_TEMPORAL"):
            gpu.pathtraceInit(sc, traceDepth=DEPTH, moments=True, temporal=True, demodulate=True)
        assert _same(gpu.readback(w * h), S)
        gpu.pathtraceFree()
        assert live() == 0


# ---- 6: quality on the device's own frames -----------------------------------------------------------------------------------------------
def test_the_textured_wall_after_a_move_is_closer_to_the_converged_frame(gpu, scenes):
    """130 x 70, the wall of 6.5-px cells: 16 samples at E0, 2 at E1, against the mean of 1024 at E1.  Over the textured back wall the flagged
    renderer's RMSE is below the temporal-only renderer's -- a condition, no ratio is fixed.  The figures printed here are the README's."""
    w, h = 130, 70
    sc = scenes[(w, h)]
    out = {}
    try:
        for kind in ("temporal", "flagged"):
            _init(gpu, sc, E0, kind=kind, free=True, max_batch=64)
            gpu.pathtrace_batch(None, 0, 1, 16)
            _init(gpu, sc, E1, kind=kind, max_batch=64)
            gpu.pathtrace_batch(None, 0, 17, 2)
            out[kind] = gpu.denoise_var(2, 5, *SIGMAS).reshape(h, w, 3)
        raw = gpu.readback(w * h).reshape(h, w, 3) / F(2)
        wall = gpu.gbuffer(1)[2].reshape(h, w) == 3
        for first in range(19, 1041, 64):
            gpu.pathtrace_batch(None, 0, first, min(64, 1041 - first))
        truth = (gpu.readback(w * h).reshape(h, w, 3) / F(1024)).astype(np.float64)
    finally:
        gpu.pathtraceFree()
    for name, m in (("frame", np.ones((h, w), bool)), ("textured wall", wall)):
        print("%-14s (%4d pixels) RMSE at 16 old + 2 new samples: unfiltered %.4f  temporal only %.4f  demodulated history %.4f" % (
            name, int(m.sum()), _rmse(raw[m], truth[m]), _rmse(out["temporal"][m], truth[m]), _rmse(out["flagged"][m], truth[m])))
    assert wall.sum() > 200
    assert _rmse(out["flagged"][wall], truth[wall]) < _rmse(out["temporal"][wall], truth[wall])


# ---- 7: the headless driver ------------------------------------------------------------------------------------------------------------------
def test_pt_render_history_albedo(gpu, tmp_path):
    from test_host import _decode_png
    W, H = 64, 48
    scene = os.path.join(SCENES, "cornell_textured.txt")
    args = [EXE, scene, "--res", str(W), str(H), "--iterations", "2", "--depth", "4", "--denoise-var", "5", "4.0", "0.35", "2.0",
            "--history-from", "0.4", "5.1", "10.3", "6"]
    for name, extra in (("t", []), ("a", ["--history-albedo"])):
        r = subprocess.run(args + extra + ["--out", str(tmp_path / name)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (name, r.stderr[-2000:])
    assert sorted(os.listdir(tmp_path)) == ["a.denoised.png", "a.png", "t.denoised.png", "t.png"]
    sc = gpu.Scene(scene)
    sc.set_resolution(W, H)
    home = tuple(float(v) for v in sc.camera["position"][0])
    mean = {}
    try:
        for kind in ("temporal", "flagged"):
            sc.camera["position"][0] = (0.4, 5.1, 10.3)
            gpu.pathtraceFree()
            gpu.pathtraceInit(sc, traceDepth=4, moments=True, max_batch=8, **KINDS[kind])
            gpu.pathtrace_batch(None, 0, 1, 6)
            sc.camera["position"][0] = home
            gpu.pathtraceInit(sc, traceDepth=4, moments=True, max_batch=8, **KINDS[kind])
            gpu.pathtrace_batch(None, 0, 7, 2)
            frame = gpu.readback(W * H).reshape(H, W, 3) / F(2)
            mean[kind] = gpu.denoise_var(2, 5, 4.0, 0.35, 2.0).reshape(H, W, 3)
    finally:
        gpu.pathtraceFree()
    conv = lambda m: (np.clip(m, 0, 1) * F(255)).astype(np.uint8)[:, ::-1]          # the driver's PNG conversion, X mirrored
    got = _decode_png(str(tmp_path / "a.denoised.png"))
    assert np.array_equal(_decode_png(str(tmp_path / "a.png")), conv(frame))         # the second view's own samples, textures bound
    assert np.array_equal(got, conv(mean["flagged"]))
    assert not np.array_equal(got, conv(mean["temporal"])) and not np.array_equal(got, _decode_png(str(tmp_path / "t.denoised.png")))
