"""The display filter (PT_FLAG_DISPLAY_FILTER) on the MI355X: the bytes a device PBO -- a torch.uint8 tensor -- receives from pathtrace /
pathtrace_batch under the flag, byte for byte against pt_denoise_var_rgba8 with the shipped setting, the numpy restatement
(tests/denoise_var_ref.py over the renderer's own accumulators and guide buffers) and pt_readback_rgba8; in every form of the last level
through the test entry; that nothing else moves; the blend with the history; buffers shared with pt_denoise_var calls of other parameters; no
allocation after pt_init; a caller's stream; pt_init's refusal; the shim under the reference's host."""
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as dr
import denoise_var_ref as dv
from conftest import ROOT, SCENES

pytestmark = pytest.mark.gpu
F = np.float32
# partial tiles on both edges, a one-pixel-high frame, a single lane
FRAMES = [(72, 40), (33, 17), (17, 1), (1, 1)]
DRIVER = os.path.join(ROOT, "oracle", "_ref", "ref_shim_driver")


@pytest.fixture(scope="module")
def gpu(pt):
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return pt


def _bits(a):
    return np.ascontiguousarray(a, F).reshape(-1).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _scene(pt, scene, w, h):
    sc = pt.Scene(os.path.join(SCENES, scene))
    sc.set_resolution(w, h)
    return sc


def _init(pt, sc, display=True, **opts):
    pt.pathtraceInit(sc, traceDepth=4, moments=True, display_filter=display, **opts)


def _pbo(w, h):
    import torch
    t = torch.full((w * h, 4), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def _read(pt, t):
    """the tensor's bytes once the renderer's stream has passed them"""
    pt.sync()
    return t.cpu().numpy()


def _setting(pt):
    return (pt.PT_DISPLAY_LEVELS, pt.PT_DISPLAY_SIGMA_LUM, pt.PT_DISPLAY_SIGMA_NORMAL, pt.PT_DISPLAY_SIGMA_POSITION)


def _restated(pt, w, h, n, guides=None):
    """the numpy restatement over the renderer's own accumulators and guide buffers of PT_DISPLAY_GUIDE_ITER, then the conversion"""
    S, Q = pt.readback(w * h).reshape(h, w, 3), pt.readback_moments().reshape(h, w)
    pos, nrm, geom = guides if guides is not None else pt.gbuffer(pt.PT_DISPLAY_GUIDE_ITER)
    c, _ = dv.denoise_var(S, Q, n, pos[:, :3].reshape(h, w, 3), nrm.reshape(h, w, 3), geom.reshape(h, w), *_setting(pt))
    assert np.isfinite(c).all()
    return dr.to_rgba8(c)


# ---- 1: the bytes equal the filter --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", FRAMES)
@pytest.mark.parametrize("scene", ["cornell.txt", "sphere.txt"])
def test_bytes_equal_the_filter(gpu, scene, w, h):
    sc = _scene(gpu, scene, w, h)
    pbo = _pbo(w, h)
    try:
        gpu.pathtraceFree()
        _init(gpu, sc, max_batch=7)
        gpu.pathtrace_batch(pbo.data_ptr(), 0, 1, 7)
        got = _read(gpu, pbo)
        host = gpu.denoise_var_rgba8(7)                          # the shipped setting is its default
        want = _restated(gpu, w, h, 7)
        assert np.array_equal(got, host) and np.array_equal(got, want) and np.array_equal(got, gpu.readback_rgba8(7, w * h))
        assert not (got[:, 3] != 0).any()
        raw = dr.to_rgba8(gpu.readback(w * h).reshape(-1, 3) / F(7))
        if h > 1:                                                # (the one-row frames' few central rays find no light in seven samples: black)
            assert raw.any()
            assert scene != "cornell.txt" or not np.array_equal(got, raw)    # the filter did something to the noisy frame
    finally:
        gpu.pathtraceFree()
    # ... and through the test entry, every form of the levels (the last included), the last level writing the bytes itself or not
    with gpu.renderer_from_test_library():
        _init(gpu, sc, display=False, max_batch=7)               # (the entry needs PT_FLAG_MOMENTS alone)
        gpu.pathtrace_batch(None, 0, 1, 7)
        for form in (0, 1, 2, 3):
            for fused in (True, False):
                pbo.fill_(0xCD)
                gpu.test_display(7, form, pbo.data_ptr(), fused=fused)
                assert np.array_equal(_read(gpu, pbo), want), (form, fused)
        gpu.test_display(1, 0, pbo.data_ptr())
        assert np.array_equal(_read(gpu, pbo), gpu.readback_rgba8(1, w * h))


# ---- 2: one sample ------------------------------------------------------------------------------------------------------------------------------
def test_one_sample_is_the_unfiltered_conversion(gpu):
    W, H = 33, 17
    sc = _scene(gpu, "cornell.txt", W, H)
    pbo = _pbo(W, H)
    try:
        gpu.pathtraceFree()
        _init(gpu, sc, display=False)
        gpu.pathtrace(None, 0, 1, readback=False)
        want = gpu.readback_rgba8(1, W * H)
        gpu.pathtraceFree()
        _init(gpu, sc)
        gpu.pathtrace(pbo.data_ptr(), 0, 1, readback=False)
        assert np.array_equal(_read(gpu, pbo), want) and want.any()
        assert np.array_equal(gpu.readback_rgba8(1, W * H), want)
    finally:
        gpu.pathtraceFree()


# ---- 3: nothing else moves ----------------------------------------------------------------------------------------------------------------------
def _schedule(gpu, name, ptr, after_call=None):
    if name == "iterate" or name == "trace_ahead":
        for it in range(1, 8):
            gpu.pathtrace(ptr, 0, it, readback=False)
            if after_call:
                after_call(it)
    elif name == "batch3+4":
        gpu.pathtrace_batch(ptr, 0, 1, 3)
        gpu.pathtrace_batch(ptr, 0, 4, 4)
    else:
        gpu.pathtrace_batch(ptr, 0, 1, 7)


@pytest.mark.parametrize("schedule", ["iterate", "batch3+4", "batch7", "trace_ahead"])
def test_nothing_else_moves(gpu, schedule):
    W, H = 72, 40
    sc = _scene(gpu, "cornell.txt", W, H)
    pbo = _pbo(W, H)
    opts = dict(max_batch=7)
    if schedule == "trace_ahead":
        opts = dict(trace_ahead=True, max_batch=4, pipeline_depth=2)
    try:
        gpu.pathtraceFree()
        _init(gpu, sc, display=False, **opts)
        _schedule(gpu, schedule, None)
        S0, Q0 = gpu.readback(W * H), gpu.readback_moments()
        var0, dn0, gb0 = gpu.variance(7), gpu.denoise_var(7, 3, 2.0, 0.5, 1.0, guide_iter=2), gpu.gbuffer(1)
        gpu.pathtraceFree()
        _init(gpu, sc, **opts)

        def check(it):
            # under the reference's protocol: the tensor after every call from the second on is the host path's at that count
            if schedule == "trace_ahead" and it >= 2:
                assert np.array_equal(_read(gpu, pbo), gpu.denoise_var_rgba8(it)), it

        _schedule(gpu, schedule, pbo.data_ptr(), check)
        assert _same(gpu.readback(W * H), S0) and _same(gpu.readback_moments(), Q0)
        assert np.array_equal(_read(gpu, pbo), gpu.denoise_var_rgba8(7))
        assert _same(gpu.variance(7), var0) and _same(gpu.denoise_var(7, 3, 2.0, 0.5, 1.0, guide_iter=2), dn0)
        assert all(np.array_equal(a, b) for a, b in zip(gpu.gbuffer(1), gb0))
        assert _same(gpu.readback(W * H), S0) and _same(gpu.readback_moments(), Q0)
    finally:
        gpu.pathtraceFree()


# ---- 4: history -------------------------------------------------------------------------------------------------------------------------------
def test_the_bytes_include_the_history(gpu):
    """moments + temporal + display_filter: eight iterations, a re-initialisation with the eye moved by 0.3 and no free in between, then two
    iterations of the new view with a PBO.  The count the bytes are made with is the one pt_iterate divides by -- its `iter` -- so the new
    view's two iterations are numbered 1, 2 for the tensor to be denoise_var_rgba8(2); numbered 9, 10 the tensor is denoise_var_rgba8(10), the
    host path at that count, which is checked as well."""
    W, H = 72, 40
    sc = _scene(gpu, "cornell.txt", W, H)
    home = tuple(float(v) for v in sc.camera["position"][0])
    moved = (home[0] + 0.3, home[1], home[2])
    pbo = _pbo(W, H)

    def views(temporal, first):
        sc.camera["position"][0] = home
        gpu.pathtraceFree()
        _init(gpu, sc, temporal=temporal)
        for it in range(1, 9):
            gpu.pathtrace(None, 0, it, readback=False)
        sc.camera["position"][0] = moved
        if not temporal:
            gpu.pathtraceFree()
        _init(gpu, sc, temporal=temporal)
        gpu.pathtrace(pbo.data_ptr(), 0, first, readback=False)
        gpu.pathtrace(pbo.data_ptr(), 0, first + 1, readback=False)
        return _read(gpu, pbo)

    try:
        got = views(True, 1)
        assert np.array_equal(got, gpu.denoise_var_rgba8(2)) and np.array_equal(got, gpu.readback_rgba8(2, W * H))
        alone = views(False, 1)
        assert np.array_equal(alone, gpu.denoise_var_rgba8(2))
        assert (got != alone).any()                              # the history is in the bytes
        got = views(True, 9)
        assert np.array_equal(got, gpu.denoise_var_rgba8(10))
        assert (got != views(False, 9)).any()
    finally:
        sc.camera["position"][0] = home
        gpu.pathtraceFree()


# ---- 5: buffers shared with pt_denoise_var -----------------------------------------------------------------------------------------------
def test_a_denoise_var_call_between_two_frames(gpu):
    W, H = 72, 40
    sc = _scene(gpu, "cornell.txt", W, H)
    pbo = _pbo(W, H)
    try:
        gpu.pathtraceFree()
        _init(gpu, sc, max_batch=3)
        g1, g3 = gpu.gbuffer(1), gpu.gbuffer(3)                  # (the cache now holds guide_iter 3: the first frame makes its own)
        gpu.pathtrace_batch(pbo.data_ptr(), 0, 1, 3)
        assert np.array_equal(_read(gpu, pbo), _restated(gpu, W, H, 3, g1))
        S, Q = gpu.readback(W * H).reshape(H, W, 3), gpu.readback_moments().reshape(H, W)
        want, _ = dv.denoise_var(S, Q, 3, g3[0][:, :3].reshape(H, W, 3), g3[1].reshape(H, W, 3), g3[2].reshape(H, W), 2, 1.0, 0.35, 2.0)
        assert _same(gpu.denoise_var(3, guide_iter=3, sigma_lum=1.0, levels=2), want)
        gpu.pathtrace_batch(pbo.data_ptr(), 0, 4, 3)
        got = _read(gpu, pbo)
        assert np.array_equal(got, _restated(gpu, W, H, 6, g1))
        assert not np.array_equal(got, _restated(gpu, W, H, 6, g3))         # (the other guides would have shown)
    finally:
        gpu.pathtraceFree()


# ---- 6: no allocation after pt_init ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("temporal", [False, True])
def test_no_allocation_after_pt_init(gpu, temporal):
    W, H = 33, 17
    sc = _scene(gpu, "cornell.txt", W, H)
    pbo = _pbo(W, H)
    live = gpu.test_lib().pt_test_live_device_buffers
    with gpu.renderer_from_test_library():
        gpu.pathtraceFree()
        _init(gpu, sc, max_batch=2, temporal=temporal)
        if temporal:                                             # a context with history
            gpu.pathtrace_batch(None, 0, 1, 2)
            _init(gpu, sc, max_batch=2, temporal=True)
        before = live()
        gpu.pathtrace_batch(pbo.data_ptr(), 0, 1, 2)
        gpu.sync()
        first = live()
        gpu.pathtrace_batch(pbo.data_ptr(), 0, 3, 2)
        gpu.sync()
        assert before > 0 and (first, live()) == (before, before)
        assert np.array_equal(gpu.readback_rgba8(4, W * H), pbo.cpu().numpy()) and live() == before
        gpu.pathtraceFree()
        assert live() == 0


# ---- 7: a caller's stream -------------------------------------------------------------------------------------------------------------------
def test_a_callers_stream(gpu):
    import torch
    W, H = 72, 40
    sc = _scene(gpu, "cornell.txt", W, H)
    try:
        gpu.pathtraceFree()
        _init(gpu, sc, max_batch=4)
        gpu.pathtrace_batch(None, 0, 1, 4)
        want = gpu.denoise_var_rgba8(4)
        gpu.pathtraceFree()
        side = torch.cuda.Stream()
        pbo = _pbo(W, H)
        _init(gpu, sc, max_batch=4, stream=side.cuda_stream)
        gpu.pathtrace_batch(pbo.data_ptr(), 0, 1, 4)
        side.synchronize()                                       # that stream alone: no pt_sync
        assert np.array_equal(pbo.cpu().numpy(), want)
    finally:
        gpu.pathtraceFree()


# ---- 8: refusals ------------------------------------------------------------------------------------------------------------------------------
def test_the_flag_without_moments_is_refused_and_leaves_the_renderer(gpu):
    W, H = 33, 17
    sc = _scene(gpu, "cornell.txt", W, H)
    pbo = _pbo(W, H)
    try:
        gpu.pathtraceFree()
        with pytest.raises(gpu.PtError, match="pt_amd error -1.*PT_FLAG_DISPLAY_FILTER"):
            gpu.pathtraceInit(sc, traceDepth=4, display_filter=True)
        assert gpu.lib().pt_readback(None) == -2                  # PT_ERR_NOT_INIT: nothing was initialised
        _init(gpu, sc, max_batch=2)
        gpu.pathtrace_batch(pbo.data_ptr(), 0, 1, 2)
        before, shown = gpu.readback(W * H), _read(gpu, pbo)
        with pytest.raises(gpu.PtError, match="pt_amd error -1.*PT_FLAG_DISPLAY_FILTER"):
            gpu.pathtraceInit(sc, traceDepth=4, display_filter=True)
        assert b"PT_FLAG_DISPLAY_FILTER" in gpu.lib().pt_last_error()
        assert _same(gpu.readback(W * H), before)                 # the live renderer is as it was ...
        gpu.pathtrace_batch(pbo.data_ptr(), 0, 3, 2)              # ... and usable, still under the flag
        got = _read(gpu, pbo)
        assert np.array_equal(got, gpu.denoise_var_rgba8(4)) and not np.array_equal(got, shown)
    finally:
        gpu.pathtraceFree()


# ---- 9: the shim under the reference's host -----------------------------------------------------------------------------------------------
def test_the_shim_under_the_references_host(gpu, tmp_path):
    if not os.path.exists(DRIVER):
        pytest.skip("oracle/_ref/ref_shim_driver is built only where /root/reference exists")
    outs = []
    for flag in (None, "1"):
        env = dict(os.environ)
        env.pop("PT_AMD_DEVICES", None)
        env.pop("PT_AMD_DISPLAY_FILTER", None)
        if flag:
            env["PT_AMD_DISPLAY_FILTER"] = flag
        out = str(tmp_path / ("o%s.bin" % (flag or "0")))
        r = subprocess.run([DRIVER, os.path.join(SCENES, "cornell.txt"), "6", out, "3", "0.5", "0.2", "-1", "0.05", "-0.1"],
                           capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "last iteration 6" in r.stdout
        outs.append(open(out, "rb").read())
    assert len(outs[0]) > 52 and outs[0] == outs[1]              # scene->state.image stays the raw sum
    # (the shim's refusal with PT_AMD_DEVICES is checked through pt_render, which every build makes from this tree's shim:
    # tests/test_display_cpu.py -- a prebuilt driver may carry an older one)
