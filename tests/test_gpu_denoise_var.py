"""Second moments, the variance of the mean and the variance-guided filter on the MI355X, every comparison bit for bit: the moments buffer
against the CPU oracle's single iterations under every commit schedule, pt_variance and pt_denoise_var against the numpy restatement
(tests/denoise_var_ref.py) fed with the device's own accumulators and guides, every form of k_atrous_*<AtrousGuided> against the others, the 8-bit form,
what the calls leave behind, the refusals and the headless driver's --denoise-var.  Frames as in test_gpu_denoise.py: widths off a multiple
of 64, heights off a multiple of 8.  pt_denoise_var (and form 0) takes 64 x 8 tiles up to step 8 (kAtrousVarTiledMaxStep) and the gather above:
the cases of five and of eight levels cross that switch -- tiled levels hand their ping-pong image to gather levels, at steps 16 and
16 .. 128 (wider than the frame) --, those of four and three levels stay below it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as dr
import denoise_var_ref as dv
from conftest import ROOT, SCENES

pytestmark = pytest.mark.gpu
F = np.float32
SIGMAS = (4.0, 0.35, 2.0)
FRAMES = [("cornell.txt", 70, 37, 5), ("sphere.txt", 48, 32, 4), ("cornell.txt", 257, 9, 3), ("cornell.txt", 70, 37, 8), ("sphere.txt", 48, 32, 6)]


@pytest.fixture(scope="module")
def gpu(pt):
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return pt


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _init(pt, scene, w, h, iterations, depth=4, free=True, moments=True, **opts):
    sc = pt.Scene(os.path.join(SCENES, scene))
    sc.set_resolution(w, h)
    if free:
        pt.pathtraceFree()
    pt.pathtraceInit(sc, traceDepth=depth, moments=moments, **opts)
    for it in range(1, iterations + 1):
        pt.pathtrace(None, 0, it, readback=False)
    return sc


def _want(pt, w, h, samples, levels, sl, sn, sp, guide_iter=1):
    """the restatement over the device's own accumulators and guide buffers: (rgb (W*H*3,), variance (W*H,))"""
    acc, q = pt.readback(w * h), pt.readback_moments()
    pos_t, nrm, geom = pt.gbuffer(guide_iter)
    c, v = dv.denoise_var(acc.reshape(h, w, 3), q.reshape(h, w), samples, pos_t[:, :3].reshape(h, w, 3), nrm.reshape(h, w, 3),
                          geom.reshape(h, w), levels, sl, sn, sp)
    return c.reshape(-1), v.reshape(-1)


# ---- 1: the second moments --------------------------------------------------------------------------------------------------------------
MW, MH, MN = 70, 37, 7


@pytest.fixture(scope="module")
def seven(gpu, oracle):
    """Cornell 70 x 37, depth 4: the oracle's seven single iterations (each into a zeroed accumulator), and the unflagged renderer's frame"""
    sc = gpu.Scene(os.path.join(SCENES, "cornell.txt"))
    sc.set_resolution(MW, MH)
    ref = oracle.Renderer(sc.camera.view(oracle.CAMERA_DTYPE), sc.geoms.view(oracle.GEOM_DTYPE), sc.materials.view(oracle.MATERIAL_DTYPE), 4)
    singles = []
    for it in range(1, MN + 1):
        one = np.zeros(MW * MH * 3, F)
        ref.iterate(it, one)
        singles.append(one.reshape(-1, 3))
    _init(gpu, "cornell.txt", MW, MH, MN, moments=False)
    try:
        frame = gpu.readback(MW * MH)
    finally:
        gpu.pathtraceFree()
    return singles, frame


def _run(gpu, schedule):
    if schedule == "iterate":
        for it in range(1, MN + 1):
            gpu.pathtrace(None, 0, it, readback=False)
    elif schedule == "batch7":
        gpu.pathtrace_batch(None, 0, 1, 7)
    else:
        gpu.pathtrace_batch(None, 0, 1, 3)
        gpu.pathtrace_batch(None, 0, 4, 4)


@pytest.mark.parametrize("schedule,opts", [("iterate", {}), ("batch7", dict(max_batch=8)), ("batch3+4", dict(max_batch=4)),
                                           ("iterate", dict(trace_ahead=True, max_batch=4)), ("iterate", dict(pipeline_depth=1)),
                                           ("batch3+4", dict(max_batch=4, pipeline_depth=3)),
                                           ("iterate", dict(trace_ahead=True, max_batch=4, pipeline_depth=3)), ("batch7", dict(max_batch=7, pipeline_depth=1))])
def test_moments_equal_the_oracles_single_iterations(gpu, seven, schedule, opts):
    singles, frame = seven
    _init(gpu, "cornell.txt", MW, MH, 0, **opts)
    try:
        _run(gpu, schedule)
        q, acc = gpu.readback_moments(), gpu.readback(MW * MH)
    finally:
        gpu.pathtraceFree()
    want = dv.moments(singles)
    assert want.any() and _same(q, want)
    assert _same(acc, frame)                                    # the accumulator does not know of the flag


def test_moments_of_a_broken_trace_ahead_sequence_and_of_a_second_init(gpu, seven):
    singles, _ = seven
    _init(gpu, "cornell.txt", MW, MH, 2, trace_ahead=True, max_batch=4)
    try:
        assert _same(gpu.readback_moments(), dv.moments(singles[:2]))        # iterations 3 and 4 are traced, parked, and do not count
        gpu.pathtrace(None, 0, 6, readback=False)                            # not the next one: what is parked is discarded
        assert _same(gpu.readback_moments(), dv.moments([singles[0], singles[1], singles[5]]))
        _init(gpu, "cornell.txt", MW, MH, 0, free=False)                     # pt_init over the live renderer
        assert not gpu.readback_moments().any()
        gpu.pathtrace(None, 0, 1, readback=False)
        assert _same(gpu.readback_moments(), dv.moments(singles[:1]))
    finally:
        gpu.pathtraceFree()


# ---- 2: the variance and the filter -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,w,h,levels", FRAMES)
def test_variance_and_filter_equal_the_restatement(gpu, scene, w, h, levels):
    _init(gpu, scene, w, h, 3)
    try:
        acc, q = gpu.readback(w * h), gpu.readback_moments()
        assert _same(gpu.variance(3), dv.variance(acc.reshape(-1, 3), q, 3))
        assert _same(gpu.variance(2), dv.variance(acc.reshape(-1, 3), q, 2))
        cases = [SIGMAS]
        if w == 70:
            cases += [(np.inf, 0.35, 2.0), (4.0, np.inf, 2.0), (4.0, 0.35, np.inf), (0.5, 1.0, 0.7)]
        for sg in cases:
            want, wantv = _want(gpu, w, h, 3, levels, *sg)
            assert np.isfinite(want).all() and np.isfinite(wantv).all() and wantv.any()
            got, gotv = gpu.denoise_var(3, levels, *sg, with_variance=True)
            assert _same(got, want) and _same(gotv, wantv), sg
            assert _same(gpu.denoise_var(3, levels, *sg), want)                 # var_host NULL: the same colours
            assert np.array_equal(gpu.denoise_var_rgba8(3, levels, *sg), dr.to_rgba8(want))
    finally:
        gpu.pathtraceFree()


@pytest.mark.parametrize("scene,w,h,levels", FRAMES)
def test_every_kernel_form_gives_the_same_bits(gpu, scene, w, h, levels):
    with gpu.renderer_from_test_library():
        _init(gpu, scene, w, h, 2)
        want, wantv = _want(gpu, w, h, 2, levels, *SIGMAS)
        outs = [gpu.test_denoise_var(2, form, levels, *SIGMAS) for form in (0, 1, 2, 3)]
    for o, v in outs:
        assert _same(o, want) and _same(v, wantv)


@pytest.mark.parametrize("scene,w,h,levels", FRAMES[:2])
def test_the_two_filters_share_one_skeleton(gpu, scene, w, h, levels):
    """AtrousPlain and AtrousGuided differ in the colour term alone once it is off: with sigma_lum = +inf the guided filter's RGB is the
    plain filter's with sigma_color = +inf, bit for bit (both terms are an exact + 0), in each kernel form, over the same accumulator,
    sample count, sigma_normal, sigma_position and guides (tests/test_denoise_var_cpu.py holds the two restatements to the same)."""
    _, sn, sp = SIGMAS
    with gpu.renderer_from_test_library():
        _init(gpu, scene, w, h, MN)
        outs = [(gpu.test_denoise(MN, form, levels, np.inf, sn, sp), gpu.test_denoise_var(MN, form, levels, np.inf, sn, sp)[0]) for form in (0, 1, 2, 3)]
    for plain, guided in outs:
        assert np.isfinite(plain).all() and plain.any() and _same(guided, plain)


# ---- 3: neighbours ------------------------------------------------------------------------------------------------------------------------
def test_the_flag_changes_nothing_else(gpu):
    W, H = 70, 37
    _init(gpu, "cornell.txt", W, H, 3, moments=False)
    try:
        plain = gpu.denoise(3, 5, 2.0, 0.35, 2.0)
        gpu.pathtrace(None, 0, 4, readback=False)
        after = gpu.readback(W * H)
    finally:
        gpu.pathtraceFree()
    live = gpu.test_lib().pt_test_live_device_buffers
    with gpu.renderer_from_test_library():
        _init(gpu, "cornell.txt", W, H, 3)
        before, q = gpu.readback(W * H), gpu.readback_moments()
        assert _same(gpu.denoise(3, 5, 2.0, 0.35, 2.0), plain)      # pt_denoise on a flagged renderer: the unflagged renderer's bits
        a = gpu.denoise_var(3, 5, *SIGMAS)
        gpu.variance(3)
        assert _same(gpu.denoise_var(3, 5, *SIGMAS), a)
        assert _same(gpu.readback(W * H), before) and _same(gpu.readback_moments(), q)      # both accumulators untouched ...
        gpu.pathtrace(None, 0, 4, readback=False)                   # ... and rendering goes on
        assert _same(gpu.readback(W * H), after)
        assert live() > 0
        gpu.pathtraceFree()
        assert live() == 0
    assert live() == 0


def test_caller_owned_accumulator(gpu):
    import torch
    W, H = 70, 37
    acc = torch.zeros(W * H * 3, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    _init(gpu, "cornell.txt", W, H, 2, accum_dev=acc.data_ptr())
    try:
        want, wantv = _want(gpu, W, H, 2, 4, *SIGMAS)
        got, gotv = gpu.denoise_var(2, 4, *SIGMAS, with_variance=True)
        gpu.sync()
        mine = acc.cpu().numpy()
        assert _same(got, want) and _same(gotv, wantv) and _same(mine, gpu.readback(W * H))
        assert gpu.readback_moments().any()                         # the moments are the library's own buffer all the same
    finally:
        gpu.pathtraceFree()


# ---- 4: refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    W, H = 16, 16
    L = gpu.lib()
    out = np.full(W * H * 3, 7, F)
    var = np.full(W * H, 7, F)
    p8 = np.zeros(W * H * 4, np.uint8)

    def call(samples=2, levels=3, guide_iter=1, sl=1.0, sn=1.0, sp=1.0, size=None):
        prm = gpu.PtDenoiseVarParams(levels, guide_iter, sl, sn, sp)
        size = C.sizeof(prm) if size is None else size
        rc = L.pt_denoise_var(samples, C.byref(prm), size, _vp(out), _vp(var))
        assert L.pt_denoise_var_rgba8(samples, C.byref(prm), size, _vp(p8)) == rc
        return rc

    _init(gpu, "cornell.txt", W, H, 2)
    try:
        before, q = gpu.readback(W * H), gpu.readback_moments()
        for bad in (dict(levels=0), dict(levels=9), dict(levels=-1), dict(sl=0.0), dict(sn=-1.0), dict(sp=float("nan")), dict(sl=float("nan")),
                    dict(sl=-2.0), dict(sn=0.0), dict(sp=-np.inf), dict(size=16), dict(size=24), dict(samples=1), dict(samples=0), dict(samples=-3),
                    dict(guide_iter=0)):
            assert call(**bad) == -1, bad                       # PT_ERR_INVALID
            assert (out == 7).all() and (var == 7).all() and not p8.any()
        assert L.pt_denoise_var(2, None, 20, _vp(out), None) == -1
        for s in (1, 0, -1):
            assert L.pt_variance(s, _vp(var)) == -1 and (var == 7).all()
        assert L.pt_variance(2, None) == -1 and L.pt_readback_moments(None) == -1
        assert call(sl=float("inf"), sn=float("inf"), sp=float("inf")) == 0          # ... and the renderer is usable afterwards
        assert _same(gpu.readback(W * H), before) and _same(gpu.readback_moments(), q)
    finally:
        gpu.pathtraceFree()
    # without the flag
    _init(gpu, "cornell.txt", W, H, 2, moments=False)
    try:
        out[:] = 7
        var[:] = 7
        assert call() == -1 and b"PT_FLAG_MOMENTS" in L.pt_last_error()
        assert L.pt_variance(2, _vp(var)) == -1 and L.pt_readback_moments(_vp(var)) == -1
        assert (out == 7).all() and (var == 7).all()
        assert gpu.denoise(2, 3).shape == (W * H * 3,)          # the plain filter is there as before
    finally:
        gpu.pathtraceFree()
    # the flag on a row shard, and in a group
    sc = gpu.Scene(os.path.join(SCENES, "cornell.txt"))
    sc.set_resolution(W, H)
    for opts in (dict(shard_rank=1, shard_count=2), dict(flags=gpu.PT_FLAG_ACCUM_SHARD_ROWS)):
        with pytest.raises(gpu.PtError, match="pt_amd error -1"):
            gpu.pathtraceInit(sc, traceDepth=4, moments=True, **opts)
        gpu.pathtraceFree()
    g = C.c_void_p()
    assert L.pt_group_create(C.byref(g), 1, None) == 0
    try:
        opt = gpu.PtOptions(0, 1, -1, gpu.PT_FLAG_MOMENTS, 0, 0, None, None, 0.0, 0.0)
        cam, geoms, mats = (np.ascontiguousarray(x) for x in (sc.camera, sc.geoms, sc.materials))
        assert L.pt_group_init(g, _vp(cam), _vp(geoms), len(geoms), _vp(mats), len(mats), 4, C.byref(opt)) == -1
        assert b"PT_FLAG_MOMENTS" in L.pt_last_error()
        opt.flags = 0
        assert L.pt_group_init(g, _vp(cam), _vp(geoms), len(geoms), _vp(mats), len(mats), 4, C.byref(opt)) == 0      # the group is usable
    finally:
        L.pt_group_destroy(g)
    _init(gpu, "cornell.txt", W, H, 2)                          # ... and so is the default context
    try:
        assert call() == 0
    finally:
        gpu.pathtraceFree()


# ---- 5: the headless driver ----------------------------------------------------------------------------------------------------------------
def test_pt_render_denoise_var(gpu, tmp_path):
    from test_host import _decode_png
    exe = os.path.join(ROOT, "project3-cuda-path-tracer_amd", "host", "pt_render")
    args = [exe, os.path.join(SCENES, "cornell.txt"), "--res", "64", "48", "--iterations", "4", "--depth", "4"]
    both = subprocess.run(args + ["--out", str(tmp_path / "no"), "--denoise", "5", "2.0", "0.35", "2.0", "--denoise-var", "5", "4.0", "0.35", "2.0"],
                          capture_output=True, text=True, timeout=120)
    assert both.returncode != 0 and "exclude" in both.stderr and os.listdir(tmp_path) == []
    r = subprocess.run(args + ["--out", str(tmp_path / "dv"), "--denoise-var", "5", "4.0", "0.35", "2.0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["dv.denoised.png", "dv.png"]
    _init(gpu, "cornell.txt", 64, 48, 4)
    try:
        frame = gpu.readback(64 * 48).reshape(48, 64, 3) / F(4)
        mean = gpu.denoise_var(4, 5, 4.0, 0.35, 2.0).reshape(48, 64, 3)
    finally:
        gpu.pathtraceFree()
    conv = lambda m: (np.clip(m, 0, 1) * F(255)).astype(np.uint8)[:, ::-1]          # the driver's PNG conversion, X mirrored
    plain = _decode_png(str(tmp_path / "dv.png"))
    got = _decode_png(str(tmp_path / "dv.denoised.png"))
    assert np.array_equal(plain, conv(frame))                   # the usual image, as a renderer without the flag writes it
    assert np.array_equal(got, conv(mean)) and not np.array_equal(got, plain)
