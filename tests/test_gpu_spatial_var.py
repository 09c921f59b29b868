"""The spatial variance estimate (PT_FLAG_SPATIAL_VARIANCE) on the MI355X, every comparison bit for bit against the numpy restatement
(tests/spatial_var_ref.py): the kernel alone in both forms and at every radius over host arrays; a one-sample frame end to end -- pt_denoise_var,
its variance, the display's bytes in every level form; that from two samples on nothing moves; a one-sample view over a context with history;
no allocation after pt_init; the refusals; pt_render and the shim's switch."""
import os
import subprocess
import types

import numpy as np
import pytest

import denoise_ref as dr
import denoise_var_ref as dv
import spatial_var_ref as sv
import temporal_ref as tr
from conftest import ROOT, SCENES

pytestmark = pytest.mark.gpu
F = np.float32
EXE = os.path.join(ROOT, "project3-cuda-path-tracer_amd", "host", "pt_render")


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


def _scene(pt, scene, w, h):
    sc = pt.Scene(os.path.join(SCENES, scene))
    sc.set_resolution(w, h)
    return sc


def _init(pt, sc, spatial=True, display=True, **opts):
    pt.pathtraceInit(sc, traceDepth=4, moments=True, display_filter=display, spatial_variance=spatial, **opts)


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


def _sums(pt, w, h):
    return pt.readback(w * h).reshape(h, w, 3), pt.readback_moments().reshape(h, w)


def _guides(pt, w, h, guide_iter=1):
    return tr.pack_guides(*pt.gbuffer(guide_iter), h, w)


# ---- 1: the kernel alone --------------------------------------------------------------------------------------------------------------------
def _random_guides(rng, h, w, misses=True):
    pos = rng.normal(0, 3, (h, w, 3)).astype(F)
    nrm = rng.normal(0, 1, (h, w, 3)).astype(F)
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True).astype(F)
    geom = rng.integers(-1 if misses else 0, 4, (h, w)).astype(np.int32)
    pos[geom < 0] = 0
    nrm[geom < 0] = 0
    return pos, nrm, geom


# a single lane; smaller than any window; one row; partial tiles on both edges (twice); three tiles across
@pytest.mark.parametrize("w,h", [(1, 1), (2, 3), (17, 1), (33, 17), (67, 9), (130, 5)])
def test_kernel_alone_every_radius_and_form(gpu, w, h):
    rng = np.random.default_rng(100 * w + h)
    pos, nrm, geom = _random_guides(rng, h, w)
    M = rng.uniform(0, 3, (h, w, 4)).astype(F)
    M[..., 3] = rng.uniform(0, 12, (h, w)).astype(F)
    M[rng.uniform(0, 1, (h, w)) < 0.1] = 0                       # (pixels no sample reached)
    N = rng.choice(np.array([1.0, 1.5, 2.0, 7.25], F), (h, w), p=[0.35, 0.35, 0.15, 0.15])
    N[0, 0] = 1.0
    if w >= 64 and h >= 4:                                       # one tile none of whose pixels takes the estimate: the tiled form's early-out
        x0 = 64 * ((w // 64) - 1)
        N[0:4, x0:x0 + 64] = rng.choice(np.array([2.0, 7.25], F), (4, 64))
    if w * h > 16:
        N[h - 1, w - 1] = np.nan                                 # a NaN count takes the window
    pos_t = np.concatenate([pos, np.ones((h, w, 1), F)], axis=2)
    _, nrm_id = tr.pack_guides(pos_t, nrm, geom, h, w)
    for sn, sp in ((0.35, 2.0), (np.inf, 0.7)):
        for radius in (1, 2, 3):
            c, v, est = sv.spatial_variance(M, N, pos, nrm, geom, radius, sn, sp)
            assert est.mean() >= 0.25 and (w * h < 64 or (~est).any())
            for form in (0, 1):
                got = gpu.test_spatial_variance(radius, form, w, h, M, N, pos_t, nrm_id, sn, sp)
                assert _same(got[:, :3], c) and _same_but_nans(got[:, 3], v), (radius, form, sn)


# ---- 2: one sample, end to end ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,w,h", [("cornell.txt", 72, 40), ("sphere.txt", 33, 17)])
def test_one_sample_end_to_end(gpu, scene, w, h):
    sc = _scene(gpu, scene, w, h)
    pbo = _pbo(w, h)
    try:
        gpu.pathtraceFree()
        _init(gpu, sc)
        gpu.pathtrace(pbo.data_ptr(), 0, 1, readback=False)
        shown = _read(gpu, pbo)
        S, Q = _sums(gpu, w, h)
        g = _guides(gpu, w, h, gpu.PT_DISPLAY_GUIDE_ITER)
        want, wantv = sv.denoise_var_spatial(S, Q, 1, *g, *_setting(gpu))
        assert np.isfinite(want).all() and np.isfinite(wantv).all()
        got, gotv = gpu.denoise_var(1, with_variance=True)
        assert _same(got, want) and _same(gotv, wantv)
        assert _same(gpu.denoise_var(1), want)
        bytes_ = dr.to_rgba8(want)
        assert np.array_equal(shown, bytes_) and np.array_equal(gpu.denoise_var_rgba8(1), bytes_)
        assert np.array_equal(gpu.readback_rgba8(1, w * h), bytes_) and not (shown[:, 3] != 0).any()
        raw = dr.to_rgba8(S.reshape(-1, 3))
        assert raw.any()
        assert scene != "cornell.txt" or not np.array_equal(shown, raw)      # the filter did something to the one-sample frame
        # other parameters than the display's: the call's own sigmas weigh the window
        want2, wantv2 = sv.denoise_var_spatial(S, Q, 1, *g, 3, 2.0, 0.5, 1.0)
        got2, gotv2 = gpu.denoise_var(1, 3, 2.0, 0.5, 1.0, with_variance=True)
        assert _same(got2, want2) and _same(gotv2, wantv2)
    finally:
        gpu.pathtraceFree()
    # ... and through the test entries, every form of the levels (the last included), the last level writing the bytes itself or not
    with gpu.renderer_from_test_library():
        _init(gpu, sc, display=False)                            # (the entries need the two flags alone)
        gpu.pathtrace(None, 0, 1, readback=False)
        for form in (0, 1, 2, 3):
            o, v = gpu.test_denoise_var(1, form, *_setting(gpu))
            assert _same(o, want) and _same(v, wantv), form
            for fused in (True, False):
                pbo.fill_(0xCD)
                gpu.test_display(1, form, pbo.data_ptr(), fused=fused)
                assert np.array_equal(_read(gpu, pbo), bytes_), (form, fused)


# ---- 3: nothing else moves --------------------------------------------------------------------------------------------------------------------
def _everything(gpu, w, h, n, pbo):
    shown = _read(gpu, pbo)
    dn, dnv = gpu.denoise_var(n, with_variance=True)
    return dict(acc=gpu.readback(w * h), q=gpu.readback_moments(), var=gpu.variance(n), dn=dn, dnv=dnv, other=gpu.denoise_var(n, 3, 2.0, 0.5, 1.0, guide_iter=2),
                stats=gpu.noise_stats(n, 0.1, tile_map=True)["tile_rel_var"]), dict(shown=shown, host=gpu.denoise_var_rgba8(n), back=gpu.readback_rgba8(n, w * h))


def _schedule(gpu, name, ptr, at):
    """seven samples; at(n) is called with 2 and with 7 of them committed"""
    if name == "batch2+5":
        gpu.pathtrace_batch(ptr, 0, 1, 2)
        at(2)
        gpu.pathtrace_batch(ptr, 0, 3, 5)
        at(7)
    else:
        for it in range(1, 8):
            gpu.pathtrace(ptr, 0, it, readback=False)
            if it in (2, 7):
                at(it)


@pytest.mark.parametrize("schedule", ["iterate", "batch2+5", "trace_ahead"])
def test_from_two_samples_on_nothing_moves(gpu, schedule):
    W, H = 72, 40
    sc = _scene(gpu, "cornell.txt", W, H)
    pbo = _pbo(W, H)
    opts = dict(trace_ahead=True, max_batch=4, pipeline_depth=2) if schedule == "trace_ahead" else dict(max_batch=7)
    seen = {}
    try:
        for spatial in (False, True):
            gpu.pathtraceFree()
            _init(gpu, sc, spatial=spatial, **opts)
            _schedule(gpu, schedule, pbo.data_ptr(), lambda n: seen.__setitem__((spatial, n), _everything(gpu, W, H, n, pbo)))
    finally:
        gpu.pathtraceFree()
    for n in (2, 7):
        (f0, b0), (f1, b1) = seen[(False, n)], seen[(True, n)]
        assert all(_same(f0[k], f1[k]) for k in f0), (n, [k for k in f0 if not _same(f0[k], f1[k])])
        assert all(np.array_equal(b0[k], b1[k]) for k in b0), (n, [k for k in b0 if not np.array_equal(b0[k], b1[k])])
        assert np.array_equal(b1["shown"], b1["host"]) and np.array_equal(b1["shown"], b1["back"]) and b1["shown"].any()


# ---- 4: with history ----------------------------------------------------------------------------------------------------------------------------
def _sphere_before_a_wall(gpu, oracle, w, h):
    """a red sphere of radius 1.5 three units in front of a white wall, a floor, a light above (tests/test_temporal_cpu.py's): a sidestep of 1.5
    uncovers the strip of wall beside the sphere"""
    mats = np.zeros(3, oracle.MATERIAL_DTYPE)
    mats["color"] = [(1, 1, 1), (0.85, 0.85, 0.85), (0.8, 0.2, 0.2)]
    mats["emittance"] = [5, 0, 0]
    geoms = np.concatenate([oracle.make_geom(1, 0, (0, 8, 3), (0, 0, 0), (6, 0.3, 6)), oracle.make_geom(1, 1, (0, 0, -3), (0, 0, 0), (20, 20, 0.2)),
                            oracle.make_geom(1, 1, (0, -3, 0), (0, 0, 0), (20, 0.2, 20)), oracle.make_geom(0, 2, (0, 0, 1), (0, 0, 0), (3, 3, 3))])
    cam = np.zeros(1, oracle.CAMERA_DTYPE)
    cam["resolution"] = (w, h)
    cam["position"], cam["view"], cam["up"] = (0.0, 0.5, 8.0), (0, 0, -1), (0, 1, 0)
    cam["fov"] = (0.0, 30.0)
    oracle.lib().orc_camera_set_resolution(cam.ctypes.data, w, h)
    return types.SimpleNamespace(geoms=np.ascontiguousarray(geoms).view(gpu.GEOM_DTYPE), materials=np.ascontiguousarray(mats).view(gpu.MATERIAL_DTYPE),
                                 camera=cam.view(gpu.CAMERA_DTYPE), traceDepth=4, image=np.zeros((h, w, 3), F))


def test_one_sample_over_a_context_with_history(gpu, oracle):
    W, H = 72, 40
    sc = _sphere_before_a_wall(gpu, oracle, W, H)
    pbo = _pbo(W, H)
    try:
        gpu.pathtraceFree()
        _init(gpu, sc, temporal=True, max_batch=16)
        cam0 = gpu.test_temporal_camera(sc.camera)
        gpu.pathtrace_batch(None, 0, 1, 16)
        S0, Q0 = _sums(gpu, W, H)
        g0 = _guides(gpu, W, H)
        sc.camera["position"][0] = (1.5, 0.5, 8.0)
        _init(gpu, sc, temporal=True, max_batch=16)              # over the live renderer: the capture
        gpu.pathtrace(pbo.data_ptr(), 0, 1, readback=False)
        shown = _read(gpu, pbo)
        S1, Q1 = _sums(gpu, W, H)
        g1 = _guides(gpu, W, H)
        hist = tr.capture_form(S0, Q0, 16, *g0, *tr.empty_history(H, W)) + (g0[0], g0[1], cam0)
        M, N = sv.moments_form(S1, Q1, 1, *g1, hist)
        hit = np.ascontiguousarray(g1[1][..., 3]).view(np.int32) >= 0
        assert (N >= 2).sum() > W * H // 4 and (hit & (N < 2)).sum() > 16 and abs(float(N.max()) - 17) < 1e-4
        want, wantv = sv.denoise_var_spatial(S1, Q1, 1, *g1, *_setting(gpu), history=hist)
        assert np.isfinite(want).all() and np.isfinite(wantv).all()
        got, gotv = gpu.denoise_var(1, with_variance=True)
        assert _same(got, want) and _same(gotv, wantv)
        assert np.array_equal(shown, dr.to_rgba8(want)) and np.array_equal(gpu.readback_rgba8(1, W * H), shown)
        # the history is in it, and so is the estimate: neither the one-sample frame alone nor the blend with the pixels' own variances
        alone, _ = sv.denoise_var_spatial(S1, Q1, 1, *g1, *_setting(gpu))
        assert not _same(want, alone)
        # the moments form of k_temporal over the same arrays
        gm, gn = gpu.test_temporal(2, W, H, 1, S1, Q1, *g1, *hist)
        assert _same(gm, M) and _same(gn, N)
    finally:
        gpu.pathtraceFree()


# ---- 5: no allocation after pt_init ---------------------------------------------------------------------------------------------------------
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
        gpu.pathtrace_batch(pbo.data_ptr(), 0, 1, 1)             # the first frame: the estimate's two launches and the levels
        gpu.sync()
        first = live()
        shown = pbo.cpu().numpy()
        assert np.array_equal(gpu.readback_rgba8(1, W * H), shown) and shown.any() and live() == before
        gpu.pathtrace_batch(pbo.data_ptr(), 0, 2, 1)
        gpu.sync()
        assert before > 0 and (first, live()) == (before, before)
        assert np.array_equal(gpu.readback_rgba8(2, W * H), pbo.cpu().numpy()) and live() == before
        gpu.pathtraceFree()
        assert live() == 0


# ---- 6: refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    W, H = 33, 17
    sc = _scene(gpu, "cornell.txt", W, H)
    try:
        gpu.pathtraceFree()
        with pytest.raises(gpu.PtError, match="pt_amd error -1.*PT_FLAG_SPATIAL_VARIANCE"):
            gpu.pathtraceInit(sc, traceDepth=4, spatial_variance=True)
        assert gpu.lib().pt_readback(None) == -2                  # PT_ERR_NOT_INIT: nothing was initialised
        _init(gpu, sc, max_batch=2)
        gpu.pathtrace_batch(None, 0, 1, 1)
        before, shown = gpu.readback(W * H), gpu.denoise_var_rgba8(1)
        with pytest.raises(gpu.PtError, match="pt_amd error -1.*PT_FLAG_SPATIAL_VARIANCE"):
            gpu.pathtraceInit(sc, traceDepth=4, spatial_variance=True)
        assert b"PT_FLAG_SPATIAL_VARIANCE" in gpu.lib().pt_last_error()
        assert _same(gpu.readback(W * H), before)                 # the live renderer is as it was, and usable, still under the flag
        assert np.array_equal(gpu.denoise_var_rgba8(1), shown)
        # no samples is refused under the flag too; what needs a variance of the pixel's own keeps its two
        for call in (lambda: gpu.denoise_var(0), lambda: gpu.denoise_var_rgba8(0)):
            with pytest.raises(gpu.PtError, match="pt_amd error -1.*samples must be >= 1"):
                call()
        for call in (lambda: gpu.variance(1), lambda: gpu.noise_stats(1, 0.1)):
            with pytest.raises(gpu.PtError, match="pt_amd error -1.*a variance needs two"):
                call()
        with pytest.raises(gpu.PtError, match="pt_amd error -1.*min_samples"):
            gpu.iterate_until(2, 0.1, 8, min_samples=1)
        assert _same(gpu.readback(W * H), before)
        # without the flag one sample is refused as it was
        gpu.pathtraceFree()
        _init(gpu, sc, spatial=False, max_batch=2)
        gpu.pathtrace_batch(None, 0, 1, 1)
        for call in (lambda: gpu.denoise_var(1), lambda: gpu.denoise_var_rgba8(1)):
            with pytest.raises(gpu.PtError, match="pt_amd error -1.*a variance needs two"):
                call()
        assert np.array_equal(gpu.readback_rgba8(1, W * H), dr.to_rgba8(gpu.readback(W * H).reshape(-1, 3)))      # the display's first frame: the raw conversion
    finally:
        gpu.pathtraceFree()


# ---- 7: the headless driver and the shim's switch ---------------------------------------------------------------------------------------------
def test_pt_render_and_the_shims_switch(gpu, tmp_path):
    """pt_render is the reference's main() over this tree's shim.  --denoise-var with one iteration is refused as it was; --spatial-variance
    (through the C ABI with --batch, through the shim without) and the shim's PT_AMD_SPATIAL_VARIANCE=1 give the filtered first frame."""
    from test_host import _decode_png
    W, H = 64, 48
    args = [EXE, os.path.join(SCENES, "cornell.txt"), "--res", str(W), str(H), "--iterations", "1", "--depth", "4", "--denoise-var", "5", "4.0", "0.35", "2.0"]
    env = dict(os.environ)
    for k in ("PT_AMD_DEVICES", "PT_AMD_DISPLAY_FILTER", "PT_AMD_SPATIAL_VARIANCE"):
        env.pop(k, None)
    r = subprocess.run(args + ["--out", str(tmp_path / "no")], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode != 0 and "a variance needs two" in r.stderr and not os.path.exists(str(tmp_path / "no.denoised.png"))
    runs = {"flag": (["--spatial-variance"], env), "batch": (["--spatial-variance", "--batch", "4"], env),
            "shim": ([], dict(env, PT_AMD_SPATIAL_VARIANCE="1")), "both": ([], dict(env, PT_AMD_SPATIAL_VARIANCE="1", PT_AMD_DISPLAY_FILTER="1"))}
    for name, (extra, e) in runs.items():
        r = subprocess.run(args + extra + ["--out", str(tmp_path / name)], capture_output=True, text=True, timeout=120, env=e)
        assert r.returncode == 0, (name, r.stderr[-2000:])
    sc = _scene(gpu, "cornell.txt", W, H)
    try:
        gpu.pathtraceFree()
        _init(gpu, sc, display=False)
        gpu.pathtrace(None, 0, 1, readback=False)
        frame = gpu.readback(W * H).reshape(H, W, 3)
        mean = gpu.denoise_var(1, 5, 4.0, 0.35, 2.0).reshape(H, W, 3)
    finally:
        gpu.pathtraceFree()
    conv = lambda m: (np.clip(m, 0, 1) * F(255)).astype(np.uint8)[:, ::-1]          # the driver's PNG conversion, X mirrored
    assert not np.array_equal(conv(mean), conv(frame))
    for name in runs:
        assert np.array_equal(_decode_png(str(tmp_path / (name + ".png"))), conv(frame)), name          # the usual image: the raw sample
        assert np.array_equal(_decode_png(str(tmp_path / (name + ".denoised.png"))), conv(mean)), name
