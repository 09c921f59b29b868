"""The denoiser on the MI355X, every comparison bit for bit: the guide buffers against the CPU oracle (camera_ray + intersect / mesh_intersect
with the nearest_hit rule), the filter against the numpy restatement (tests/denoise_ref.py) fed with the device's own readback and guides --
frames that cross tile borders, residue classes and frame borders in both axes --, every form of k_atrous_*<AtrousPlain> against the others, the 8-bit
form, what the calls leave behind, the refusals and the headless driver's --denoise."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as dr
from conftest import ROOT, SCENES

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def gpu(pt):
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return pt


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _init(pt, scene, w, h, iterations, depth=4, free=True, **opts):
    sc = pt.Scene(os.path.join(SCENES, scene))
    sc.set_resolution(w, h)
    if free:
        pt.pathtraceFree()
    pt.pathtraceInit(sc, traceDepth=depth, **opts)
    for it in range(1, iterations + 1):
        pt.pathtrace(None, 0, it, readback=False)
    return sc


def _want(pt, w, h, samples, levels, sc_, sn, sp, guide_iter=1):
    """the restatement over the device's own accumulator and guide buffers"""
    acc = pt.readback(w * h)
    pos_t, nrm, geom = pt.gbuffer(guide_iter)
    return dr.denoise(acc.reshape(h, w, 3), samples, pos_t[:, :3].reshape(h, w, 3), nrm.reshape(h, w, 3), geom.reshape(h, w), levels, sc_, sn,
                      sp).reshape(-1)


# ---- 1: the guide buffers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,w,h,guide_iter,lens", [("cornell.txt", 70, 37, 1, None), ("sphere.txt", 48, 32, 3, None),
                                                       ("mesh_small.txt", 48, 48, 1, None), ("mesh_attributes.txt", 32, 32, 2, None),
                                                       ("cornell.txt", 33, 21, 5, (0.4, 12.5))])
def test_gbuffer_equals_the_oracle(gpu, oracle, scene, w, h, guide_iter, lens):
    extras = dict(lens_radius=lens[0], focal_distance=lens[1]) if lens else {}
    sc = _init(gpu, scene, w, h, 0, **extras)
    try:
        pos_t, nrm, geom = gpu.gbuffer(guide_iter)
    finally:
        gpu.pathtraceFree()
    ref = oracle.Renderer(sc.camera.view(oracle.CAMERA_DTYPE), sc.geoms.view(oracle.GEOM_DTYPE), sc.materials.view(oracle.MATERIAL_DTYPE), 4,
                          meshes=getattr(sc, "meshes", None), mesh_normals=getattr(sc, "mesh_normals", None))
    if lens:
        ref.set_extras(lens_radius=lens[0], focal_distance=lens[1])
    w_pos, w_nrm, w_geom = dr.oracle_guides(oracle, ref, guide_iter, getattr(sc, "meshes", None), getattr(sc, "mesh_normals", None))
    assert (w_geom >= 0).any()                               # the frame has hits (sphere.txt at 48 x 32: 20 pixels of one small sphere) ...
    if scene == "sphere.txt":
        assert (w_geom < 0).any()                            # ... and misses
    if scene == "mesh_attributes.txt":
        assert sc.mesh_normals                               # vertex normals: the blended shading normal
    assert np.array_equal(geom, w_geom)
    assert _same(pos_t, w_pos) and _same(nrm, w_nrm)
    assert _same(pos_t[geom < 0], np.tile(np.array([0, 0, 0, -1], F), ((geom < 0).sum(), 1)))


# ---- 2: the filter ----------------------------------------------------------------------------------------------------------------------
CASES = [("cornell.txt", 70, 37, 5, 2.0, 0.35, 2.0),          # odd sides; taps at +-32 leave the frame on every side
         ("cornell.txt", 16, 16, 1, 0.6, 0.35, 1.0),          # one level: the first is the last
         ("cornell.txt", 257, 9, 3, 1.0, 0.5, 1.5),           # five tiles wide at step 1, one pixel into the fifth
         ("sphere.txt", 48, 32, 4, 2.0, 0.35, 2.0),           # hits next to misses
         ("cornell.txt", 70, 37, 4, 0.8, np.inf, 0.7),        # a term switched off
         ("cornell.txt", 130, 40, 8, 3.0, 0.6, 3.0)]          # every level there is: steps up to 128, wider than the frame


@pytest.mark.parametrize("scene,w,h,levels,sc_,sn,sp", CASES)
def test_denoise_equals_the_restatement(gpu, scene, w, h, levels, sc_, sn, sp):
    _init(gpu, scene, w, h, 3)
    try:
        want = _want(gpu, w, h, 3, levels, sc_, sn, sp)
        got = gpu.denoise(3, levels, sc_, sn, sp)
        rgba = gpu.denoise_rgba8(3, levels, sc_, sn, sp)
    finally:
        gpu.pathtraceFree()
    assert np.isfinite(want).all()
    assert _same(got, want)
    assert np.array_equal(rgba, dr.to_rgba8(want))


@pytest.mark.parametrize("scene,w,h,levels", [("cornell.txt", 70, 37, 5), ("sphere.txt", 48, 32, 4), ("cornell.txt", 257, 9, 3),
                                              ("cornell.txt", 130, 40, 8)])
def test_every_kernel_form_gives_the_same_bits(gpu, scene, w, h, levels):
    """the plain gather, LDS tiles of 64 x 4 and of 64 x 8, and the product's choice per level: the result does not depend on the tile shape"""
    with gpu.renderer_from_test_library():
        _init(gpu, scene, w, h, 2)
        want = _want(gpu, w, h, 2, levels, 1.5, 0.35, 2.0)
        outs = [gpu.test_denoise(2, form, levels, 1.5, 0.35, 2.0) for form in (0, 1, 2, 3)]
    for o in outs:
        assert _same(o, want)


def test_exp_neg_poly_on_the_device(gpu):
    rng = np.random.default_rng(5)
    a = np.concatenate([rng.uniform(0, 100, 20000), rng.uniform(0, 1, 5000), [0.0, 87.3, 87.4, 1e3, 3e38, np.inf, np.nan, 1e-30]]).astype(F)
    assert _same(gpu.test_exp_neg_poly(a), dr.exp_neg_poly(a))


# ---- 3: state ---------------------------------------------------------------------------------------------------------------------------
def test_denoise_leaves_the_renderer_as_it_was(gpu):
    W, H = 70, 37
    _init(gpu, "cornell.txt", W, H, 3)
    try:
        before = gpu.readback(W * H)
        a = gpu.denoise(3, 5, 2.0, 0.35, 2.0)
        b = gpu.denoise(3, 5, 2.0, 0.35, 2.0)
        assert _same(a, b)                                      # two calls, the same bits
        assert _same(gpu.readback(W * H), before)               # the accumulator is untouched ...
        g1 = gpu.gbuffer(1)
        g2 = gpu.gbuffer(2)
        assert not _same(g1[0], g2[0])                          # another iteration's jitter: other guides ...
        assert all(_same(x, y) for x, y in zip(g1[:2], gpu.gbuffer(1))) and np.array_equal(g1[2], gpu.gbuffer(1)[2])   # ... and back
        assert not _same(gpu.denoise(3, 5, 2.0, 0.35, 2.0, guide_iter=2), a)
        assert _same(gpu.denoise(3, 5, 2.0, 0.35, 2.0, guide_iter=1), a)
        gpu.pathtrace(None, 0, 4, readback=False)               # ... and rendering goes on
        after = gpu.readback(W * H)
        a4 = gpu.denoise(4, 5, 2.0, 0.35, 2.0)
    finally:
        gpu.pathtraceFree()
    _init(gpu, "cornell.txt", W, H, 4)
    try:
        assert _same(gpu.readback(W * H), after)                # the frame that never denoised
        assert _same(gpu.denoise(4, 5, 2.0, 0.35, 2.0), a4)
    finally:
        gpu.pathtraceFree()


def test_another_scene_leaves_nothing_stale(gpu):
    _init(gpu, "cornell.txt", 70, 37, 2)
    try:
        gpu.denoise(2, 3, 2.0, 0.35, 2.0)
        _init(gpu, "sphere.txt", 48, 32, 2, free=False)         # pt_init over the live renderer: other frame size, other guides
        want = _want(gpu, 48, 32, 2, 3, 2.0, 0.35, 2.0)
        assert _same(gpu.denoise(2, 3, 2.0, 0.35, 2.0), want)
    finally:
        gpu.pathtraceFree()


def test_caller_owned_accumulator(gpu):
    import torch
    W, H = 70, 37
    acc = torch.zeros(W * H * 3, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    _init(gpu, "cornell.txt", W, H, 2, accum_dev=acc.data_ptr())
    try:
        want = _want(gpu, W, H, 2, 4, 2.0, 0.35, 2.0)
        got = gpu.denoise(2, 4, 2.0, 0.35, 2.0)
        gpu.sync()
        mine = acc.cpu().numpy()
        assert _same(got, want) and _same(mine, gpu.readback(W * H))
    finally:
        gpu.pathtraceFree()


# ---- 4: refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    W, H = 16, 16
    _init(gpu, "cornell.txt", W, H, 1)
    L = gpu.lib()
    out = np.full(W * H * 3, 7, F)
    p8 = np.zeros(W * H * 4, np.uint8)

    def call(samples=1, levels=3, guide_iter=1, sc_=1.0, sn=1.0, sp=1.0, size=None):
        prm = gpu.PtDenoiseParams(levels, guide_iter, sc_, sn, sp)
        rc = L.pt_denoise(samples, C.byref(prm), C.sizeof(prm) if size is None else size, out.ctypes.data_as(C.c_void_p))
        assert L.pt_denoise_rgba8(samples, C.byref(prm), C.sizeof(prm) if size is None else size, p8.ctypes.data_as(C.c_void_p)) == rc
        return rc

    try:
        before = gpu.readback(W * H)
        for bad in (dict(levels=0), dict(levels=9), dict(levels=-1), dict(sc_=0.0), dict(sn=-1.0), dict(sp=float("nan")), dict(sc_=float("nan")),
                    dict(sn=0.0), dict(sp=-np.inf), dict(size=16), dict(size=24), dict(samples=0), dict(samples=-3), dict(guide_iter=0)):
            assert call(**bad) == -1, bad                       # PT_ERR_INVALID
            assert (out == 7).all() and not p8.any()
        assert L.pt_denoise(1, None, 20, out.ctypes.data_as(C.c_void_p)) == -1
        assert call(sn=float("inf"), sp=float("inf"), sc_=float("inf")) == 0
        assert _same(gpu.readback(W * H), before)
    finally:
        gpu.pathtraceFree()
    # a sharded renderer's accumulator is not a frame
    for opts in (dict(shard_rank=1, shard_count=2), dict(flags=2)):
        _init(gpu, "cornell.txt", W, H, 1, **opts)
        try:
            assert call() == -1 and b"shard" in L.pt_last_error()
            assert L.pt_gbuffer(1, out.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == -1
        finally:
            gpu.pathtraceFree()


# ---- 5: the headless driver ----------------------------------------------------------------------------------------------------------------
def test_pt_render_denoise(gpu, tmp_path):
    from test_host import _decode_png
    exe = os.path.join(ROOT, "project3-cuda-path-tracer_amd", "host", "pt_render")
    args = [exe, os.path.join(SCENES, "cornell.txt"), "--res", "64", "48", "--iterations", "4", "--depth", "4"]
    r = subprocess.run(args + ["--out", str(tmp_path / "plain")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(args + ["--out", str(tmp_path / "dn"), "--denoise", "5", "2.0", "0.35", "2.0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["dn.denoised.png", "dn.png", "plain.png"]
    plain = _decode_png(str(tmp_path / "plain.png"))
    assert np.array_equal(_decode_png(str(tmp_path / "dn.png")), plain)
    _init(gpu, "cornell.txt", 64, 48, 4)
    try:
        mean = gpu.denoise(4, 5, 2.0, 0.35, 2.0).reshape(48, 64, 3)
        want = (np.clip(mean, 0, 1) * F(255)).astype(np.uint8)[:, ::-1]          # the driver's PNG conversion, X mirrored
    finally:
        gpu.pathtraceFree()
    got = _decode_png(str(tmp_path / "dn.denoised.png"))
    assert np.array_equal(got, want) and not np.array_equal(got, plain)
