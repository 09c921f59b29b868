"""Who owns device memory: every table of a renderer is held by one owner type (csrc/pt_api.hip: DevBuf), and the test library counts the
allocations those owners hold (pt_test_live_device_buffers).  Renderers that use every group of tables -- meshes, their walks, textures,
height maps and a lens; the swept, grouped and row tables of a sphere-heavy scene; the camera list -- are initialised one over the other
as the reference restarts (Free -> Init inside pt_init, no pt_free between), and nothing may be left behind: the same scene holds the same
number of buffers and renders the same bits the second time, pt_free brings the count to zero -- after the denoiser's lazily allocated
buffers too.  A pt_init that is refused touches nothing: pt_init plans the scene on the host (csrc/pt_scene_plan.h) before it releases or
allocates anything, so the renderer that was there keeps its buffers, goes on rendering the same bits, and its state is the plan's.
Every refusal here is a host-side argument check."""
import ctypes as C
import os
import types

import numpy as np
import pytest

from conftest import SCENES

pytestmark = pytest.mark.gpu

W = H = 32
DEPTH = 3

MATERIALS = """MATERIAL 0
RGB 1 1 1
SPECEX 0
SPECRGB 0 0 0
REFL 0
REFR 0
REFRIOR 0
EMITTANCE 5

MATERIAL 1
RGB .9 .8 .7
SPECEX 0
SPECRGB 0 0 0
REFL 0
REFR 0
REFRIOR 0
EMITTANCE 0

CAMERA
RES 32 32
FOVY 45
ITERATIONS 1
DEPTH 3
FILE buffers
EYE 0.0 5 10.5
VIEW 0 0 -1
UP 0 1 0

"""
BOX = [("cube", 0, "0 10 0", "0 0 0", "3 .3 3"), ("cube", 1, "0 0 0", "0 0 0", "10 .01 10"), ("cube", 1, "0 10 0", "0 0 90", ".01 10 10"),
       ("cube", 1, "0 5 -5", "0 90 0", ".01 10 10"), ("cube", 1, "-5 5 0", "0 0 0", ".01 10 10"), ("cube", 1, "5 5 0", "0 0 0", ".01 10 10")]


def _scene_text(objects):
    out = [MATERIALS]
    for i, (kind, mat, trans, rot, scale, *extra) in enumerate(objects):
        out.append("OBJECT %d\n%s\nmaterial %d\nTRANS %s\nROTAT %s\nSCALE %s\n%s\n" % (i, kind, mat, trans, rot, scale, "".join(e + "\n" for e in extra)))
    return "".join(out)


def _ppm(path, rgb):
    with open(path, "wb") as f:
        f.write(b"P6\n4 4\n255\n" + np.asarray(rgb, np.uint8).tobytes())


@pytest.fixture(scope="module")
def gpu(pt):
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return pt


@pytest.fixture(scope="module")
def scenes(gpu, tmp_path_factory):
    d = tmp_path_factory.mktemp("buffers")
    rng = np.random.default_rng(7)
    _ppm(d / "tex.ppm", rng.integers(0, 256, (4, 4, 3)))
    _ppm(d / "height.ppm", np.repeat(rng.integers(0, 256, (4, 4, 1)), 3, axis=2))
    a = d / "a.txt"       # the small UV mesh in a box, a 4 x 4 texture and a 4 x 4 height map bound to it
    a.write_text(_scene_text(BOX + [("mesh " + os.path.join(SCENES, "models", "torus_uv.obj"), 1, "0 4 0", "50 0 25", "5 5 5",
                                     "TEXTURE %s" % (d / "tex.ppm"), "BUMP %s 0.05" % (d / "height.ppm"))]))
    b = d / "b.txt"       # 16 small spheres in a box
    b.write_text(_scene_text(BOX + [("sphere", 1, "%g %g %g" % (-3 + 2 * (i % 4), 2 + 2 * (i // 4), -1 + 0.5 * (i % 3)), "0 0 0", ".8 .8 .8")
                                    for i in range(16)]))
    out = {}
    for name, path in (("a", str(a)), ("b", str(b)), ("c", os.path.join(SCENES, "cornell.txt"))):
        sc = gpu.Scene(path)
        sc.set_resolution(W, H)
        out[name] = sc
    assert len(out["a"].meshes) == 1 and len(out["a"].mesh_uvs) == 1 and len(out["a"].textures) == 2
    assert out["a"].geom_textures[6] == 0 and out["a"].geom_bumps[6] == 1 and int((out["b"].geoms["type"] == 0).sum()) == 16
    # one sphere and 4096 materials: refused by pt_init's checks of the scene's size, the last ones of its plan
    sph = out["b"].geoms[out["b"].geoms["type"] == 0][:1].copy()
    sph["materialid"] = 0
    out["refused"] = types.SimpleNamespace(geoms=sph, materials=np.repeat(out["b"].materials[:1], 4096), camera=out["b"].camera.copy(),
                                           traceDepth=DEPTH, image=np.zeros((H, W, 3), np.float32))
    return out


def _frame(gpu, sc, **kw):
    """pt_init over whatever renderer there is, one iteration, the frame and the buffers the library then holds"""
    gpu.pathtraceInit(sc, traceDepth=DEPTH, **kw)
    live = gpu.test_lib().pt_test_live_device_buffers()
    gpu.pathtrace(None, 0, 1, readback=False)
    return gpu.readback(W * H).view(np.uint32), live


def test_restarts_leave_no_device_buffer_behind(gpu, scenes, monkeypatch):
    live = gpu.test_lib().pt_test_live_device_buffers
    with gpu.renderer_from_test_library():
        gpu.pathtraceFree()
        assert live() == 0
        lens = dict(lens_radius=0.1, focal_distance=9.0)
        a1, na1 = _frame(gpu, scenes["a"], **lens)
        monkeypatch.setenv("PT_AMD_GROUPS", "1")
        b1, nb = _frame(gpu, scenes["b"])
        monkeypatch.delenv("PT_AMD_GROUPS")
        c1, nc = _frame(gpu, scenes["c"])
        gpu.gbuffer(1)                                  # the denoiser's buffers, allocated on first use
        gpu.denoise(1, levels=3)
        assert live() > nc
        a2, na2 = _frame(gpu, scenes["a"], **lens)
        assert a1.any() and b1.any() and c1.any()
        assert np.array_equal(a1, a2)
        assert na1 == na2 and na1 > 0 and nb > 0 and nc > 0
        gpu.pathtraceFree()
        assert live() == 0
    assert live() == 0


def test_a_refused_init_leaves_no_device_buffer_behind(gpu, scenes):
    live = gpu.test_lib().pt_test_live_device_buffers
    with gpu.renderer_from_test_library():
        gpu.pathtraceInit(scenes["c"], traceDepth=DEPTH)                 # iterations 1 and 2, uninterrupted
        gpu.pathtrace(None, 0, 1, readback=False)
        gpu.pathtrace(None, 0, 2, readback=False)
        want = gpu.readback(W * H).view(np.uint32).copy()
        c1, _ = _frame(gpu, scenes["c"])                                  # ... and with a refused pt_init between them
        held = live()
        with pytest.raises(gpu.PtError, match="pt_amd error -1"):        # PT_ERR_INVALID
            gpu.pathtraceInit(scenes["refused"], traceDepth=DEPTH)
        assert live() == held > 0                       # (nothing allocated, nothing released)
        gpu.pathtrace(None, 0, 2, readback=False)       # (the renderer that was there is still initialised)
        c2 = gpu.readback(W * H).view(np.uint32)
        assert c1.any() and not np.array_equal(c1, c2) and np.array_equal(c2, want)
        gpu.pathtraceFree()
        assert live() == 0


def test_the_renderer_state_is_the_plans(gpu, scenes, monkeypatch):
    state = C.c_uint32(0)
    with gpu.renderer_from_test_library():
        for name, env, kw in (("a", None, dict(lens_radius=0.1, focal_distance=9.0)), ("a", None, {}), ("b", None, {}), ("b", "PT_AMD_GROUPS", {}),
                              ("c", None, {})):
            if env:
                monkeypatch.setenv(env, "1")
            gpu.pathtraceInit(scenes[name], traceDepth=DEPTH, **kw)
            assert gpu.test_lib().pt_test_renderer_state(C.byref(state)) == 0, gpu.test_lib().pt_last_error()
            assert state.value == gpu.scene_plan(scenes[name], traceDepth=DEPTH, **kw).state_bits, (name, env, kw)
            if env:
                monkeypatch.delenv(env)
        gpu.pathtraceFree()
