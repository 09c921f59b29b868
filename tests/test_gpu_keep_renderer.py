"""PT_FLAG_KEEP_RENDERER on the MI355X: a full pt_init that repeats the live renderer's own call with another pose moves the camera in place
(pathtraceInit(..., keep=True)); any difference makes it the full call.  Either way the result is the full call's, bit for bit.

Every case walks its views twice or three times in the test library's renderer -- with the flag, with plain full calls, where history is
concerned with pathtraceSetCamera too -- and compares after every view what a caller can read: the accumulator, the second moments, the
counters, pt_denoise_var with its variance where moments are kept, the display bytes where the display filter runs.  Frames of 48 x 32, or
37 x 23 for a partial last block; depth 3 - 4; 2 - 4 iterations a view.

1  the same scene at a new pose goes the fast way from the second call on (camera_move_info: fast, bytes uploaded) -- which it does not on a
   library without the flag, where a full-argument call never reports a move;
2  each difference alone -- scene, options, resolution, anything registered -- is named by the comparison (keep_mismatch) and renders the
   full call's frame; equal content registered again from other host arrays is no difference;
3  under PT_FLAG_TEMPORAL the history the flagged calls leave behind is pathtraceSetCamera's and the full calls';
4  what the full call refuses is refused, and the old view renders on; pt_group_init refuses the flag;
5  pt_render --protocol (pathtraceFree(); pathtraceInit(scene); through the shim with both switches on) writes the PNGs of --in-place and
   of the plain run."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import camera_poses
from conftest import SCENES

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def gpu(pt):
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return pt


def _scene(pt, name, w, h):
    sc = pt.Scene(os.path.join(SCENES, name))
    sc.set_resolution(w, h)
    return sc


def _poses(gpu, name, sc, labels=("own", "side_0.3", "yaw_30", "side_1")):
    """the labelled poses of tests/camera_poses.py for this scene; a scene without the thin wall that family's dolly poses need gets the
    same sidesteps and turns, made the same way"""
    cam0 = sc.camera.view(gpu.CAMERA_DTYPE)
    try:
        by = dict(camera_poses.poses(name, cam0, sc.geoms.view(gpu.GEOM_DTYPE)))
    except ValueError:
        eye, view, up = (np.asarray(cam0[k][0], np.float64) for k in ("position", "view", "up"))
        right = camera_poses._unit(np.cross(view, up))
        by = {"own": np.array(cam0, copy=True)}
        for label, d in (("side_0.3", 0.3), ("side_1", 1.0)):
            by[label] = np.array(cam0, copy=True)
            by[label]["position"][0] = (eye + d * right).astype(F)
        for deg in (5, 30):
            by["yaw_%d" % deg] = np.array(cam0, copy=True)
            by["yaw_%d" % deg]["view"][0] = camera_poses._rotate(view, up, deg).astype(F)
    return [by[label] for label in labels]


def _counters(gpu):
    c = gpu.counters()
    return (tuple(c.live), tuple(c.ended_early), c.misses, c.light_hits, c.iterations)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


def _render(gpu, sc, n, opts, first=1, single=False):
    """n iterations first .. first + n - 1 of a view that has none yet, then everything the renderer's options let a caller read"""
    if single:
        for it in range(first, first + n):
            gpu.pathtrace(None, 0, it, readback=False)
    else:
        step = max(int(opts.get("max_batch", 0)), 1)
        for it in range(first, first + n, step):
            gpu.pathtrace_batch(None, 0, it, min(step, first + n - it))
    res = sc.camera["resolution"][0]
    P = int(res[0]) * int(res[1])
    got = {"accum": gpu.readback(P).copy(), "counters": _counters(gpu)}
    if opts.get("moments"):
        got["moments"] = gpu.readback_moments()
        if n >= 2 or (opts.get("spatial_variance") and n >= 1):
            got["dv"], got["dv_var"] = gpu.denoise_var(n, with_variance=True)
    if opts.get("display_filter") and n >= 1:
        got["rgba8"] = gpu.readback_rgba8(n, P)
    return got


def _same(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        if k == "counters":
            assert a[k] == b[k], "%s: counters differ" % what
        else:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), "%s: %s differs" % (what, k)


def _walk(gpu, sc, cams, how, opts, counts, zero=None, single=False, numbered_on=False, first=1):
    """The views `cams` reached by `how`: "keep" (pathtraceInit(keep=True) every time), "full" (plain pathtraceInit every time) or "move"
    (pathtraceInit, then pathtraceSetCamera); counts[i] iterations at view i (numbered on from the view before where numbered_on: fresh
    random numbers for a history).  -> per view what _render read, per later view camera_move_info()."""
    own = np.array(sc.camera, copy=True)
    out, infos = [], []
    gpu.pathtraceFree()
    try:
        for i, cam in enumerate(cams):
            if zero is not None:
                zero()
            if how == "move" and i:
                gpu.pathtraceSetCamera(cam)
            else:
                sc.camera[:] = cam
                gpu.pathtraceInit(sc, keep=(how == "keep"), **opts)
            if i:
                infos.append((gpu.camera_move_info(), gpu.keep_mismatch()))
            out.append(_render(gpu, sc, counts[i], opts, first, single))
            if numbered_on:
                first += counts[i]
    finally:
        gpu.pathtraceFree()
        sc.camera[:] = own
    return out, infos


# ---- 1: the same scene at a new pose -------------------------------------------------------------------------------------------------------
SAME_SCENE = [
    # (id, scene, W, H, pathtraceInit's options, one pathtrace call per iteration)
    ("cornell_moments", "cornell.txt", 48, 32, dict(traceDepth=4, moments=True), False),
    ("textured_display_partial_block", "cornell_textured.txt", 37, 23, dict(traceDepth=3, moments=True, display_filter=True, max_batch=4), False),
    ("mesh_small", "mesh_small.txt", 48, 32, dict(traceDepth=3, moments=True), False),
    ("spheres64", "spheres64.txt", 48, 32, dict(traceDepth=4, max_batch=4, pipeline_depth=2), False),
    ("thin_lens", "cornell.txt", 48, 32, dict(traceDepth=4, lens_radius=0.2, focal_distance=10.0), False),
    ("direct_lighting", "cornell.txt", 37, 23, dict(traceDepth=3, direct_lighting=True, max_batch=4), False),
    ("batches_parked", "cornell.txt", 48, 32, dict(traceDepth=4, max_batch=4, pipeline_depth=3, trace_ahead=True), True),
]
COUNTS4 = (2, 3, 4, 2)


def _check_fast(infos, n):
    assert len(infos) == n
    for j, (info, why) in enumerate(infos):
        assert info["fast"] is True, "call %d ran the full call: %r" % (j + 2, why)
        assert info["bytes_uploaded"] > 0 and info["tables_uploaded"] >= 1 and why == ""


@pytest.mark.parametrize("cid,name,W,H,opts,single", SAME_SCENE, ids=[c[0] for c in SAME_SCENE])
def test_the_same_scene_at_a_new_pose_moves_in_place(gpu, cid, name, W, H, opts, single):
    sc = _scene(gpu, name, W, H)
    cams = _poses(gpu, name, sc)
    with gpu.renderer_from_test_library():
        want, _ = _walk(gpu, sc, cams, "full", opts, COUNTS4, single=single)
        got, infos = _walk(gpu, sc, cams, "keep", opts, COUNTS4, single=single)
    for i, (a, b) in enumerate(zip(want, got)):
        _same(a, b, "view %d" % i)
    _check_fast(infos, 3)
    assert not np.array_equal(want[0]["accum"], want[1]["accum"])


def test_a_callers_accumulator_stays_the_callers_to_zero(gpu):
    import torch
    sc = _scene(gpu, "cornell.txt", 48, 32)
    cams = _poses(gpu, "cornell.txt", sc)
    acc = torch.zeros(48 * 32 * 3, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def zero():
        acc.zero_()
        torch.cuda.synchronize()

    opts = dict(traceDepth=4, max_batch=4, accum_dev=acc.data_ptr())
    with gpu.renderer_from_test_library():
        want, _ = _walk(gpu, sc, cams, "full", opts, COUNTS4, zero=zero)
        got, infos = _walk(gpu, sc, cams, "keep", opts, COUNTS4, zero=zero)
    for i, (a, b) in enumerate(zip(want, got)):
        _same(a, b, "view %d" % i)
    _check_fast(infos, 3)


def test_a_renderer_initialised_without_the_flag_is_not_moved_and_the_next_call_matches(gpu):
    sc = _scene(gpu, "cornell.txt", 48, 32)
    cams = _poses(gpu, "cornell.txt", sc)
    opts = dict(traceDepth=4)
    with gpu.renderer_from_test_library():
        gpu.pathtraceFree()
        try:
            sc.camera[:] = cams[0]
            gpu.pathtraceInit(sc, **opts)
            sc.camera[:] = cams[1]
            gpu.pathtraceInit(sc, keep=True, **opts)
            assert gpu.camera_move_info()["fast"] is None and gpu.keep_mismatch() == "flags"
            sc.camera[:] = cams[2]
            gpu.pathtraceInit(sc, keep=True, **opts)
            assert gpu.camera_move_info()["fast"] is True and gpu.keep_mismatch() == ""
        finally:
            gpu.pathtraceFree()


# ---- 2: each difference alone ----------------------------------------------------------------------------------------------------------------
def _bump_scene(gpu, w=48, h=32):
    """cornell_bump.txt: textures, height maps with scales, a mesh with UVs -- and a face-material array (-1: the object's own) for its mesh"""
    sc = _scene(gpu, "cornell_bump.txt", w, h)
    sc.mesh_materials = {7: np.full(len(sc.meshes[7]), -1, np.int32)}
    return sc


def _d_material(sc, o): sc.materials["color"][1][0] = F(0.31)
def _d_translation(sc, o): sc.geoms["translation"][4][1] += F(0.25)      # (the record's bytes: the matrices stay, and so does the frame)
def _d_depth(sc, o): o["traceDepth"] = 4
def _d_max_batch(sc, o): o["max_batch"] = 2
def _d_pipeline(sc, o): o["pipeline_depth"] = 2
def _d_lens(sc, o): o.update(lens_radius=0.1, focal_distance=9.0)
def _d_flag(sc, o): o["mixture_weighted"] = True
def _d_texel(sc, o): sc.textures[0][3, 5, 0] += F(0.125)
def _d_uv(sc, o): sc.mesh_uvs[7][10, 2] += F(0.0625)
def _d_vertex(sc, o): sc.meshes[7][17, 4] += F(0.03125)
def _d_face_material(sc, o): sc.mesh_materials[7][20] = 1
def _d_bump_scale(sc, o): sc.bump_scales[3] = F(0.08)
def _d_texture_added(sc, o): sc.textures.append(np.full((2, 2, 3), 0.5, F))
def _d_meshes_cleared(sc, o): sc.meshes, sc.mesh_materials, sc.mesh_uvs = {}, {}, {}


def _d_fresh_arrays(sc, o):
    """the same content in host arrays at other addresses"""
    sc.geoms, sc.materials = sc.geoms.copy(), sc.materials.copy()
    sc.meshes = {g: t.copy() for g, t in sc.meshes.items()}
    sc.mesh_materials = {g: t.copy() for g, t in sc.mesh_materials.items()}
    sc.mesh_uvs = {g: t.copy() for g, t in sc.mesh_uvs.items()}
    sc.textures = [t.copy() for t in sc.textures]
    sc.geom_textures, sc.geom_bumps, sc.bump_scales = sc.geom_textures.copy(), sc.geom_bumps.copy(), sc.bump_scales.copy()


DIFFERENCES = [
    # (id, the change, the comparison that must name it, or None where the call must still move in place)
    ("material_colour", _d_material, "materials"),
    ("geom_translation", _d_translation, "geoms"),
    ("traceDepth", _d_depth, "traceDepth"),
    ("max_batch", _d_max_batch, "max_batch"),
    ("pipeline_depth", _d_pipeline, "pipeline_depth"),
    ("lens_radius", _d_lens, "lens_radius"),
    ("flag_bit", _d_flag, "flags"),
    ("resolution", None, "resolution"),
    ("texel", _d_texel, "texels"),
    ("uv", _d_uv, "texture UVs"),
    ("triangle_vertex", _d_vertex, "mesh triangles"),
    ("face_material", _d_face_material, "mesh face materials"),
    ("bump_scale", _d_bump_scale, "bump scale"),
    ("texture_added", _d_texture_added, "texture count"),
    ("meshes_cleared", _d_meshes_cleared, "mesh count"),
    ("equal_content_fresh_arrays", _d_fresh_arrays, None),
]


@pytest.mark.parametrize("did,change,why", DIFFERENCES, ids=[d[0] for d in DIFFERENCES])
def test_each_difference_alone_takes_the_full_call(gpu, did, change, why):
    """view 0 with the scene as the file gives it, view 1 at another pose with one thing changed: the flagged walk against the plain one.
    (meshes cleared: the full call refuses a mesh object without triangles -- then both walks are refused alike, before anything is
    touched, and the old view renders on in both.)"""
    results = []
    with gpu.renderer_from_test_library():
        for keep in (False, True):
            sc = _bump_scene(gpu)
            opts = dict(traceDepth=3, moments=True, max_batch=4, pipeline_depth=3)
            cams = _poses(gpu, "cornell_bump.txt", sc, ("own", "side_0.3"))
            gpu.pathtraceFree()
            try:
                sc.camera[:] = cams[0]
                gpu.pathtraceInit(sc, keep=keep, **opts)
                first = _render(gpu, sc, 2, opts)
                if did == "resolution":
                    sc = _bump_scene(gpu, 37, 23)
                    cams = _poses(gpu, "cornell_bump.txt", sc, ("own", "side_0.3"))
                else:
                    change(sc, opts)
                sc.camera[:] = cams[1]
                refused = None
                try:
                    gpu.pathtraceInit(sc, keep=keep, **opts)
                except gpu.PtError as e:
                    refused = str(e)
                info, named = gpu.camera_move_info(), gpu.keep_mismatch()
                if refused is None:
                    second = _render(gpu, sc, 3, opts)
                else:                                    # the renderer of view 0 is still there, two iterations in
                    gpu.pathtrace_batch(None, 0, 3, 1)
                    second = {"accum": gpu.readback(48 * 32).copy(), "counters": _counters(gpu)}
                results.append((first, second, refused, info, named))
            finally:
                gpu.pathtraceFree()
    (f0, s0, r0, i0, _), (f1, s1, r1, i1, named) = results
    _same(f0, f1, "view 0")
    _same(s0, s1, "view 1")
    assert r0 == r1 and (r0 is None) == (did != "meshes_cleared")
    if why is None:
        assert i1["fast"] is True and i1["bytes_uploaded"] > 0 and named == ""
    else:
        assert i1 == {"fast": None, "tables_uploaded": 0, "bytes_uploaded": 0} and named == why


# ---- 3: history --------------------------------------------------------------------------------------------------------------------------------
HISTORY = [
    ("temporal", "cornell.txt", dict(traceDepth=4, moments=True, temporal=True), (2, 2, 2)),
    ("demod_history_spatial_display", "cornell_textured.txt",
     dict(traceDepth=3, moments=True, temporal=True, demodulate=True, demod_history=True, spatial_variance=True, display_filter=True), (2, 1, 2)),
    # the middle view commits nothing: the history it finds is the one it leaves
    ("a_view_without_an_iteration", "cornell_textured.txt",
     dict(traceDepth=3, moments=True, temporal=True, demodulate=True, demod_history=True, spatial_variance=True, display_filter=True), (2, 0, 1)),
]


@pytest.mark.parametrize("hid,name,opts,counts", HISTORY, ids=[h[0] for h in HISTORY])
def test_the_history_is_that_of_the_move_and_of_the_full_calls(gpu, hid, name, opts, counts):
    sc = _scene(gpu, name, 48, 32)
    cams = _poses(gpu, name, sc, ("own", "side_0.3", "yaw_5"))
    with gpu.renderer_from_test_library():
        full, _ = _walk(gpu, sc, cams, "full", opts, counts, numbered_on=True)
        move, minfo = _walk(gpu, sc, cams, "move", opts, counts, numbered_on=True)
        keep, kinfo = _walk(gpu, sc, cams, "keep", opts, counts, numbered_on=True)
        # the last view alone, the same iterations: what it shows without a history
        alone, _ = _walk(gpu, sc, cams[2:], "full", opts, counts[2:], first=1 + counts[0] + counts[1])
    for i in range(3):
        _same(full[i], keep[i], "view %d against the full calls" % i)
        _same(move[i], keep[i], "view %d against pathtraceSetCamera" % i)
    _check_fast(kinfo, 2)
    assert all(info["fast"] is True for info, _ in minfo)
    assert "dv" in keep[2] and "dv" in keep[0]
    if hid == "a_view_without_an_iteration":
        # view 1 committed nothing, so view 2 blends with view 0's samples: its filtered frame is not the one it has alone
        assert np.array_equal(_bits(keep[2]["accum"]), _bits(alone[0]["accum"]))
        assert not np.array_equal(_bits(keep[2]["dv"]), _bits(alone[0]["dv"]))


# ---- 4: refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing(gpu):
    P = 48 * 32
    frames = []
    with gpu.renderer_from_test_library():
        for disturb in (False, True):
            sc = _scene(gpu, "mesh_attributes.txt", 48, 32)
            opts = dict(traceDepth=3, moments=True)
            gpu.pathtraceFree()
            try:
                gpu.pathtraceInit(sc, keep=True, **opts)
                for it in (1, 2):
                    gpu.pathtrace_batch(None, 0, it, 1)
                if disturb:
                    L = gpu.lib()
                    geoms, mats = np.ascontiguousarray(sc.geoms), np.ascontiguousarray(sc.materials)
                    status = []
                    for flags in (gpu.PT_FLAG_MOMENTS, gpu.PT_FLAG_MOMENTS | gpu.PT_FLAG_KEEP_RENDERER):
                        opt = gpu.PtOptions(0, 1, -1, flags, 0, 0, None, None, 0.0, 0.0)
                        status.append(L.pt_init(None, geoms.ctypes.data_as(C.c_void_p), len(geoms), mats.ctypes.data_as(C.c_void_p), len(mats), 3,
                                                C.byref(opt)))
                    assert status[0] == status[1] == -1                      # PT_ERR_INVALID for the NULL camera, flag or no flag
                    assert gpu.camera_move_info()["fast"] is None
                    # a face whose material the scene does not have: the same refusal with and without the flag
                    bad = _scene(gpu, "mesh_attributes.txt", 48, 32)
                    bad.mesh_materials[5][3] = len(bad.materials)
                    bad.camera[:] = _poses(gpu, "mesh_attributes.txt", bad, ("side_0.3",))[0]
                    said = []
                    for keep in (False, True):
                        with pytest.raises(gpu.PtError) as e:
                            gpu.pathtraceInit(bad, keep=keep, **opts)
                        said.append(str(e.value))
                    assert said[0] == said[1] and "error -1" in said[0]
                    assert gpu.camera_move_info()["fast"] is None and gpu.keep_mismatch() == "mesh face materials"
                for it in (3, 4):
                    gpu.pathtrace_batch(None, 0, it, 1)
                frames.append((gpu.readback(P).copy(), gpu.readback_moments(), _counters(gpu), gpu.denoise_var(4)))
            finally:
                gpu.pathtraceFree()
    a, b = frames
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1])) and a[2] == b[2]
    assert np.array_equal(_bits(a[3]), _bits(b[3]))


def test_a_group_refuses_the_flag(gpu):
    sc = _scene(gpu, "cornell.txt", 48, 32)
    g = gpu.Group(2, devices=[0, 0])
    try:
        with pytest.raises(gpu.PtError, match="error -1.*PT_FLAG_KEEP_RENDERER"):
            g.init(sc, traceDepth=3, flags=gpu.PT_FLAG_KEEP_RENDERER)
        g.init(sc, traceDepth=3)                         # (and is as usable as before)
    finally:
        g.destroy()


# ---- 5: the shim, through pt_render --------------------------------------------------------------------------------------------------------
EXE = os.path.join(os.path.dirname(SCENES), "project3-cuda-path-tracer_amd", "host", "pt_render")


def test_pt_render_protocol_writes_the_same_pngs(gpu, tmp_path):
    """pathtraceFree(); pathtraceInit(scene); with the renderer parked and the flag set, against pt_init's same-scene form and against the
    full call over the live renderer: the same files.  With PT_AMD_KEEP_RENDERER=0 the restart frees the renderer, and the history with
    it: the run still renders the view's own samples."""
    args = [EXE, os.path.join(SCENES, "cornell_textured.txt"), "--res", "48", "32", "--iterations", "2", "--denoise-var", "5", "4", "0.35", "2",
            "--history-from", "0.3", "5", "10.5", "3"]
    env = dict(os.environ)
    for k in ("PT_AMD_DEVICES", "PT_AMD_DISPLAY_FILTER", "PT_AMD_SPATIAL_VARIANCE", "PT_AMD_DEMODULATE", "PT_AMD_KEEP_RENDERER", "PT_AMD_TEMPORAL",
              "PT_AMD_TRACE_AHEAD"):
        env.pop(k, None)
    runs = (("protocol", ["--protocol"], {}), ("inplace", ["--in-place"], {}), ("full", [], {}), ("freed", ["--protocol"], {"PT_AMD_KEEP_RENDERER": "0"}))
    for name, more, extra in runs:
        r = subprocess.run(args + more + ["--out", str(tmp_path / name)], capture_output=True, text=True, timeout=120, env=dict(env, **extra))
        assert r.returncode == 0, (name, r.stderr[-2000:])
    png = {name: [open(str(tmp_path / (name + suffix)), "rb").read() for suffix in (".png", ".denoised.png")] for name, _, _ in runs}
    assert len(png["full"][0]) > 100 and len(png["full"][1]) > 100
    assert png["protocol"] == png["inplace"] == png["full"]
    assert png["freed"][0] == png["full"][0]
    assert png["freed"][1] != png["full"][1]             # (no history survived the Free: the filter saw two samples, not five)
    r = subprocess.run(args + ["--protocol", "--in-place"], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode != 0 and "exclude each other" in r.stderr
