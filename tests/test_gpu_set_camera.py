"""The camera move (pt_init's same-scene form, PT_SAME_SCENE; pathtraceSetCamera) on the MI355X: the camera of a live renderer moved in place, against the definition -- pt_init called over the live
renderer with the scene it was initialised with and the new camera -- bit for bit.

Certificates: for every pose of the family (tests/camera_poses.py; its ledger is tests/test_set_camera_cpu.py's) and once for Cornell at
1280 x 720, the work list with its face certificates evaluated on the device (k_camera_faces, csrc/pt_camera_faces.h) equals the host's
in all four arrays, for shards (0, 1) and (1, 3).

Moves: chains of four to six poses are walked twice, by pathtraceInit over the live renderer and by pathtraceSetCamera, and after every
move, with 1 - 4 iterations rendered, everything a caller can read is compared: the accumulator, the second moments, the counters, the guide
buffers, pt_denoise_var with the history the moves leave behind, the display filter's bytes.  Every such move must have gone the fast way
(camera_move_info), and the number of live device buffers stays what it was across a move, apart from the camera tables of a work list
that comes or goes: from the second move on (the first makes the two scratch buffers of the device certificates), under
PT_FLAG_TEMPORAL from the third (the first two captures allocate the history's two halves, as pt_init's do).

A move after a re-registration: pt_set_textures / pt_set_meshes between pathtraceInit and the move leave the move -- fast or slow -- with
the scene the renderer was initialised with, and serve the next full pathtraceInit.

Slow path and refusals: a renderer whose fault word is set by hand is rebuilt by pt_init inside the call and renders the right frame; a
camera of another resolution is refused and the old view goes on bit for bit; a move in one context leaves another alone."""
import os

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


# ---- certificates -----------------------------------------------------------------------------------------------------------------------
def _lists_equal(gpu, cam, geoms, rank, count):
    want = gpu.camera_resolved(cam, geoms, rank, count)
    got = gpu.camera_resolved_device(cam, geoms, rank, count)
    assert (want is None) == (got is None)
    if want is not None:
        for a, b in zip(want, got):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    return want


def test_device_certificates_equal_the_hosts_over_the_pose_family(gpu):
    resolved_waves = poses = 0
    for name, W, H, label, cam, geoms in camera_poses.family(gpu, SCENES):
        for rank, count in ((0, 1), (1, 3)):
            want = _lists_equal(gpu, cam, geoms, rank, count)
            if want is not None:
                resolved_waves += int((want[3] >= 0).sum())
        poses += 1
    print("%d poses, %d resolved waves compared" % (poses, resolved_waves))
    assert poses == 84 and resolved_waves > 0


def test_device_certificates_equal_the_hosts_at_1280x720(gpu):
    sc = _scene(gpu, "cornell.txt", 1280, 720)
    cam, geoms = sc.camera.view(gpu.CAMERA_DTYPE), sc.geoms.view(gpu.GEOM_DTYPE)
    for rank, count in ((0, 1), (1, 3)):
        want = _lists_equal(gpu, cam, geoms, rank, count)
        lanes = want[0].reshape(-1, 64)
        share = ((lanes != 0xFFFFFFFF) & (want[3][:, None] >= 0)).sum() / max((lanes != 0xFFFFFFFF).sum(), 1)
        assert share >= 0.80            # (tests/test_camera_resolve_cpu.py's floor for this frame: not an equality of nothing)


# ---- moves ------------------------------------------------------------------------------------------------------------------------------
def _pose(sc, de=(0, 0, 0), yaw=0.0):
    """the scene's camera record with the eye moved by `de` and the view turned by `yaw` degrees about up"""
    cam = np.array(sc.camera, copy=True)
    cam["position"][0] = (np.asarray(cam["position"][0], np.float64) + np.asarray(de, np.float64)).astype(F)
    if yaw:
        cam["view"][0] = camera_poses._rotate(cam["view"][0], cam["up"][0], yaw).astype(F)
    return cam


def _family_poses(gpu, sc, name, labels):
    by = dict(camera_poses.poses(name, sc.camera.view(gpu.CAMERA_DTYPE), sc.geoms.view(gpu.GEOM_DTYPE)))
    return [by[label] for label in labels]


def _counters(gpu):
    c = gpu.counters()
    return (tuple(c.live), tuple(c.ended_early), c.misses, c.light_hits, c.iterations)


def _walk(gpu, sc, cams, in_place, opts, schedule="single", reads=(), pbo=None, zero=None, before_move=None):
    """The chain `cams` walked by pathtraceInit over the live renderer (in_place False) or by pathtraceSetCamera; after every pose
    n = 1 + i % 4 iterations (2 + i % 3 where a read needs two samples), then what `reads` names.  -> per pose a dict of arrays, and per
    move (camera_move_info, live device buffers before, after)."""
    own = np.array(sc.camera, copy=True)
    out, moves = [], []
    live = gpu.test_lib().pt_test_live_device_buffers
    gpu.pathtraceFree()
    try:
        for i, cam in enumerate(cams):
            if zero is not None:
                zero()                                   # (a caller-owned accumulator is the caller's to zero: both ways)
            if i and before_move:
                before_move()
            if i == 0 or not in_place:
                sc.camera[:] = cam
                gpu.pathtraceInit(sc, **opts)
            else:
                before = live()
                gpu.pathtraceSetCamera(cam)
                moves.append((gpu.camera_move_info(), before, live()))
            n = 2 + i % 3 if "denoise_var" in reads else 1 + i % 4
            p = pbo.data_ptr() if pbo is not None else None
            if schedule == "single":
                for it in range(1, n + 1):
                    gpu.pathtrace(p, 0, it, readback=False)
            else:
                gpu.pathtrace_batch(p, 0, 1, n)
            P = int(sc.camera["resolution"][0][0]) * int(sc.camera["resolution"][0][1])
            got = {"accum": gpu.readback(P).copy(), "counters": _counters(gpu)}
            if "moments" in reads:
                got["moments"] = gpu.readback_moments()
            if "gbuffer" in reads:
                got["pos_t"], got["nrm"], got["geom"] = gpu.gbuffer(1)
            if "denoise_var" in reads:
                got["dv"], got["dv_var"] = gpu.denoise_var(n, with_variance=True)
            if "denoise_var1" in reads:
                got["dv1"] = gpu.denoise_var(n)
            if pbo is not None:
                gpu.sync()
                got["pbo"] = pbo.cpu().numpy().copy()
            out.append(got)
    finally:
        gpu.pathtraceFree()
        sc.camera[:] = own
    return out, moves


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


def _compare(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys()
        for k in x:
            if k == "counters":
                assert x[k] == y[k], "pose %d: counters differ" % i
            else:
                assert np.array_equal(_bits(x[k]), _bits(y[k])), "pose %d: %s differs" % (i, k)


def _all_fast(moves, temporal, nmoves, has_list=False):
    """every move fast, and the live device buffers across it: unchanged -- but for the first move, which makes the two scratch buffers of
    the device certificates, and, under PT_FLAG_TEMPORAL, the first two, whose captures allocate the history's two halves as pt_init's do.
    has_list: a scene that takes the packed work list where it fits -- its four camera tables come and go together with it."""
    assert len(moves) == nmoves
    for j, (info, before, after) in enumerate(moves):
        assert info["fast"] is True, "move %d took the slow path" % (j + 1)
        if temporal and j < 2:
            continue
        allowed = {0, 2} if j == 0 else {0}
        if has_list:
            allowed |= {a + t for a in allowed for t in (4, -4)}
        assert after - before in allowed, "move %d: %d -> %d live device buffers" % (j + 1, before, after)


CHAINS = [
    # (id, scene, W, H, poses, pathtraceInit's options, schedule, reads)
    ("cornell_plain", "cornell.txt", 97, 61, ("own", "side_0.3", "yaw_30", "dolly_0.52", "outside", "side_1"),
     dict(traceDepth=4, moments=True, temporal=True), "single", ("moments", "gbuffer", "denoise_var")),
    ("textured_batch4_three_slots", "cornell_textured.txt", 48, 32, [((0, 0, 0), 0), ((0.4, 0.1, -0.3), 0), ((0.4, 0.1, -0.3), 12), ((-0.8, 0, 0.2), -20)],
     dict(traceDepth=4, pipeline_depth=3, max_batch=4), "batch", ()),
    ("mesh", "cornell_mesh.txt", 48, 32, [((0, 0, 0), 0), ((0.3, 0.2, -0.2), 0), ((0.3, 0.2, -0.2), 15), ((-0.5, 0, 0), -10)],
     dict(traceDepth=3, moments=True, temporal=True), "single", ("moments", "gbuffer", "denoise_var")),
    ("spheres64_many_trace_ahead", "spheres64.txt", 48, 36, [((0, 0, 0), 0), ((0.5, 0, 0), 0), ((0.5, 0.3, -0.5), 10), ((0, 0, 0), -15), ((0, 0.2, 0), 0)],
     dict(traceDepth=4, pipeline_depth=2, max_batch=4, trace_ahead=True), "single", ()),
    ("thin_lens_two_shards", "cornell.txt", 97, 61, [((0, 0, 0), 0), ((0.3, 0, 0), 0), ((0.3, 0, -0.5), 8), ((-1, 0.2, 0), -5)],
     dict(traceDepth=4, lens_radius=0.2, focal_distance=10.0, shard_rank=1, shard_count=2), "single", ()),
    ("direct_lighting", "cornell.txt", 97, 61, ("own", "side_1", "yaw_5", "outside", "own"),
     dict(traceDepth=4, direct_lighting=True, max_batch=4), "batch", ()),
    ("through_nothing_demod_history", "cornell.txt", 97, 61, ("own", "away", "own", "side_0.3", "yaw_30"),
     dict(traceDepth=4, moments=True, temporal=True, demodulate=True, demod_history=True, spatial_variance=True, display_filter=True, max_batch=4),
     "batch", ("moments", "gbuffer", "denoise_var1", "pbo")),
    # the table rules no chain above reaches: the groups' table (it has a buffer even when empty) and the rows kept in global memory ...
    ("spheres64_grouped", "spheres64.txt", 48, 36, [((0, 0, 0), 0), ((0.5, 0, 0), 0), ((0.5, 0.3, -0.5), 10), ((0, 0, 0), -15)],
     dict(traceDepth=3), "single", ()),
    # ... and the three bump tables with the tables of a mesh that carries UVs
    ("bump_mapped", "cornell_bump.txt", 48, 32, [((0, 0, 0), 0), ((0.4, 0.1, -0.3), 0), ((0.4, 0.1, -0.3), 12), ((-0.8, 0, 0.2), -20)],
     dict(traceDepth=3), "single", ()),
]
CHAIN_ENV = {"spheres64_grouped": {"PT_AMD_GROUPS": "1"}}      # (set for the whole walk, both ways)


def _chain_cams(gpu, sc, name, poses):
    if isinstance(poses[0], str):
        return _family_poses(gpu, sc, name, poses)
    return [_pose(sc, de, yaw) for de, yaw in poses]


@pytest.mark.parametrize("cid,name,W,H,poses,opts,schedule,reads", CHAINS, ids=[c[0] for c in CHAINS])
def test_a_chain_of_moves_equals_the_chain_of_reinitialisations(gpu, monkeypatch, cid, name, W, H, poses, opts, schedule, reads):
    import torch
    for k, v in CHAIN_ENV.get(cid, {}).items():
        monkeypatch.setenv(k, v)
    sc = _scene(gpu, name, W, H)
    if name == "cornell_bump.txt":                       # (as tests/test_gpu_keep_renderer.py loads it: a face-material array for its mesh)
        sc.mesh_materials = {7: np.full(len(sc.meshes[7]), -1, np.int32)}
    cams = _chain_cams(gpu, sc, name, poses)
    pbo = torch.zeros((W * H, 4), dtype=torch.uint8, device="cuda") if "pbo" in reads else None
    reads = tuple(r for r in reads if r != "pbo")
    with gpu.renderer_from_test_library():
        a, _ = _walk(gpu, sc, cams, False, opts, schedule, reads, pbo)
        b, moves = _walk(gpu, sc, cams, True, opts, schedule, reads, pbo)
    _compare(a, b)
    has_list = name == "cornell.txt" and not opts.get("lens_radius")
    _all_fast(moves, bool(opts.get("temporal")), len(cams) - 1, has_list)
    uploaded = [m[0]["tables_uploaded"] for m in moves]
    print("%s: tables uploaded per move %r, bytes %r" % (cid, uploaded, [m[0]["bytes_uploaded"] for m in moves]))
    assert not np.array_equal(a[0]["accum"], a[1]["accum"])          # (the poses differ: not a chain of one view)


def test_a_move_with_batches_parked_discards_them(gpu):
    """PT_FLAG_TRACE_AHEAD: one iteration asked for, batches of four traced ahead and parked; the move discards them, and the slots'
    iteration masks are found zeroed by the new view's batches -- or its frames would carry the old view's light."""
    sc = _scene(gpu, "cornell.txt", 97, 61)
    cams = _family_poses(gpu, sc, "cornell.txt", ("own", "side_1", "yaw_30", "own"))
    opts = dict(traceDepth=4, pipeline_depth=3, max_batch=4, trace_ahead=True)
    with gpu.renderer_from_test_library():
        a, _ = _walk(gpu, sc, cams, False, opts, "single")
        b, moves = _walk(gpu, sc, cams, True, opts, "single")
    _compare(a, b)
    _all_fast(moves, False, 3)
    # (pose 3 is pose 0 again: its first sample is the first pose's frame only if nothing of the views between survived in the slots)
    assert all(m[0]["tables_uploaded"] >= 1 for m in moves)


def test_a_caller_owned_accumulator_on_a_callers_stream(gpu):
    import torch
    sc = _scene(gpu, "cornell.txt", 97, 61)
    cams = _family_poses(gpu, sc, "cornell.txt", ("own", "side_0.3", "yaw_5", "outside"))
    stream = torch.cuda.Stream()
    acc = torch.zeros(97 * 61 * 3, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def zero():
        with torch.cuda.stream(stream):
            acc.zero_()
        stream.synchronize()

    opts = dict(traceDepth=4, max_batch=4, accum_dev=acc.data_ptr(), stream=stream.cuda_stream)
    with gpu.renderer_from_test_library():
        a, _ = _walk(gpu, sc, cams, False, opts, "batch", zero=zero)
        b, moves = _walk(gpu, sc, cams, True, opts, "batch", zero=zero)
    _compare(a, b)
    _all_fast(moves, False, 3)


def test_the_final_pose_against_the_cpu_oracle(gpu, oracle):
    sc = _scene(gpu, "cornell.txt", 97, 61)
    cams = _family_poses(gpu, sc, "cornell.txt", ("own", "yaw_30", "side_1"))
    with gpu.renderer_from_test_library():
        b, moves = _walk(gpu, sc, cams, True, dict(traceDepth=4), "single")
    _all_fast(moves, False, 2)
    last = np.array(sc.camera, copy=True)
    last[:] = cams[-1]
    ref = oracle.Renderer(last.view(oracle.CAMERA_DTYPE), sc.geoms.view(oracle.GEOM_DTYPE), sc.materials.view(oracle.MATERIAL_DTYPE), 4)
    want = np.zeros(97 * 61 * 3, F)
    for it in range(1, 4):                               # (pose 2 renders n = 1 + 2 % 4 = 3 iterations)
        ref.iterate(it, want)
    got = b[-1]["accum"]
    rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-6)
    assert int((rel > 1e-3).sum()) == 0                  # (the criterion of the package's smoke run)


# ---- a move after a re-registration --------------------------------------------------------------------------------------------------------
def _other_textures(gpu, sc, new):
    new.textures = [np.ascontiguousarray(np.roll(np.asarray(t, F), 1, axis=-1)) for t in sc.textures]      # (every texel's channels rotated)
    assert any(not np.array_equal(a, b) for a, b in zip(new.textures, sc.textures))
    return lambda: gpu.set_textures(*gpu._scene_textures(new))


def _other_meshes(gpu, sc, new):
    new.meshes = {g: np.asarray(t, F) + F(0.25) for g, t in sc.meshes.items()}                             # (translated in object space)
    return lambda: gpu.set_meshes(new.meshes, getattr(new, "mesh_normals", None), getattr(new, "mesh_materials", None))


@pytest.mark.parametrize("name,other", [("cornell_textured.txt", _other_textures), ("cornell_mesh.txt", _other_meshes)], ids=["textures", "meshes"])
def test_a_move_after_a_re_registration_renders_what_the_renderer_was_initialised_with(gpu, name, other):
    """pt_set_textures / pt_set_meshes between pathtraceInit and the move: the move -- the fast way, and the slow one of a faulted renderer --
    renders the scene the renderer was initialised with, and what was registered since serves the next full pathtraceInit."""
    W, H = 48, 32
    P = W * H
    sc, new = _scene(gpu, name, W, H), _scene(gpu, name, W, H)
    register_new = other(gpu, sc, new)
    own = np.array(sc.camera, copy=True)
    pose2 = _pose(sc, (0.4, 0.1, -0.3), 12)

    def frame():
        for it in (1, 2):
            gpu.pathtrace(None, 0, it, readback=False)
        return gpu.readback(P).copy(), _counters(gpu)

    def init(scene, cam):
        scene.camera[:] = cam
        gpu.pathtraceInit(scene, traceDepth=3)
        return frame()

    def same(a, b):
        return np.array_equal(_bits(a[0]), _bits(b[0])) and a[1] == b[1]

    with gpu.renderer_from_test_library():
        gpu.pathtraceFree()
        try:
            want_old = init(sc, pose2)
            gpu.pathtraceFree()
            want_new = init(new, pose2)
            gpu.pathtraceFree()
            assert not same(want_old, want_new)
            for fault in (False, True):
                init(sc, own)
                register_new()
                if fault:
                    gpu.force_fault(2)
                gpu.pathtraceSetCamera(pose2)
                assert gpu.camera_move_info()["fast"] is (not fault)
                assert same(frame(), want_old), "fault %r: the move rendered something else than the renderer's own scene" % fault
                if not fault:                            # the full call over the moved renderer: what is registered now
                    got = init(new, pose2)
                    assert not same(got, want_old) and same(got, want_new)
                gpu.pathtraceFree()
        finally:
            gpu.pathtraceFree()
            sc.camera[:] = own
            new.camera[:] = own


# ---- slow path and refusals ---------------------------------------------------------------------------------------------------------------
def test_a_faulted_renderer_takes_the_slow_path_and_renders_the_right_frame(gpu):
    sc = _scene(gpu, "cornell.txt", 97, 61)
    cams = _family_poses(gpu, sc, "cornell.txt", ("own", "side_1"))
    opts = dict(traceDepth=4)
    with gpu.renderer_from_test_library():
        a, _ = _walk(gpu, sc, cams, False, opts, "single")
        b, moves = _walk(gpu, sc, cams, True, opts, "single", before_move=lambda: gpu.force_fault(2))
    assert len(moves) == 1 and moves[0][0]["fast"] is False
    _compare(a, b)                                       # (the fault word went with the old renderer: the readback reports none)


def test_a_camera_of_another_resolution_is_refused_and_the_old_view_goes_on(gpu):
    sc = _scene(gpu, "cornell.txt", 97, 61)
    P = 97 * 61
    with gpu.renderer_from_test_library():
        gpu.pathtraceFree()
        frames = []
        for refuse in (False, True):
            gpu.pathtraceInit(sc, traceDepth=4)
            gpu.pathtrace(None, 0, 1, readback=False)
            if refuse:
                other = np.array(sc.camera, copy=True)
                other["resolution"][0] = (96, 61)
                with pytest.raises(gpu.PtError, match="resolution"):
                    gpu.pathtraceSetCamera(other)
                assert gpu.camera_move_info()["fast"] is None
                with pytest.raises(gpu.PtError, match="null camera"):
                    gpu._check(gpu.lib().pt_init(None, None, 0, None, 0, gpu.PT_SAME_SCENE, None))
            gpu.pathtrace(None, 0, 2, readback=False)
            frames.append((gpu.readback(P).copy(), _counters(gpu)))
            gpu.pathtraceFree()
    assert np.array_equal(_bits(frames[0][0]), _bits(frames[1][0])) and frames[0][1] == frames[1][1]


def test_a_move_in_one_context_leaves_the_default_one_alone(gpu):
    sc = _scene(gpu, "cornell.txt", 97, 61)
    other = _scene(gpu, "cornell.txt", 97, 61)
    moved = _family_poses(gpu, sc, "cornell.txt", ("yaw_30",))[0]
    P = 97 * 61
    with gpu.renderer_from_test_library():
        gpu.pathtraceFree()
        frames = []
        for move in (False, True):
            gpu.pathtraceInit(sc, traceDepth=4)
            gpu.pathtrace(None, 0, 1, readback=False)
            ctx = gpu.Context()
            try:
                with ctx:
                    gpu.pathtraceInit(other, traceDepth=4)
                    gpu.pathtrace(None, 0, 1, readback=False)
                    if move:
                        gpu.pathtraceSetCamera(moved)
                        assert gpu.camera_move_info()["fast"] is True
                        gpu.pathtrace(None, 0, 1, readback=False)
                    inner = gpu.readback(P).copy()
                    gpu.lib().pt_free()
            finally:
                ctx.destroy()
            gpu.pathtrace(None, 0, 2, readback=False)
            frames.append((gpu.readback(P).copy(), _counters(gpu), inner))
            gpu.pathtraceFree()
    assert np.array_equal(_bits(frames[0][0]), _bits(frames[1][0])) and frames[0][1] == frames[1][1]
    assert not np.array_equal(frames[0][2], frames[1][2])            # (the other context did move)


# ---- pt_render --in-place -------------------------------------------------------------------------------------------------------------------
EXE = os.path.join(os.path.dirname(SCENES), "project3-cuda-path-tracer_amd", "host", "pt_render")


@pytest.mark.parametrize("scene,extra", [("cornell.txt", []), ("cornell.txt", ["--spatial-variance", "--batch", "4"]),
                                         ("cornell_textured.txt", ["--history-albedo"])], ids=["denoise_var", "spatial_batch4", "history_albedo"])
def test_pt_render_in_place_writes_the_same_pngs(gpu, tmp_path, scene, extra):
    """pt_render --history-from EX EY EZ N renders N iterations from that eye, moves to the scene's camera and writes <out>.png and, from the
    blend with the history the move left behind, <out>.denoised.png; with --in-place the move is pt_init's same-scene form instead of the
    full call.  The files of the two runs are the same bytes."""
    import subprocess
    args = [EXE, os.path.join(SCENES, scene), "--res", "72", "40", "--iterations", "3", "--depth", "4", "--denoise-var", "5", "4.0", "0.35", "2.0",
            "--history-from", "0.4", "5.1", "10.3", "5"] + extra
    env = dict(os.environ)
    for k in ("PT_AMD_DEVICES", "PT_AMD_DISPLAY_FILTER", "PT_AMD_SPATIAL_VARIANCE"):
        env.pop(k, None)
    for name, more in (("full", []), ("inplace", ["--in-place"])):
        r = subprocess.run(args + more + ["--out", str(tmp_path / name)], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, (name, r.stderr[-2000:])
    for suffix in (".png", ".denoised.png"):
        a, b = (open(str(tmp_path / (name + suffix)), "rb").read() for name in ("full", "inplace"))
        assert len(a) > 100 and a == b, suffix
    r = subprocess.run([EXE, os.path.join(SCENES, scene), "--in-place"], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode != 0 and "--in-place needs --history-from" in r.stderr
