"""PT_FLAG_MOTION on the MI355X: 16 poses across the shutter, one pose per iteration.

THE LAW (include/pt_amd.h, "motion blur"): after iterations 1..n of a motion-blurred render both accumulators, the counters and every
read-back equal, bit for bit, what comes of adding, in iteration order, iteration i of an UNFLAGGED renderer initialised with the geoms of
step PT_MOTION_STEP(i).  The random numbers are keyed on iteration, pixel and depth and a batch equals its single calls, so nothing but the
pose distinguishes the two.

How the expectation is built (class Reference): one unflagged renderer per step over a caller-owned accumulator, a torch tensor; the
accumulator is zeroed, pt_iterate(i) runs alone, and the frame, its squared luminance and the tallies are read back.  The frames are added
in numpy, in fp32, in iteration order.  One case does the same with the CPU oracle's single iterations.  Every comparison is of bits, after
every call.  A build that ignores the flag renders step 0 throughout and fails every case here.

Frames are 37 x 23 (a partial last block of 256) to 64 x 48, depth 3 - 4."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import motion_scenes as ms
from conftest import ROOT, SCENES

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def gpu(pt):
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return pt


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("motion")


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _load(gpu, work, name, text, w, h):
    sc = gpu.Scene(ms.write(work, name + ".txt", text))
    sc.set_resolution(w, h)
    assert sc.step_geoms is not None
    return sc


def _tallies(c, depth):
    return (tuple(c.live[:depth + 3]), int(c.light_hits), int(c.misses))


class Reference:
    """iteration i of the unflagged renderer of step PT_MOTION_STEP(i), computed once per iteration and kept"""

    def __init__(self, gpu, torch, sc, depth, steps=None, **opts):
        self.gpu, self.torch, self.sc, self.depth, self.opts = gpu, torch, sc, depth, opts
        self.steps = sc.step_geoms if steps is None else np.asarray(steps).reshape(gpu.PT_MOTION_STEPS, -1)
        res = sc.camera["resolution"][0]
        self.P = int(res[0]) * int(res[1])
        self.acc = torch.zeros(self.P * 3, dtype=torch.float32, device="cuda")
        self.rec = {}

    def need(self, iterations):
        gpu = self.gpu
        missing = sorted(set(i for i in iterations if i not in self.rec))
        if not missing:
            return
        for s in sorted(set(gpu.motion_step(i) for i in missing)):
            static = ms.StaticScene(self.sc, self.steps[s])
            gpu.pathtraceFree()
            gpu.pathtraceInit(static, traceDepth=self.depth, accum_dev=self.acc.data_ptr(), motion=False, pipeline_depth=1, **self.opts)
            for i in (i for i in missing if gpu.motion_step(i) == s):
                gpu.pathtraceSetCamera(static.camera)                  # the same view anew: moments and tallies zeroed
                self.acc.zero_()
                self.torch.cuda.synchronize()
                gpu.pathtrace(None, 0, i, readback=False)
                rec = {"accum": gpu.readback(self.P).copy(), "tallies": _tallies(gpu.counters(), self.depth)}
                if self.opts.get("moments"):
                    rec["moments"] = gpu.readback_moments().copy()
                self.rec[i] = rec
        gpu.pathtraceFree()

    def total(self, iterations):
        self.need(iterations)
        out = {"accum": np.zeros(self.P * 3, F)}
        if self.opts.get("moments"):
            out["moments"] = np.zeros(self.P, F)
        live, hits, misses = np.zeros(self.depth + 3, np.int64), 0, 0
        for i in iterations:
            r = self.rec[i]
            for k in ("accum", "moments"):
                if k in out:
                    out[k] = (out[k] + np.asarray(r[k], F).reshape(-1)).astype(F)
            live += np.array(r["tallies"][0], np.int64)
            hits += r["tallies"][1]
            misses += r["tallies"][2]
        out["tallies"] = (tuple(int(v) for v in live), hits, misses)
        return out


def _compare(gpu, ref, done, what, tallies=True):
    want = ref.total(done)
    assert np.array_equal(_bits(gpu.readback(ref.P)), _bits(want["accum"])), "%s: the accumulator after iterations %s" % (what, done[-3:])
    if "moments" in want:
        assert np.array_equal(_bits(gpu.readback_moments()), _bits(want["moments"])), "%s: the moments" % what
    c = gpu.counters()
    assert c.iterations == len(done), "%s: the iterations counted" % what
    if tallies:
        assert _tallies(c, ref.depth) == want["tallies"], "%s: the tallies" % what


def _run(gpu, ref, schedule, what, steps=None, tallies=True, **opts):
    """a flagged renderer over the reference's scene and accumulator through `schedule`, compared after every call"""
    ref.need([i for op in schedule for i in range(op[1], op[1] + (op[2] if op[0] != "one" else 1))])
    gpu.pathtraceFree()
    ref.acc.zero_()
    ref.torch.cuda.synchronize()
    kw = dict(ref.opts)
    kw.update(opts)
    gpu.pathtraceInit(ref.sc, traceDepth=ref.depth, accum_dev=ref.acc.data_ptr(), motion=True if steps is None else steps, **kw)
    done = []
    try:
        for op in schedule:
            if op[0] == "one":
                gpu.pathtrace(None, 0, op[1], readback=False)
                done.append(op[1])
            elif op[0] == "batch":
                gpu.pathtrace_batch(None, 0, op[1], op[2])
                done += list(range(op[1], op[1] + op[2]))
            else:                                                      # ("until", first, count, check_every, lookahead): never converges
                _, n = gpu.iterate_until(op[1], 1e-6, op[1] + op[2] - 1, check_every=op[3], lookahead=op[4])
                assert n == op[1] + op[2] - 1
                done += list(range(op[1], op[1] + op[2]))
            _compare(gpu, ref, done, "%s %s" % (what, op), tallies)
    finally:
        gpu.pathtraceFree()


# ---- the schedules, on Cornell's sphere translating through the left wall -------------------------------------------------------------------
@pytest.fixture(scope="module")
def wall(gpu, torch, work):
    sc = _load(gpu, work, "wall", ms.SPHERE_THROUGH_WALL(), 37, 23)
    return Reference(gpu, torch, sc, 3, moments=True)


def test_the_spheres_class_changes_between_steps(gpu, wall):
    sc = wall.sc
    plans = [gpu.scene_plan(ms.StaticScene(sc, sc.step_geoms[s]), traceDepth=3) for s in range(16)]
    assert len({p.nLocalPad for p in plans}) > 1                                      # the camera rays' scene rectangle is each pose's own
    x = [float(sc.step_geoms[s][6]["translation"][0]) for s in range(16)]
    assert max(x) > -5 + 1.5 and min(x) < -5 - 1.5 and any(-6.5 < v < -3.5 for v in x)  # inside, outside, through the wall


SCHEDULES = {
    "first_1_count_8": (8, [("batch", 1, 8)]),
    "first_6_count_8_spans_two_runs": (8, [("batch", 6, 8)]),
    "single_calls_across_a_boundary": (8, [("one", i) for i in range(6, 12)]),
    "iterations_120_to_136_wrap_the_cycle": (32, [("batch", 120, 17)]),
    "batches_then_singles_then_a_batch": (8, [("batch", 1, 8), ("batch", 9, 3), ("one", 12), ("one", 13), ("batch", 14, 8)]),
}


@pytest.mark.parametrize("name", list(SCHEDULES))
def test_batches_are_cut_at_run_boundaries(gpu, wall, name):
    max_batch, schedule = SCHEDULES[name]
    _run(gpu, wall, schedule, name, max_batch=max_batch)


@pytest.mark.parametrize("pipeline_depth", [1, 3])
def test_a_batch_of_64_is_eight_pieces_on_fewer_slots(gpu, wall, pipeline_depth):
    _run(gpu, wall, [("batch", 1, 64), ("batch", 65, 64)], "64 at depth %d" % pipeline_depth, max_batch=64, pipeline_depth=pipeline_depth)


def test_trace_ahead_ends_its_batches_with_the_run(gpu, wall):
    # (the path tallies of a renderer that traces ahead count the batches it has parked and discarded too: here the frames, the moments and
    # the iterations counted are compared after every call)
    schedule = [("one", i) for i in range(1, 41)] + [("one", 50), ("one", 51), ("one", 3)]
    _run(gpu, wall, schedule, "trace ahead", tallies=False, max_batch=32, trace_ahead=True, pipeline_depth=3)


def test_a_piece_of_one_iteration_does_not_trace_ahead(gpu, wall):
    # a batch call cut at a run boundary into [8] and [9, 10]: the piece of one iteration is no pt_iterate call, nothing is traced ahead of
    # it, and the tallies are the sum's -- as they are for the same call on a renderer without the flag
    _run(gpu, wall, [("batch", 8, 3), ("batch", 11, 6), ("batch", 17, 8)], "pieces under trace ahead", max_batch=8, trace_ahead=True,
         pipeline_depth=3)


@pytest.mark.parametrize("lookahead", [0, 1])
def test_iterate_until_rounds_go_through_the_same_path(gpu, wall, lookahead):
    _run(gpu, wall, [("until", 1, 12, 12, lookahead), ("until", 13, 12, 12, lookahead), ("until", 25, 12, 12, lookahead)],
         "until, lookahead %d" % lookahead, max_batch=8)
    _run(gpu, wall, [("until", 1, 36, 12, lookahead)], "until in one call, lookahead %d" % lookahead, max_batch=8)


def test_two_row_shards(gpu, torch, wall):
    for rank in (0, 1):
        ref = Reference(gpu, torch, wall.sc, 3, shard_rank=rank, shard_count=2)
        _run(gpu, ref, [("batch", 5, 8), ("one", 13)], "shard %d" % rank, max_batch=8)


def test_the_cpu_oracle_defines_the_static_iterations(gpu, oracle, wall):
    sc = wall.sc
    iterations = list(range(5, 13))
    wall.need(iterations)
    by_step = {}
    for i in iterations:
        s = gpu.motion_step(i)
        if s not in by_step:
            by_step[s] = oracle.Renderer(sc.camera.view(oracle.CAMERA_DTYPE), np.ascontiguousarray(sc.step_geoms[s]).view(oracle.GEOM_DTYPE),
                                          sc.materials.view(oracle.MATERIAL_DTYPE), 3)
        img = np.zeros(wall.P * 3, F)
        by_step[s].iterate(i, img)
        assert np.array_equal(_bits(img), _bits(wall.rec[i]["accum"])), "iteration %d of step %d" % (i, s)
    assert len(by_step) == 2


# ---- the scenes -----------------------------------------------------------------------------------------------------------------------------
def test_poses_take_different_forms_of_k_bounce(gpu, torch, work):
    sc = _load(gpu, work, "slab", ms.TURNING_SLAB(), 48, 32)
    forms = []
    for s in range(16):
        p = gpu.scene_plan(ms.StaticScene(sc, sc.step_geoms[s]), traceDepth=3)
        pair = []
        for first in (1, 0):
            f = C.c_uint32(0)
            assert gpu.test_lib().pt_test_bounce_form(p.state_bits | first, C.byref(f)) == 0
            pair.append(f.value)
        forms.append(tuple(pair))
    assert len(set(forms)) == 2 and forms[0] != forms[15], forms                       # swept with the spheres (CUBES), then binned
    ref = Reference(gpu, torch, sc, 3, moments=True)
    # runs 1 - 4 are steps 0, 8, 4, 12: both forms, in flight on neighbouring slots
    assert len({forms[gpu.motion_step(i)] for i in (1, 9, 17, 25)}) == 2
    _run(gpu, ref, [("batch", 1, 32), ("batch", 33, 8)], "turning slab", max_batch=32, pipeline_depth=3)


def test_a_textured_sphere_and_a_uv_mapped_mesh_move(gpu, torch, work):
    sc = _load(gpu, work, "textured", ms.TEXTURED(), 48, 32)
    ref = Reference(gpu, torch, sc, 3, moments=True)
    _run(gpu, ref, [("batch", 1, 8), ("batch", 9, 16), ("one", 25)], "textured", max_batch=16)


def test_texels_and_mesh_records_are_held_once(gpu, torch, work):
    """The tables no pose changes are allocated once.  The test library counts the live device allocations (every one has an owner that counts)
    and says what pt_init planned to allocate of scene tables (pt_test_pose_tables): a flagged renderer holds EXACTLY 15 x a pose's own
    tables more than the unflagged renderer of step 0 -- one more buffer per pose, the texels or the mesh records uploaded again, and the count
    is off --, and the two tables held once are the texels and the mesh records, by their bytes."""
    sc = _load(gpu, work, "textured_once", ms.TEXTURED(), 48, 32)
    T = gpu.test_lib()

    def held(motion):
        n0 = T.pt_test_live_device_buffers()
        gpu.pathtraceInit(sc if motion else ms.StaticScene(sc, sc.step_geoms[0]), traceDepth=3, motion=motion, max_batch=8)
        out = (T.pt_test_live_device_buffers() - n0, gpu.pose_tables())
        gpu.pathtraceFree()
        return out

    with gpu.renderer_from_test_library():
        gpu.pathtraceFree()
        n1, t1 = held(False)
        n16, t16 = held(True)
        assert T.pt_test_live_device_buffers() == 0
    assert t1["poses"] == 1 and t16["poses"] == 16
    assert t1["shared_buffers"] == t16["shared_buffers"] == 2 and t1["own_buffers"] == t16["own_buffers"] > 2
    assert n16 - n1 == 15 * t1["own_buffers"], (n1, n16, t1, t16)
    texels = sum(t.shape[0] * t.shape[1] for t in sc.textures)
    assert t16["shared_bytes"] == t1["shared_bytes"] > 16 * texels                     # (float4 texels; the rest: the mesh's records)
    assert t16["all_own_bytes"] > 15 * t16["own_bytes"] // 2 and t1["all_own_bytes"] == t1["own_bytes"]


def test_a_moving_emitter_under_direct_lighting(gpu, torch, work):
    sc = _load(gpu, work, "emitter", ms.MOVING_EMITTER(), 48, 32)
    ref = Reference(gpu, torch, sc, 3, direct_lighting=True, moments=True)
    _run(gpu, ref, [("batch", 3, 8), ("batch", 11, 16)], "moving emitter", max_batch=16)
    weighted = Reference(gpu, torch, sc, 3, direct_lighting=True, mixture_weighted=True)
    _run(gpu, weighted, [("batch", 7, 4)], "moving emitter, weighted mixture", max_batch=4)


def test_a_thin_lens_and_kernel_timing(gpu, torch):
    sc = gpu.Scene(os.path.join(SCENES, "cornell_motion.txt"))
    sc.set_resolution(64, 48)
    ref = Reference(gpu, torch, sc, 4, lens_radius=0.3, focal_distance=9.0, moments=True)
    _run(gpu, ref, [("batch", 1, 8), ("batch", 9, 8), ("batch", 17, 5)], "thin lens", max_batch=8, flags=gpu.PT_FLAG_KERNEL_TIMING)


def test_sixteen_identical_steps_are_the_unflagged_renderer(gpu, torch):
    sc = gpu.Scene(os.path.join(SCENES, "cornell.txt"))
    sc.set_resolution(37, 23)
    P = 37 * 23
    got = {}
    for motion in (False, np.tile(sc.geoms, 16)):
        gpu.pathtraceFree()
        gpu.pathtraceInit(sc, traceDepth=4, moments=True, max_batch=8, motion=motion, flags=gpu.PT_FLAG_KERNEL_TIMING)
        for first in (1, 9, 17):
            gpu.pathtrace_batch(None, 0, first, 8)
        c = gpu.counters()
        got[motion is False] = (gpu.readback(P).copy(), gpu.readback_moments().copy(), _tallies(c, 4), c.bounce_launches, c.iterations)
        gpu.pathtraceFree()
    a, b = got[True], got[False]
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    assert a[2:] == b[2:] and a[3] == 3 * 4                                            # launches included: an aligned batch of 8 stays one set


# ---- refusals, the same-scene move, pt_render -----------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_live_renderer_rendering(gpu, torch, wall):
    sc = wall.sc
    wall.need(range(1, 9))
    gpu.pathtraceFree()
    wall.acc.zero_()
    torch.cuda.synchronize()
    kw = dict(traceDepth=3, accum_dev=wall.acc.data_ptr(), moments=True, max_batch=4)
    gpu.pathtraceInit(sc, motion=True, **kw)
    try:
        gpu.pathtrace_batch(None, 0, 1, 4)
        for bad in (dict(temporal=True), dict(temporal=True, object_history=True), dict(display_filter=True), dict(demodulate=True),
                    dict(spatial_variance=True), dict(keep=True)):
            with pytest.raises(gpu.PtError, match="PT_FLAG_MOTION"):
                gpu.pathtraceInit(sc, motion=True, **dict(kw, **bad))
        other = sc.step_geoms.copy()
        other["materialid"][9, 6] = 1
        with pytest.raises(gpu.PtError, match="step 9"):
            gpu.pathtraceInit(sc, motion=other, **kw)
        other = sc.step_geoms.copy()
        other["type"][3, 6] = 1
        with pytest.raises(gpu.PtError, match="step 3"):
            gpu.pathtraceInit(sc, motion=other, **kw)
        other = sc.step_geoms.copy()
        other["materialid"][:, 2] = 99                                                 # (every step names it: the plan of step 0 refuses)
        with pytest.raises(gpu.PtError, match="step 0"):
            gpu.pathtraceInit(sc, motion=other, **kw)
        with pytest.raises(gpu.PtError):
            gpu.pathtraceInit(sc, motion=sc.step_geoms[:8], **kw)                      # (the Python layer: not 16 x ngeoms records)
        for call in (lambda: gpu.denoise(4), lambda: gpu.denoise_rgba8(4), lambda: gpu.denoise_var(4), lambda: gpu.denoise_var_rgba8(4),
                     lambda: gpu.gbuffer(1)):
            with pytest.raises(gpu.PtError, match="PT_FLAG_MOTION"):
                call()
        g = gpu.Group(2, devices=[0, 0])
        try:
            with pytest.raises(gpu.PtError, match="PT_FLAG_MOTION"):
                g.init(sc, traceDepth=3, flags=gpu.PT_FLAG_MOTION)
        finally:
            g.destroy()
        gpu.pathtrace_batch(None, 0, 5, 4)
        _compare(gpu, wall, list(range(1, 9)), "after the refusals")
    finally:
        gpu.pathtraceFree()


def test_the_same_scene_move_is_the_full_call(gpu, torch, wall):
    sc = wall.sc
    cam2 = np.array(sc.camera, copy=True)
    cam2["position"][0] = (np.asarray(cam2["position"][0]) + F([0.4, -0.2, 0.3])).astype(F)
    P = wall.P
    got = []
    with gpu.renderer_from_test_library():
        for how in ("move", "full"):
            gpu.pathtraceFree()
            own = np.array(sc.camera, copy=True)
            try:
                gpu.pathtraceInit(sc, traceDepth=3, moments=True, max_batch=8, motion=True)
                gpu.pathtrace_batch(None, 0, 1, 8)
                if how == "move":
                    gpu.pathtraceSetCamera(cam2)
                    assert gpu.camera_move_info()["fast"] is False
                else:
                    sc.camera[:] = cam2
                    gpu.pathtraceInit(sc, traceDepth=3, moments=True, max_batch=8, motion=True)
                gpu.pathtrace_batch(None, 0, 5, 8)
                c = gpu.counters()
                got.append((gpu.readback(P).copy(), gpu.readback_moments().copy(), _tallies(c, 3), c.iterations))
            finally:
                sc.camera[:] = own
                gpu.pathtraceFree()
    assert np.array_equal(_bits(got[0][0]), _bits(got[1][0])) and np.array_equal(_bits(got[0][1]), _bits(got[1][1])) and got[0][2:] == got[1][2:]
    assert got[0][0].any()


@pytest.mark.parametrize("name", ["cornell_motion", "bumped_and_textured"])
def test_pt_render_blurs_a_scene_with_the_keywords(gpu, work, name):
    exe = os.path.join(ROOT, "project3-cuda-path-tracer_amd", "host", "pt_render")
    path = os.path.join(SCENES, "cornell_motion.txt")
    if name == "bumped_and_textured":      # a rippled mirror sphere and a textured, ridged torus moving: textures and height maps registered
        path = ms.write(work, "bump_motion.txt", ms.cornell({"base": "cornell_bump.txt", 6: {"TRANS_END": "0.5 4.5 0", "ROTAT_END": "0 60 0"},
                                                             7: {"TRANS_END": "1.5 3 1", "ROTAT_END": "20 40 25"}}))
    args = ["--res", "48", "36", "--iterations", "20", "--depth", "4", "--batch", "8"]
    subprocess.run([exe, path] + args + ["--out", str(work / "blur")], check=True, capture_output=True)
    subprocess.run([exe, path] + args + ["--out", str(work / "still"), "--no-motion"], check=True, capture_output=True)
    step0 = ms.write(work, "cornell_step0.txt", ms.static_text(open(path).read(), 0))
    subprocess.run([exe, step0] + args + ["--out", str(work / "step0")], check=True, capture_output=True)
    sc = gpu.Scene(path)
    sc.set_resolution(48, 36)
    gpu.pathtraceFree()
    gpu.pathtraceInit(sc, traceDepth=4, max_batch=8)                                   # (motion=None: the scene defines it)
    try:
        for first, n in ((1, 8), (9, 8), (17, 4)):
            gpu.pathtrace_batch(None, 0, first, n)
        gpu.save_png(str(work / "python"), gpu.readback(48 * 36).reshape(36, 48, 3), 20)
    finally:
        gpu.pathtraceFree()
    png = lambda name: open(str(work / (name + ".png")), "rb").read()
    assert png("blur") == png("python")
    if name == "bumped_and_textured":                                                  # ... and the height maps are in that frame
        sc.geom_bumps[:] = -1
        gpu.pathtraceInit(sc, traceDepth=4, max_batch=8)
        try:
            for first, n in ((1, 8), (9, 8), (17, 4)):
                gpu.pathtrace_batch(None, 0, first, n)
            gpu.save_png(str(work / "unbumped"), gpu.readback(48 * 36).reshape(36, 48, 3), 20)
        finally:
            gpu.pathtraceFree()
        assert png("unbumped") != png("blur")
    assert png("still") == png("step0") and png("still") != png("blur")
