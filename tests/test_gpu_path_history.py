"""History-coded path pools on the device (csrc/pt_trace.h: PathPool, k_bounce<..., PLAIN>): a path carries the ordered list of its
scatters' (material, diffuse | specular) codes in one word instead of its throughput, and the emitter hit replays the products.

The scenes are generated here: a box of five walls, a light, a sphere and a small cube over EIGHT materials, three of them half mirrors
whose specular colour differs from their colour (a swapped code, a swapped bit or a code at the wrong position changes the frame).  At
96x64, batches of 1 and of 4, one and two batches in flight:

  a. depth 9 (4 bits x 8 scatters: the word is full) plans the history form; the frame equals the CPU oracle's bit for bit;
  b. depth 10, and depth 9 with a ninth material, plan the general form; the same outcome;
  c. through the test library's pool dump (which rebuilds the throughput from the history on the host) every queued path's origin,
     direction and throughput equal the oracle's after every bounce 0 .. 8 -- bounce 8's code is the word's last nibble;
  d. the paths that end on the light at their first hit (a depth-1 render) and those that reach it at the last bounce (the pixels in which
     the depth-9 frame of one iteration differs from the depth-8 frame) contribute the oracle's radiance, and there are such paths;
  e. a mesh whose faces name materials of their own (`usemtl`) between two other materials: scenes with meshes have no PLAIN form, so this
     plans the general layout (histBits 0) -- the frame and the per-bounce throughput, which carries the FACE's colour, equal the oracle's;
  f. with a thin lens the camera-ray launch is a general form (there is no PLAIN one with a lens) that feeds the PLAIN launches' history
     pool: the plan says dof|plain with history bits, and the frame equals the oracle's.
"""
import os
import types

import numpy as np
import pytest

from conftest import SCENES
from test_kernel_select_cpu import STATE, names

pytestmark = pytest.mark.gpu

W, H = 96, 64
NPIX = W * H


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def gpu(pt):
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return pt


def _materials(pt, ninth=False):
    rows = [((1, 1, 1), (0, 0, 0), 0, 5),                           # 0 the light
            ((.98, .97, .96), (0, 0, 0), 0, 0),                     # 1 - 4 diffuse
            ((.85, .35, .33), (0, 0, 0), 0, 0),
            ((.31, .84, .37), (0, 0, 0), 0, 0),
            ((.40, .45, .90), (0, 0, 0), 0, 0),
            ((.90, .95, .80), (.97, .90, .85), 1, 0),               # 5 - 7 half mirror, half diffuse: specular colour != colour
            ((.70, .60, .95), (.99, .93, .60), 1, 0),
            ((.93, .72, .52), (.62, .91, .97), 1, 0)]
    if ninth:
        rows.append(((.5, .6, .7), (0, 0, 0), 0, 0))
    m = np.zeros(len(rows), pt.MATERIAL_DTYPE)
    for i, (col, spec, refl, emit) in enumerate(rows):
        m[i] = (col, 0, spec, refl, 0, 0, emit)
    return m


def _geoms(orc, ninth=False):
    S = orc.make_geom
    return [S(1, 0, (0, 10, 0), (0, 0, 0), (4, .3, 4)),             # the light
            S(1, 1, (0, 0, 0), (0, 0, 0), (10, .01, 10)),           # floor
            S(1, 4, (0, 10, 0), (0, 0, 90), (.01, 10, 10)),         # ceiling
            S(1, 5, (0, 5, -5), (0, 90, 0), (.01, 10, 10)),         # back wall: a mirror
            S(1, 2, (-5, 5, 0), (0, 0, 0), (.01, 10, 10)),
            S(1, 3, (5, 5, 0), (0, 0, 0), (.01, 10, 10)),
            S(0, 6, (-1.6, 3.2, -0.5), (0, 0, 0), (3, 3, 3)),       # a mirror sphere
            S(1, 8 if ninth else 7, (2.0, 1.2, 1.0), (0, 30, 0), (2.2, 2.4, 2.2))]   # a small cube: the third mirror (or the ninth material)


def _scene(pt, orc, ninth=False, extra=(), meshes=None, mesh_materials=None):
    cam = pt.Scene(os.path.join(SCENES, "cornell.txt"))
    cam.set_resolution(W, H)
    g = np.concatenate(_geoms(orc, ninth) + list(extra)).view(pt.GEOM_DTYPE)
    return types.SimpleNamespace(geoms=g, materials=_materials(pt, ninth), camera=cam.camera.copy(), traceDepth=9, meshes=meshes or {}, mesh_normals={},
                                 mesh_materials=mesh_materials or {}, image=np.zeros((H, W, 3), np.float32))


_oracle_frames = {}


def _want(orc, sc, key, depth, iters):
    """the oracle's accumulator after each of `iters` iterations (computed once per scene and depth, never changed)"""
    k = (key, depth)
    if k not in _oracle_frames or len(_oracle_frames[k]) < iters:
        ref = orc.Renderer(sc.camera.view(orc.CAMERA_DTYPE), sc.geoms.view(orc.GEOM_DTYPE), sc.materials.view(orc.MATERIAL_DTYPE), depth,
                           meshes=sc.meshes or None, mesh_materials=sc.mesh_materials or None)
        acc, frames = np.zeros(NPIX * 3, np.float32), []
        for it in range(1, iters + 1):
            ref.iterate(it, acc)
            frames.append(acc.copy())
            frames[-1].setflags(write=False)
        _oracle_frames[k] = frames
    return _oracle_frames[k][iters - 1]


def _render(gpu, sc, depth, max_batch, pipeline, iters):
    gpu.pathtraceFree()
    gpu.pathtraceInit(sc, traceDepth=depth, max_batch=max_batch, pipeline_depth=pipeline)
    try:
        if max_batch == 1:
            for it in range(1, iters + 1):
                gpu.pathtrace(None, 0, it, readback=False)
        else:
            for first in range(1, iters + 1, max_batch):
                gpu.pathtrace_batch(None, 0, first, max_batch)
        return gpu.readback(NPIX)
    finally:
        gpu.pathtraceFree()


# (batch, batches in flight, iterations: four -- eight where two batches of four are to be in flight)
RUNS = [(1, 1, 4), (1, 2, 4), (4, 1, 4), (4, 2, 8)]


@pytest.mark.parametrize("max_batch,pipeline,iters", RUNS)
def test_a_depth_nine_takes_the_history_form_and_renders_the_oracles_frame(gpu, oracle, max_batch, pipeline, iters):
    sc = _scene(gpu, oracle)
    plan = gpu.scene_plan(sc, traceDepth=9, max_batch=max_batch, pipeline_depth=pipeline)
    assert names(plan.state_bits, STATE) == "plain" and plan.histBits == 4
    got = _render(gpu, sc, 9, max_batch, pipeline, iters)
    want = _want(oracle, sc, "eight", 9, iters)
    assert want.max() > 0
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("max_batch,pipeline,iters", RUNS)
@pytest.mark.parametrize("ninth,depth", [(False, 10), (True, 9)])
def test_b_beyond_one_word_the_general_form_renders_the_same(gpu, oracle, ninth, depth, max_batch, pipeline, iters):
    sc = _scene(gpu, oracle, ninth)
    plan = gpu.scene_plan(sc, traceDepth=depth, max_batch=max_batch, pipeline_depth=pipeline)
    assert names(plan.state_bits, STATE) == "0" and plan.histBits == 0
    got = _render(gpu, sc, depth, max_batch, pipeline, iters)
    want = _want(oracle, sc, "nine" if ninth else "eight", depth, iters)
    assert want.max() > 0
    assert np.array_equal(bits(got), bits(want))


def _paths_equal_the_oracles(gpu, oracle, sc, depth, bounces, iters=(1, 37)):
    ref = oracle.Renderer(sc.camera.view(oracle.CAMERA_DTYPE), sc.geoms.view(oracle.GEOM_DTYPE), sc.materials.view(oracle.MATERIAL_DTYPE), depth,
                          meshes=sc.meshes or None, mesh_materials=sc.mesh_materials or None)
    gpu.pathtraceFree()
    gpu.pathtraceInit(sc, traceDepth=depth)
    seen = set()
    try:
        for it in iters:
            for b in bounces:
                o, d, c, pix = gpu.debug_trace_paths(it, b, NPIX)
                wo, wd, wc, wpix = ref.dump_paths(it, b)
                assert len(pix) == len(wpix) and np.array_equal(pix, wpix), (it, b)
                for g, w, what in ((o, wo, "origin"), (d, wd, "direction"), (c, wc, "throughput")):
                    assert np.array_equal(bits(g), bits(w)), (it, b, what)
                if b == bounces[-1]:
                    assert len(pix) > 0, (it, b)                        # (paths are still alive behind the last bounce looked at)
                seen.update(map(tuple, np.unique(bits(c).reshape(-1, 3), axis=0)[:64].tolist()))
    finally:
        gpu.pathtraceFree()
    return seen


def test_c_every_queued_paths_throughput_equals_the_oracles_at_every_bounce(gpu, oracle):
    sc = _scene(gpu, oracle)
    assert gpu.scene_plan(sc, traceDepth=9).histBits == 4
    seen = _paths_equal_the_oracles(gpu, oracle, sc, 9, list(range(0, 9)))
    assert len(seen) > 8                                                 # (more throughputs than materials: products of several codes)


def test_d_first_hit_and_last_bounce_emitter_paths_contribute_the_oracles_radiance(gpu, oracle):
    sc = _scene(gpu, oracle)
    # the first hit: at depth 1 nothing else contributes (the history is empty: the throughput is (1, 1, 1))
    first = _render(gpu, sc, 1, 1, 1, 1)
    assert np.array_equal(bits(first), bits(_want(oracle, sc, "eight", 1, 1))) and np.count_nonzero(first) > 0
    # the last bounce: one iteration has one path per pixel, and a path contributes once -- the pixels in which the depth-9 frame differs from
    # the depth-8 frame are the paths that reach the light at bounce 9, behind a full word of eight codes
    nine, eight = _render(gpu, sc, 9, 1, 1, 1), _render(gpu, sc, 8, 1, 1, 1)
    w9, w8 = _want(oracle, sc, "eight", 9, 1), _want(oracle, sc, "eight", 8, 1)
    last = np.flatnonzero((bits(w9) != bits(w8)).reshape(-1, 3).any(axis=1))
    assert len(last) > 0 and not w8.reshape(-1, 3)[last].any()
    assert np.array_equal(bits(nine), bits(w9)) and np.array_equal(bits(eight), bits(w8))
    assert np.array_equal(bits(nine.reshape(-1, 3)[last]), bits(w9.reshape(-1, 3)[last]))


def _cube_triangles():
    c = np.array([[x, y, z] for x in (-.5, .5) for y in (-.5, .5) for z in (-.5, .5)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = []
    for a, b, cc, d in quads:
        tris += [np.concatenate([c[a], c[b], c[cc]]), np.concatenate([c[a], c[cc], c[d]])]
    return np.stack(tris).astype(np.float32)


def test_e_a_usemtl_face_between_two_other_materials(gpu, oracle):
    # object material 2; its faces name 5 (a mirror), the object's (-1), 3, 6, 1, 7: a path meets the face's material between the walls'
    mesh = oracle.make_geom(2, 2, (1.5, 4.5, -1.5), (20, 35, 10), (2.6, 2.6, 2.6))
    sc = _scene(gpu, oracle, extra=[mesh], meshes={8: _cube_triangles()}, mesh_materials={8: np.repeat(np.array([5, -1, 3, 6, 1, 7], np.int32), 2)})
    plan = gpu.scene_plan(sc, traceDepth=9)
    assert names(plan.state_bits, STATE) == "mesh|plain" and plan.histBits == 0          # (scenes with meshes have no PLAIN form)
    got = _render(gpu, sc, 9, 4, 2, 4)
    want = _want(oracle, sc, "mesh", 9, 4)
    assert want.max() > 0 and np.array_equal(bits(got), bits(want))
    _paths_equal_the_oracles(gpu, oracle, sc, 9, [1, 2, 5, 8], iters=(1,))


def test_f_a_lens_camera_launch_feeds_the_history_pool(gpu, oracle):
    sc = _scene(gpu, oracle)
    lens = dict(lens_radius=0.3, focal_distance=10.0)
    plan = gpu.scene_plan(sc, traceDepth=9, max_batch=4, pipeline_depth=2, **lens)
    assert names(plan.state_bits, STATE) == "dof|plain" and plan.histBits == 4
    ref = oracle.Renderer(sc.camera.view(oracle.CAMERA_DTYPE), sc.geoms.view(oracle.GEOM_DTYPE), sc.materials.view(oracle.MATERIAL_DTYPE), 9)
    ref.set_extras(**lens)
    want = np.zeros(NPIX * 3, np.float32)
    for it in range(1, 5):
        ref.iterate(it, want)
    gpu.pathtraceFree()
    gpu.pathtraceInit(sc, traceDepth=9, max_batch=4, pipeline_depth=2, **lens)
    try:
        gpu.pathtrace_batch(None, 0, 1, 4)
        got = gpu.readback(NPIX)
    finally:
        gpu.pathtraceFree()
    assert want.max() > 0 and np.array_equal(bits(got), bits(want))
