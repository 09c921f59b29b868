"""Where a path goes next, on the MI355X, against float64 laws (tests/scatter_laws.py): the camera ray, the diffuse hemisphere, the REFL
mixture, the Phong lobe, the dielectric, the direct-lighting ray, the new origin, the light's contribution -- read from the state of the
test library's own renderer after EVERY bounce -- an exact furnace, and the denoiser's guide buffers (pt_gbuffer) against the camera rays'
float64 hits.  Seventeen cases and two furnaces: seven of the cases hold vertex normals (radial, bent, behind their faces, zero), face
materials (a face that emits on a dark object, dark faces on an emissive one, a scene lit by one face alone, a face-only emitter the
direct-lighting bounce aims at) and the weighted mixture (PT_FLAG_MIXTURE_WEIGHTED).  tests/test_scatter_laws_cpu.py runs the same laws on
the CPU oracle's paths (which validates the reference, the scenes, the caps and the bounds without a GPU), lists what each case measures,
checks that the cases reach the state bits dof, many, sweptCubes, mesh, grouped and plain, and records the mutations the laws were seen to
catch.  Nothing here reads the oracle: a mistake made alike in the oracle and in the kernels fails here.

Mutations of csrc this file was seen to catch (each built apart and run once; arithmetic only, none reads or writes out of bounds):
hemisphereDraws with up = u01 instead of its square root -- the eight law cases fail, L2 cos^2 KS 28.9 (few) to 41.8 (phong); Schlick's
cosx = -c from inside the glass too -- `glass` fails, L5 Fresnel z -8.1, and `mesh-direct2`, -3.3; the direct-lighting weight without
`cover` -- `many-direct` and `mesh-direct2` fail L6, a point aimed at a box in full view is not recovered; lr = lensRadius * u01 in both
lens samplers -- `many_mesh-lens` fails, L1 lens r^2 KS 29.8; the blend's u and v swapped in meshWinner and meshIntersectionTest --
`vn-smooth` and `vn-bent` fail L10, the guide normal 6027 and 5523 times its tolerance; the turn to the face's side dropped in both --
`vn-bent` fails L10, 19921 times; the weight 2 of PT_FLAG_MIXTURE_WEIGHTED inside the mirror branch only -- `few-weighted` and
`mesh-weighted` fail L3, a REFL hit with neither colour; k_gbuffer's meshIntersectionTest never taking the blend -- `vn-smooth` and
`vn-bent` fail L10, 3534 and 4179 times.  The oracle under the same mutations gives the same figures (tests/test_scatter_laws_cpu.py,
which lists more, and says which were not repeated here because they would change an index)."""
import ctypes as C

import pytest

import scatter_laws as sl

pytestmark = pytest.mark.gpu

_furnace = {}                       # name: (paths, frame, misses) of the unbatched run


@pytest.fixture(scope="module")
def gpu(pt):
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return pt


def _trace(gpu, sc, iterate, **init):
    """in the test library's own renderer: its state bits, the frame after `iterate(gpu)`, its misses, the paths after every bounce"""
    n = sc.image.shape[0] * sc.image.shape[1]
    gpu.pathtraceFree()
    with gpu.renderer_from_test_library():
        gpu.pathtraceInit(sc, **sc.extras, **sc.init, **init)
        bits = C.c_uint32(0xffffffff)
        assert gpu.test_lib().pt_test_renderer_state(C.byref(bits)) == 0, gpu.test_lib().pt_last_error()
        iterate(gpu)
        frame = gpu.readback(n).reshape(-1, 3)
        misses = int(gpu.counters().misses)
        paths, guides = None, None
        if not init:
            guides = {it: tuple(a.copy() for a in gpu.gbuffer(it)) for it in sc.guide_iters}          # (L10: pt_gbuffer, the denoiser's guides)
            paths = {it: [tuple(a.copy() for a in gpu.debug_trace_paths(it, k, n)) for k in range(sc.traceDepth + 1)] for it in sc.iters}
        gpu.pathtraceFree()
    assert bits.value == sl.state_bits(sc.state), ([k for i, k in enumerate(sl.STATE) if (bits.value >> i) & 1], sc.state)
    return paths, frame, misses, guides


@pytest.mark.parametrize("name", list(sl.CASES))
def test_every_bounce_keeps_the_scatter_laws(gpu, oracle, name):
    sc = sl.build(gpu, oracle, name)                      # (`oracle` builds the primitives' matrices; nothing of it renders here)
    paths, frame, _, guides = _trace(gpu, sc, lambda g: g.pathtrace(None, 0, sc.iters[0], readback=False))
    sl.run(sc, paths, frame, guides=guides)


def _furnace_run(gpu, oracle, name):
    if name not in _furnace:
        sc = sl.build(gpu, oracle, name)
        _furnace[name] = (sc,) + _trace(gpu, sc, lambda g: [g.pathtrace(None, 0, it, readback=False) for it in sc.iters])
    return _furnace[name]


@pytest.mark.parametrize("name", sl.FURNACES)
def test_the_furnace_is_exact(gpu, oracle, name):
    sc, paths, frame, misses, _ = _furnace_run(gpu, oracle, name)
    sl.furnace(sc, paths, frame, misses)


def test_the_batched_commit_keeps_the_furnace(gpu, oracle):
    """the same eight iterations as two batches of four (pathtrace_batch, max_batch 4): the same exact frame"""
    sc, paths, _, _, _ = _furnace_run(gpu, oracle, "furnace-half")
    assert len(sc.iters) == 8
    _, frame, misses, _ = _trace(gpu, sc, lambda g: [g.pathtrace_batch(None, 0, first, 4) for first in (1, 5)], max_batch=4)
    sl.furnace(sc, paths, frame, misses)
