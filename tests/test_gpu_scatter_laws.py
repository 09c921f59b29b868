"""Where a path goes next, on the MI355X, against float64 laws (tests/scatter_laws.py): the camera ray, the diffuse hemisphere, the REFL
mixture, the Phong lobe, the dielectric, the direct-lighting ray, the new origin, the light's contribution -- read from the state of the
test library's own renderer after EVERY bounce -- and an exact furnace.  Ten cases; tests/test_scatter_laws_cpu.py runs the same laws on
the CPU oracle's paths (which validates the reference, the scenes, the caps and the bounds without a GPU), lists what each case measures,
checks that the cases reach the state bits dof, many, sweptCubes, mesh, grouped and plain, and records the mutations the laws were seen to
catch.  Nothing here reads the oracle: a mistake made alike in the oracle and in the kernels fails here.

Mutations of csrc this file was seen to catch (each built apart and run once; arithmetic only, none reads or writes out of bounds):
hemisphereDraws with up = u01 instead of its square root -- the eight law cases fail, L2 cos^2 KS 28.9 (few) to 41.8 (phong); Schlick's
cosx = -c from inside the glass too -- `glass` fails, L5 Fresnel z -8.1, and `mesh-direct2`, -3.3; the direct-lighting weight without
`cover` -- `many-direct` and `mesh-direct2` fail L6, a point aimed at a box in full view is not recovered; lr = lensRadius * u01 in both
lens samplers -- `many_mesh-lens` fails, L1 lens r^2 KS 29.8.  The oracle under the same mutations gives the same figures
(tests/test_scatter_laws_cpu.py, which lists four more)."""
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
        gpu.pathtraceInit(sc, **sc.extras, **init)
        bits = C.c_uint32(0xffffffff)
        assert gpu.test_lib().pt_test_renderer_state(C.byref(bits)) == 0, gpu.test_lib().pt_last_error()
        iterate(gpu)
        frame = gpu.readback(n).reshape(-1, 3)
        misses = int(gpu.counters().misses)
        paths = None
        if not init:
            paths = {it: [tuple(a.copy() for a in gpu.debug_trace_paths(it, k, n)) for k in range(sc.traceDepth + 1)] for it in sc.iters}
        gpu.pathtraceFree()
    assert bits.value == sl.state_bits(sc.state), ([k for i, k in enumerate(sl.STATE) if (bits.value >> i) & 1], sc.state)
    return paths, frame, misses


@pytest.mark.parametrize("name", list(sl.CASES))
def test_every_bounce_keeps_the_scatter_laws(gpu, oracle, name):
    sc = sl.build(gpu, oracle, name)                      # (`oracle` builds the primitives' matrices; nothing of it renders here)
    paths, frame, _ = _trace(gpu, sc, lambda g: g.pathtrace(None, 0, sc.iters[0], readback=False))
    sl.run(sc, paths, frame)


def _furnace_run(gpu, oracle, name):
    if name not in _furnace:
        sc = sl.build(gpu, oracle, name)
        _furnace[name] = (sc,) + _trace(gpu, sc, lambda g: [g.pathtrace(None, 0, it, readback=False) for it in sc.iters])
    return _furnace[name]


@pytest.mark.parametrize("name", sl.FURNACES)
def test_the_furnace_is_exact(gpu, oracle, name):
    sc, paths, frame, misses = _furnace_run(gpu, oracle, name)
    sl.furnace(sc, paths, frame, misses)


def test_the_batched_commit_keeps_the_furnace(gpu, oracle):
    """the same eight iterations as two batches of four (pathtrace_batch, max_batch 4): the same exact frame"""
    sc, paths, _, _ = _furnace_run(gpu, oracle, "furnace-half")
    assert len(sc.iters) == 8
    _, frame, misses = _trace(gpu, sc, lambda g: [g.pathtrace_batch(None, 0, first, 4) for first in (1, 5)], max_batch=4)
    sl.furnace(sc, paths, frame, misses)
