"""The GROUPED family on the device against the CPU oracle, bit for bit: the seeded scenes of tests/grouped_scenes.py, whose later bounces take the
two-level sweep k_bounce<..., GROUPS> by themselves (128 to 2200 swept primitives; PT_AMD_GROUPS is never set), and beside them the flat sweeps
without a mesh that the older generators never plan.  tests/test_grouped_fuzz_cpu.py is the ledger of what these inputs cover.

Per seed, through tests/test_gpu_fuzz.py's own `_check` under its `_schedule` (1 .. 3 shards, batches of 1, 3 or 8, 1 .. 3 batches in flight, a third
traced ahead): the accumulator, the paths alive per bounce, and every queued path's origin, direction, throughput and pixel behind a random
bounce.  The threshold scenes' twins of 127 swept primitives -- the flat sweep -- are held to the oracle in the same way.

Tallies (pt_test_group_tally: the test library's renderer counts, the product's kernels count nothing): every scene once more in the test
library -- the global scenes and the two tables of 1288 entries run level 2 from global memory and never from LDS, every other grouped scene
the reverse; every rounds scene runs more rounds than twice its waves (some wave ran three: a table of more than 128 groups); each of the
three onion scenes the ledger names calls passes() from inside the group loop with twelve words parked; no lane ever parks more than twelve;
the twins and the swept kinds tally nothing.

Certificates: pt_test_sphere_group_sweep with 2^20 rays on every global, onion and cubes scene, 0 violations.  Refusals: the lens scenes the
ledger records as refused for LDS are refused by pt_init on the device, which then holds no device buffer.

Mutations of csrc/pt_trace.h, each built apart:
  * GEOM of the global path returning entry e's index from ent[2 * e + 1].x (cullK) modulo 128: the first five scenes that read level 2
    from global memory (seeds 3, 4, 15, 16, 17) differed from the oracle.  The mutant is NOT in bounds, as the run showed: a wrong index
    hands cubes to the sphere test, whose float normal the shading then reads as a face index.  Described here, never to be run again.
  * `rd` kept across two rounds of passes(); gG0 rounded up to a multiple of 32 (a cluster's first groups skipped); gG0 rounded down to a
    multiple of 32 (expected to pass: it only sweeps groups of cluster 0 again, a conservative change): built, and not run for want of a
    GPU slot when this was written."""
import numpy as np
import pytest

import grouped_scenes as gs
import test_gpu_fuzz as fuzz
from test_grouped_fuzz_cpu import GROUPED_KINDS, LENS_REFUSED, _state
from test_kernel_select_cpu import STATE, names

pytestmark = pytest.mark.gpu

SEEDS = range(gs.N_SEEDS)
OF_KIND = {k: [s for s in SEEDS if gs.KINDS[s % len(gs.KINDS)] == k] for k in set(gs.KINDS)}


@pytest.fixture(scope="module")
def gpu(pt):
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return pt


_SCENES = {}


def _scene(gpu, oracle, seed):
    """grouped_scene(seed), generated once for the tests of this module: the scene, its frame, its extras and a generator in the state the scene's left it"""
    if seed not in _SCENES:
        sc, res, extras, rng = gs.grouped_scene(gpu, oracle, seed)
        _SCENES[seed] = (sc, res, extras, rng.bit_generator.state)
    sc, res, extras, state = _SCENES[seed]
    rng = np.random.default_rng(0)
    rng.bit_generator.state = state
    return sc, res, extras, rng


@pytest.mark.parametrize("seed", SEEDS)
def test_family_scene(gpu, oracle, seed):
    sc, (W, H), extras, rng = _scene(gpu, oracle, seed)
    o = gs.plan_options(gpu, extras)
    assert names(gpu.scene_plan(sc, **o).state_bits, STATE) == _state(sc, extras, gpu.sphere_groups(sc, **o), sc.kind in GROUPED_KINDS), seed
    fuzz._check(gpu, oracle, sc, W, H, extras, rng, seed)


@pytest.mark.parametrize("seed", OF_KIND["threshold"])
def test_threshold_twin_takes_the_flat_sweep(gpu, oracle, seed):
    sc, (W, H), extras, rng = _scene(gpu, oracle, seed)
    twin = gs.threshold_twin(gpu, sc)
    assert "grouped" not in names(gpu.scene_plan(twin, **gs.plan_options(gpu, extras)).state_bits, STATE) and twin.nswept == 127, seed
    fuzz._check(gpu, oracle, twin, W, H, extras, rng, seed)


def _tally(gpu, sc, extras):
    """pt_test_group_tally over one batch of two iterations in the test library's renderer"""
    with gpu.renderer_from_test_library():
        try:
            gpu.pathtraceInit(sc, traceDepth=sc.traceDepth, max_batch=2, pipeline_depth=1, **extras)
            gpu.group_tally()
            gpu.pathtrace_batch(None, 0, 1, 2)
            gpu.sync()
            return [int(v) for v in gpu.group_tally()]
        finally:
            gpu.pathtraceFree()


@pytest.mark.parametrize("seed", SEEDS)
def test_group_tally(gpu, oracle, seed):
    sc, (W, H), extras, rng = _scene(gpu, oracle, seed)
    g = gpu.sphere_groups(sc, **gs.plan_options(gpu, extras))
    rounds, lds, glob, full, parked, most = t = _tally(gpu, sc, extras)
    print("seed %d %s (%d swept, %d groups): rounds %d, waves from LDS %d, from global memory %d, full columns %d, words parked %d, most %d"
          % (seed, sc.kind, sc.nswept, g.nSphGroups, rounds, lds, glob, full, parked, most))
    if sc.kind not in GROUPED_KINDS:
        assert t == [0] * 6, seed
        return
    assert rounds > 0 and parked > 0 and 1 <= most <= 12 and rounds >= lds + glob, (seed, t)
    if len(g.table) > 1280:                                     # every global scene, and the lds-edge scenes of 1288 entries
        assert glob > 0 and lds == 0, (seed, t)
    else:
        assert lds > 0 and glob == 0, (seed, t)
    assert (sc.kind == "global") <= (glob > 0), seed
    if sc.kind == "rounds":                                     # (a wave of one cluster runs two rounds, of both three: more than two in some wave)
        assert rounds > 2 * (lds + glob), (seed, t)
    if seed in gs.FULL_COLUMN:
        assert full > 0 and most == 12, (seed, t)
    assert (full > 0) <= (most == 12), (seed, t)
    if sc.kind == "threshold":
        assert _tally(gpu, gs.threshold_twin(gpu, sc), extras) == [0] * 6, seed


@pytest.mark.parametrize("seed", sorted(OF_KIND["global"] + OF_KIND["onion"] + OF_KIND["cubes"]))
def test_group_certificates(gpu, oracle, seed):
    sc, (W, H), extras, rng = _scene(gpu, oracle, seed)
    certified, violations, ngroups = gpu.test_sphere_group_sweep(sc.geoms, 4100 + seed, 1 << 20)
    print("seed %d %s: %d groups of spheres, %d certificates, %d violations" % (seed, sc.kind, ngroups, certified, violations))
    assert violations == 0 and certified > 0 and ngroups > 0, seed


@pytest.mark.parametrize("count,cubes", sorted(LENS_REFUSED))
def test_refused_lens_scene_leaves_nothing_on_the_device(gpu, oracle, count, cubes):
    sc, (W, H), extras = gs.lens_global_scene(gpu, oracle, count, cubes)
    live = gpu.test_lib().pt_test_live_device_buffers
    with gpu.renderer_from_test_library():
        gpu.pathtraceFree()
        with pytest.raises(gpu.PtError, match=r"pt_amd error -1: pt_init: scene does not fit the 160 KiB LDS \(%d B\)" % LENS_REFUSED[(count, cubes)]):
            gpu.pathtraceInit(sc, traceDepth=sc.traceDepth, **extras)
        assert live() == 0
