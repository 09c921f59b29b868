"""The PLAIN family on the device against the CPU oracle, bit for bit: the seeded scenes of tests/plain_scenes.py, whose later bounces take
k_bounce<..., PLAIN> with history-coded pools at every width of the code (1 .. 9 bits) and at a full, a nearly full, an empty and a
one-code word.  tests/test_plain_fuzz_cpu.py is the ledger of what these inputs cover.

Per seed, under a schedule drawn like tests/test_gpu_fuzz.py's (1 .. 3 shards, batches of 1, 3 or 8, 1 .. 3 batches in flight, a third
traced ahead, 2 .. 8 iterations): the accumulator, the paths alive per bounce, and every queued path's origin, direction, throughput and
pixel behind bounce 1, behind a random bounce and behind bounce depth - 1 -- the deepest word the pool dump rebuilds a throughput from -- for
the first and the last iteration rendered.  A quarter of the unsharded seeds also sum the second moments: they equal the fp32 sum of the
squared luminances of the oracle's single iterations, and the accumulator keeps its bits.

Twins across the boundary: thirteen family scenes (one per table, at the full word) with ONE thing changed -- a depth one past the word, an
unused material that widens the code, a wall turned by 3 degrees (a plane wall), PT_AMD_NO_PLAIN=1 -- plan the general form (histBits 0) and
render the oracle's frame as well; under the switch the frame also has the bits of the unswitched run.

Evidence that the family reaches the PLAIN-only shortcuts: the test library's tallies, summed over all seeds -- waves took a certified wall
face and lanes fell back, candidate tiles exist, binned nearest hits occur, and the second certificate thins the candidates."""
import numpy as np
import pytest

import denoise_var_ref as dv
import plain_scenes as ps
from test_gpu_fuzz import _schedule
from test_kernel_select_cpu import STATE, names

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(pt):
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return pt


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _draw(rng, H):
    world, rank, batch, iters, pipeline, ahead = _schedule(rng)
    world = min(world, H)                                       # (the frame of one pixel has one row: one shard)
    return world, min(rank, world - 1), batch, iters, pipeline, ahead


def _oracle(oracle, sc, extras, sched, singles=False):
    """(accumulator, paths alive per bounce, the single iterations' radiance or None) of the oracle under the schedule's shard"""
    world, rank, batch, iters, pipeline, ahead = sched
    W, H = (int(v) for v in sc.camera["resolution"][0])
    ref = ps.oracle_renderer(oracle, sc, extras)
    want, live = np.zeros(W * H * 3, np.float32), np.zeros(64, np.int64)
    for k in iters:
        live += np.array(ref.iterate(k, want, rank, world).live[:64])
    ones = None
    if singles:
        ones = []
        for k in iters:
            one = np.zeros(W * H * 3, np.float32)
            ref.iterate(k, one, rank, world)
            ones.append(one.reshape(-1, 3))
    return ref, want, live, ones


def _render(gpu, sc, extras, sched, moments=False):
    """(accumulator, counters, second moments or None); the renderer stays initialised: the caller frees it"""
    world, rank, batch, iters, pipeline, ahead = sched
    W, H = (int(v) for v in sc.camera["resolution"][0])
    gpu.pathtraceFree()
    gpu.pathtraceInit(sc, traceDepth=sc.traceDepth, max_batch=batch, pipeline_depth=pipeline, shard_rank=rank, shard_count=world, trace_ahead=ahead,
                      moments=moments, **extras)
    it = iters[0]
    while it <= iters[-1]:
        n = 1 if ahead else min(batch, iters[-1] - it + 1)
        gpu.pathtrace_batch(None, 0, it, n)
        it += n
    return gpu.readback(W * H), gpu.counters(), (gpu.readback_moments() if moments else None)


def _check(gpu, oracle, sc, extras, rng, seed, moments=False, dump=True):
    W, H = (int(v) for v in sc.camera["resolution"][0])
    depth = sc.traceDepth
    sched = _draw(rng, H)
    world, rank, batch, iters, pipeline, ahead = sched
    moments = moments and world == 1
    ref, want, live, ones = _oracle(oracle, sc, extras, sched, singles=moments)
    hist = gpu.scene_plan(sc, **extras).histBits != 0
    try:
        got, cnt, q = _render(gpu, sc, extras, sched, moments)
        if not (ahead and batch > 1):                           # (the tallies also cover iterations traced ahead)
            assert [int(cnt.live[d]) for d in range(1, depth + 2)] == live[1:depth + 2].tolist(), seed
        assert cnt.iterations == len(iters), seed
        assert np.array_equal(bits(got), bits(want)), seed
        if moments:
            assert np.array_equal(bits(q), bits(dv.moments(ones))), seed
        if dump:
            # behind bounce 1, a random bounce and bounce depth - 1: a history-coded pool holds depth - 1 codes at the most (depth 1: the camera rays)
            last = depth - 1 if hist else depth
            bounces = sorted({1, int(rng.integers(1, last + 1)), last}) if last >= 1 else [0]
            for it in (iters[0], iters[-1]):
                for b in bounces:
                    o, d, c, pix = gpu.debug_trace_paths(it, b, W * H)
                    wo, wd, wc, wpix = ref.dump_paths(it, b, rank, world)
                    assert np.array_equal(pix, wpix), (seed, it, b)
                    for g, w, what in ((o, wo, "origin"), (d, wd, "direction"), (c, wc, "throughput")):
                        assert np.array_equal(bits(g), bits(w)), (seed, it, b, what)
    finally:
        gpu.pathtraceFree()
    return got


@pytest.mark.parametrize("seed", range(ps.N_SEEDS))
def test_family_scene(gpu, oracle, seed):
    sc, (W, H), extras, rng = ps.plain_scene(gpu, oracle, seed)
    plan = gpu.scene_plan(sc, **extras)
    assert names(plan.state_bits, STATE) == ("dof|plain" if extras else "plain") and plan.histBits == sc.bits, seed
    _check(gpu, oracle, sc, extras, rng, seed, moments=seed % 4 == 1)


# one twin per table, all at the full word (seeds 0 .. 12): (seed, what is changed)
TWINS = [(0, "material"), (1, "deeper"), (2, "wall"), (3, "switch"), (4, "deeper"), (5, "material"), (6, "wall"), (7, "switch"),
         (8, "deeper"), (9, "material"), (10, "wall"), (11, "switch"), (12, "deeper")]


@pytest.mark.parametrize("seed,change", TWINS, ids=["%d-%s" % t for t in TWINS])
def test_twin_across_the_boundary(gpu, oracle, monkeypatch, seed, change):
    sc, (W, H), extras, rng = ps.plain_scene(gpu, oracle, seed)
    assert sc.depth_kind == "full" and gpu.scene_plan(sc, **extras).histBits == sc.bits
    state = rng.bit_generator.state
    if change == "deeper":                                      # one code more than the word holds
        sc.traceDepth += 1
    elif change == "material":                                  # an unused material: 2 nmats codes need one bit more
        assert sc.nmats & (sc.nmats - 1) == 0
        extra = np.zeros(1, gpu.MATERIAL_DTYPE)
        extra["color"] = (0.5, 0.6, 0.7)
        sc.materials = np.concatenate([sc.materials, extra])
        assert ps.code_bits(len(sc.materials)) * (sc.traceDepth - 1) > 32
    elif change == "wall":                                      # the back wall turned by 3 degrees: a plane wall
        g = sc.geoms.view(oracle.GEOM_DTYPE)
        w = g[sc.walls[2]:sc.walls[2] + 1]
        turned = oracle.make_geom(1, int(w["materialid"][0]), tuple(w["translation"][0]), tuple(w["rotation"][0] + np.float32([0, 3, 0])), tuple(w["scale"][0]))
        g[sc.walls[2]] = turned[0]
    else:
        plain = _check(gpu, oracle, sc, extras, rng, seed, dump=False)
        rng.bit_generator.state = state                         # (the same schedule for both runs)
        monkeypatch.setenv("PT_AMD_NO_PLAIN", "1")
    plan = gpu.scene_plan(sc, **extras)
    assert plan.histBits == 0 and "plain" not in names(plan.state_bits, STATE), seed
    frame = _check(gpu, oracle, sc, extras, rng, seed)
    if change == "switch":
        assert np.array_equal(bits(frame), bits(plain)), seed


def test_the_family_reaches_the_plain_only_shortcuts(gpu, oracle):
    wall, cand = np.zeros(4, np.int64), np.zeros(8, np.int64)
    with gpu.renderer_from_test_library():
        for seed in range(ps.N_SEEDS):
            sc, (W, H), extras, rng = ps.plain_scene(gpu, oracle, seed)
            try:
                gpu.pathtraceInit(sc, traceDepth=sc.traceDepth, max_batch=2, pipeline_depth=1, **extras)
                gpu.wall_resolve_tally(), gpu.candidate_tally()
                gpu.pathtrace_batch(None, 0, 1, 2)
                gpu.sync()
                wall += np.array(gpu.wall_resolve_tally(), np.int64)
                cand += np.array(gpu.candidate_tally(), np.int64)
            finally:
                gpu.pathtraceFree()
    print("wall resolve tally over %d seeds (later wave-tiles, one-wall tiles with a face, waves that took it, lanes that fell back): %s" % (ps.N_SEEDS, wall.tolist()))
    print("candidate tally over %d seeds (later wave-tiles, candidate tiles, of one wall with a face, binned hits in them, scatters of binning scenes, "
          "candidates by the balls, by the rule in force, by the balls beside it): %s" % (ps.N_SEEDS, cand.tolist()))
    assert wall[2] > 0 and wall[3] > 0
    assert cand[1] > 0 and cand[3] > 0 and cand[6] < cand[5]
