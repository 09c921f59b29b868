"""The ledger of the PLAIN family (tests/plain_scenes.py), without a GPU: conditions on the INPUTS of tests/test_gpu_plain_fuzz.py, read off
the host-only plan (pt_test_scene_plan, pt_test_wall_faces) and the CPU oracle.  Where one fails the generator changes, never the condition.

  * every family scene plans `plain` (`dof|plain` with a lens) with histBits = history_code_bits(nmats): none is left out;
  * every width 1 .. 9 is planned by three scenes or more; the word is full (32 bits) twice at each of the widths 1, 2, 4 and 8; a top code
    with unused bits above it (27 .. 31 bits used) occurs twice or more; depth 1 and depth 2 at four widths or more;
  * the history matters: in the scenes of three materials or more and depth 3 or more at a full or nearly full word, the oracle's paths
    behind bounce depth - 1 carry more distinct throughputs than the table has materials -- in two such scenes per width, in three quarters
    of all of them.  (Width 2 is a table of TWO materials; there the same is asked of the two-material scenes, twice.)
  * the full word is used: in every scene of width 2 or more at its deepest trace -- a full 32-bit word at the widths 2, 4 and 8, a top code
    with unused bits above it at the others -- a path reaches the light at the last bounce;
  * binned primitives, a planned wall face, a lens: five scenes each or more; and the cases the generator is to build occur;
  * the older generators (tests/test_gpu_fuzz.py) plan exactly the states recorded here, none of them history-coded."""
import collections
import os

import numpy as np
import pytest

import plain_scenes as ps
import test_gpu_fuzz as fuzz
from conftest import SCENES
from test_kernel_select_cpu import STATE, names


@pytest.fixture(scope="module")
def family(pt, oracle):
    """[(seed, scene, (W, H), extras, plan)] of every seed"""
    out = []
    for seed in range(ps.N_SEEDS):
        sc, res, extras, _ = ps.plain_scene(pt, oracle, seed)
        out.append((seed, sc, res, extras, pt.scene_plan(sc, **extras)))
    return out


def _used(sc):
    return sc.bits * (sc.traceDepth - 1)


def test_the_generators_width_is_the_plans(pt):
    assert [ps.code_bits(n) for n in ps.NMATS] == [1, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 8, 9]
    assert ps.N_SEEDS >= 60


def test_every_family_scene_plans_plain_at_its_width(family):
    for seed, sc, res, extras, plan in family:
        assert len(sc.materials) == sc.nmats == ps.NMATS[seed % len(ps.NMATS)], seed       # (no table had to be cut down for LDS)
        assert names(plan.state_bits, STATE) == ("dof|plain" if extras else "plain"), seed
        assert plan.histBits == sc.bits, seed
        m = sc.materials
        assert not m["hasRefractive"].any() and not m["specularExponent"].any() and m["emittance"][0] > 0, seed
        assert set(extras) <= {"lens_radius", "focal_distance"}, seed
        assert res == (1, 1) or (res[0] in ps.WIDTHS and res[1] in ps.HEIGHTS), seed
    assert [res for seed, sc, res, extras, plan in family].count((1, 1)) == 1


def test_every_width_is_covered(family):
    by_width = collections.Counter(plan.histBits for seed, sc, res, extras, plan in family)
    print("scenes per width:", dict(sorted(by_width.items())))
    assert all(by_width[b] >= 3 for b in range(1, 10))
    full = collections.Counter(sc.bits for seed, sc, res, extras, plan in family if _used(sc) == 32)
    print("full words per width:", dict(sorted(full.items())))
    assert all(full[b] >= 2 for b in (1, 2, 4, 8))
    top = [seed for seed, sc, res, extras, plan in family if 27 <= _used(sc) <= 31]
    print("a top code with unused bits above it:", top)
    assert len(top) >= 2
    for depth in (1, 2):
        assert len({sc.bits for seed, sc, res, extras, plan in family if sc.traceDepth == depth}) >= 4, depth


def test_the_history_matters(family, oracle):
    held, asked = collections.Counter(), collections.Counter()
    for seed, sc, res, extras, plan in family:
        # (a table of two materials IS width 2: the two-material scenes stand for it)
        if sc.nmats < (2 if sc.bits == 2 else 3) or sc.traceDepth < 3 or sc.depth_kind not in ("full", "full-1"):
            continue
        o, d, c, pix = ps.oracle_renderer(oracle, sc, extras).dump_paths(1, sc.traceDepth - 1)
        distinct = len(np.unique(c.view(np.uint32).reshape(-1, 3), axis=0)) if len(pix) else 0
        asked[sc.bits] += 1
        held[sc.bits] += len(pix) > 0 and distinct > sc.nmats
    print("the history matters in", dict(sorted(held.items())), "of", dict(sorted(asked.items())))
    assert all(held[b] >= 2 for b in range(2, 10))
    assert 4 * sum(v for b, v in held.items() if b != 2) >= 3 * sum(v for b, v in asked.items() if b != 2)


def test_the_full_word_is_used(family, oracle):
    n = collections.Counter()
    for seed, sc, (W, H), extras, plan in family:
        if sc.depth_kind != "full" or sc.bits < 2:
            continue
        last, before = np.zeros(W * H * 3, np.float32), np.zeros(W * H * 3, np.float32)
        ps.oracle_renderer(oracle, sc, extras).iterate(1, last)
        ps.oracle_renderer(oracle, sc, extras, sc.traceDepth - 1).iterate(1, before)
        # one iteration is one path per pixel, and a path contributes once: these are the paths that reach the light behind a full word
        differ = np.flatnonzero((last.view(np.uint32) != before.view(np.uint32)).reshape(-1, 3).any(axis=1))
        assert len(differ) > 0 and not before.reshape(-1, 3)[differ].any(), seed
        n[_used(sc) == 32] += 1
    print("scenes whose deepest word is used: %d full, %d with unused bits above the top code" % (n[True], n[False]))
    assert n[True] >= 6 and n[False] >= 6


def test_each_primitive_case_is_reached(pt, family):
    n = collections.Counter()
    for seed, sc, res, extras, plan in family:
        face, _ = pt.wall_faces(sc, **extras)
        n["binned"] += plan.nBinned > 0
        n["wall face"] += bool((face >= 0).any())
        n["lens"] += bool(extras)
        for case in sc.cases:
            n[str(case)] += 1
        g = sc.geoms
        n["emissive object"] += bool((g["materialid"][len(sc.walls) + 1:] == 0).any()) and sc.nmats > 1
        n["black"] += sc.black is not None and bool((g["materialid"] == sc.black).any())
        n["no object"] += len(g) == len(sc.walls) + 1
        n["closed"] += len(sc.walls) == 6
    print("cases:", dict(sorted(n.items())))
    for case in ("binned", "wall face", "lens", "small", "poke", "duplicate", "floor", "free", "open", "closed", "turned wall", "emissive object",
                 "black", "no object"):
        assert n[case] >= 5, case


# what the 56 scenes of tests/test_gpu_fuzz.py plan: none of them PLAIN
OLD_STATES = {"many": 16, "many|mesh": 12, "mesh": 9, "0": 7, "many|sweptCubes|mesh": 5, "dof": 3, "dof|many|mesh": 2, "dof|mesh": 2}


def test_the_older_generators_plan_no_plain_scene(pt, oracle):
    small = pt.Scene(os.path.join(SCENES, "mesh_small.txt"))
    tris = {"icosphere": small.meshes[3], "torus": small.meshes[4]}
    scenes = [fuzz._random_scene(pt, oracle, 5650 + seed, tris) for seed in range(40)] + [fuzz._sphere_field(pt, oracle, 8800 + seed) for seed in range(16)]
    states = collections.Counter()
    for sc, res, extras, _ in scenes:
        flags = pt.PT_FLAG_DIRECT_LIGHTING if extras.get("direct_lighting") else 0
        plan = pt.scene_plan(sc, flags=flags, **{k: v for k, v in extras.items() if k != "direct_lighting"})
        assert plan.histBits == 0
        states[names(plan.state_bits, STATE)] += 1
    assert dict(states) == OLD_STATES
