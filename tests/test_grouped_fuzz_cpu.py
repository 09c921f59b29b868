"""The ledger of the GROUPED family (tests/grouped_scenes.py), without a GPU: conditions on the INPUTS of tests/test_gpu_grouped_fuzz.py, read off
the host-only plan (pt_test_scene_plan), the host-only view of the swept primitives' table (pt_test_sphere_groups) and the CPU oracle.  Where
one fails the generator changes, never the condition.

  * every family scene plans the state its kind names, with no environment variable: `grouped` (with `sweptCubes` and `dof` where the scene has
    swept cubes and a lens), the threshold twins `many` without `grouped`, the swept kinds many|sweptCubes, dof|many, dof|many|sweptCubes;
  * counts: 48 seeds or more, every kind four times (global six), a lens on five grouped scenes, direct lighting on five, an emissive swept
    sphere in five;
  * the table's edges: a padded table of exactly 1280 entries staged in LDS and one of 1288 read from global memory; cluster 0 padded to an even
    number of groups (its last group twice) in three scenes; a last group padded with copies in five; no clusters in three; more than 128
    groups in four; a grpN0 that is no multiple of 32 in four;
  * the table is sound as data: every swept primitive appears, padding repeats a group's last entry, cluster 0 comes first and lies on one
    side of a plane, and in float64 every member's certificate ball lies inside its group's ball for origins within grpOMax (the comment
    above build_sphere_groups, csrc/pt_host_scene.h);
  * the full column is reached: in the onion scenes of gs.FULL_COLUMN some path of the oracle, behind a bounce that is not the last, passes
    24 groups or more within half their balls' radii -- candidates whatever fp32 rounds to, twice the twelve words a lane can park;
  * a lens on a large table: which of the lens scenes of 1400 .. 2200 swept primitives plan_lds refuses (PT_ERR_INVALID, its message) is
    recorded in LENS_REFUSED;
  * direct lighting: a scene with more emissive primitives than the direct-lighting bounce samples (eight) is refused under the flag, and
    the family holds scenes with exactly eight and with fewer;
  * the states the family plans are recorded in NEW_STATES, as tests/test_plain_fuzz_cpu.py::OLD_STATES records the older generators'."""
import collections
import types

import numpy as np
import pytest

import grouped_scenes as gs
from test_kernel_select_cpu import STATE, names

GROUPED_KINDS = ("threshold", "rounds", "lds-edge", "global", "onion", "cubes", "open")


@pytest.fixture(scope="module")
def family(pt, oracle):
    """[(seed, scene, (W, H), extras, plan, table)] of every seed"""
    out = []
    for seed in range(gs.N_SEEDS):
        sc, res, extras, _ = gs.grouped_scene(pt, oracle, seed)
        o = gs.plan_options(pt, extras)
        out.append((seed, sc, res, extras, pt.scene_plan(sc, **o), pt.sphere_groups(sc, **o)))
    return out


def _state(sc, extras, g, grouped):
    cubes = bool((sc.geoms["type"][g.table] == 1).any())
    return "|".join((["dof"] if "lens_radius" in extras else []) + ["many"] + (["sweptCubes"] if cubes else []) + (["grouped"] if grouped else []))


def test_every_family_scene_plans_the_state_its_kind_names(pt, family, monkeypatch):
    monkeypatch.delenv("PT_AMD_GROUPS", raising=False)
    for seed, sc, res, extras, plan, g in family:
        assert sc.kind == gs.KINDS[seed % len(gs.KINDS)] and not sc.meshes, seed
        assert res[0] in gs.WIDTHS and res[1] in gs.HEIGHTS and 2 <= sc.traceDepth <= 6, seed
        assert set(extras) <= {"lens_radius", "focal_distance", "direct_lighting"}, seed
        m = sc.materials
        assert m["emittance"][0] > 0 and m["hasRefractive"].any() and m["hasReflective"].any(), seed
        state = names(plan.state_bits, STATE)
        assert g.grouped == (sc.kind in GROUPED_KINDS) and g.nswept == sc.nswept and plan.nSphCull == len(g.table), seed
        assert state == _state(sc, extras, g, sc.kind in GROUPED_KINDS), (seed, state)
        assert (plan.nSphGroups > 0) == g.grouped and plan.nSphGroups == g.nSphGroups and plan.histBits == 0, seed
        column = seed % len(gs.KINDS)
        if sc.kind == "threshold":
            assert sc.nswept == 128, seed
            twin = gs.threshold_twin(pt, sc)
            o = gs.plan_options(pt, extras)
            tp, tg = pt.scene_plan(twin, **o), pt.sphere_groups(twin, **o)
            assert tg.nswept == 127 and not tg.grouped and tp.nSphCull == 128 and tp.nSphGroups == 0, seed
            assert names(tp.state_bits, STATE) == state.replace("|grouped", ""), seed
        elif sc.kind == "rounds":
            assert 520 <= sc.nswept <= 1100 and g.nSphGroups > 128 and g.n0 > 0 and plan.grpLds == 1, seed
        elif sc.kind == "lds-edge":
            assert len(g.table) in (1280, 1288) and plan.grpLds == (1 if len(g.table) == 1280 else 0) and "sweptCubes" not in state, seed
        elif sc.kind == "global":
            assert 1400 <= sc.nswept <= 2200 and plan.grpLds == 0 and ("sweptCubes" in state) == bool(seed % 2), seed
        elif sc.kind == "onion":
            assert 200 <= sc.nswept <= 400 and "sweptCubes" not in state and m["hasRefractive"][sc.geoms["materialid"]].sum() > 50, seed
        elif sc.kind == "cubes":
            assert 130 <= sc.nswept <= 300 and "sweptCubes" in state and 2 * (sc.geoms["type"][np.unique(g.table)] == 1).sum() > sc.nswept, seed
        elif sc.kind == "open":
            assert sc.walls == "absent" and (g.n0 == 0) == ("never culled" in sc.cases), seed
        else:
            assert 5 <= sc.nswept <= 127 and state == {10: "many|sweptCubes", 11: "dof|many", 12: "dof|many|sweptCubes"}[column], (seed, state)
        if sc.kind in GROUPED_KINDS and sc.kind != "global" and sc.kind != "lds-edge":
            assert plan.grpLds == 1, seed


def test_counts(family):
    assert gs.N_SEEDS >= 48
    kinds = collections.Counter(sc.kind for seed, sc, res, extras, plan, g in family)
    n = collections.Counter()
    for seed, sc, res, extras, plan, g in family:
        n["lens on a grouped scene"] += g.grouped and "lens_radius" in extras
        n["direct lighting"] += bool(extras.get("direct_lighting"))
        n["emissive swept sphere"] += bool(((sc.geoms["materialid"][g.table] == 0) & (sc.geoms["type"][g.table] == 0)).any())
        n["walls " + sc.walls] += 1
        n["emitter " + sc.emitter] += 1
        for case in sc.cases:
            n[str(case)] += not str(case).startswith("walls")
    print("kinds:", dict(sorted(kinds.items())))
    print("cases:", dict(sorted(n.items())))
    assert all(kinds[k] >= 4 for k in set(gs.KINDS)) and kinds["global"] >= 6
    assert n["lens on a grouped scene"] >= 5 and n["direct lighting"] >= 5 and n["emissive swept sphere"] >= 5
    assert n["direct lighting, eight emitters"] >= 2 and n["direct lighting, fewer emitters"] >= 2
    assert all(n[c] >= 3 for c in ("walls present", "walls partly", "walls absent", "emitter light", "emitter sphere", "emitter both", "duplicate", "plate"))


def _groups(g):
    return g.table.reshape(-1, 8)


def _last_group_twice(g):
    t = _groups(g)
    return g.grpN0 >= 2 and np.array_equal(t[g.grpN0 - 1], t[g.grpN0 - 2])


def test_the_tables_edges(family):
    n = collections.Counter()
    for seed, sc, res, extras, plan, g in family:
        if not g.grouped:
            continue
        t = _groups(g)
        n["1280 entries in LDS"] += len(g.table) == 1280 and plan.grpLds == 1
        n["1288 entries in global memory"] += len(g.table) == 1288 and plan.grpLds == 0
        n["cluster 0 padded to an even group count"] += _last_group_twice(g)
        ends = [len(t) - 1] + ([g.grpN0 - 1] if g.n0 else [])
        n["a last group padded with copies"] += any(t[e][-1] == t[e][-2] for e in ends)
        n["no clusters"] += g.n0 == 0
        n["more than 128 groups"] += g.nSphGroups > 128
        n["grpN0 no multiple of 32"] += g.n0 > 0 and g.grpN0 % 32 != 0
    print("table edges:", dict(sorted(n.items())))
    assert n["1280 entries in LDS"] >= 1 and n["1288 entries in global memory"] >= 1
    assert n["cluster 0 padded to an even group count"] >= 3 and n["a last group padded with copies"] >= 5 and n["no clusters"] >= 3
    assert n["more than 128 groups"] >= 4 and n["grpN0 no multiple of 32"] >= 4


def test_the_table_is_sound_as_data(family):
    for seed, sc, res, extras, plan, g in family:
        if not g.grouped:
            continue
        t, types = _groups(g), sc.geoms["type"]
        assert len(g.table) % 8 == 0 and g.nSphGroups == len(t) and g.n0 % 8 == 0 and g.grpN0 == g.n0 // 8 and g.grpN0 % 2 == 0, seed
        # every swept primitive appears: every sphere, and nswept primitives in all, spheres and cubes
        assert set(np.flatnonzero(types == 0)) <= set(g.table) and len(set(g.table)) == g.nswept and set(types[g.table]) <= {0, 1}, seed
        # padding repeats a group's last entry: without cluster 0's second last group, and with every cluster's trailing run cut to one entry,
        # a cluster holds a primitive twice only where its odd count was made even before the grouping -- once at the most
        halves = [g.table[:g.n0 - (8 if _last_group_twice(g) else 0)], g.table[g.n0:]] if g.n0 else [g.table]
        seen = set()
        for h in halves:
            assert len(h) > 0, seed
            k = len(h)
            while k > 1 and h[k - 2] == h[-1]:
                k -= 1
            assert len(h) - k < 8 and len(h[:k]) - len(set(h[:k])) <= 1, (seed, len(h), k)
            assert not (seen & set(h)), seed                       # (a primitive belongs to one cluster)
            seen |= set(h)
        assert len(seen) == g.nswept, seed
        # cluster 0 comes first: its centres lie on one side of a plane across an axis, cluster 1's on the other
        if g.n0:
            a, b = g.centre[:g.n0].astype(np.float64), g.centre[g.n0:].astype(np.float64)
            assert any(a[:, x].max() <= b[:, x].min() or b[:, x].max() <= a[:, x].min() for x in range(3)), seed
        # every member's certificate ball inside its group's, in float64: r_i = sqrt(T_i + K_i (grpOMax + |c_i|)^2) around c_i, the group's
        # R = sqrt(T) / sphDirScale around C
        c, T, K = g.centre.astype(np.float64), g.threshold.astype(np.float64), g.K.astype(np.float64)
        C, R = g.balls[:, :3].astype(np.float64), np.sqrt(g.balls[:, 3].astype(np.float64)) / g.sphDirScale
        assert g.grpOMax > 0 and g.sphDirScale >= 1 and (K[np.isfinite(T)] >= 1e-4).all(), seed
        r = np.sqrt(T + K * (g.grpOMax + np.linalg.norm(c, axis=1)) ** 2)
        reach = np.linalg.norm(c - np.repeat(C, 8, axis=0), axis=1) + r
        with np.errstate(invalid="ignore"):
            inside = (reach <= np.repeat(R, 8)) | (np.isinf(r) & np.isinf(np.repeat(R, 8)))
        assert inside.all(), (seed, int((~inside).sum()))
        assert ("never culled" in sc.cases) == bool(np.isinf(T).any()), seed


def candidate_groups(g, o, d):
    """per ray: the groups whose centre lies within half their ball's radius of the half-line (float64); cluster 0's second last group counts once"""
    keep = np.ones(g.nSphGroups, bool)
    if _last_group_twice(g):
        keep[g.grpN0 - 1] = False
    C, R = g.balls[keep, :3].astype(np.float64), np.sqrt(g.balls[keep, 3].astype(np.float64)) / g.sphDirScale
    o, d = o.astype(np.float64), d.astype(np.float64)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    oc = C[None, :, :] - o[:, None, :]
    t = np.maximum(np.einsum("rgk,rk->rg", oc, d), 0.0)
    dist = np.linalg.norm(oc - t[:, :, None] * d[:, None, :], axis=2)
    return (dist <= 0.5 * R[None, :]).sum(axis=1)


def test_the_full_column_is_reached(family, oracle):
    most = {}
    for seed, sc, res, extras, plan, g in family:
        if sc.kind != "onion":
            continue
        ref = oracle.Renderer(sc.camera.view(oracle.CAMERA_DTYPE), sc.geoms.view(oracle.GEOM_DTYPE), sc.materials.view(oracle.MATERIAL_DTYPE), sc.traceDepth)
        ref.set_extras(**extras)
        best = 0
        for b in range(1, sc.traceDepth):
            o, d, c, pix = ref.dump_paths(1, b)
            if len(pix):
                best = max(best, int(candidate_groups(g, o, d).max()))
        most[seed] = (best, g.nSphGroups)
    print("onion scenes, the most candidate groups of a path (of the scene's groups):", most)
    assert len(gs.FULL_COLUMN) == 3 and all(most[s][0] >= 24 for s in gs.FULL_COLUMN)


# which lens scenes of 1400 .. 2200 swept primitives the plan refuses for LDS: (count, cubes) -> the bytes plan_lds names.  The camera-ray launch of
# a grouped scene under a lens stages the flat form's tables: 216 B of face frames per cube beside every primitive's hit record
# Recorded: spheres alone are never refused up to 2200; with a quarter of cubes the refusals start between 1200 and 1400 swept primitives.
LENS_COUNTS = [(1400, False), (1800, False), (2200, False), (1200, True), (1400, True), (1800, True), (2200, True)]
LENS_REFUSED = {(1400, True): 177728, (1800, True): 236624, (2200, True): 281680}


def lens_refusals(pt, oracle):
    """{(count, cubes): bytes} of the refused scenes, {(count, cubes): state} of the planned ones"""
    refused, planned = {}, {}
    for count, cubes in LENS_COUNTS:
        sc, res, extras = gs.lens_global_scene(pt, oracle, count, cubes)
        assert sc.nswept == count
        try:
            planned[(count, cubes)] = names(pt.scene_plan(sc, **extras).state_bits, STATE)
        except pt.PtError as e:
            head, tail = "pt_amd error -1: pt_init: scene does not fit the 160 KiB LDS (", " B)"
            assert str(e).startswith(head) and str(e).endswith(tail), str(e)          # PT_ERR_INVALID, plan_lds' message
            refused[(count, cubes)] = int(str(e)[len(head):-len(tail)])
            assert refused[(count, cubes)] > 160 * 1024
    return refused, planned


def test_a_lens_on_a_large_table(pt, oracle):
    refused, planned = lens_refusals(pt, oracle)
    print("lens scenes refused for LDS:", refused, "planned:", planned)
    assert refused == LENS_REFUSED
    assert all(state == ("dof|many|sweptCubes|grouped" if cubes else "dof|many|grouped") for (count, cubes), state in planned.items())


def test_direct_lighting_refuses_more_emitters_than_it_samples(pt, oracle):
    """Found by this family (onion scenes whose shells glow, under direct lighting): the direct-lighting bounce chooses among the first kEmitMax = 8
    emissive primitives, the oracle among all of them, and with a ninth the frames differed.  pt_init now refuses such a scene under the flag."""
    sc, res, extras, _ = gs.grouped_scene(pt, oracle, 0)
    assert sc.kind == "threshold" and "direct_lighting" not in extras
    lit = types.SimpleNamespace(**vars(sc))
    lit.geoms = sc.geoms.copy()
    spheres = np.flatnonzero(lit.geoms["type"] == 0)
    lit.geoms["materialid"][lit.geoms["materialid"] == 0] = 1
    lit.geoms["materialid"][spheres[:gs.EMIT_MAX]] = 0
    assert names(pt.scene_plan(lit, flags=pt.PT_FLAG_DIRECT_LIGHTING).state_bits, STATE) == "many|grouped"
    lit.geoms["materialid"][spheres[gs.EMIT_MAX]] = 0
    assert names(pt.scene_plan(lit).state_bits, STATE) == "many|grouped"                  # (without the flag nothing samples the emitters)
    with pytest.raises(pt.PtError) as e:
        pt.scene_plan(lit, flags=pt.PT_FLAG_DIRECT_LIGHTING)
    assert str(e.value) == "pt_amd error -1: pt_init: PT_FLAG_DIRECT_LIGHTING samples at most 8 emissive primitives, the scene has 9"


# what the family plans (tests/test_plain_fuzz_cpu.py::OLD_STATES: what the 56 older scenes plan -- no `grouped`, no many|sweptCubes or dof|many without a mesh)
NEW_STATES = {"many|grouped": 18, "dof|many|grouped": 5, "many|sweptCubes|grouped": 11, "dof|many|sweptCubes|grouped": 6, "many|sweptCubes": 4, "dof|many": 4,
              "dof|many|sweptCubes": 6, "many": 2}


def test_the_states_the_family_plans(pt, family):
    states = collections.Counter(names(plan.state_bits, STATE) for seed, sc, res, extras, plan, g in family)
    for seed, sc, res, extras, plan, g in family:
        if sc.kind == "threshold":
            states[names(pt.scene_plan(gs.threshold_twin(pt, sc), **gs.plan_options(pt, extras)).state_bits, STATE)] += 1
    print("states:", dict(states))
    assert dict(states) == NEW_STATES
    from test_plain_fuzz_cpu import OLD_STATES
    holes = {"many|sweptCubes", "dof|many", "dof|many|sweptCubes", "many|grouped", "many|sweptCubes|grouped", "dof|many|grouped", "dof|many|sweptCubes|grouped"}
    assert holes <= set(NEW_STATES) and not (holes & set(OLD_STATES)) and all("mesh" not in s for s in NEW_STATES)
