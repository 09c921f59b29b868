"""The two device walks -- ptd::meshIntersectionTest (pt_test_mesh_intersect2, k_gbuffer) and k_mesh_walk (the renders) -- held to the
brute-force rule "nearest object-space t, ties to the lower file index" on the adversarial meshes of tests/adversarial_meshes.py: exact ties,
stacks filled to the hierarchy's need, the median rebuild, walks of very unequal length, queues that overflow, degenerate triangles, boxes
that are mostly margin.  What the known answers and tolerances rest on is checked without a GPU in tests/test_adversarial_meshes_cpu.py."""
import numpy as np
import pytest

import adversarial_meshes as am
import denoise_ref as dr
from conftest import SCENES
from test_gpu_mesh import _render_both

pytestmark = pytest.mark.gpu
f32 = np.float32
FAMILIES = {f.name: f for f in am.families()}
IDENT = ((0, 0, 0), (0, 0, 0), (1, 1, 1))
W, H, DEPTH = 64, 48, 4


@pytest.fixture(scope="module")
def gpu(pt):
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return pt


def _bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


_cache = {}


def _reference(oracle, name):
    """the family's rays (at most 1024, the comb's stack-filling ones among them) under its transform, the oracle's answer per ray and the
    float64 cast: computed once, shared by the walk through the hierarchy and the one through the flat list"""
    if name not in _cache:
        fam = FAMILIES[name]
        geom = oracle.make_geom(2, am.MAT_B, *fam.transform)
        rays = am.to_world(geom, *am.per_ray_set(fam))
        assert len(rays) <= 1024
        want = [oracle.mesh_intersect(geom, fam.tris, r) for r in rays]
        cast = None if name.startswith("lattice") else am.mesh_cast(geom, fam.tris, rays, am.TOL[name.split("-")[0]][0])
        _cache[name] = (geom, rays, want, cast)
    return _cache[name]


def _against_the_oracle(fam, rays, want, got):
    t, p, n, o, culled, tri, fm = got
    assert not np.isnan(t[culled != 0]).any(), "the bounding-ball test rejected a ray the full test hits"
    hits = 0
    for i, (wt, wp, wn, wo, wtri) in enumerate(want):
        assert tri[i] == wtri, (fam.name, i, rays[i], tri[i], wtri)
        assert _bits(t[i]) == _bits(wt), (fam.name, i, rays[i], t[i], wt)
        assert np.array_equal(_bits(p[i]), _bits(wp)) and o[i] == wo, (fam.name, i, p[i], wp)
        assert fm[i] == (fam.mats[wtri] if wtri >= 0 else -1), (fam.name, i, fm[i], wtri)
        if wtri >= 0:
            assert np.array_equal(_bits(n[i]), _bits(wn)), (fam.name, i, n[i], wn)
            hits += 1
    return hits


@pytest.mark.parametrize("flat", [False, True], ids=["tree", "flat"])
@pytest.mark.parametrize("name", list(FAMILIES) + ["comb-b-rebuilt"])
def test_per_ray(gpu, oracle, monkeypatch, name, flat):
    rebuilt = name.endswith("-rebuilt")
    name = name.replace("-rebuilt", "")
    fam = FAMILIES[name]
    if rebuilt:                                   # the median rebuild (no mesh of <= 4096 triangles takes it by itself: adversarial_meshes.py)
        monkeypatch.setenv("PT_AMD_MESH_STACK_MAX", str(am.COMB_NEED[name] - 1))
    geom, rays, want, cast = _reference(oracle, name)
    got = gpu.test_mesh_intersect2(geom, fam.tris, rays, materials=fam.mats, flat=flat)
    hits = _against_the_oracle(fam, rays, want, got)
    assert hits >= 300
    t, p, n, o, culled, tri, fm = got
    if cast is not None:
        # ... and where float64 can tell, the same triangle, distance and point within twice the oracle's own deviation from float64
        tol_t, tol_p = am.TOL[name.split("-")[0]]
        k = np.flatnonzero(~cast.ambiguous)
        assert cast.ambiguous.mean() <= am.PER_RAY_AMBIGUOUS[name.split("-")[0]]
        assert np.array_equal(tri[k], cast.tri[k])
        k = k[cast.hit[k]]
        scale = np.maximum(np.maximum(1.0, np.abs(rays[k, :3]).max(1)), np.maximum(cast.t[k], np.abs(cast.P[k]).max(1)))
        dev_t, dev_p = np.abs(t[k] - cast.t[k]) / scale, np.abs(p[k] - cast.P[k]).max(1) / scale
        print(name, "float64: worst t %.2g (allowed %.2g), point %.2g (allowed %.2g), %d hits" % (dev_t.max(), tol_t, dev_p.max(), tol_p, len(k)))
        assert len(k) >= 300 and dev_t.max() <= tol_t and dev_p.max() <= tol_p


@pytest.mark.parametrize("flat", [False, True], ids=["tree", "flat"])
@pytest.mark.parametrize("name", ["lattice", "lattice-dup", "lattice-flip"])
def test_lattice_known_answers(gpu, oracle, name, flat):
    # the answers in integer arithmetic (adversarial_meshes.lattice_answers; the CPU tests hold the oracle to them too)
    fam = FAMILIES[name]
    o, d = fam.rays(1024)
    want_tri, want_outside, nacc = am.lattice_answers(fam, o)
    assert (nacc >= 2).sum() >= 200 and (nacc >= (6 if name == "lattice" else 12)).sum() >= 40
    for transform in (IDENT, fam.transform):
        geom = oracle.make_geom(2, am.MAT_B, *transform)
        rays = am.to_world(geom, o, d)
        t, p, n, outside, culled, tri, fm = gpu.test_mesh_intersect2(geom, fam.tris, rays, materials=fam.mats, flat=flat)
        want_t, want_p = am.lattice_expected(o, transform)
        hit = want_tri >= 0
        assert np.array_equal(tri, want_tri)
        assert np.all(t[~hit] == -1.0) and np.array_equal(_bits(t[hit]), _bits(want_t[hit]))
        assert np.array_equal(_bits(p[hit]), _bits(want_p[hit])) and np.array_equal(outside[hit], want_outside[hit].astype(np.int32))
        assert np.array_equal(n[hit], np.tile(f32([0, 0, 1]), (int(hit.sum()), 1)))
        assert np.array_equal(fm[hit], fam.mats[want_tri[hit]]) and np.all(fm[~hit] == -1)
        assert name == "lattice" or not np.isin(fm, am.HIDDEN).any()          # a copy never wins


# ---- the production walk ------------------------------------------------------------------------------------------------------------------
def _scene(gpu, oracle, name, res=(W, H)):
    if name.startswith("stacked"):
        return am.stacked_scene(gpu, oracle, SCENES, int(name.split("-")[1]), res)
    return am.family_scene(gpu, oracle, SCENES, FAMILIES[name], res), []


def _no_hidden_material(gpu, sc):
    """independent of the oracle: no path, after any bounce, carries the colour factor of a material that an exact duplicate earlier in the
    file hides (the visible colours are powers of two in every channel, the hidden ones carry a factor 3)"""
    gpu.pathtraceFree()
    gpu.pathtraceInit(sc, traceDepth=DEPTH, max_batch=4, pipeline_depth=2)
    try:
        coloured = 0
        for b in range(1, DEPTH + 1):
            o, d, c, pix = gpu.debug_trace_paths(1, b, W * H)
            assert not am.carries_hidden_factor(c).any(), (b, c[am.carries_hidden_factor(c)][:4])
            coloured += int((c != 1).any(1).sum())
    finally:
        gpu.pathtraceFree()
    assert coloured > 200                         # (paths did take the visible materials' colours)


SCENE_NAMES = ["lattice", "lattice-dup", "lattice-flip", "comb", "comb-b", "soup", "outlier", "cocentric", "stacked-24", "stacked-40"]
VARIANTS = {"pinhole": {}, "lens": dict(lens_radius=0.2, focal_distance=7.0), "direct": dict(direct_lighting=True), "grid8": {}}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_production_walk(gpu, oracle, monkeypatch, name, variant):
    # 64 x 48, depth 4, iterations 1, 2 and 37: the frame, the live counts and the path state after bounces 1 - 4 are the oracle's, bit for bit.
    # (comb, comb-b: every camera ray fills a lane's stack to the hierarchy's need -- tests/test_adversarial_meshes_cpu.py counts them)
    sc, pairs = _scene(gpu, oracle, name)
    assert not name.startswith("stacked") or len(pairs) == 2
    if variant == "grid8":
        monkeypatch.setenv("PT_AMD_MAX_GRID", "8")
    for iters in ([1, 2], [37]):
        _render_both(gpu, oracle, sc, DEPTH, iters, (W, H), dump_bounces=(1, 2, 3, 4), **VARIANTS[variant])


def test_production_walk_rows_in_lds_and_in_global_memory(gpu, oracle, monkeypatch):
    # 24 meshes keep the walk's rows in LDS by themselves: the same scene with the rows read from global memory
    sc, pairs = _scene(gpu, oracle, "stacked-24")
    frames = []
    for rows_global in ("0", "1"):
        monkeypatch.setenv("PT_AMD_WALK_ROWS_GLOBAL", rows_global)
        frames.append(_render_both(gpu, oracle, sc, DEPTH, [1, 2], (W, H), dump_bounces=(1, 2, 3, 4)))
    assert np.array_equal(_bits(frames[0]), _bits(frames[1]))


@pytest.mark.parametrize("name", ["lattice-dup", "lattice-flip", "stacked-24", "stacked-40"])
def test_no_path_takes_a_hidden_duplicates_material(gpu, oracle, name):
    _no_hidden_material(gpu, _scene(gpu, oracle, name)[0])


def test_per_ray_with_vertex_normals(gpu, oracle):
    # pt_test_mesh_intersect2's `normals`: random unit vertex normals on the soup (degenerate faces included), the blended shading normal
    # against the oracle's, bit for bit, through the hierarchy and the flat list
    fam = FAMILIES["soup"]
    geom, rays, want_flat, _ = _reference(oracle, "soup")
    nrm = np.random.default_rng(41).normal(size=(len(fam.tris), 3, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=2, keepdims=True)).reshape(-1, 9).astype(f32)
    want = [oracle.mesh_intersect(geom, fam.tris, r, normals=nrm) for r in rays]
    differ = sum(1 for a, b in zip(want, want_flat) if a[4] >= 0 and not np.array_equal(a[2], b[2]))
    assert differ > 300                                                       # (the blend is not the face normal)
    for flat in (False, True):
        got = gpu.test_mesh_intersect2(geom, fam.tris, rays, normals=nrm, materials=fam.mats, flat=flat)
        assert _against_the_oracle(fam, rays, want, got) >= 300


@pytest.mark.parametrize("name", ["comb", "comb-b-rebuilt", "lattice-dup", "soup"])
def test_guides_against_the_oracle(gpu, oracle, monkeypatch, name):
    # k_gbuffer walks with ptd::meshIntersectionTest on a stack of its own, meshStackNeed levels: the comb fills it
    if name.endswith("-rebuilt"):
        name = name.replace("-rebuilt", "")
        monkeypatch.setenv("PT_AMD_MESH_STACK_MAX", str(am.COMB_NEED[name] - 1))
    sc, _ = _scene(gpu, oracle, name, (32, 24))
    gpu.pathtraceFree()
    gpu.pathtraceInit(sc, traceDepth=DEPTH)
    try:
        pos_t, nrm, geom = gpu.gbuffer(1)
    finally:
        gpu.pathtraceFree()
    ref = oracle.Renderer(sc.camera.view(oracle.CAMERA_DTYPE), sc.geoms.view(oracle.GEOM_DTYPE), sc.materials.view(oracle.MATERIAL_DTYPE), DEPTH, meshes=sc.meshes)
    w_pos, w_nrm, w_geom = dr.oracle_guides(oracle, ref, 1, sc.meshes, None)
    assert (w_geom == 1).sum() > 100                                         # (the mesh fills a good part of the view)
    assert np.array_equal(geom, w_geom)
    assert np.array_equal(_bits(pos_t), _bits(w_pos)) and np.array_equal(_bits(nrm), _bits(w_nrm))
