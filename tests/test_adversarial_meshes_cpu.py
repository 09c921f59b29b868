"""The adversarial mesh families of tests/adversarial_meshes.py on the CPU (no GPU): the hierarchy the product builds for them keeps its
invariants in all eight octant copies, the CPU copy of the kernel's walk finds the oracle's brute-force winner, the lattice's integer known
answers ARE the oracle's, the comb fills a lane's stack, and the oracle agrees with a float64 cast where float64 can tell.

Recorded numbers (this file prints them; run with -s):
  needs           lattice 7, lattice-dup 8, lattice-flip 8, comb 23 (natural, no rebuild), comb-b 20 (natural) -> 9 after the median rebuild
                  under PT_AMD_MESH_STACK_MAX = 19, soup 9, outlier 8, cocentric 7.  No mesh of <= 4096 triangles with a natural need > 24 was found.
  stack-filling   comb 48 of 48 axis rays reach deepest == 23; comb-b 48 of 48 reach 20, and 48 of 48 reach 9 in the rebuilt hierarchy
  ties            of 1024 rays: lattice 455 with two or more accepting triangles, 49 with six; lattice-dup / -flip 808 with two or more, 49 with twelve
  float64         tolerances and their measured bases: see the docstring of tests/adversarial_meshes.py
  ambiguous       (rays64, 1024 rays) comb 5.2 %, comb-b 0.1 %, soup 14.6 %, outlier 22.0 %, cocentric 0.1 %; unambiguous hits 970, 1022, 794, 799, 976
                  (per-ray set of the GPU tests) comb 46.7 %, comb-b 40.0 %, soup 16.7 %, outlier 49.5 %, cocentric 0.0 %; unambiguous hits 531, 585, 738, 485, 923
  camera rays     of the comb scenes' own camera rays (every eighth pixel of 64 x 48 at iterations 1, 2 and 37, every second of 32 x 24 at iteration 1),
                  384 of 384 fill the stack to the need in every case: comb 23, comb-b 20, comb-b rebuilt 9
  lattice         the hit point stops 1e-4 short of the surface, so the world distance is not 4 sz but |fl(o.z - fl(sz z + Tz))| with
                  z = 4 - fl(4 - 1e-4): still known without the library (adversarial_meshes.lattice_expected), and equal to the oracle's bit for bit

Mutations (each applied to a scratch copy, never committed) and the tests that failed on them:
  the tie clause `(t == tbest) & (tri < best)` removed in meshIntersectionTest   test_gpu_adversarial_meshes.py::test_per_ray[lattice-tree], [lattice-dup-tree], [lattice-flip-tree],
                                                                                  [soup-tree], test_lattice_known_answers[lattice-tree], [lattice-dup-tree], [lattice-flip-tree] and
                                                                                  test_guides_against_the_oracle[soup]
  the tie clause `(kt == keyT) & (ki < keyI)` removed in k_mesh_walk             test_gpu_adversarial_meshes.py::test_production_walk[lattice-dup], [lattice-flip], [soup]
  the atomic minimum on the distance alone (the low word no part of the key)     test_gpu_adversarial_meshes.py::test_production_walk[stacked-24], [stacked-40]
  halfBitsDirected rounding to nearest instead of outwards                       test_hierarchy_invariants_in_all_octants (all eight families); tests/test_mesh_cpu.py::test_hierarchy_invariants
                                                                                  and ::test_half_precision_planes_round_outwards_everywhere
  medianOnly never set                                                           test_comb_needs_and_stack_filling_rays (the rebuilt need stays 20)"""
import numpy as np
import pytest

import adversarial_meshes as am

f32 = np.float32
FAMILIES = {f.name: f for f in am.families()}
IDENT = ((0, 0, 0), (0, 0, 0), (1, 1, 1))


def _bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


@pytest.mark.parametrize("name", list(FAMILIES))
def test_hierarchy_invariants_in_all_octants(pt, name):
    tris = FAMILIES[name].tris
    nt = len(tris)
    # a surface-area split leaves at least an eighth on each side, a median split a half: at most ceil(7 n / 8) below a node of n > 4
    bound = int(np.ceil(np.log(nt) / np.log(8.0 / 7.0))) + 3
    needs = set()
    for octant in range(8):
        depth, need_here, need = am.check_hierarchy(pt, tris, octant)
        assert depth <= bound and need <= 24
        needs.add(need)
    assert len(needs) == 1
    print(name, "need", needs.pop())


@pytest.mark.parametrize("name", list(FAMILIES))
def test_cpu_walk_finds_the_brute_force_winner(pt, oracle, name):
    fam = FAMILIES[name]
    copies = [pt.mesh_bvh(fam.tris, o) for o in range(8)]
    hits = 0
    for transform in (IDENT, fam.transform):
        geom = oracle.make_geom(2, 0, *transform)
        rays = am.to_world(geom, *fam.rays(48 if name == "comb" else 160))
        for ray in rays:
            wt, wp, wn, wo, wtri = oracle.mesh_intersect(geom, fam.tris, ray)
            ro, rd, octant = am.object_ray(oracle, geom, ray)
            best, tbest, vis, deepest = am.walk(*copies[octant][:3], fam.tris, oracle, ro, rd, copies[octant][3])     # (asserts deepest <= need)
            assert best == wtri, (name, ray, best, wtri)
            hits += best >= 0
    assert hits > (120 if name != "comb" else 40)


@pytest.mark.parametrize("name", ["lattice", "lattice-dup", "lattice-flip"])
def test_lattice_known_answers_are_the_oracles(oracle, name):
    fam = FAMILIES[name]
    o, d = fam.rays(1024)
    tri, outside, nacc = am.lattice_answers(fam, o)
    copies = 2 if name != "lattice" else 1
    print(name, "rays", len(o), "two or more", int((nacc >= 2).sum()), "six", int((nacc >= 6).sum()), "twelve", int((nacc >= 12).sum()))
    assert (nacc >= 2).sum() >= 200 and (nacc >= 6 * copies).sum() >= 40 and (tri < 0).sum() >= 20
    assert name == "lattice" or np.all(tri < 128)                              # (a copy never wins: its original comes first)
    for transform in (IDENT, fam.transform):
        geom = oracle.make_geom(2, 0, *transform)
        rays = am.to_world(geom, o, d)
        tr, sc = np.array(transform[0], np.float64), np.array(transform[2], np.float64)
        assert np.array_equal(rays[:, :3].astype(np.float64), o * sc + tr)      # (integers and powers of two: exact)
        want_t, want_p = am.lattice_expected(o, transform)
        for i, ray in enumerate(rays):
            wt, wp, wn, wo, wtri = oracle.mesh_intersect(geom, fam.tris, ray)
            assert wtri == tri[i], (i, ray, wtri, tri[i])
            if tri[i] < 0:
                assert wt == -1.0
                continue
            assert np.array_equal(_bits(wt), _bits(want_t[i])) and wo == int(outside[i]), (i, wt, want_t[i], wo, outside[i])
            assert np.array_equal(_bits(wp), _bits(want_p[i])), (i, wp, want_p[i])
            assert np.array_equal(wn, f32([0, 0, 1]))                            # (turned to the ray's side)


def test_comb_needs_and_stack_filling_rays(pt, oracle, monkeypatch):
    for name in ("comb", "comb-b"):
        fam = FAMILIES[name]
        need = pt.mesh_bvh(fam.tris, 0)[3]
        assert need == am.COMB_NEED[name] and 16 <= need <= 24                   # natural: pt_init does not rebuild it
        for stack_max in ((None,) if name == "comb" else (None, need - 1)):
            if stack_max:
                monkeypatch.setenv("PT_AMD_MESH_STACK_MAX", str(stack_max))
            copies = [pt.mesh_bvh(fam.tris, o) for o in range(8)]
            monkeypatch.delenv("PT_AMD_MESH_STACK_MAX", raising=False)
            here = copies[0][3]
            if stack_max:
                assert here <= int(np.ceil(np.log2(len(fam.tris)))) < need       # the median rebuild ran
            geom = oracle.make_geom(2, 0, *IDENT)
            rays = am.to_world(geom, *am.comb_axis_rays(fam, 48), unit_share=1.0)
            full = 0
            for ray in rays:
                wtri = oracle.mesh_intersect(geom, fam.tris, ray)[4]
                ro, rd, octant = am.object_ray(oracle, geom, ray)
                best, tbest, vis, deepest = am.walk(*copies[octant][:3], fam.tris, oracle, ro, rd, here)
                assert best == wtri
                full += deepest == here
            print(name, "stack max", stack_max, "need", here, "rays that fill the stack", full, "of", len(rays))
            assert full >= 32


@pytest.mark.parametrize("name", ["comb", "comb-b", "comb-b-rebuilt"])
def test_comb_scene_camera_rays_fill_the_stack(pt, oracle, monkeypatch, name):
    # the scenes of the GPU tests' renders and guide buffers: the oracle's own camera rays (every eighth pixel of 64 x 48 at iterations 1, 2, 37,
    # every second of 32 x 24), walked on the CPU until the stack is full
    from conftest import SCENES
    rebuilt = name.endswith("-rebuilt")
    fam = FAMILIES[name.replace("-rebuilt", "")]
    if rebuilt:
        monkeypatch.setenv("PT_AMD_MESH_STACK_MAX", str(am.COMB_NEED[fam.name] - 1))
    copies = [pt.mesh_bvh(fam.tris, o) for o in range(8)]
    monkeypatch.delenv("PT_AMD_MESH_STACK_MAX", raising=False)
    need = copies[0][3]
    assert need == (am.COMB_NEED[fam.name] if not rebuilt else 9)
    for res, iterations, step in (((64, 48), (1, 2, 37), 8), ((32, 24), (1,), 2)):
        sc = am.family_scene(pt, oracle, SCENES, fam, res)
        ref = oracle.Renderer(sc.camera.view(oracle.CAMERA_DTYPE), sc.geoms.view(oracle.GEOM_DTYPE), sc.materials.view(oracle.MATERIAL_DTYPE), 4, meshes=sc.meshes)
        geom = sc.geoms[1:2].view(oracle.GEOM_DTYPE)
        for it in iterations:
            full = total = 0
            for pix in range(0, res[0] * res[1], step):
                ro, rd, octant = am.object_ray(oracle, geom, ref.camera_ray(it, pix))
                full += am.walk(*copies[octant][:3], fam.tris, oracle, ro, rd, need, until_deepest=need)[3] == need
                total += 1
            print(name, res, "iteration", it, "need", need, "camera rays that fill the stack", full, "of", total)
            assert full >= 32


@pytest.mark.parametrize("name", ["comb", "comb-b", "soup", "outlier", "cocentric"])
def test_float64_cast_against_the_oracle(oracle, name):
    fam = FAMILIES[name]
    tol_t, tol_p = am.TOL[name.split("-")[0]]
    geom = oracle.make_geom(2, 0, *fam.transform)
    worst_t = worst_p = 0.0
    # the float64 check's own rays, on which its conditions hold, and the rays of the per-ray GPU tests: the tolerance covers both sets
    for which, (o, d) in (("rays64", fam.rays64(1024)), ("per-ray set", am.per_ray_set(fam))):
        rays = am.to_world(geom, o, d)
        ref = am.mesh_cast(geom, fam.tris, rays, tol_t)
        keep = ref.hit & ~ref.ambiguous
        print(name, which, "ambiguous %.1f %%" % (100 * ref.ambiguous.mean()), "unambiguous hits", int(keep.sum()))
        assert ref.ambiguous.mean() <= (0.25 if which == "rays64" else am.PER_RAY_AMBIGUOUS[name.split("-")[0]])
        assert keep.sum() >= 300
        for i in np.flatnonzero(~ref.ambiguous):
            wt, wp, wn, wo, wtri = oracle.mesh_intersect(geom, fam.tris, rays[i])
            assert wtri == ref.tri[i], (i, wtri, ref.tri[i])
            if wtri < 0:
                continue
            scale = max(1.0, float(np.abs(rays[i, :3]).max()), float(ref.t[i]), float(np.abs(ref.P[i]).max()))
            worst_t = max(worst_t, abs(float(wt) - ref.t[i]) / scale)
            worst_p = max(worst_p, float(np.abs(wp.astype(np.float64) - ref.P[i]).max()) / scale)
    print(name, "oracle against float64: t %.2g, point %.2g (allowed %.2g, %.2g)" % (worst_t, worst_p, tol_t, tol_p))
    assert worst_t <= tol_t and worst_p <= tol_p
