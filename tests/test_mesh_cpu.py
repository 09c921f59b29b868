"""Triangle meshes, CPU side (no GPU): the two OBJ / scene loaders (host library and oracle) agree; the oracle's mesh test
behaves like the analytic primitives it approximates; the hierarchy the product builds (pt_test_mesh_bvh, host code) has the
properties the traversal's equivalence with the brute-force rule rests on -- and a CPU walk of it, following the kernel's
rule in fp32, returns the oracle's brute-force result."""
import os

import numpy as np
import pytest

from adversarial_meshes import check_hierarchy, walk as _walk
from conftest import SCENES

f32 = np.float32


def test_loaders_agree_on_mesh_scenes(pt, oracle):
    for name in ("mesh_small.txt", "cornell_mesh.txt"):
        a = pt.Scene(os.path.join(SCENES, name))
        b = oracle.Scene(os.path.join(SCENES, name))
        assert a.geoms.tobytes() == b.geoms.tobytes() and a.materials.tobytes() == b.materials.tobytes()
        assert sorted(a.meshes) == sorted(b.meshes) and len(a.meshes) == 2
        for g in a.meshes:
            assert a.geoms["type"][g] == 2 and a.meshes[g].tobytes() == b.meshes[g].tobytes()
    assert pt.Scene(os.path.join(SCENES, "cornell_mesh.txt")).meshes[6].shape == (1280, 9)
    assert pt.Scene(os.path.join(SCENES, "cornell_mesh.txt")).meshes[7].shape == (2304, 9)     # quads fanned into triangles


def test_obj_statements(pt, oracle, tmp_path):
    (tmp_path / "m.obj").write_text(
        "# comment\no thing\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvn 0 0 1\nvt 0 0\n"
        "f 1/1/1 2/1/1 3/1/1 4/1/1\n"          # a quad with texture / normal references: two triangles
        "v 0 0 1\nf -1 1//1 2//1\n"            # negative = relative to the vertices read so far
        "f 1 2 99\nf 1 2\ns off\n")            # out-of-range reference and a two-vertex face: ignored
    (tmp_path / "s.txt").write_text(
        "MATERIAL 0\nRGB 1 1 1\nSPECEX 0\nSPECRGB 0 0 0\nREFL 0\nREFR 0\nREFRIOR 0\nEMITTANCE 1\n\n"
        "CAMERA\nRES 8 8\nFOVY 45\nITERATIONS 1\nDEPTH 2\nFILE x\nEYE 0 0 5\nVIEW 0 0 -1\nUP 0 1 0\n\n"
        "OBJECT 0\nmesh m.obj\nmaterial 0\nTRANS 0 0 0\nROTAT 0 0 0\nSCALE 1 1 1\n\n"
        "OBJECT 1\nflubber\nmaterial 0\nTRANS 0 0 0\nROTAT 0 0 0\nSCALE 1 1 1\n\n")
    want = np.array([[0, 0, 0, 1, 0, 0, 1, 1, 0], [0, 0, 0, 1, 1, 0, 0, 1, 0], [0, 0, 1, 0, 0, 0, 1, 0, 0]], f32)
    for mod in (pt, oracle):
        sc = mod.Scene(str(tmp_path / "s.txt"))
        assert list(sc.meshes) == [0] and np.array_equal(sc.meshes[0], want)
        assert list(sc.geoms["type"]) == [2, 0]       # an unknown type line leaves the default type (the reference's behaviour)
    # a mesh object whose file is missing, unreadable or holds no triangle fails the LOAD (it used to render as a unit sphere
    # with the mesh's transform and material)
    (tmp_path / "empty.obj").write_text("# no faces\nv 0 0 0\nv 1 0 0\n")
    for bad in ("missing.obj", "empty.obj"):
        (tmp_path / "bad.txt").write_text((tmp_path / "s.txt").read_text().replace("flubber", "mesh " + bad))
        for mod in (pt, oracle):
            with pytest.raises(IOError):
                mod.Scene(str(tmp_path / "bad.txt"))


def test_loaders_agree_on_mesh_attributes(pt, oracle, tmp_path):
    # `vn` + the third field of a face corner = vertex normals (kept only when every corner of every face names one), `usemtl <k>` = a
    # scene material per face: the product's host loader and the oracle's read the same arrays
    name = os.path.join(SCENES, "mesh_attributes.txt")
    a, b = pt.Scene(name), oracle.Scene(name)
    assert a.geoms.tobytes() == b.geoms.tobytes() and sorted(a.meshes) == sorted(b.meshes) == [3, 4, 5]
    assert sorted(a.mesh_normals) == sorted(b.mesh_normals) == [3] and sorted(a.mesh_materials) == sorted(b.mesh_materials) == [5]
    assert a.mesh_normals[3].shape == (80, 9) and a.mesh_normals[3].tobytes() == b.mesh_normals[3].tobytes()
    # (the model's normals are its vertices' radial directions: vertices on a sphere of diameter 1)
    assert np.allclose(a.mesh_normals[3], 2 * a.meshes[3], atol=2e-6)
    want = np.repeat(np.array([2, 3, 4, 0, 5, -1], np.int32), 2)               # six quads = twelve triangles, `usemtl object` = the object's
    assert np.array_equal(a.mesh_materials[5], want) and np.array_equal(b.mesh_materials[5], want)
    # a face corner without a normal makes the whole mesh flat; a name that is no integer returns to the object's material
    (tmp_path / "m.obj").write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvn 0 0 1\nusemtl 1\nf 1//1 2//1 3//1\nusemtl shiny\nf 1//1 3//1 4\n")
    (tmp_path / "s.txt").write_text(
        "MATERIAL 0\nRGB 1 1 1\nSPECEX 0\nSPECRGB 0 0 0\nREFL 0\nREFR 0\nREFRIOR 0\nEMITTANCE 1\n\n"
        "MATERIAL 1\nRGB 1 0 0\nSPECEX 0\nSPECRGB 0 0 0\nREFL 0\nREFR 0\nREFRIOR 0\nEMITTANCE 0\n\n"
        "CAMERA\nRES 8 8\nFOVY 45\nITERATIONS 1\nDEPTH 2\nFILE x\nEYE 0 0 5\nVIEW 0 0 -1\nUP 0 1 0\n\n"
        "OBJECT 0\nmesh m.obj\nmaterial 0\nTRANS 0 0 0\nROTAT 0 0 0\nSCALE 1 1 1\n\n")
    for mod in (pt, oracle):
        sc = mod.Scene(str(tmp_path / "s.txt"))
        assert sc.mesh_normals == {} and np.array_equal(sc.mesh_materials[0], np.array([1, -1], np.int32))


def test_vertex_normals_of_an_icosphere_are_the_spheres_normals(oracle):
    # The model's vertex normals are the radial directions of its vertices, which lie on the sphere of diameter 1: the barycentric
    # blend of the normals at a hit is then parallel to the same blend of the vertices -- the hit point itself.  So the shading
    # normal of the smooth icosphere must be the normal the SPHERE primitive's formula gives at that object-space point,
    # normalize(invTranspose * (p_obj, 0)) (src/intersections.h:137-140), whatever the (anisotropic) transform -- and the flat
    # icosphere's normal must not (it is constant per face).
    sc = oracle.Scene(os.path.join(SCENES, "mesh_attributes.txt"))
    tris, normals = sc.meshes[3], sc.mesh_normals[3]
    rng = np.random.default_rng(5)
    worst_smooth, worst_flat, hits = 0.0, 0.0, 0
    for scale in ((4, 3, 4), (1, 1, 1), (0.5, 2.0, 1.0)):
        geom = oracle.make_geom(2, 0, (-1.5, 3, 0), (10, 20, 30), scale)
        M = geom["transform"][0].astype(np.float64).reshape(4, 4).T          # (column-major in the struct)
        invT = np.linalg.inv(M[:3, :3]).T
        for _ in range(400):
            o = np.array([-1.5, 3, 0]) + rng.normal(size=3) * 6
            target = np.array([-1.5, 3, 0]) + rng.normal(size=3) * 0.8
            d = (target - o) / np.linalg.norm(target - o)
            ray = tuple(o.astype(f32)) + tuple(d.astype(f32))
            t, p, n, outside, tri = oracle.mesh_intersect(geom, tris, ray, normals=normals)
            tf, pf, nf, of, trif = oracle.mesh_intersect(geom, tris, ray)
            assert np.float32(t).view(np.uint32) == np.float32(tf).view(np.uint32) and tri == trif       # the normals change the shading only
            if t <= 0:
                continue
            assert np.array_equal(p.view(np.uint32), pf.view(np.uint32)) and outside == of
            pobj = np.linalg.inv(M) @ np.append(p.astype(np.float64), 1.0)
            want = invT @ pobj[:3]
            want /= np.linalg.norm(want)
            if not outside:
                want = -want
            worst_smooth = max(worst_smooth, float(np.abs(n - want).max()))
            worst_flat = max(worst_flat, float(np.abs(nf - want).max()))
            hits += 1
    assert hits > 300
    assert worst_smooth < 2e-3, worst_smooth          # (the hit point is offset by 1e-4 along the ray: 2e-4 of the radius at most)
    assert worst_flat > 0.05                           # an 80-triangle icosphere's face normals are up to ~15 degrees off


def test_face_materials_in_the_oracle(oracle):
    # `usemtl`: a face takes the scene material it names.  (i) naming the object's own material for every face changes nothing, bit for
    # bit; (ii) the cube mesh of mesh_attributes.txt has an emissive face (material 0): paths end there as on a light
    sc = oracle.Scene(os.path.join(SCENES, "mesh_attributes.txt"))
    sc.set_resolution(48, 48)

    def render(mats):
        ref = oracle.Renderer(sc.camera, sc.geoms, sc.materials, 5, meshes=sc.meshes, mesh_normals=sc.mesh_normals, mesh_materials=mats)
        img = np.zeros(48 * 48 * 3, f32)
        lights = 0
        for it in (1, 2, 3):
            lights += ref.iterate(it, img).lightHits
        return img, lights
    base, lights_base = render({})
    own = {5: np.full(12, int(sc.geoms["materialid"][5]), np.int32)}
    same, lights_same = render(own)
    assert np.array_equal(base.view(np.uint32), same.view(np.uint32)) and lights_base == lights_same
    with_faces, lights_faces = render(sc.mesh_materials)
    assert lights_faces > lights_base + 50 and not np.array_equal(base, with_faces)


def _cube_mesh():
    c = np.array([[x, y, z] for x in (-.5, .5) for y in (-.5, .5) for z in (-.5, .5)], f32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]      # outward counter-clockwise
    tris = []
    for a, b, cc, d in quads:
        tris += [np.concatenate([c[a], c[b], c[cc]]), np.concatenate([c[a], c[cc], c[d]])]
    return np.array(tris, f32)


def test_mesh_of_a_cube_matches_the_box_primitive(oracle):
    tris = _cube_mesh()
    rng = np.random.default_rng(5)
    box = oracle.make_geom(1, 0, (1, 2, 3), (20, 30, 40), (2, 1, 3))
    mesh = box.copy()
    mesh["type"] = 2
    hits = inside = 0
    for i in range(600):
        if i % 3 == 2:
            o = np.array([1, 2, 3]) + rng.uniform(-0.3, 0.3, 3)                # inside
        else:
            o = rng.uniform(-8, 8, 3)
        d = np.array([1, 2, 3]) + rng.uniform(-1.2, 1.2, 3) - o if i % 3 != 2 else rng.normal(size=3)
        d = d / np.linalg.norm(d)
        ray = np.concatenate([o, d]).astype(f32)
        tb, pb, nb, ob = oracle.intersect(box, ray)
        tm, pm, nm, om, tri = oracle.mesh_intersect(mesh, tris, ray)
        assert (tb > 0) == (tm > 0), (i, tb, tm)
        if tb > 0:
            assert abs(tb - tm) < 1e-4 * max(1, tb) and np.allclose(pb, pm, atol=2e-4) and ob == om
            assert np.allclose(nb, nm, atol=1e-4), (nb, nm)
            hits += 1
            inside += 1 - om
    assert hits > 250 and inside > 100


def test_icosphere_mesh_approximates_the_sphere(oracle):
    sc = oracle.Scene(os.path.join(SCENES, "cornell_mesh.txt"))
    tris = sc.meshes[6]
    sph = oracle.make_geom(0, 0, (-1, 4, -1), (0, 0, 0), (3, 3, 3))
    mesh = sph.copy()
    mesh["type"] = 2
    rng = np.random.default_rng(6)
    n = 0
    for _ in range(300):
        o = rng.uniform(-9, 9, 3)
        d = np.array([-1, 4, -1]) + rng.normal(size=3) * 0.6 - o
        ray = np.concatenate([o, d / np.linalg.norm(d)]).astype(f32)
        ts, ps, ns, os_ = oracle.intersect(sph, ray)
        tm, pm, nm, om, tri = oracle.mesh_intersect(mesh, tris, ray)
        if ts > 0 and tm > 0 and -(ray[3:] @ ns) > 0.5:                                # (away from the silhouette)
            assert abs(ts - tm) < 0.03 and os_ == om and nm @ ns > 0.99          # 1280 facets of a radius-1.5 ball
            n += 1
    assert n > 150


def test_hierarchy_invariants(pt):
    sc = pt.Scene(os.path.join(SCENES, "cornell_mesh.txt"))
    cases = [(t, o) for t in sc.meshes.values() for o in (0, 5)] + [(_cube_mesh(), o) for o in range(8)] + [(_cube_mesh()[:1], 3)]
    for tris, octant in cases:
        # (the checker, shared with the adversarial meshes' tests: tests/adversarial_meshes.py)
        depth, need_here, need = check_hierarchy(pt, tris, octant)
        if len(tris) == 1:
            continue
        assert depth <= 3 * int(np.ceil(np.log2(max(len(tris), 1)))) + 2              # no side of a split below an eighth: logarithmic
        assert need_here <= need <= depth and need <= 24


def test_median_rebuild_bounds_the_stack(pt, oracle, monkeypatch):
    # a hierarchy that would need more stack levels than the threshold (24; lowered here through the tests' switch) is rebuilt by
    # median splits alone: need <= ceil(log2 ntris), the same invariants, the same winners as the loop over every triangle
    sc = pt.Scene(os.path.join(SCENES, "cornell_mesh.txt"))
    tris = sc.meshes[7]
    _, _, _, need_sah = pt.mesh_bvh(tris, 0)
    monkeypatch.setenv("PT_AMD_MESH_STACK_MAX", str(need_sah - 1))
    copies = [pt.mesh_bvh(tris, o) for o in range(8)]
    monkeypatch.delenv("PT_AMD_MESH_STACK_MAX")
    need = copies[0][3]
    assert need <= int(np.ceil(np.log2(len(tris)))) and need < need_sah + 1
    ident = oracle.make_geom(2, 0, (0, 0, 0), (0, 0, 0), (1, 1, 1))
    rng = np.random.default_rng(11)
    hits = 0
    for i in range(200):
        o = (rng.normal(size=3) * 2.0).astype(f32)
        tgt = tris[rng.integers(len(tris))].reshape(3, 3).mean(0) + rng.normal(size=3) * 0.02
        d = ((tgt - o) / np.linalg.norm(tgt - o)).astype(f32)
        rd = oracle.normalize(d)
        wt, wp, wn, wo, wtri = oracle.mesh_intersect(ident, tris, np.concatenate([o, d]))
        octant = int(np.signbit(rd[0])) | int(np.signbit(rd[1])) << 1 | int(np.signbit(rd[2])) << 2
        best, tbest, vis, _ = _walk(*copies[octant][:3], tris, oracle, o, rd, copies[octant][3])
        assert best == wtri
        hits += best >= 0
    assert hits > 150


def test_half_precision_planes_round_outwards_everywhere(pt):
    # halfBitsDirected (pt_mesh.h) on boxes from 1e-9 to 1e6, both signs: a node's planes contain the exact box, by less than
    # one step of half precision; beyond the half range they are the largest finite half or infinity, on the permitted side
    rng = np.random.default_rng(5)
    for scale in (1e-9, 3e-7, 6e-5, 1e-3, 1.0, 300.0, 65504.0, 7e4, 1e6):
        tris = (rng.uniform(-1, 1, (6, 9)) * scale).astype(f32)
        recs, nodes, first, need = pt.mesh_bvh(tris, 0)
        margin = f32(1e-5) * np.abs(tris).max()
        v = tris.reshape(-1, 3, 3)
        for nd in nodes:
            for ref, planes in ((int(nd["ref"]), nd["planes"]), (int(nd["far_ref"]), nd["far_planes"])):
                if not ref & pt.MESH_LEAF:
                    continue
                t = (ref & ~pt.MESH_LEAF) // 3
                lo, hi = v[t].min(0) - margin, v[t].max(0) + margin
                pl = planes.astype(np.float64)
                assert np.all(pl[:3] <= lo) and np.all(pl[3:] >= hi)                      # (octant 0: entry = lo, exit = hi)
                lo16, hi16 = planes[:3], planes[3:]
                fin = np.isfinite(lo16.astype(np.float64))
                assert np.all(np.nextafter(lo16, np.float16(np.inf)).astype(np.float64)[fin] > lo[fin])   # the nearest half below
                fin = np.isfinite(hi16.astype(np.float64))
                assert np.all(np.nextafter(hi16, np.float16(-np.inf)).astype(np.float64)[fin] < hi[fin])
                exact = np.concatenate([lo, hi]).astype(np.float64)
                big = np.abs(exact) > 65504.0                                             # beyond the half range
                assert np.all((np.abs(pl[big]) == 65504.0) | np.isinf(pl[big]))


def test_hierarchy_walk_equals_the_brute_force_rule(pt, oracle):
    sc = pt.Scene(os.path.join(SCENES, "cornell_mesh.txt"))
    ident = oracle.make_geom(2, 0, (0, 0, 0), (0, 0, 0), (1, 1, 1))       # identity: world space = object space
    rng = np.random.default_rng(7)
    for g in (6, 7):
        tris = sc.meshes[g]
        copies = [pt.mesh_bvh(tris, o) for o in range(8)]
        hits = visited = 0
        for i in range(400):
            o = (rng.normal(size=3) * (0.2 if i % 4 == 0 else 2.0)).astype(f32)
            tgt = tris[rng.integers(len(tris))].reshape(3, 3).mean(0) + rng.normal(size=3) * 0.02
            d = (tgt - o) if i % 5 else rng.normal(size=3)
            d = (d / np.linalg.norm(d)).astype(f32)
            if i % 7 == 3:                        # axis-parallel components, +0 and -0: the copy is chosen by the SIGN BIT of the reciprocal
                d[i % 3] = f32(0.0) if i % 2 else f32(-0.0)
                d = (d / np.linalg.norm(d)).astype(f32)
            # (the oracle normalises once more in object space; feed it the direction it will actually use)
            rd = oracle.normalize(d)
            wt, wp, wn, wo, wtri = oracle.mesh_intersect(ident, tris, np.concatenate([o, d]))
            octant = int(np.signbit(rd[0])) | int(np.signbit(rd[1])) << 1 | int(np.signbit(rd[2])) << 2
            best, tbest, vis, _ = _walk(*copies[octant][:3], tris, oracle, o, rd, copies[octant][3])
            assert best == wtri, (g, i, best, wtri)
            hits += best >= 0
            visited += vis
        assert hits > 250
        assert visited / 400 < 0.05 * (2 * len(tris) - 1)      # ... and it is a hierarchy: a fraction of the records per ray
        print('mesh', g, 'records fetched per ray', visited / 400)
