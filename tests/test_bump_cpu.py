"""Bump mapping on the host (no GPU): the BUMP line of the scene format and its refusals, the Python Scene's fields, the C ABI's new symbols
and struct, and the numpy float32 restatement of the device's gradient, tangents and shading normal (tests/bump_ref.py) against float64
formulas, with its exact properties."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bump_ref as br
import texture_ref as tr
from conftest import ROOT, SCENES
from test_textures_cpu import QUAD, _obj, _scene

F = np.float32


# ---- the scene format --------------------------------------------------------------------------------------------------------------------
def test_bump_line_parses_and_shares_files_with_texture(pt, tmp_path):
    (tmp_path / "h.ppm").write_text("P3 2 1 255 10 10 10 200 200 200\n")
    (tmp_path / "c.ppm").write_text("P3 1 1 255 1 2 3\n")
    sc = pt.Scene(_scene(tmp_path, [("cube", ["BUMP h.ppm 0.25"]), ("sphere", ["TEXTURE h.ppm"]), ("sphere", []),
                                    ("cube", ["TEXTURE c.ppm", "BUMP h.ppm -1.5e-2"])]))
    assert len(sc.textures) == 2 and sc.texture_paths[0].endswith("h.ppm")
    assert sc.geom_bumps.tolist() == [0, -1, -1, 0] and sc.geom_textures.tolist() == [-1, 0, -1, 1]
    assert sc.geom_bumps.dtype == np.int32 and sc.bump_scales.dtype == np.float32
    assert sc.bump_scales.tolist() == [F(0.25), 0, 0, F(-1.5e-2)]
    # the BUMP line sits among TRANS / ROTAT / SCALE and changes none of them
    plain = pt.Scene(_scene(tmp_path, [("cube", []), ("sphere", []), ("sphere", []), ("cube", [])], name="p.txt"))
    assert sc.geoms.tobytes() == plain.geoms.tobytes() and sc.materials.tobytes() == plain.materials.tobytes()


def test_bumped_mesh_keeps_its_uvs(pt, tmp_path):
    a = _obj(tmp_path, "a.obj", QUAD + "f 1/1 2/2 3/3 4/4\n")
    (tmp_path / "h.ppm").write_text("P3 1 1 255 9 9 9\n")
    sc = pt.Scene(_scene(tmp_path, [("mesh " + a, ["BUMP h.ppm 1"])]))
    assert sc.geom_bumps.tolist() == [0] and sc.mesh_uvs[0].shape == (2, 6)


def test_loader_refuses_bad_bump_lines(pt, tmp_path):
    noUv = _obj(tmp_path, "n.obj", QUAD + "f 1 2 3\n")
    (tmp_path / "h.ppm").write_text("P3 1 1 255 1 2 3\n")
    for objects in ([("mesh " + noUv, ["BUMP h.ppm 0.1"])], [("cube", ["BUMP h.ppm"])], [("cube", ["BUMP h.ppm nan"])],
                    [("cube", ["BUMP h.ppm inf"])], [("cube", ["BUMP h.ppm 1e40"])], [("cube", ["BUMP h.ppm 0.1x"])],
                    [("sphere", ["BUMP missing.ppm 0.1"])]):
        with pytest.raises(IOError):
            pt.Scene(_scene(tmp_path, objects))
    pt.Scene(_scene(tmp_path, [("mesh " + noUv, [])]))                         # unbumped: fine


def test_bump_scene_loads_like_its_unbumped_twin(pt, tmp_path):
    src = open(os.path.join(SCENES, "cornell_bump.txt")).read()
    for d in ("models", "textures"):
        (tmp_path / d).symlink_to(os.path.join(SCENES, d))
    (tmp_path / "plain.txt").write_text(re.sub(r"BUMP .*\n", "", src))
    bump = pt.Scene(os.path.join(SCENES, "cornell_bump.txt"))
    plain = pt.Scene(str(tmp_path / "plain.txt"))
    for f in ("geoms", "materials", "camera"):
        assert getattr(bump, f).tobytes() == getattr(plain, f).tobytes()
    # (the height maps come first in the file: the colour texture's index differs, not its file)
    assert [os.path.basename(bump.texture_paths[k]) if k >= 0 else None for k in bump.geom_textures] == \
        [os.path.basename(plain.texture_paths[k]) if k >= 0 else None for k in plain.geom_textures]
    assert (plain.geom_bumps == -1).all() and (plain.bump_scales == 0).all()
    # a bumped cube wall, a bumped mirror sphere, a torus with both TEXTURE and BUMP
    kinds = sorted(int(bump.geoms[g]["type"]) for g in range(len(bump.geoms)) if bump.geom_bumps[g] >= 0)
    assert kinds == [0, 1, 2]
    torus = [g for g in bump.meshes][0]
    assert bump.geom_bumps[torus] >= 0 and bump.geom_textures[torus] >= 0 and bump.geom_bumps[torus] != bump.geom_textures[torus]
    sphere = [g for g in range(len(bump.geoms)) if bump.geom_bumps[g] >= 0 and bump.geoms[g]["type"] == 0][0]
    assert bump.materials[bump.geoms[sphere]["materialid"]]["hasReflective"] > 0


def test_unbumped_scenes_have_no_bump_fields_set(pt):
    for name in ("cornell.txt", "cornell_mesh.txt", "cornell_textured.txt", "spheres64.txt"):
        sc = pt.Scene(os.path.join(SCENES, name))
        assert (sc.geom_bumps == -1).all() and (sc.bump_scales == 0).all() and len(sc.geom_bumps) == len(sc.geoms)


def test_make_scenes_leaves_every_committed_file_as_it_is(tmp_path):
    import shutil
    dst = tmp_path / "scenes"
    shutil.copytree(SCENES, dst)
    subprocess.run([sys.executable, str(dst / "make_scenes.py")], check=True, capture_output=True, timeout=300)
    for dp, _, files in os.walk(SCENES):
        for f in files:
            if f.endswith(".pyc"):
                continue
            rel = os.path.relpath(os.path.join(dp, f), SCENES)
            assert open(os.path.join(SCENES, rel), "rb").read() == open(dst / rel, "rb").read(), rel


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_bump_symbols_and_struct(pt):
    for s in ("pt_set_bump_maps", "pt_group_set_bump_maps"):
        assert s in pt.ABI_SYMBOLS and hasattr(pt.lib(), s)
    assert "pt_test_bump_normal" in pt.TEST_ABI_SYMBOLS and hasattr(pt.test_lib(), "pt_test_bump_normal")
    assert not hasattr(pt.lib(), "pt_test_bump_normal")
    assert C.sizeof(pt.PtBumpBinding) == 24 and pt.PtBumpBinding.uvs.offset == 16 and pt.PtBumpBinding.scale.offset == 8
    assert pt.PT_AMD_ABI_VERSION == 7 and pt.lib().pt_abi_version() == 7
    hdr = open(os.path.join(ROOT, "include", "pt_amd.h")).read()
    assert "typedef struct PtBumpBinding" in hdr and "int pt_set_bump_maps(" in hdr


def test_set_bump_maps_checks_its_arguments_without_a_gpu(pt):
    L = pt.lib()
    b = (pt.PtBumpBinding * 1)(pt.PtBumpBinding(0, 0, 0.5, 0, None))
    assert L.pt_set_bump_maps(b, 1, 20) == -1 and "PtBumpBinding" in L.pt_last_error().decode()
    assert L.pt_set_bump_maps(None, 1, C.sizeof(pt.PtBumpBinding)) == -1
    assert L.pt_set_bump_maps((pt.PtBumpBinding * 1)(pt.PtBumpBinding(0, 0, 0.5, 3, None)), 1, C.sizeof(pt.PtBumpBinding)) == -1
    assert L.pt_set_bump_maps(b, 1, C.sizeof(pt.PtBumpBinding)) == 0
    assert L.pt_set_bump_maps(None, 0, C.sizeof(pt.PtBumpBinding)) == 0       # clears


# ---- the restatement against float64 -----------------------------------------------------------------------------------------------------
def test_gradient_of_a_ramp_matches_float64(rng=np.random.default_rng(21)):
    W, H = 32, 16
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    height = (0.25 * xs / W + 0.5 * (H - 1 - ys) / H).astype(np.float32)      # rises along +u and +v (row 0 = top)
    uv = rng.uniform(0.2, 0.7, (5000, 2)).astype(np.float32)
    s = np.full(len(uv), 0.3, np.float32)
    hu, hv = br.gradient(height, s, uv)
    assert np.allclose(hu, 0.3 * 0.25, rtol=1e-4) and np.allclose(hv, 0.3 * 0.5, rtol=1e-4)


def test_tangents_match_float64_derivatives(rng=np.random.default_rng(22)):
    # sphere: finite differences of the float64 (u, v) -> q map
    u = rng.uniform(0.05, 0.95, 4000)
    v = rng.uniform(0.1, 0.9, 4000)
    q64 = lambda u, v: 0.5 * np.stack([np.cos(np.pi * (v - .5)) * np.cos(2 * np.pi * (u - .5)), np.sin(np.pi * (v - .5)),
                                       np.cos(np.pi * (v - .5)) * np.sin(2 * np.pi * (u - .5))], 1)
    q = q64(u, v).astype(np.float32)
    tu, tv, ok = br.sphere_tangents(q)
    e = 1e-6
    assert ok.all()
    assert np.allclose(tu, (q64(u + e, v) - q64(u - e, v)) / (2 * e), atol=1e-4)
    assert np.allclose(tv, (q64(u, v + e) - q64(u, v - e)) / (2 * e), atol=1e-4)
    # ... and the sphere's own UV map inverts the parametrisation (the tangents belong to the texture's coordinates)
    assert np.allclose(tr.sphere_uv(q), np.stack([u, v], 1), atol=1e-5)
    # mesh: P(uv) is affine over the triangle, so P0 + Tu du + Tv dv reproduces the corners
    tri = rng.normal(size=(3000, 9)).astype(np.float32)
    uvs = rng.uniform(-1, 2, (3000, 6)).astype(np.float32)
    tu, tv, ok = br.mesh_tangents(tri, uvs)
    d64 = uvs.astype(np.float64)
    det = (d64[:, 2] - d64[:, 0]) * (d64[:, 5] - d64[:, 1]) - (d64[:, 4] - d64[:, 0]) * (d64[:, 3] - d64[:, 1])
    good = np.abs(det) > 0.05
    for c in (1, 2):
        rec = tri[:, :3] + tu * (d64[:, 2 * c] - d64[:, 0])[:, None] + tv * (d64[:, 2 * c + 1] - d64[:, 1])[:, None]
        assert np.allclose(rec[good], tri[good, 3 * c:3 * c + 3], atol=2e-3)
    # cube: the transform's columns
    xf = rng.normal(size=(6, 12)).astype(np.float32)
    pu, pv = br.cube_tangents(xf, np.arange(6))
    for f in range(6):
        a = f >> 1
        assert np.array_equal(pu[f], xf[f, 3 * ((a + 1) % 3):3 * ((a + 1) % 3) + 3])
        assert np.array_equal(pv[f], xf[f, 3 * ((a + 2) % 3):3 * ((a + 2) % 3) + 3])


def _frames(rng, n):
    N = rng.normal(size=(n, 3))
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    Pu = rng.normal(size=(n, 3))
    Pv = rng.normal(size=(n, 3))
    return N.astype(np.float32), Pu.astype(np.float32), Pv.astype(np.float32)


def test_shading_normal_matches_float64(rng=np.random.default_rng(23)):
    n = 20000
    N, Pu, Pv = _frames(rng, n)
    hu, hv = rng.uniform(-0.5, 0.5, n).astype(np.float32), rng.uniform(-0.5, 0.5, n).astype(np.float32)
    d = -N                                                          # head-on: never the facing fallback
    Ns, ok = br.bump_normal(N, Pu, Pv, hu, hv, np.ones(n, bool), d)
    N64, Pu64, Pv64 = N.astype(np.float64), Pu.astype(np.float64), Pv.astype(np.float64)
    J = np.einsum("ij,ij->i", N64, np.cross(Pu64, Pv64))
    g = (hu[:, None] * np.cross(Pv64, N64) + hv[:, None] * np.cross(N64, Pu64)) / J[:, None]
    want = N64 - g
    want /= np.linalg.norm(want, axis=1, keepdims=True)
    sel = ok & (np.abs(J) > 0.05)
    assert sel.sum() > n // 2
    assert np.allclose(Ns[sel], want[sel], atol=2e-4)
    # g is the surface gradient: perpendicular to N, and N - g is the normal of the displaced surface P + h N to first order
    assert np.allclose(np.einsum("ij,ij->i", g, N64)[sel], 0, atol=1e-3 * (1 + np.abs(g[sel]).max()))


def test_constant_map_and_zero_scale_return_N_bit_for_bit(rng=np.random.default_rng(24)):
    n = 5000
    N, Pu, Pv = _frames(rng, n)
    uv = rng.uniform(-3, 3, (n, 2)).astype(np.float32)
    c = np.full((5, 7), rng.uniform(0, 1), np.float32)
    hu, hv = br.gradient(c, np.full(n, 0.7, np.float32), uv)
    assert (hu == 0).all() and (hv == 0).all()
    Ns, ok = br.bump_normal(N, Pu, Pv, hu, hv, rng.integers(0, 2, n).astype(bool), -N)
    assert not ok.any() and np.array_equal(Ns.view(np.uint32), N.view(np.uint32))
    ramp = rng.uniform(0, 1, (5, 7)).astype(np.float32)
    hu, hv = br.gradient(ramp, np.zeros(n, np.float32), uv)
    assert (hu == 0).all() and (hv == 0).all()


def test_inside_is_the_negated_outside_bit_for_bit(rng=np.random.default_rng(25)):
    n = 20000
    N, Pu, Pv = _frames(rng, n)
    hu, hv = rng.uniform(-2, 2, n).astype(np.float32), rng.uniform(-2, 2, n).astype(np.float32)
    d = (-N + rng.normal(scale=0.3, size=(n, 3))).astype(np.float32)
    out, ok_o = br.bump_normal(N, Pu, Pv, hu, hv, np.ones(n, bool), d)
    ins, ok_i = br.bump_normal(-N, Pu, Pv, hu, hv, np.zeros(n, bool), -d)
    assert np.array_equal(ok_o, ok_i) and ok_o.sum() > n // 2
    assert np.array_equal(ins.view(np.uint32), (-out).view(np.uint32))


def test_rising_u_tilts_towards_minus_Pu(rng=np.random.default_rng(26)):
    n = 5000
    N, Pu, Pv = _frames(rng, n)
    Pu = (Pu - N * np.einsum("ij,ij->i", Pu, N)[:, None]).astype(np.float32)  # tangent to the surface
    Pv = (Pv - N * np.einsum("ij,ij->i", Pv, N)[:, None]).astype(np.float32)
    hu = rng.uniform(0.05, 0.5, n).astype(np.float32)
    for outside in (True, False):
        NN = N if outside else -N
        Ns, ok = br.bump_normal(NN, Pu, Pv, hu, np.zeros(n, np.float32), np.full(n, outside), -NN)
        assert ok.sum() > 0.9 * n
        # outside: towards -Pu; inside, one surface seen from below: the outside normal negated, towards +Pu
        assert ((np.einsum("ij,ij->i", Ns, Pu)[ok] < 0) == outside).all()


def test_unbumped_cases(rng=np.random.default_rng(27)):
    N = np.array([[0, 0, 1]] * 5, np.float32)
    Pu = np.array([[1, 0, 0], [1, 0, 0], [1, 0, 0], [1, 0, 0], [0, 0, 1]], np.float32)
    Pv = np.array([[0, 1, 0], [1, 0, 0], [0, 1, 0], [0, 1, 0], [0, 1, 0]], np.float32)   # row 1: J == 0
    hu = np.array([0.3, 0.3, np.inf, 100.0, 0.3], np.float32)
    hv = np.zeros(5, np.float32)
    d = np.array([[0, 0, -1]] * 3 + [[-0.99, 0, -0.01]] + [[0, 0, -1]], np.float32)    # row 3: Ns faces away from the ray; row 4: J == 0
    Ns, ok = br.bump_normal(N, Pu, Pv, hu, hv, np.ones(5, bool), d)
    assert ok.tolist() == [True, False, False, False, False]
    assert np.array_equal(Ns[~ok], N[~ok])
    tu, tv, okp = br.sphere_tangents(np.array([[0, 0.5, 0], [0, -0.5, 0], [0.5, 0, 0]], np.float32))
    assert okp.tolist() == [False, False, True]
    tu, tv, okm = br.mesh_tangents(np.zeros((2, 9), np.float32), np.array([[0, 0, 1, 1, 2, 2], [0, 0, 1, 0, 0, 1]], np.float32))
    assert okm.tolist() == [False, True]
