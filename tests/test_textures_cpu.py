"""Texture mapping on the host (no GPU): the TEXTURE line of the scene format, the PPM / PFM reader, OBJ texture coordinates, the
loader's refusals, the Python Scene's fields, and the numpy float32 restatement of the device's sampler and UV maps (tests/texture_ref.py)
against float64 formulas."""
import os
import re
import struct

import numpy as np
import pytest

import texture_ref as tr
from conftest import SCENES

SCENE_HEAD = """MATERIAL 0
RGB 1 1 1
SPECEX 0
SPECRGB 0 0 0
REFL 0
REFR 0
REFRIOR 0
EMITTANCE 5

MATERIAL 1
RGB .5 .6 .7
SPECEX 0
SPECRGB 0 0 0
REFL 0
REFR 0
REFRIOR 0
EMITTANCE 0

CAMERA
RES 32 24
FOVY 45
ITERATIONS 4
DEPTH 4
FILE t
EYE 0 5 10
VIEW 0 0 -1
UP 0 1 0

"""


def _scene(tmp_path, objects, name="s.txt"):
    """objects: (type line, extra lines) per OBJECT block"""
    s = SCENE_HEAD
    for i, (kind, extra) in enumerate(objects):
        s += "OBJECT %d\n%s\nmaterial 1\nTRANS 0 %d 0\nROTAT 0 0 0\nSCALE 1 1 1\n%s\n" % (i, kind, i, "".join(l + "\n" for l in extra))
    p = tmp_path / name
    p.write_text(s)
    return str(p)


def _write_pfm(path, rows, little=True, grey=False):
    with open(path, "wb") as fp:
        fp.write(b"%s\n%d %d\n%s\n" % (b"Pf" if grey else b"PF", len(rows[0]), len(rows), b"-1.0" if little else b"1.0"))
        for row in reversed(rows):                # (PFM: bottom row first)
            for p in row:
                fp.write(struct.pack(("<" if little else ">") + ("f" if grey else "3f"), *((p,) if grey else p)))


def test_ppm_and_pfm_values_and_orientation(pt, tmp_path):
    rows = [[(0, 1, 2), (3, 4, 5), (255, 128, 7)], [(10, 20, 30), (40, 50, 60), (70, 80, 90)]]      # 3 x 2, row 0 = top
    (tmp_path / "a.ppm").write_text("P3\n# comment\n3 2\n255\n" + "\n".join(" ".join("%d %d %d" % p for p in r) for r in rows) + "\n")
    (tmp_path / "b.ppm").write_bytes(b"P6\n3 2\n255\n" + bytes(c for r in rows for p in r for c in p))
    frows = [[(0.25, -1.5, 3.0), (1e-3, 2.0, 4.5)], [(7.0, 8.0, 9.0), (0.1, 0.2, 0.3)]]
    _write_pfm(str(tmp_path / "c.pfm"), frows)
    _write_pfm(str(tmp_path / "d.pfm"), frows, little=False)
    _write_pfm(str(tmp_path / "e.pfm"), [[0.5, 2.0], [3.0, 4.0]], grey=True)
    sc = pt.Scene(_scene(tmp_path, [("cube", ["TEXTURE a.ppm"]), ("sphere", ["TEXTURE b.ppm"]), ("cube", ["TEXTURE c.pfm"]),
                                    ("cube", ["TEXTURE d.pfm"]), ("sphere", ["TEXTURE e.pfm"])]))
    want = np.array(rows, np.float32) / np.float32(255)
    assert sc.textures[0].shape == (2, 3, 3)
    assert np.array_equal(sc.textures[0], want) and np.array_equal(sc.textures[1], want)
    assert np.array_equal(sc.textures[2], np.array(frows, np.float32)) and np.array_equal(sc.textures[3], np.array(frows, np.float32))
    assert np.array_equal(sc.textures[4], np.repeat(np.array([[0.5, 2.0], [3.0, 4.0]], np.float32)[:, :, None], 3, 2))
    assert sc.geom_textures.tolist() == [0, 1, 2, 3, 4]


def test_texture_line_shares_files_and_leaves_others_untextured(pt, tmp_path):
    (tmp_path / "t.ppm").write_text("P3 1 1 255 10 20 30\n")
    sc = pt.Scene(_scene(tmp_path, [("cube", []), ("sphere", ["TEXTURE t.ppm"]), ("cube", ["TEXTURE t.ppm"]), ("sphere", [])]))
    assert len(sc.textures) == 1 and sc.geom_textures.tolist() == [-1, 0, 0, -1]
    assert sc.texture_paths[0].endswith("t.ppm")
    # the TEXTURE line sits among TRANS / ROTAT / SCALE and changes none of them
    plain = pt.Scene(_scene(tmp_path, [("cube", []), ("sphere", []), ("cube", []), ("sphere", [])], name="p.txt"))
    assert sc.geoms.tobytes() == plain.geoms.tobytes() and sc.materials.tobytes() == plain.materials.tobytes()


def _obj(tmp_path, name, body):
    (tmp_path / name).write_text(body)
    return name


QUAD = "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nvn 0 0 1\n"


def test_obj_texture_coordinates(pt, tmp_path):
    a = _obj(tmp_path, "a.obj", QUAD + "f 1/1 2/2 3/3 4/4\n")                   # a quad: fanned into (1 2 3), (1 3 4)
    b = _obj(tmp_path, "b.obj", QUAD + "f 1/1/1 2/2/1 3/3/1\nf -4/-4/-1 -2/-2/-1 -1/-1/-1\n")   # i/j/k, negative indices
    c = _obj(tmp_path, "c.obj", QUAD + "f 1/1 2/2 3/3\nf 1 3 4\n")              # one face without: none kept (all or nothing)
    d = _obj(tmp_path, "d.obj", QUAD + "f 1//1 2//1 3//1\n")                    # normals only
    sc = pt.Scene(_scene(tmp_path, [("mesh " + a, []), ("mesh " + b, []), ("mesh " + c, []), ("mesh " + d, [])]))
    want = np.array([[0, 0, 1, 0, 1, 1], [0, 0, 1, 1, 0, 1]], np.float32)
    assert np.array_equal(sc.mesh_uvs[0], want) and np.array_equal(sc.mesh_uvs[1], want)
    assert 2 not in sc.mesh_uvs and 3 not in sc.mesh_uvs
    assert 1 in sc.mesh_normals and 3 in sc.mesh_normals           # (the vn rule is unchanged)


def test_loader_refuses_what_cannot_be_rendered(pt, tmp_path):
    noUv = _obj(tmp_path, "n.obj", QUAD + "f 1 2 3\n")
    (tmp_path / "t.ppm").write_text("P3 1 1 255 1 2 3\n")
    (tmp_path / "bad.ppm").write_text("P3 1 1 65535 1 2 3\n")                 # 16-bit PPM: not read
    (tmp_path / "short.ppm").write_bytes(b"P6\n2 2\n255\n\x01\x02")
    for objects in ([("mesh " + noUv, ["TEXTURE t.ppm"])], [("cube", ["TEXTURE missing.ppm"])], [("cube", ["TEXTURE bad.ppm"])],
                    [("sphere", ["TEXTURE short.ppm"])]):
        with pytest.raises(IOError):
            pt.Scene(_scene(tmp_path, objects))
    pt.Scene(_scene(tmp_path, [("mesh " + noUv, [])]))                         # untextured: fine


def test_textured_scene_loads_like_its_untextured_twin(pt, tmp_path):
    src = open(os.path.join(SCENES, "cornell_textured.txt")).read()
    (tmp_path / "models").symlink_to(os.path.join(SCENES, "models"))
    (tmp_path / "plain.txt").write_text(re.sub(r"TEXTURE .*\n", "", src))
    tex = pt.Scene(os.path.join(SCENES, "cornell_textured.txt"))
    plain = pt.Scene(str(tmp_path / "plain.txt"))
    for f in ("geoms", "materials", "camera"):
        assert getattr(tex, f).tobytes() == getattr(plain, f).tobytes()
    assert sorted(tex.meshes) == sorted(plain.meshes) and all(np.array_equal(tex.meshes[g], plain.meshes[g]) for g in tex.meshes)
    assert plain.textures == [] and plain.geom_textures.tolist() == [-1] * len(plain.geoms)
    # the scene of the feature: a checker cube (the back wall), a textured sphere and a UV-mapped mesh
    kinds = [int(tex.geoms[g]["type"]) for g in range(len(tex.geoms)) if tex.geom_textures[g] >= 0]
    assert sorted(kinds) == [0, 1, 2] and len(tex.textures) == 3
    mesh = [g for g in tex.meshes if tex.geom_textures[g] >= 0][0]
    assert tex.mesh_uvs[mesh].shape == (len(tex.meshes[mesh]), 6)


def test_untextured_scenes_have_no_texture_fields_set(pt):
    for name in ("cornell.txt", "cornell_mesh.txt", "mesh_attributes.txt", "spheres64.txt"):
        sc = pt.Scene(os.path.join(SCENES, name))
        assert sc.textures == [] and sc.mesh_uvs == {} and (sc.geom_textures == -1).all() and len(sc.geom_textures) == len(sc.geoms)


def test_abi_version_and_struct_layouts(pt):
    import ctypes as C
    assert pt.PT_AMD_ABI_VERSION == 7 and pt.lib().pt_abi_version() == 7
    assert C.sizeof(pt.PtTexture) == 16 and C.sizeof(pt.PtTexBinding) == 24


# ---- the numpy restatement against float64 formulas -------------------------------------------------------------------------------------
def test_sphere_uv_restatement_matches_float64(rng=np.random.default_rng(11)):
    q = np.concatenate([rng.normal(size=(200000, 3)) * rng.choice([1e-3, 0.5, 1, 40], (200000, 1)),
                        [[1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, 0, -1], [0, 1, 0], [0, -1, 0], [-1, 0, -1e-9], [-1, 0, 1e-9]]]).astype(np.float32)
    got = tr.sphere_uv(q).astype(np.float64)
    # float64 formulas on the float32 unit direction the device forms (near the poles asin magnifies that rounding itself: sqrt(2^-23) of
    # v for d.y next to 1, whatever the polynomial -- the spec is asin of the normalised direction)
    d = (q * (np.float32(1) / np.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]))[:, None]).astype(np.float64)
    u = 0.5 + np.arctan2(d[:, 2], d[:, 0]) / (2 * np.pi)
    v = 0.5 + np.arcsin(np.clip(d[:, 1], -1, 1)) / np.pi
    du = np.abs(got[:, 0] - u)
    du = np.minimum(du, 1 - du)                     # (the seam: u = 0 and u = 1 are the same longitude)
    assert du.max() < 2 ** -20 and np.abs(got[:, 1] - v).max() < 2 ** -20


def test_cube_and_mesh_uv_restatements_match_float64(rng=np.random.default_rng(12)):
    n = 100000
    q = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
    face = rng.integers(0, 6, n)
    got = tr.cube_uv(q, face).astype(np.float64)
    a = face >> 1
    qd = q.astype(np.float64)
    assert np.abs(got[:, 0] - (qd[np.arange(n), (a + 1) % 3] + 0.5)).max() < 2 ** -20
    assert np.abs(got[:, 1] - (qd[np.arange(n), (a + 2) % 3] + 0.5)).max() < 2 ** -20
    bu = rng.uniform(0, 1, n)
    bv = rng.uniform(0, 1, n) * (1 - bu)
    corners = rng.uniform(-2, 3, (n, 6))
    e = np.concatenate([np.stack([bu, bv], 1), corners], 1).astype(np.float32)
    got = tr.mesh_uv(e).astype(np.float64)
    ed = e.astype(np.float64)
    w = 1 - ed[:, 0] - ed[:, 1]
    for k in range(2):
        want = ed[:, 2 + k] * w + ed[:, 4 + k] * ed[:, 0] + ed[:, 6 + k] * ed[:, 1]
        assert np.abs(got[:, k] - want).max() < 2 ** -20 * 16       # (|corner| <= 3: 2^-20 of the coordinates' scale)


def test_sample_restatement(rng=np.random.default_rng(13)):
    for H, W in ((1, 1), (1, 7), (5, 3), (64, 64)):
        tex = rng.uniform(0, 1, (H, W, 3)).astype(np.float32)
        # texel centres return the texel exactly; float64 bilinear elsewhere
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        uv = np.stack([(xs.ravel() + 0.5) / W, 1 - (ys.ravel() + 0.5) / H], 1).astype(np.float32)
        ok = (np.float32(uv[:, 0]) * np.float32(W) - np.float32(0.5) == xs.ravel()) & \
             ((np.float32(1) - uv[:, 1]) * np.float32(H) - np.float32(0.5) == ys.ravel())
        assert np.array_equal(tr.sample(tex, uv)[ok], tex[ys.ravel(), xs.ravel()][ok]) and ok.mean() > 0.5
        uv = rng.uniform(-3, 3, (20000, 2)).astype(np.float32)
        got = tr.sample(tex, uv).astype(np.float64)
        u = np.mod(uv[:, 0].astype(np.float64), 1.0)
        v = np.mod(uv[:, 1].astype(np.float64), 1.0)
        x, y = u * W - 0.5, (1 - v) * H - 0.5
        x0, y0 = np.floor(x), np.floor(y)
        fx, fy = (x - x0)[:, None], (y - y0)[:, None]
        x0, y0 = x0.astype(int) % W, y0.astype(int) % H
        x1, y1 = (x0 + 1) % W, (y0 + 1) % H
        t = tex.astype(np.float64)
        want = (t[y0, x0] * (1 - fx) + t[y0, x1] * fx) * (1 - fy) + (t[y1, x0] * (1 - fx) + t[y1, x1] * fx) * fy
        assert np.abs(got - want).max() < 1e-5


def test_sample_constant_texture_is_exact_and_bounded():
    c = np.array([0.3, 0.7, 0.123456789], np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 0, 1, -1, 0.5, 1 - 2 ** -24, -2 ** -30, 3.4e38, -3.4e38, 1e-45], np.float32)
    uv = np.stack(np.meshgrid(special, special), -1).reshape(-1, 2)
    uv = np.concatenate([uv, np.random.default_rng(14).uniform(-1e6, 1e6, (50000, 2)).astype(np.float32)])
    for H, W in ((1, 1), (1, 5), (3, 7), (16, 16)):
        tex = np.broadcast_to(c, (H, W, 3)).copy()
        got = tr.sample(tex, uv)
        assert np.array_equal(got.view(np.uint32), np.broadcast_to(c, got.shape).view(np.uint32))
