"""Texture mapping on the MI355X: the device sampler and UV maps bit for bit against the numpy restatement (tests/texture_ref.py), identity
renders pinned to untextured frames the oracle checks (white textures, constant colours, per-face cells), the texture's orientation read from
the paths of bounce 1, invariance across the batching / pipelining / sharding knobs, the headless driver, and pt_init's refusals."""
import os
import subprocess
import types

import numpy as np
import pytest

import texture_ref as tr
from conftest import ROOT, SCENES

pytestmark = pytest.mark.gpu

W, H = 160, 120


@pytest.fixture(scope="module")
def gpu(pt):
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return pt


def _ns(sc, **over):
    """a mutable copy of a Scene's renderer inputs (what pathtraceInit reads)"""
    d = dict(geoms=sc.geoms.copy(), materials=sc.materials.copy(), camera=sc.camera.copy(), traceDepth=sc.traceDepth,
             meshes=dict(sc.meshes), mesh_normals=dict(sc.mesh_normals), mesh_materials=dict(sc.mesh_materials),
             textures=list(getattr(sc, "textures", [])), geom_textures=np.array(getattr(sc, "geom_textures", [-1] * len(sc.geoms)), np.int32),
             mesh_uvs=dict(getattr(sc, "mesh_uvs", {})))
    d.update(over)
    res = d["camera"]["resolution"][0]
    d["image"] = np.zeros((int(res[1]), int(res[0]), 3), np.float32)
    return types.SimpleNamespace(**d)


def _load(gpu, name, w=W, h=H):
    sc = gpu.Scene(os.path.join(SCENES, name))
    sc.set_resolution(w, h)
    return sc


def _render(gpu, sc, iters=8, **kw):
    res = sc.camera["resolution"][0]
    n = int(res[0]) * int(res[1])
    gpu.pathtraceFree()
    gpu.pathtraceInit(sc, **kw)
    gpu.pathtrace_batch(None, 0, 1, iters) if kw.get("max_batch", 0) >= iters else [gpu.pathtrace(None, 0, it, readback=False) for it in range(1, iters + 1)]
    img = gpu.readback(n)
    gpu.pathtraceFree()
    return img


def _oracle(oracle, sc, iters=8, extras=None, mesh_materials=None):
    ref = oracle.Renderer(sc.camera.view(oracle.CAMERA_DTYPE), sc.geoms.view(oracle.GEOM_DTYPE), sc.materials.view(oracle.MATERIAL_DTYPE),
                          sc.traceDepth, meshes=sc.meshes, mesh_normals=sc.mesh_normals,
                          mesh_materials=sc.mesh_materials if mesh_materials is None else mesh_materials)
    if extras:
        ref.set_extras(**extras)
    res = sc.camera["resolution"][0]
    img = np.zeros(int(res[0]) * int(res[1]) * 3, np.float32)
    for it in range(1, iters + 1):
        ref.iterate(it, img)
    return img


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _random_uvs(sc, rng):
    return {g: rng.uniform(-2, 3, (len(t), 6)).astype(np.float32) for g, t in sc.meshes.items()}


# ---- 1: the device functions bit for bit ------------------------------------------------------------------------------------------------
def test_device_sampler_matches_restatement_bit_for_bit(gpu):
    rng = np.random.default_rng(501)
    special = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 3.4e38, -3.4e38, 0, -0.0, 1, -1, 0.5, 1 - 2 ** -24, -2 ** -30, 2 ** -149,
                        0.25, 0.75, 7.5, -7.5], np.float32)
    edge = np.stack(np.meshgrid(special, special), -1).reshape(-1, 2)
    for h, w in ((1, 1), (1, 9), (9, 1), (7, 13), (512, 512)):
        tex = rng.uniform(0, 1, (h, w, 3)).astype(np.float32)
        ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        centres = np.stack([(xs.ravel() + 0.5) / w, 1 - (ys.ravel() + 0.5) / h], 1).astype(np.float32)
        uv = np.concatenate([edge, centres[:4096], rng.uniform(-2, 3, (100000, 2)).astype(np.float32),
                             rng.uniform(-1e7, 1e7, (4096, 2)).astype(np.float32),
                             (np.array([[0, 0], [1, 1], [0, 1], [1, 0]], np.float32)[None] +
                              rng.uniform(-1e-6, 1e-6, (1024, 4, 2)).astype(np.float32)).reshape(-1, 2)])
        got = gpu.test_texture_sample(tex, uv)
        want = tr.sample(tex, uv)
        assert _same(got, want), (h, w, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5])
        assert np.isfinite(got).all()
        c = np.broadcast_to(rng.uniform(0, 1, 3).astype(np.float32), (h, w, 3)).copy()
        assert _same(gpu.test_texture_sample(c, uv), np.broadcast_to(c[0, 0], (len(uv), 3)))


def test_device_uv_maps_match_restatement_bit_for_bit(gpu):
    rng = np.random.default_rng(502)
    n = 120000
    q = (rng.normal(size=(n, 3)) * rng.choice([1e-3, 0.5, 1.0, 30.0], (n, 1))).astype(np.float32)
    q[:12] = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [-1, 0, -1e-9], [-1, 0, 1e-9], [0, 0, 0],
              [np.nan, 0, 0], [np.inf, 1, 0], [1e30, 1e30, 1e30]]
    assert _same(gpu.test_texture_uv(0, q), tr.sphere_uv(q))
    cq = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
    face = rng.integers(0, 6, n).astype(np.int32)
    assert _same(gpu.test_texture_uv(1, cq, face), tr.cube_uv(cq, face))
    bu = rng.uniform(0, 1, n)
    e = np.concatenate([np.stack([bu, rng.uniform(0, 1, n) * (1 - bu)], 1), rng.uniform(-3, 3, (n, 6))], 1).astype(np.float32)
    assert _same(gpu.test_texture_uv(2, e), tr.mesh_uv(e))


# ---- 2: white textures change nothing ---------------------------------------------------------------------------------------------------
WHITE_CASES = [("cornell.txt", {}), ("cornell_mesh.txt", {}), ("spheres64.txt", {}), ("cubes64.txt", {}),
               ("cornell.txt", {"lens_radius": 0.3, "focal_distance": 10.0}), ("cornell_mesh.txt", {"direct_lighting": True})]


@pytest.mark.parametrize("name,extras", WHITE_CASES, ids=["cornell", "cornell_mesh", "spheres64", "cubes64", "dof", "direct"])
def test_white_texture_is_the_identity(gpu, oracle, name, extras):
    sc = _load(gpu, name)
    rng = np.random.default_rng(503)
    plain = _render(gpu, _ns(sc), 3, **extras)
    white = [np.ones((3, 5, 3), np.float32), np.ones((1, 1, 3), np.float32)]
    tex = _ns(sc, textures=white, geom_textures=np.arange(len(sc.geoms), dtype=np.int32) % 2, mesh_uvs=_random_uvs(sc, rng))
    got = _render(gpu, tex, 3, **extras)
    assert _same(got, plain)
    assert _same(got, _oracle(oracle, sc, 3, extras=extras))


# ---- 3: a 1 x 1 texture of colour c on an RGB 1 1 1 material is the material of colour c ------------------------------------------------
@pytest.mark.parametrize("seed", range(8))
def test_constant_texture_is_the_material_colour(gpu, oracle, seed):
    from test_gpu_fuzz import _random_scene
    small = gpu.Scene(os.path.join(SCENES, "mesh_small.txt"))
    sc, (w, h), extras, rng = _random_scene(gpu, oracle, 5650 + seed, {"icosphere": small.meshes[3], "torus": small.meshes[4]})
    sc.mesh_materials = {}                       # (a face's own material would not see the object's texture)
    want = _oracle(oracle, sc, 4, extras)
    mats = sc.materials.copy()
    textures = [np.broadcast_to(m["color"].astype(np.float32), (1, 1, 3)).copy() for m in sc.materials]
    mats["color"] = 1.0
    tex = _ns(sc, materials=mats, textures=textures, geom_textures=sc.geoms["materialid"].astype(np.int32),
              mesh_uvs=_random_uvs(sc, np.random.default_rng(seed)))
    assert _same(_render(gpu, tex, 4, **extras), want), seed


# ---- 4: every face at the centre of a cell of a multi-cell texture = the face materials of those colours --------------------------------
def test_per_face_cells_equal_face_materials(gpu, oracle):
    sc = _load(gpu, "mesh_attributes.txt")
    g = 5                                                          # the cube mesh whose faces carry materials of their own
    ntris = len(sc.meshes[g])
    rng = np.random.default_rng(504)
    cells = rng.uniform(0.1, 1.0, (2, 4, 3)).astype(np.float32)   # 4 x 2 cells of 3 x 3 texels: a texel centre's neighbours share its colour
    tex = np.repeat(np.repeat(cells, 3, 0), 3, 1)
    pick = rng.integers(0, 8, ntris)
    cy, cx = pick // 4, pick % 4
    uv = np.stack([(3 * cx + 1.5) / 12, 1 - (3 * cy + 1.5) / 6], 1).astype(np.float32)
    base = sc.materials.copy()
    mats = np.concatenate([base, np.repeat(base[1:2], 8)])         # diffuse materials of the cells' colours, behind the scene's own
    mats["color"][len(base):] = cells.reshape(8, 3)
    face_mats = (len(base) + pick).astype(np.int32)
    ref_sc = _ns(sc, materials=mats, mesh_materials={g: face_mats})
    # the textured twin: the object's material white and diffuse (as the cells' materials are), no face materials
    tmats = mats.copy()
    own = len(mats)
    tmats = np.concatenate([tmats, base[1:2]])
    tmats["color"][own] = 1.0
    geoms = sc.geoms.copy()
    geoms["materialid"][g] = own
    gt = np.full(len(geoms), -1, np.int32)
    gt[g] = 0
    textured = _ns(sc, materials=tmats, geoms=geoms, mesh_materials={}, textures=[tex], geom_textures=gt,
                   mesh_uvs={g: np.repeat(uv, 3, 0).reshape(ntris, 6)})
    got = _render(gpu, textured)
    want = _oracle(oracle, ref_sc)
    assert _same(got, want)


# ---- 5: orientation: the colour a path carries after bounce 1 is the cell the float64 map puts its hit in --------------------------------
CHECK = 64                                                          # texels per side, 8 x 8-texel cells
CELLS = np.array([[(0.1 + 0.1 * i, 0.15 + 0.1 * j, 0.9 - 0.05 * (i + j)) for i in range(8)] for j in range(8)], np.float32)   # [row][col]


def _checker():
    return np.repeat(np.repeat(CELLS, 8, 0), 8, 1)


def _one_object(gpu, oracle, kind, rot):
    light = oracle.make_geom(1, 0, (0, 14, 4), (0, 0, 0), (8, 0.3, 8))
    obj = oracle.make_geom(kind, 1, (0, 5, 0), rot, (9, 9, 9))
    sc = _load(gpu, "cornell.txt")
    geoms = np.concatenate([light, obj]).view(gpu.GEOM_DTYPE)
    mats = sc.materials[:2].copy()
    mats["color"][1] = (0.9, 0.8, 0.7)
    meshes, uvs = {}, {}
    if kind == 2:                                                   # a UV-mapped square in z = 0: uv = (x + 0.5, y + 0.5)
        quad = np.array([[-.5, -.5, 0, .5, -.5, 0, .5, .5, 0], [-.5, -.5, 0, .5, .5, 0, -.5, .5, 0]], np.float32)
        meshes = {1: quad}
        uvs = {1: (quad.reshape(2, 3, 3)[:, :, :2] + np.float32(0.5)).reshape(2, 6)}
    return _ns(sc, geoms=geoms, materials=mats, traceDepth=3, meshes=meshes, mesh_normals={}, mesh_materials={},
               textures=[_checker()], geom_textures=np.array([-1, 0], np.int32), mesh_uvs=uvs)


def _uv64(kind, g, p):
    inv = np.array(g["inverseTransform"], np.float64).reshape(4, 4).T      # (column-major)
    q = (np.c_[p.astype(np.float64), np.ones(len(p))] @ inv.T)[:, :3]
    if kind == 0:
        d = q / np.linalg.norm(q, axis=1, keepdims=True)
        return 0.5 + np.arctan2(d[:, 2], d[:, 0]) / (2 * np.pi), 0.5 + np.arcsin(np.clip(d[:, 1], -1, 1)) / np.pi
    if kind == 1:
        a = np.argmax(np.abs(q), 1)
        i = np.arange(len(q))
        return q[i, (a + 1) % 3] + 0.5, q[i, (a + 2) % 3] + 0.5
    return q[:, 0] + 0.5, q[:, 1] + 0.5


@pytest.mark.parametrize("kind,rot", [(1, (20, 35, 10)), (0, (10, 60, 0)), (2, (15, -20, 5))], ids=["cube", "sphere", "mesh"])
def test_texture_orientation_in_the_render(gpu, oracle, kind, rot):
    sc = _one_object(gpu, oracle, kind, rot)
    gpu.pathtraceFree()
    gpu.pathtraceInit(sc)
    o, d, c, pix = gpu.debug_trace_paths(1, 1, W * H)
    gpu.pathtraceFree()
    u, v = _uv64(kind, sc.geoms[1], o)
    u, v = u - np.floor(u), v - np.floor(v)
    x, y = u * CHECK, (1 - v) * CHECK
    far = (np.abs(x / 8 - np.round(x / 8)) * 8 > 1.5) & (np.abs(y / 8 - np.round(y / 8)) * 8 > 1.5)
    if kind == 0:                                                   # (the seam and the poles: u wraps, v's cells shrink to points)
        far &= np.abs(v - 0.5) < 0.4
    assert far.sum() > 500, int(far.sum())
    cx, cy = (x[far] // 8).astype(int) % 8, (y[far] // 8).astype(int) % 8
    want = np.float32(sc.materials["color"][1]) * CELLS[cy, cx]
    assert _same(c[far], want), (kind, int(far.sum()), int((c[far] != want).any(1).sum()))


# ---- 6: textured frames do not depend on how the work is cut ------------------------------------------------------------------------------
def test_textured_frames_are_invariant(gpu):
    sc = _load(gpu, "cornell_textured.txt", 96, 72)
    ns = lambda: _ns(sc)
    base = _render(gpu, ns(), 8)
    assert _same(_render(gpu, ns(), 8, max_batch=8), base)
    assert _same(_render(gpu, ns(), 8, max_batch=3, pipeline_depth=1), base)
    assert _same(_render(gpu, ns(), 8, max_batch=4, pipeline_depth=3, trace_ahead=True), base)
    shards = sum(_render(gpu, ns(), 8, shard_rank=r, shard_count=2) for r in range(2))
    assert _same(shards, base)
    grp = gpu.Group(2, devices=[0, 0])
    try:
        grp.init(ns())
        for it in range(1, 9):
            grp.iterate(it)
        got = grp.readback()
    finally:
        grp.destroy()
    assert _same(got.reshape(-1), base)
    # ... and the texture does show: the frame differs from the untextured one
    assert not _same(_render(gpu, _ns(sc, geom_textures=np.full(len(sc.geoms), -1, np.int32)), 8), base)


# ---- 7: the headless driver, and pt_init's refusals ----------------------------------------------------------------------------------------
def test_headless_driver_renders_the_textured_scene(gpu, tmp_path):
    from test_host import _decode_png
    exe = os.path.join(ROOT, "project3-cuda-path-tracer_amd", "host", "pt_render")
    base = str(tmp_path / "textured")
    r = subprocess.run([exe, os.path.join(SCENES, "cornell_textured.txt"), "--res", "96", "64", "--iterations", "4", "--depth", "8",
                        "--out", base], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    img = _decode_png(base + ".png")
    assert img.shape == (64, 96, 3) and img.max() > 0


def _init_direct(gpu, sc, textures, bindings):
    """pt_set_textures + pt_init through the C ABI: (status, pt_last_error)"""
    import ctypes as C
    t = (gpu.PtTexture * max(len(textures), 1))(*textures)
    b = (gpu.PtTexBinding * max(len(bindings), 1))(*bindings)
    gpu.set_meshes(sc.meshes, sc.mesh_normals, sc.mesh_materials)
    assert gpu.lib().pt_set_textures(t, len(textures), C.sizeof(gpu.PtTexture), b, len(bindings), C.sizeof(gpu.PtTexBinding)) == 0
    geoms, mats, cam = (np.ascontiguousarray(x) for x in (sc.geoms, sc.materials, sc.camera))
    rc = gpu.lib().pt_init(gpu._p(cam), gpu._p(geoms), len(geoms), gpu._p(mats), len(mats), 4, None)
    return rc, gpu.lib().pt_last_error().decode()


def test_pt_init_refuses_bad_bindings(gpu):
    sc = _load(gpu, "cornell_textured.txt", 32, 24)
    mesh = [g for g in sc.meshes][0]
    good = dict(textures=list(sc.textures), geom_textures=sc.geom_textures.copy(), mesh_uvs=dict(sc.mesh_uvs))
    gt_bad_tex = sc.geom_textures.copy()
    gt_bad_tex[0] = 7
    gt_bad_geom = np.concatenate([sc.geom_textures, [-1] * 3, [0]]).astype(np.int32)
    bad = [
        ("texture 7", dict(geom_textures=gt_bad_tex)),
        ("no UVs", dict(mesh_uvs={})),
        ("triangles", dict(mesh_uvs={mesh: sc.mesh_uvs[mesh][:-1]})),
        ("non-finite", dict(textures=[sc.textures[0], np.full((2, 2, 3), np.nan, np.float32), sc.textures[2]])),
        ("1..16384", dict(textures=[sc.textures[0], np.zeros((1, 16385, 3), np.float32), sc.textures[2]])),
        ("geom %d of %d" % (len(sc.geoms) + 3, len(sc.geoms)), dict(geom_textures=gt_bad_geom)),
    ]
    for what, over in bad:
        gpu.pathtraceFree()
        with pytest.raises(gpu.PtError):
            gpu.pathtraceInit(_ns(sc, **{**good, **over}))
        assert what in gpu.lib().pt_last_error().decode(), (what, gpu.lib().pt_last_error())
    # through the C ABI: UVs on a cube, a geom bound twice, 2^28 texels (sizes in range: registered without reading the texels)
    tiny = np.zeros(12, np.float32)
    u = np.zeros((2, 6), np.float32)
    ok = gpu.PtTexture(1, 1, tiny.ctypes.data)
    for what, textures, bindings in [
            ("not a mesh", [ok], [gpu.PtTexBinding(3, 0, 2, u.ctypes.data)]),
            ("two texture bindings", [ok], [gpu.PtTexBinding(3, 0, 0, None), gpu.PtTexBinding(3, 0, 0, None)]),
            ("2^28", [ok, gpu.PtTexture(16384, 16384, tiny.ctypes.data)], [gpu.PtTexBinding(3, 0, 0, None)])]:
        gpu.pathtraceFree()
        rc, msg = _init_direct(gpu, sc, textures, bindings)
        assert rc == -1 and what in msg, (what, rc, msg)
    gpu.set_textures([], None, {})
    gpu.pathtraceFree()
    gpu.pathtraceInit(_ns(sc))                        # the good bindings initialise
    gpu.pathtraceFree()
