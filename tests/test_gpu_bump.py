"""Bump mapping on the MI355X: the device gradient, tangents and shading normal bit for bit against the numpy restatement (tests/bump_ref.py),
constant and zero-scale height maps as the identity (against the unbumped frame and the oracle), the tilt read from the paths of bounce 1
(mirror and diffuse), the geometric side rule, invariance across the batching / pipelining / sharding knobs, the headless driver,
pt_init's refusals, and no bump map outliving its scene."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bump_ref as br
from conftest import ROOT, SCENES
from test_gpu_textures import _load, _ns, _oracle, _render, _same

pytestmark = pytest.mark.gpu

W, H = 160, 120
PW, PH = 400, 300                                                  # (the path-reading tests: enough paths for their statistics)


@pytest.fixture(scope="module")
def gpu(pt):
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return pt


def _bns(sc, **over):
    """_ns plus the bump fields (none bound unless given)"""
    d = dict(geom_bumps=np.array(getattr(sc, "geom_bumps", [-1] * len(sc.geoms)), np.int32),
             bump_scales=np.array(getattr(sc, "bump_scales", [0] * len(sc.geoms)), np.float32))
    d.update(over)
    ns = _ns(sc, **{k: v for k, v in d.items() if k not in ("geom_bumps", "bump_scales")})
    ns.geom_bumps, ns.bump_scales = d["geom_bumps"], d["bump_scales"]
    return ns


def _same_or_nan(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


# ---- 1: the device functions bit for bit ------------------------------------------------------------------------------------------------
def _inputs(rng, n):
    kind = rng.integers(0, 3, n).astype(np.int32)
    e = np.zeros((n, 40), np.float32)
    e[:, 0] = rng.choice([0.0, 0.01, 0.3, -0.7, 5.0, 1e30], n)
    e[:, 1] = rng.integers(0, 2, n)
    N = _unit(rng, n)
    e[:, 2:5] = N
    d = (-N * rng.uniform(0.05, 1, (n, 1)) + rng.normal(scale=0.4, size=(n, 3))).astype(np.float32)
    e[:, 5:8] = d
    e[:, 8:20] = rng.normal(size=(n, 12)) * rng.choice([0.1, 1.0, 9.0], (n, 1))
    sph, cub, msh = kind == 0, kind == 1, kind == 2
    e[sph, 20:23] = rng.normal(size=(sph.sum(), 3)) * 0.5
    e[cub, 20:23] = rng.uniform(-0.5, 0.5, (cub.sum(), 3))
    e[cub, 23] = rng.integers(0, 6, cub.sum())
    bu = rng.uniform(0, 1, msh.sum())
    e[msh, 20] = bu
    e[msh, 21] = rng.uniform(0, 1, msh.sum()) * (1 - bu)
    e[msh, 22:28] = rng.uniform(-2, 3, (msh.sum(), 6))
    e[msh, 28:37] = rng.normal(size=(msh.sum(), 9))
    return kind, e


def test_device_bump_matches_restatement_bit_for_bit(gpu):
    rng = np.random.default_rng(601)
    kind, e = _inputs(rng, 60000)
    # special cases: the poles, the sphere's centre, degenerate UVs, a non-finite direction, a zero scale, a huge one
    sp = np.zeros((10, 40), np.float32)
    sp[:, 0] = [0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.0, 1e30, 0.5, 0.5]
    sp[:, 1] = [1, 0, 1, 1, 1, 0, 1, 1, 1, 0]
    sp[:, 2:5] = [0, 0, 1]
    sp[:, 5:8] = [0, 0, -1]
    sp[8, 5:8] = [np.nan, 0, -1]
    sp[:, 8:20] = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]                # (the identity)
    sk = np.array([0, 0, 0, 2, 2, 2, 1, 1, 0, 1], np.int32)
    sp[0, 20:23], sp[1, 20:23], sp[2, 20:23] = [0, 0.5, 0], [0, -0.5, 0], [0, 0, 0]
    sp[3, 22:28] = [0, 0, 1, 1, 2, 2]                              # collinear UVs: det == 0
    sp[4, 22:28] = [0.5, 0.5, 0.5, 0.5, 0.5, 0.5]
    sp[5, 22:28] = [0, 0, 1, 0, 0, 1]
    sp[3:6, 28:37] = [0, 0, 0, 1, 0, 0, 0, 1, 0]
    sp[[6, 7, 9], 20:24] = [0.1, 0.2, 0.5, 5]
    sp[8, 20:23] = [0.3, 0.1, 0.2]
    kind, e = np.concatenate([kind, sk]), np.concatenate([e, sp])
    for hh, ww in ((1, 1), (5, 1), (7, 13), (64, 32)):
        height = rng.uniform(0, 1, (hh, ww)).astype(np.float32)
        got = gpu.test_bump_normal(height, kind, e)
        want = br.evaluate(height, kind, e)
        bad = ~(((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all(1))
        assert not bad.any(), (hh, ww, np.argwhere(bad)[:5].ravel(), got[bad][:2], want[bad][:2])
        if hh > 1 and ww > 1:
            assert got[:, 11].sum() > len(kind) // 4               # (many hits are bumped)
        # the unbumped ones carry N bit for bit
        nb = got[:, 11] == 0
        assert np.array_equal(got[nb, 8:11].view(np.uint32), e[nb, 2:5].view(np.uint32))
    assert (got[-10:, 11] == 0)[[0, 1, 2, 3, 4, 6, 7, 8]].all()     # poles, centre, det == 0, s == 0, huge s, NaN direction
    # a constant map leaves every hit unbumped
    c = np.full((4, 6), 0.37, np.float32)
    out = gpu.test_bump_normal(c, kind, e)
    assert (out[:, 11] == 0).all() and np.array_equal(out[:, 8:11].view(np.uint32), e[:, 2:5].view(np.uint32))


# ---- 2: constant maps and zero scales change nothing -----------------------------------------------------------------------------------
IDENTITY_CASES = [("cornell.txt", {}, True), ("cornell_glass.txt", {}, True), ("cornell_mesh.txt", {}, True), ("mesh_attributes.txt", {}, True),
                  ("cornell_textured.txt", {}, False), ("cornell.txt", {"lens_radius": 0.3, "focal_distance": 10.0}, True),
                  ("cornell_mesh.txt", {"direct_lighting": True}, True), ("spheres64.txt", {}, True)]


@pytest.mark.parametrize("name,extras,with_oracle", IDENTITY_CASES,
                         ids=["cornell", "glass", "cornell_mesh", "mesh_vn", "textured", "dof", "direct", "spheres64"])
def test_constant_or_zero_scale_height_map_is_the_identity(gpu, oracle, name, extras, with_oracle):
    sc = _load(gpu, name)
    rng = np.random.default_rng(602)
    plain = _render(gpu, _bns(sc), 3, **extras)
    ramp = rng.uniform(0, 1, (5, 9, 3)).astype(np.float32)
    const = np.full((3, 4, 3), 0.6, np.float32)
    textures = list(getattr(sc, "textures", [])) + [const, ramp]
    k0 = len(textures) - 2
    n = len(sc.geoms)
    gb = np.where(np.arange(n) % 2 == 0, k0, k0 + 1).astype(np.int32)          # even geoms: a constant map; odd: a ramp at scale 0
    scales = np.where(np.arange(n) % 2 == 0, 3.0, 0.0).astype(np.float32)
    uvs = dict(getattr(sc, "mesh_uvs", {}))
    for g, t in sc.meshes.items():
        uvs.setdefault(g, rng.uniform(-2, 3, (len(t), 6)).astype(np.float32))
    got = _render(gpu, _bns(sc, textures=textures, mesh_uvs=uvs, geom_bumps=gb, bump_scales=scales), 3, **extras)
    assert _same(got, plain)
    if with_oracle:
        assert _same(got, _oracle(oracle, sc, 3, extras=extras))


# ---- 3: the tilt, read from the paths that leave the object after bounce 1 ----------------------------------------------------------------
RAMP_W = 64
SLOPE = 2.0                                                        # world units of height per unit of u: hu = SLOPE (a texel ramp of 1 / W)


def _ramp():
    row = np.arange(RAMP_W, dtype=np.float32) / np.float32(RAMP_W)
    return np.repeat(np.broadcast_to(row, (4, RAMP_W))[:, :, None], 3, 2).copy()


def _slab(gpu, oracle, mat, rot=(0, 20, 0)):
    """a light and a 9 x 9 slab facing the camera (its +z face), material `mat`, a ramp rising along +u bound at SLOPE"""
    light = oracle.make_geom(1, 0, (0, 14, 4), (0, 0, 0), (8, 0.3, 8))
    slab = oracle.make_geom(1, 1, (0, 5, 0), rot, (9, 9, 0.2))
    sc = _load(gpu, "cornell.txt", PW, PH)
    geoms = np.concatenate([light, slab]).view(gpu.GEOM_DTYPE)
    mats = np.concatenate([sc.materials[:1], sc.materials[mat:mat + 1]])
    return _bns(sc, geoms=geoms, materials=mats, traceDepth=3, meshes={}, mesh_normals={}, mesh_materials={}, mesh_uvs={},
                textures=[_ramp()], geom_textures=np.array([-1, -1], np.int32), geom_bumps=np.array([-1, 0], np.int32),
                bump_scales=np.array([0, SLOPE], np.float32))


def _slab_frame(sc):
    """float64: the slab's outward +z normal N, its tangents Pu, Pv and the predicted shading normal Ns"""
    M = np.array(sc.geoms[1]["transform"], np.float64).reshape(4, 4).T       # (column-major)
    IT = np.array(sc.geoms[1]["invTranspose"], np.float64).reshape(4, 4).T
    N = IT[:3, 2] / np.linalg.norm(IT[:3, 2])
    Pu, Pv = M[:3, 0], M[:3, 1]
    g = (SLOPE * np.cross(Pv, N)) / np.dot(N, np.cross(Pu, Pv))
    Ns = (N - g) / np.linalg.norm(N - g)
    return N, Pu, Ns, M


def _leaving(gpu, sc, N, M):
    gpu.pathtraceFree()
    gpu.pathtraceInit(sc)
    o, d, c, pix = gpu.debug_trace_paths(1, 1, PW * PH)
    gpu.pathtraceFree()
    o, d = o.astype(np.float64), d.astype(np.float64)
    centre = M[:3, 3]
    off = (o - centre) @ N                                           # the +z face lies 0.1 in front of the centre, the origin 0.001 beyond
    on = np.abs(off - (0.1 + 0.001)) < 2e-3
    eye = np.array(sc.camera["position"][0], np.float64)
    return o[on], d[on] / np.linalg.norm(d[on], axis=1, keepdims=True), eye


def test_mirror_paths_reflect_about_the_tilted_normal(gpu, oracle):
    sc = _slab(gpu, oracle, 4)                                       # REFL 1, SPECEX 0: half mirror, half diffuse
    N, Pu, Ns, M = _slab_frame(sc)
    assert np.dot(Ns, Pu) < 0                                        # (rising +u tilts towards -Pu)
    o, d, eye = _leaving(gpu, sc, N, M)
    assert len(o) > 10000, len(o)
    P = o - 0.001 * N
    inc = (P - eye) / np.linalg.norm(P - eye, axis=1, keepdims=True)
    refl = lambda n: inc - 2 * (inc @ n)[:, None] * n
    near_bumped = (np.abs(d - refl(Ns)) < 1e-4).all(1)
    near_flat = (np.abs(d - refl(N)) < 1e-4).all(1)
    # (the ramp wraps at u = 0 / 1: the texels there see the jump, a few per cent of the face)
    assert 0.35 < near_bumped.mean() < 0.6, near_bumped.mean()
    assert near_flat.mean() < 0.01, near_flat.mean()


def test_diffuse_paths_centre_on_the_tilted_normal(gpu, oracle):
    sc = _slab(gpu, oracle, 1)                                       # diffuse white
    N, Pu, Ns, M = _slab_frame(sc)
    o, d, eye = _leaving(gpu, sc, N, M)
    assert len(o) > 10000, len(o)
    # the prediction: cosine-weighted about Ns, the draws below the geometric surface ended (the side rule), in float64
    rng = np.random.default_rng(603)
    m = 400000
    up = np.sqrt(rng.uniform(0, 1, m))
    phi = rng.uniform(0, 2 * np.pi, m)
    a = np.cross(Ns, [1.0, 0, 0] if abs(Ns[0]) < 0.5 else [0, 1.0, 0])
    a /= np.linalg.norm(a)
    b = np.cross(Ns, a)
    s = np.sqrt(1 - up * up)
    smp = up[:, None] * Ns + (s * np.cos(phi))[:, None] * a + (s * np.sin(phi))[:, None] * b
    smp = smp[smp @ N > 0]
    want = smp.mean(0)
    # (the wrap texels: a few per cent of the face, tilted the other way -- excluded by where they leave from)
    u = ((o - M[:3, 3]) @ (Pu / np.linalg.norm(Pu))) / np.linalg.norm(Pu) + 0.5
    keep = np.abs(u - 0.5) < 0.45
    got = d[keep].mean(0)
    tol = 5 * d[keep].std(0) / np.sqrt(keep.sum()) + 1e-3
    assert (np.abs(got - want) < tol).all(), (got, want, tol)
    flat = np.array(N) * (2.0 / 3.0)
    assert np.linalg.norm(got - flat) > 2 * np.linalg.norm(tol)       # (and visibly not the unbumped hemisphere's)


# ---- 4: the geometric side rule ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mat", [1, 4, 5], ids=["diffuse", "mirror", "glass"])
def test_every_path_leaves_towards_its_origins_side(gpu, oracle, mat):
    rng = np.random.default_rng(604 + mat)
    light = oracle.make_geom(1, 0, (0, 14, 4), (0, 0, 0), (8, 0.3, 8))
    ball = oracle.make_geom(0, 1, (0, 5, 0), (0, 0, 0), (6, 6, 6))
    sc = _load(gpu, "cornell.txt", PW, PH)
    src = _load(gpu, "cornell_glass.txt").materials[4:5] if mat == 5 else sc.materials[mat:mat + 1]   # diffuse, specular white, glass
    mats = np.concatenate([sc.materials[:1], src])
    noise = rng.uniform(0, 1, (16, 32, 3)).astype(np.float32)
    bs = _bns(sc, geoms=np.concatenate([light, ball]).view(gpu.GEOM_DTYPE), materials=mats, traceDepth=3, meshes={}, mesh_normals={},
              mesh_materials={}, mesh_uvs={}, textures=[noise], geom_textures=np.array([-1, -1], np.int32),
              geom_bumps=np.array([-1, 0], np.int32), bump_scales=np.array([0, 0.4], np.float32))
    gpu.pathtraceFree()
    gpu.pathtraceInit(bs)
    o, d, c, pix = gpu.debug_trace_paths(1, 1, PW * PH)
    gpu.pathtraceFree()
    o, d = o.astype(np.float64), d.astype(np.float64)
    r = np.linalg.norm(o - [0, 5, 0], axis=1)
    near = np.abs(r - 3.0) < 0.01
    assert near.sum() > 3000, int(near.sum())
    n = (o[near] - [0, 5, 0]) / r[near, None]
    side = np.where(r[near] > 3.0, 1.0, -1.0)                         # the origin offset's side: outside, or inside (refracted in)
    assert (side * np.einsum("ij,ij->i", d[near], n) > -1e-5).all()
    # (and the bump does act: the rule removed some paths, which the unbumped ball keeps)
    bs.geom_bumps = np.array([-1, -1], np.int32)
    gpu.pathtraceInit(bs)
    o2, _, _, _ = gpu.debug_trace_paths(1, 1, PW * PH)
    gpu.pathtraceFree()
    assert len(o2) > len(o)


# ---- 5: bumped frames do not depend on how the work is cut ------------------------------------------------------------------------------
def test_bumped_frames_are_invariant(gpu):
    sc = _load(gpu, "cornell_bump.txt", 96, 72)
    ns = lambda: _bns(sc)
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
    # ... and the bumps do show: the frame differs from the unbumped twin's
    assert not _same(_render(gpu, _bns(sc, geom_bumps=np.full(len(sc.geoms), -1, np.int32)), 8), base)


# ---- 6: the headless driver ------------------------------------------------------------------------------------------------------------
def test_headless_driver_renders_the_bump_scene(gpu, tmp_path):
    from test_host import _decode_png
    exe = os.path.join(ROOT, "project3-cuda-path-tracer_amd", "host", "pt_render")
    base = str(tmp_path / "bump")
    r = subprocess.run([exe, os.path.join(SCENES, "cornell_bump.txt"), "--res", "96", "64", "--iterations", "4", "--depth", "8",
                        "--out", base], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    img = _decode_png(base + ".png")
    assert img.shape == (64, 96, 3) and img.max() > 0


# ---- 7: pt_init's refusals -------------------------------------------------------------------------------------------------------------
def test_pt_init_refuses_bad_bump_bindings(gpu):
    sc = _load(gpu, "cornell_bump.txt", 32, 24)
    mesh = [g for g in sc.meshes][0]
    n = len(sc.geoms)
    gb_tex = sc.geom_bumps.copy()
    gb_tex[3] = 9
    gb_geom = np.concatenate([sc.geom_bumps, [-1] * 3, [0]]).astype(np.int32)
    sc_nan = sc.bump_scales.copy()
    sc_nan[3] = np.nan
    no_tex = sc.geom_textures.copy()
    no_tex[mesh] = -1
    bad = [
        ("bump binding", dict(geom_bumps=gb_tex), "texture 9"),
        ("bump binding", dict(geom_bumps=gb_geom, bump_scales=np.concatenate([sc.bump_scales, [0] * 4]).astype(np.float32)),
         "geom %d of %d" % (n + 3, n)),
        ("scale", dict(bump_scales=sc_nan), "non-finite scale"),
        ("no UVs", dict(mesh_uvs={}, geom_textures=no_tex), "bumped mesh geom %d has no UVs" % mesh),
        ("triangles", dict(mesh_uvs={mesh: sc.mesh_uvs[mesh][:-1]}, geom_textures=no_tex), "for bumped mesh geom %d" % mesh),
    ]
    for _, over, what in bad:
        gpu.pathtraceFree()
        with pytest.raises(gpu.PtError):
            gpu.pathtraceInit(_bns(sc, **over))
        assert what in gpu.lib().pt_last_error().decode(), (what, gpu.lib().pt_last_error())
    # through the C ABI: UVs on a cube, a geom bound twice
    u = np.zeros((2, 6), np.float32)
    for what, binds in [("not a mesh", [gpu.PtBumpBinding(3, 0, 0.1, 2, u.ctypes.data)]),
                        ("two bump bindings", [gpu.PtBumpBinding(3, 0, 0.1, 0, None), gpu.PtBumpBinding(3, 0, 0.2, 0, None)])]:
        gpu.pathtraceFree()
        gpu.set_meshes(sc.meshes, sc.mesh_normals, sc.mesh_materials)
        gpu.set_textures(sc.textures, None, {})
        arr = (gpu.PtBumpBinding * len(binds))(*binds)
        assert gpu.lib().pt_set_bump_maps(arr, len(binds), C.sizeof(gpu.PtBumpBinding)) == 0
        geoms, mats, cam = (np.ascontiguousarray(x) for x in (sc.geoms, sc.materials, sc.camera))
        rc = gpu.lib().pt_init(gpu._p(cam), gpu._p(geoms), len(geoms), gpu._p(mats), len(mats), 4, None)
        msg = gpu.lib().pt_last_error().decode()
        assert rc == -1 and what in msg, (what, rc, msg)
    gpu.set_bump_maps(None)
    gpu.set_textures([], None, {})
    gpu.pathtraceFree()
    gpu.pathtraceInit(_bns(sc))                                      # the good bindings initialise
    gpu.pathtraceFree()


# ---- 8: no bump map outlives its scene --------------------------------------------------------------------------------------------------
def test_no_stale_bump_maps(gpu):
    sc = _load(gpu, "cornell_bump.txt", 64, 48)
    unbumped = _render(gpu, _bns(sc, geom_bumps=np.full(len(sc.geoms), -1, np.int32)), 4)
    bumped = _render(gpu, _bns(sc), 4)
    assert not _same(bumped, unbumped)
    # a scene object without the bump fields (the older tests' SimpleNamespace scenes) clears them
    plain = _ns(sc)
    assert not hasattr(plain, "geom_bumps")
    assert _same(_render(gpu, plain, 4), unbumped)
    assert _same(_render(gpu, _bns(sc), 4), bumped)
    # ... and so does one whose fields are None
    none = _ns(sc)
    none.geom_bumps, none.bump_scales = None, None
    assert _same(_render(gpu, none, 4), unbumped)
    # the bindings are kept across pt_free (the reference's Free -> Init restart) and cleared by set_bump_maps(None)
    gpu.pathtraceFree()
    gpu.pathtraceInit(_bns(sc))
    gpu.pathtraceFree()
    gpu.set_bump_maps(None)
    gpu.set_bump_maps(sc.geom_bumps, sc.bump_scales, sc.mesh_uvs)
    gpu.set_bump_maps(None)
