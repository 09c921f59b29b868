"""The TEXTURED family: seeded scenes that take the 24 TEX / TEX|BUMP forms of k_bounce with what the four hand-built scenes of
tests/textured_scenes.py never vary -- non-square textures of eight sizes at offsets of their own in the texel table, unbound primitives
beside bound ones, meshes that are textured only, bumped only or both (so that the UV rows of the two tables part), vertex normals and
face materials under a texture, a textured emitter, plane walls, a thin lens, direct lighting, frames of 1 x 1 to 130 x 5 and depths 1 .. 6.

    sc = textured_scene(pt, oracle, seed)                        # seed: 0 .. N_SEEDS - 1, numpy seeds SEED0 + seed

sc.kind names what the seed is for:

    mixed     seeds 0 .. 47.  The state is the seed's: bit 0 many (five or more spheres: the flat sweep), bit 1 mesh (one to three meshes),
              bit 2 a thin lens, bit 3 bump -- every one of the 16 states three times.  CELL textures: cx x cy cells of one colour each, every
              cell at least 8 texels wide, so the bilinear sampler returns a cell's colour exactly away from the borders
    affine    seeds 48 .. 53.  Every texture samples a + b u + c v per channel at its texel centres: the bilinear interpolant is that same
              function away from the wrap, so the blend itself is checked inside a render, to the tolerance below
    crowd     seeds 54, 55.  Small spheres and cubes, a third of them textured, in a frame of 48 x 36: the flat TEX|MANY|CUBES sweep at
              sizes no other textured test reaches (untextured scenes of these sizes are grouped).  Seed 54 draws 130 .. 200 of them.
              Seed 55 asks for CROWD_ASKED, more than LDS holds: the plan's refusal is recorded in sc.refused and the count comes down
              by 300 at a time until the plan accepts it (900: the largest flat table the ledger sees planned, 143088 B of LDS)
    constant  no seed of its own: constant_twin(sc) of every seed without a tilt -- each texture replaced by ONE colour of the same size, so
              that the CPU oracle renders the same frame from a material table with a copy per (material, texture) pair that occurs

sc.iters = (1, a drawn iteration), sc.checked the bounces held (1, a drawn one, the last; sc.coloured: those whose colours are held too), sc.extras the lens and direct lighting,
sc.cases what the generator put in (the ledger, tests/test_textured_fuzz_cpu.py, counts them), sc.identity "zero scale" / "constant map" for
the two bump seeds whose tilt is none: their paths are the unbumped twin's, bit for bit.

Height maps are ramps (tests/textured_scenes.py: ramp) on non-square textures with unequal slopes, or the constant map; sc.slopes holds every
texture's slopes, sc.specs its (W, H, cx, cy, margin) and sc.cells its cells' colours, as textured_scenes.step reads them.

The affine tolerance (hold d of tests/test_gpu_textured_fuzz.py).  The GPU's geometry is the oracle's bit for bit, so the texel a path reads
differs from the float64 reference's by the UV the fp32 hit point is off by, and by fp32's own products: per hit and channel

    tol = M * (|b| / |Pu| + |c| / |Pv|) * E + 2^-20 * |a + b u + c v|,        M = 2 (the margin of tests/adversarial_meshes.py)

with Pu, Pv from path_ref.tangents and E the largest distance, over every kept path of every seed without a tilt, between the oracle twin's
new origin and where the float64 reference puts it.  Measured by the ledger from the reference and the oracle alone (no GPU):

    E                                          E_MEASURED = 2.4e-04 world units (rooms of 9 .. 12): a sphere met at a cosine of 0.1, where fp32's
                                               quadratic leaves the root 1e-4 off; the median over the kept paths is 1e-6
    M (|b| / |Pu| + |c| / |Pv|) E / |texel|    median over the bound hits 4.4e-05 (a texel step of these textures is |b| / W = 1e-3 .. 9e-3 of its value),
                                               largest 2.5e-02, on the 0.01 thick side of a wall, where |Pu| = 0.01

Hits met at a cosine under 0.05 are left out of E and of the hold: what fp32 leaves of the distance to the surface moves such a hit ALONG the
surface by that over the cosine.
"""
import types

import numpy as np

import textured_scenes as ts

N_MIXED, N_AFFINE, N_CROWD = 48, 6, 2
N_SEEDS = N_MIXED + N_AFFINE + N_CROWD
SEED0 = 11200                           # (numpy seeds 11200 .. 11255)
TINY, STRIP = 20, 37                    # the seeds with a frame of 1 x 1 and of 130 x 5
ZERO_SCALE, CONSTANT_MAP = 8, 9         # the identity seeds: state bump, no lens
# (W, H) -> (cx, cy): cells of 8 texels or more; the small ones are one cell
SIZES = {(1, 1): (1, 1), (1, 9): (1, 1), (9, 1): (1, 1), (7, 13): (1, 1), (96, 32): (3, 2), (32, 96): (2, 3), (128, 128): (4, 4), (60, 90): (3, 5)}
LARGE = [(96, 32), (32, 96), (128, 128), (60, 90)]
RAMPS = [((96, 32), (0.5, 0.25)), ((32, 96), (0.25, 0.5)), ((60, 90), (0.4, -0.2))]          # non-square, SLOPE_U != SLOPE_V
M_TOL = 2.0
E_MEASURED = 2.4e-04
CROWD_ASKED = 2400
EMIT_MAX = 8                            # kEmitMax of csrc/pt_trace.h


def _materials(oracle, rng):
    m = np.zeros(9, oracle.MATERIAL_DTYPE)
    m["color"] = rng.uniform(0.3, 1.0, (9, 3))
    m["emittance"][0] = rng.uniform(3, 6)                           # 0 the light
    for i in (4, 6):                                                # 4 half mirror; 6 half mirror with an exponent (SPECEX)
        m["hasReflective"][i], m["specColor"][i] = 1.0, rng.uniform(0.5, 1.0, 3)
    m["specExponent"][6] = float(rng.choice([5.0, 300.0]))
    m["hasRefractive"][5], m["indexOfRefraction"][5], m["specColor"][5] = 1.0, 1.5, rng.uniform(0.8, 1.0, 3)      # 5 glass
    m["emittance"][7] = rng.uniform(1, 3)                           # 7 a second, dimmer emitter (1 - 3, 8 diffuse)
    return m


def _cell_uvs(ntris, cx, cy, rng, outside):
    """corner UVs that keep triangle i inside cell i % (cx cy), drawn towards its centre -- a wrong row is another cell; `outside`: some
    triangles moved by whole units of u and v (the sampler repeats)"""
    c = np.arange(ntris) % (cx * cy)
    centre = np.stack([(c % cx + 0.5) / cx, 1 - (c // cx + 0.5) / cy], 1)
    corners = centre[:, None, :] + np.array([[-.28 / cx, -.24 / cy], [.28 / cx, -.24 / cy], [0, .28 / cy]])[None]
    if outside:
        corners = corners + rng.integers(-2, 3, (ntris, 1, 2))
    return corners.reshape(-1, 6).astype(np.float32)


def _quad():
    quad = np.array([[-.5, -.5, 0, .5, -.5, 0, .5, .5, 0], [-.5, -.5, 0, .5, .5, 0, -.5, .5, 0]], np.float32)
    xy = quad.reshape(2, 3, 3)[:, :, :2].astype(np.float64)
    # UVs affine in object space that span every cell and reach past 1 in u
    quv = np.stack([0.06 + 1.1 * (xy[..., 0] + 0.5), 0.1 + 0.8 * (xy[..., 1] + 0.5)], -1)
    return quad, quv.reshape(2, 6).astype(np.float32)


def _bent_normals(tris, rng):
    t = tris.reshape(-1, 3, 3).astype(np.float64)
    fn = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    fn /= np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 1e-30)
    vn = fn[:, None, :] + rng.uniform(-0.4, 0.4, t.shape)
    return (vn / np.linalg.norm(vn, axis=2, keepdims=True)).reshape(-1, 9).astype(np.float32)


def _rotation_without_seam(orc, rng, t, eye):
    """a rotation under which the sphere's seam (u = 0 | 1: the object's -x side) and its poles face away from the camera"""
    for _ in range(64):
        r = tuple(rng.uniform(-180, 180, 3))
        L = np.array(orc.make_geom(0, 0, (0, 0, 0), r, (1, 1, 1))["transform"], np.float64).reshape(4, 4).T[:3, :3]
        to_eye = (eye - t) / np.linalg.norm(eye - t)
        if (L @ np.array([-1.0, 0, 0])) @ to_eye < -0.3 and abs((L @ np.array([0, 1.0, 0])) @ to_eye) < 0.8:
            return r
    return r


def textured_scene(pt, oracle, seed):
    rng = np.random.default_rng(SEED0 + seed)
    kind = "mixed" if seed < N_MIXED else ("affine" if seed < N_MIXED + N_AFFINE else "crowd")
    state = seed % 16 if kind == "mixed" else ((seed - N_MIXED) % 8 if kind == "affine" else (1 + 8 * (seed % 2)))
    many, mesh, lens, bump = bool(state & 1), bool(state & 2), bool(state & 4), bool(state & 8)
    round_ = seed // 16
    mats = _materials(oracle, rng)
    cases = set()
    S = float(rng.uniform(9, 12))
    eye = np.array([rng.uniform(-1, 1), S / 2 + rng.uniform(-1, 1), S / 2 - 0.6])

    # ---- the room: up to six walls, some missing, some turned by a few degrees (plane walls); the ceiling light
    rooms = [((0, 0, 0), (S, 0.01, S)), ((0, S, 0), (S, 0.01, S)), ((0, S / 2, -S / 2), (S, S, 0.01)),
             ((-S / 2, S / 2, 0), (0.01, S, S)), ((S / 2, S / 2, 0), (0.01, S, S)), ((0, S / 2, S / 2), (S, S, 0.01))]
    geoms, kinds = [], []
    for k, (t, s) in enumerate(rooms):
        if (k in (1, 3, 4) and rng.random() < 0.12) or (k == 5 and rng.random() < 0.5):
            cases.add("open")
            continue
        r = (0, 0, 0)
        if k in (2, 3, 4) and rng.random() < 0.2:
            r = tuple(float(v) for v in rng.uniform(-4, 4, 3))
            cases.add("turned wall")
        geoms.append(oracle.make_geom(1, int(rng.integers(1, 4)), t, r, s))
        kinds.append("wall")
    geoms.append(oracle.make_geom(1, 0, (0, S - 0.2, 0), (0, 0, 0), (S / 2.5, 0.3, S / 2.5)))
    kinds.append("light")

    # ---- spheres and cubes: arbitrary rotation, non-uniform scale; diffuse, half mirror (with and without an exponent) or glass
    def place():
        return np.array([rng.uniform(-0.32, 0.32) * S, rng.uniform(0.15, 0.7) * S, rng.uniform(-0.35, 0.1) * S])

    if kind == "crowd":
        asked = CROWD_ASKED if seed % 2 else int(rng.integers(130, 201))
        base = 0.42 * S / 200 ** (1 / 3)
        for k in range(asked):
            cube = bool(rng.random() < 0.4)
            d = base * rng.uniform(0.6, 1.3)
            s = d * rng.uniform(0.7, 1.3, 3)
            t = np.array([0, S / 2, -0.1 * S]) + rng.uniform(-1, 1, 3) * np.array([0.4, 0.38, 0.3]) * S
            geoms.append(oracle.make_geom(1 if cube else 0, int(rng.choice([1, 2, 3, 4, 5, 8])), tuple(t), tuple(rng.uniform(-180, 180, 3)), tuple(s)))
            kinds.append("cube" if cube else "sphere")
    else:
        n = int(rng.integers(5, 9)) if many else int(rng.integers(2, 5))
        if not many and len(geoms) == 7:                                # (six walls leave the light among the swept cubes: three more at the most)
            n = min(n, 3)
        room = 4 if len(geoms) < 7 else 3
        for k in range(n):
            cube = bool(k >= 5 and rng.random() < 0.7) if many else bool(rng.random() < 0.5)  # (many: the first five are spheres, all swept)
            t = place()
            s = rng.uniform(1.3, 3.0) * rng.uniform(0.7, 1.3, 3) * (0.55 if many else 1.0) * S / 10
            mat = int(rng.choice([1, 2, 3, 4, 4, 5, 6, 8] if many else [1, 2, 3, 4, 4, 5, 8]))
            if k == 0:
                mat = 4                                                 # (every scene has a half mirror: the bump laws read mirrored paths)
            elif not many and k == n - 1 and rng.random() < 0.4:        # (the lobe's paths are left out of the colour holds: on small objects only)
                mat, s = 6, s * 0.5
            if cube:
                mat = 8 if mat == 5 else mat                            # (glass on spheres: the reference leaves out every ray that starts inside a cube)
                geoms.append(oracle.make_geom(1, mat, tuple(t), tuple(rng.uniform(-180, 180, 3)), tuple(s)))
            else:
                geoms.append(oracle.make_geom(0, mat, tuple(t), _rotation_without_seam(oracle, rng, t, eye), tuple(s)))
            kinds.append("cube" if cube else "sphere")
        if (many or n < room) and rng.random() < 0.5:                      # a second emitter, always textured (few: four swept at the most)
            cube = bool(rng.random() < 0.5)
            t = place()
            t[1] = rng.uniform(0.55, 0.8) * S
            s = rng.uniform(1.0, 1.8, 3) * S / 10
            r = tuple(rng.uniform(-180, 180, 3)) if cube else _rotation_without_seam(oracle, rng, t, eye)
            geoms.append(oracle.make_geom(1 if cube else 0, 7, tuple(t), r, tuple(s)))
            kinds.append("emitter")

    # ---- meshes from the committed scenes' OBJ data: one to three; vertex normals on some, face materials on some (one face emissive)
    meshes, normals, fmats = {}, {}, {}
    mesh_modes = {}
    if mesh:
        small = pt.Scene(_scene_path("mesh_small.txt"))
        stock = {"icosphere": small.meshes[3], "torus": small.meshes[4], "quad": _quad()[0]}
        names = [["torus", "quad"], ["icosphere", "torus", "quad"], ["quad"]][(seed // 2 + round_) % 3]
        order = rng.permutation(len(names))
        spots = [((0.05, 0.34, 0.08), (4, 4, 4)), ((-0.25, 0.55, -0.15), (3, 3, 3)), ((0.05, 0.5, -0.36), (5.5, 4.5, 1))]
        for j in order:
            name = names[j]
            at, sz = spots[["torus", "icosphere", "quad"].index(name)]
            g = len(geoms)
            meshes[g] = stock[name]
            r = (-10 + rng.uniform(-8, 8), 15 + rng.uniform(-10, 10), rng.uniform(-8, 8)) if name == "quad" else tuple(rng.uniform(-60, 60, 3))
            geoms.append(oracle.make_geom(2, int(rng.choice([1, 2, 3, 4])), tuple(np.array(at) * S + rng.uniform(-0.3, 0.3, 3)), r, tuple(np.array(sz) * S / 10)))
            kinds.append("mesh")
            if rng.random() < 0.5:
                normals[g] = _bent_normals(stock[name], rng)
            if rng.random() < 0.5:
                fm = rng.integers(-1, 5, len(stock[name])).astype(np.int32)
                fm[int(rng.integers(0, len(fm)))] = 7                   # one face emits
                fmats[g] = fm
    ngeoms = len(geoms)
    kinds = np.array(kinds)

    # ---- textures: two to seven, every size at an offset of its own in the texel table
    ntex = int(rng.integers(2, 8))
    sizes = [LARGE[int(rng.integers(0, 4))] for _ in range(2)] + [list(SIZES)[int(rng.integers(0, len(SIZES)))] for _ in range(ntex - 2)]
    sizes = [sizes[i] for i in rng.permutation(ntex)]
    if kind == "affine":                                                # (a texture of a few texels is all wrap)
        sizes = [sz if sz in LARGE else LARGE[i % 4] for i, sz in enumerate(sizes)]
    specs = [(w, h) + SIZES[(w, h)] + (1.0,) for w, h in sizes]
    cells = rng.uniform(0.3, 1.0, (ntex, 16, 3)).astype(np.float32)
    affine = None
    if kind == "affine":
        specs = [(w, h, 1, 1, 1.0) for w, h in sizes]
        b, c = rng.uniform(0.1, 0.3, (2, ntex, 3)) * rng.choice([-1, 1], (2, ntex, 3))
        a = rng.uniform(0.25, 0.4, (ntex, 3)) - np.minimum(b, 0) - np.minimum(c, 0)
        affine = np.stack([a, b, c], 2)                                 # (texture, channel, {a, b, c})
        textures = []
        for (w, h), k in zip(sizes, affine):
            u, v = (np.arange(w) + 0.5) / w, 1 - (np.arange(h) + 0.5) / h
            textures.append((k[None, None, :, 0] + k[None, None, :, 1] * u[None, :, None] + k[None, None, :, 2] * v[:, None, None]).astype(np.float32))
    else:
        textures = [ts.spec_texture(sp, col) for sp, col in zip(specs, cells)]
    slopes = [(0.0, 0.0)] * ntex

    # ---- bindings: each primitive bound with probability 0.6 (a third in a crowd); the walls rarely; the second emitter always
    p_bound = np.where(kinds == "wall", 0.5, 0.33 if kind == "crowd" else 0.6)
    gt = np.where(rng.random(ngeoms) < p_bound, rng.integers(0, ntex, ngeoms), -1).astype(np.int32)
    gt[kinds == "emitter"] = int(rng.integers(0, ntex))
    large = [i for i, sz in enumerate(sizes) if sz in LARGE and sz != (128, 128)] or [i for i, sz in enumerate(sizes) if sz in LARGE]
    for want in ("sphere", "cube", "mesh"):                              # one of every kind on a large texture, one unbound beside it
        of = np.flatnonzero(kinds == want)
        if len(of) >= 1:
            gt[of[0]] = large[int(rng.integers(0, len(large)))]
        if len(of) >= 2:
            gt[of[1]] = -1
    mesh_geoms = sorted(meshes)
    if len(mesh_geoms) >= 2 and seed % 4 >= 2:                          # an untextured mesh in front of a textured one, in file order
        gt[mesh_geoms[0]], gt[mesh_geoms[-1]] = -1, large[0]
    gb, scales = np.full(ngeoms, -1, np.int32), np.zeros(ngeoms, np.float32)
    identity = None
    if bump:
        identity = {ZERO_SCALE: "zero scale", CONSTANT_MAP: "constant map"}.get(seed)
        nramps = int(rng.integers(1, 3))
        for j in range(nramps):
            (w, h), sl = RAMPS[(seed + j) % len(RAMPS)]
            if identity == "constant map":
                (w, h), sl = (9, 1), (0.0, 0.0)
            textures.append(np.full((h, w, 3), 0.5, np.float32) if identity == "constant map" else ts.ramp(w, h, *sl))
            specs.append((w, h, 1, 1, 1.0))
            slopes.append(sl)
        objs = np.flatnonzero((kinds == "sphere") | (kinds == "cube") | (kinds == "mesh") | (kinds == "emitter"))
        chosen = objs[rng.random(len(objs)) < (0.2 if kind == "crowd" else 0.55)]
        chosen = np.union1d(chosen, objs[:1])                           # (the half mirror)
        if len(mesh_geoms) >= 2:                                        # the meshes' two tables part: one bumped only, one textured only
            chosen = np.union1d(np.setdiff1d(chosen, mesh_geoms[1:2]), mesh_geoms[0:1])
            if round_ != 1:
                gt[mesh_geoms[0]] = -1
            gt[mesh_geoms[1]] = large[0]
        elif len(mesh_geoms) == 1 and round_ == 2:
            chosen, gt[mesh_geoms[0]] = np.union1d(chosen, mesh_geoms), -1
        for g in chosen:
            gb[g] = ntex + int(rng.integers(0, nramps))
            scales[g] = (0.0 if identity == "zero scale" else float(rng.uniform(1.0, 3.0) * rng.choice([-1, 1]))) * (0.5 if kinds[g] != "sphere" else 1.0)
    cells = np.concatenate([cells, np.ones((len(textures) - ntex, 16, 3), np.float32)])

    # ---- the meshes' UVs: inside their texture's cells (a bumped-only mesh: inside the middle of its height map)
    uvs = {}
    for g in mesh_geoms:
        cx, cy = (specs[gt[g]][2], specs[gt[g]][3]) if gt[g] >= 0 else (2, 2)
        if len(meshes[g]) == 2:
            uvs[g] = _quad()[1]
        else:
            uvs[g] = _cell_uvs(len(meshes[g]), cx, cy, rng, outside=bool(rng.random() < 0.5))
            if np.abs(uvs[g]).max() > 1:
                cases.add("UVs outside [0, 1]")

    # ---- frame, depth, camera, extras
    W, H = int(rng.integers(37, 97)), int(rng.integers(23, 73))
    if kind != "crowd" and seed not in (TINY, STRIP) and W * H < 3600:  # (the 200-kept condition needs the paths: most frames are 60 x 60 and up)
        W, H = max(W, 72), max(H, 54)
    if seed == TINY:
        W, H = 1, 1
    elif seed == STRIP:
        W, H = 130, 5
    elif kind == "crowd":
        W, H = 48, 36
    depth = int(rng.integers(1, 7))
    if kind == "affine" or (bump and not identity):
        depth = max(depth, 3)
    cam = np.zeros(1, oracle.CAMERA_DTYPE)
    cam["resolution"] = (W, H)
    cam["position"] = tuple(eye)
    cam["view"], cam["up"] = (rng.uniform(-0.12, 0.12), rng.uniform(-0.12, 0.05), -1), (0, 1, 0)
    cam["fov"] = (0.0, rng.uniform(32, 48))
    oracle.lib().orc_camera_set_resolution(cam.ctypes.data, W, H)
    extras = {}
    if lens:
        extras.update(lens_radius=float(rng.uniform(0.05, 0.3)), focal_distance=float(S / 2))
    if seed % 7 == 3:
        extras.update(direct_lighting=True)
    iters = (1, int(rng.integers(2, 100)))
    checked = sorted({1, int(rng.integers(1, depth + 1)), depth})
    # (under direct lighting the last bounce's diffuse scatter aims at a light and carries the cosine and the emitter's share of the
    # hemisphere in its colour: its paths are held, its colours are the constant twin's to hold)
    coloured = [k for k in checked if not (extras.get("direct_lighting") and k == depth)]

    def assemble(m):
        keep = np.arange(ngeoms) < m
        sc = types.SimpleNamespace(
            geoms=np.concatenate(geoms[:m]).view(pt.GEOM_DTYPE), materials=mats.view(pt.MATERIAL_DTYPE), camera=cam.view(pt.CAMERA_DTYPE), traceDepth=depth,
            meshes=meshes, mesh_normals=normals, mesh_materials=fmats, mesh_uvs=uvs, textures=textures, geom_textures=gt[keep], geom_bumps=gb[keep],
            bump_scales=scales[keep], image=np.zeros((H, W, 3), np.float32), specs=np.array(specs, np.float64), cells=cells, slopes=np.array(slopes),
            affine=affine, kind=kind, cases=cases, iters=iters, checked=checked, coloured=coloured, extras=extras, identity=identity, res=(W, H), seed=seed, ntex=ntex,
            bump=bump, refused=None, kinds=kinds[keep], wants=dict(many=many, mesh=mesh, lens=lens, bump=bump))
        return sc
    sc = assemble(ngeoms)
    if kind == "crowd":                                                 # the plan may refuse for LDS: the count comes down until it is accepted
        m = ngeoms
        while True:
            try:
                pt.scene_plan(sc, **plan_options(pt, extras))
                break
            except pt.PtError as e:
                if sc.refused is None:
                    refused = (m, str(e))
                m -= 300
                sc = assemble(m)
                sc.refused = refused
    return sc


def _scene_path(name):
    import os
    from conftest import SCENES
    return os.path.join(SCENES, name)


def plan_options(pt, extras):
    """the extras of a scene as pt.scene_plan takes them"""
    o = {k: v for k, v in extras.items() if k != "direct_lighting"}
    if extras.get("direct_lighting"):
        o["flags"] = pt.PT_FLAG_DIRECT_LIGHTING
    return o


def tilted(sc):
    """does any height map of the scene tilt a normal?  (not the identity seeds')"""
    return bool(sc.bump and not sc.identity)


def untextured_twin(sc):
    """the same geometry, meshes, vertex normals, face materials and camera without a texture or a height map: what the CPU oracle renders"""
    n = len(sc.geoms)
    return types.SimpleNamespace(**{**vars(sc), "textures": [], "geom_textures": np.full(n, -1, np.int32), "geom_bumps": np.full(n, -1, np.int32),
                                    "bump_scales": np.zeros(n, np.float32), "mesh_uvs": {}})


def oracle_renderer(oracle, sc):
    ref = oracle.Renderer(sc.camera.view(oracle.CAMERA_DTYPE), sc.geoms.view(oracle.GEOM_DTYPE), sc.materials.view(oracle.MATERIAL_DTYPE), sc.traceDepth,
                          meshes=sc.meshes, mesh_normals=sc.mesh_normals, mesh_materials=sc.mesh_materials)
    ref.set_extras(**sc.extras)
    return ref


def constant_twin(sc):
    """-> (the scene with every colour texture replaced by one colour c_t of its size, the untextured scene the oracle renders in its place,
    {(material, texture): the copy's index}).  The copy of material m under texture t has the colour float32(colour_m * c_t) -- the product
    k_bounce forms first -- and every other field of m; a bound primitive takes its material's copy, a bound mesh's faces theirs."""
    rng = np.random.default_rng(SEED0 + 500 + sc.seed)
    consts = rng.uniform(0.3, 1.0, (sc.ntex, 3)).astype(np.float32)
    textures = [np.broadcast_to(consts[t], sc.textures[t].shape).copy() if t < sc.ntex else sc.textures[t] for t in range(len(sc.textures))]
    const = types.SimpleNamespace(**{**vars(sc), "textures": textures, "kind": "constant", "consts": consts})
    mats, pairs = [sc.materials[i:i + 1].copy() for i in range(len(sc.materials))], {}

    def copy_of(m, t):
        if (m, t) not in pairs:
            pairs[(m, t)] = len(mats)
            c = sc.materials[m:m + 1].copy()
            c["color"] = sc.materials["color"][m].astype(np.float32) * consts[t]
            mats.append(c)
        return pairs[(m, t)]
    geoms, fmats = sc.geoms.copy(), dict(sc.mesh_materials)
    for g in np.flatnonzero(sc.geom_textures >= 0):
        t, m = int(sc.geom_textures[g]), int(sc.geoms["materialid"][g])
        if g in sc.mesh_materials:
            fm = np.asarray(sc.mesh_materials[g], np.int32)
            fmats[g] = np.array([copy_of(int(f), t) if f >= 0 else -1 for f in fm], np.int32)
            if not (fm < 0).any():
                continue
        geoms["materialid"][g] = copy_of(m, t)
    twin = untextured_twin(sc)
    twin.geoms, twin.mesh_materials, twin.materials, twin.kind = geoms, fmats, np.concatenate(mats), "constant twin"
    return const, twin, pairs


def affine_texel(sc, tex, u, v):
    """float64 a + b u + c v of texture `tex` per hit at the wrapped (u, v); 1 for an unbound hit -> (n, 3), and the mask of the hits
    within one texel of the wrap, where the sampler's four texels straddle it"""
    k = sc.affine[np.maximum(tex, 0)]
    fu, fv = u - np.floor(u), v - np.floor(v)
    val = k[:, :, 0] + k[:, :, 1] * fu[:, None] + k[:, :, 2] * fv[:, None]
    w, h = sc.specs[np.maximum(tex, 0), 0], sc.specs[np.maximum(tex, 0), 1]
    wrap = (np.minimum(fu, 1 - fu) * w < 1) | (np.minimum(fv, 1 - fv) * h < 1)
    bound = tex >= 0
    return np.where(bound[:, None], val, 1.0), wrap & bound
