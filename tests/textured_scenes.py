"""The scenes of the textured-path tests (tests/test_textured_paths_cpu.py, tests/test_gpu_textured_paths.py) and the one step both take
through the float64 reference (tests/path_ref.py): a path at bounce k matched to itself at bounce k - 1, its ray cast, the texture cell
and the colour predicted.

Every primitive carries a CELL texture: 4 x 4 cells of 32 x 32 texels, one colour per cell, every cell another colour.  The bilinear sampler
returns a cell's colour exactly (a + (b - a) * fx with a == b) wherever its two texels lie in one cell, so the colour after a bounce is known
to the bit although (u, v) is only known to float64 accuracy.  Four such textures are shared round the primitives (geom g: texture g % 4).

The seeded family of tests/textured_fuzz_scenes.py takes the same step with a spec PER TEXTURE (sc.specs: W, H, cells across and down, margin;
sc.cells their colours; sc.slopes every height map's ramp), unbound primitives (texel 1), face materials and vertex normals; a scene that
names no specs, like the ones built here, has SPEC for every texture."""
import os
import types

import numpy as np

import path_ref as pr
from conftest import SCENES

W, H, DEPTH = 96, 72, 6
ITERS = (1, 37)
SPEC = (128, 128, 4, 4, 1.0)                                        # a texture's (W, H, cells across, cells down, margin in texels): path_ref.cell
LENS = dict(lens_radius=0.3, focal_distance=10.0)
STATE = ("first", "dof", "many", "sweptCubes", "mesh", "grouped", "tex", "bump", "plain")      # the bits of pt_test_bounce_form's state
SLOPE_U, SLOPE_V = 0.5, 0.25                                        # the ramp's rise per unit of u and of v: unequal, so that swapped tangents show
BUMP_SCALE = {"sphere": 4.0, "cube": 1.5, "mirror_cube": 1.5, "quad": 1.5}
CASES = [(s, lens, bump) for s in ("few", "many", "mesh", "many_mesh") for lens in (False, True) for bump in (False, True)]
CASE_IDS = ["%s%s%s" % (s, "-lens" if l else "", "-bump" if b else "") for s, l, b in CASES]


def cell_colours():
    """(4 textures, 16 cells, 3): distinct, well away from 0"""
    return np.random.default_rng(811).uniform(0.3, 1.0, (4, 16, 3)).astype(np.float32)


def cell_texture(colours):
    return spec_texture(SPEC, colours)


def spec_texture(spec, colours):
    """the cell texture of `spec`: (H, W, 3), cell row * cx + column in colours[row * cx + column]"""
    w, h, cx, cy, _ = spec
    return np.repeat(np.repeat(np.asarray(colours, np.float32)[:cx * cy].reshape(cy, cx, 3), h // cy, 0), w // cx, 1).copy()


def ramp(w=SPEC[0], h=SPEC[1], slope_u=SLOPE_U, slope_v=SLOPE_V):
    """height = slope_u * u + slope_v * v at the texel centres of a w x h map (128 x 128: multiples of 1 / 512, exact), so away from the
    wrap hu = scale * slope_u and hv = scale * slope_v whatever w and h are"""
    au, av = np.arange(w, dtype=np.float32) / np.float32(w), np.arange(h, dtype=np.float32) / np.float32(h)
    ht = np.float32(slope_u) * au[None, :] + np.float32(slope_v) * av[::-1][:, None]
    return np.repeat(ht[:, :, None], 3, 2).copy()


def _materials(pt):
    m = np.zeros(6, pt.MATERIAL_DTYPE)
    rows = [((1, 1, 1), (0, 0, 0), 0, 0, 0, 5),                     # 0 the light
            ((.98, .98, .98), (0, 0, 0), 0, 0, 0, 0),               # 1 diffuse white
            ((.85, .35, .35), (0, 0, 0), 0, 0, 0, 0),               # 2 diffuse red
            ((.35, .85, .35), (0, 0, 0), 0, 0, 0, 0),               # 3 diffuse green
            ((.9, .95, .8), (.97, .9, .85), 1, 0, 0, 0),            # 4 REFL 1, SPECEX 0: half mirror, half diffuse
            ((.95, .9, .98), (.92, .96, .9), 0, 1, 1.5, 0)]         # 5 glass
    for i, (col, spec, refl, refr, ior, emit) in enumerate(rows):
        m[i] = (col, 0, spec, refl, refr, ior, emit)
    return m


def build(pt, orc, name, bump):
    """the scene `name` (few, many, mesh, many_mesh) as pathtraceInit reads it, with ramp height maps bound when `bump`"""
    cam = pt.Scene(os.path.join(SCENES, "cornell.txt"))
    cam.set_resolution(W, H)
    g = [orc.make_geom(1, 0, (0, 10, 0), (0, 0, 0), (4, .3, 4)),                    # 0 the light (a third wider than Cornell's: more paths end on it)
         orc.make_geom(1, 1, (0, 0, 0), (0, 0, 0), (10, .01, 10)),                  # 1-5 the Cornell walls
         orc.make_geom(1, 1, (0, 10, 0), (0, 0, 90), (.01, 10, 10)),
         orc.make_geom(1, 1, (0, 5, -5), (0, 90, 0), (.01, 10, 10)),
         orc.make_geom(1, 2, (-5, 5, 0), (0, 0, 0), (.01, 10, 10)),
         orc.make_geom(1, 3, (5, 5, 0), (0, 0, 0), (.01, 10, 10)),
         orc.make_geom(0, 4, (-2.2, 6, -1.5), (20, 40, 10), (3.4, 3.0, 3.2)),       # 6 a rotated sphere, half mirror
         orc.make_geom(1, 1, (2.4, 2.2, -1.5), (15, 30, 10), (2.4, 4.0, 2.0)),      # 7 a rotated, non-uniformly scaled cube
         orc.make_geom(0, 5, (1.8, 6.8, 1.5), (0, 0, 0), (2.4, 2.4, 2.4)),          # 8 a glass sphere
         orc.make_geom(1, 4, (-2.4, 1.6, 1.8), (0, -25, 0), (2.6, 3.0, 2.6))]       # 9 a REFL 1 cube
    named = {"sphere": 6, "cube": 7, "mirror_cube": 9}
    if name.startswith("many"):                                                      # six small ones: more than kBinMax = 4 are swept
        g += [orc.make_geom(0, 1, (0.2, 0.5, 3.2), (0, 0, 0), (.9, .9, .9)),
              orc.make_geom(0, 2, (-4, 8, -3), (0, 30, 0), (.9, .9, .9)),
              orc.make_geom(0, 3, (3.9, 4.8, 2.5), (40, 0, 0), (.9, .9, .9)),
              orc.make_geom(1, 3, (0, 4.2, -0.5), (30, 20, 10), (.8, .8, .8)),
              orc.make_geom(1, 1, (-3.8, 5, 3), (0, 45, 0), (.8, .8, .8)),
              orc.make_geom(1, 2, (4, 8.5, -3.5), (10, 10, 40), (.8, .8, .8))]
    meshes, uvs = {}, {}
    if name.endswith("mesh"):
        # the torus under an atlas: triangle i's corners inside cell i % 16, drawn towards its centre -- a wrong row is a wrong cell
        torus = pt.Scene(os.path.join(SCENES, "mesh_small.txt")).meshes[4]
        c = np.arange(len(torus)) % 16
        centre = np.stack([(c % 4 + 0.5) / 4, 1 - (c // 4 + 0.5) / 4], 1)
        corners = centre[:, None, :] + np.array([[-.07, -.06], [.07, -.06], [0, .07]])[None]
        meshes[len(g)], uvs[len(g)] = torus, corners.reshape(-1, 6).astype(np.float32)
        g.append(orc.make_geom(2, 3, (0.2, 3.4, 1.0), (60, 10, 0), (4, 4, 4)))
        # a quad whose UVs are affine in object space and span every cell -- a swapped barycentric is another cell
        quad = np.array([[-.5, -.5, 0, .5, -.5, 0, .5, .5, 0], [-.5, -.5, 0, .5, .5, 0, -.5, .5, 0]], np.float32)
        xy = quad.reshape(2, 3, 3)[:, :, :2].astype(np.float64)
        quv = np.stack([0.06 + 0.88 * (xy[..., 0] + 0.5), 0.1 + 0.8 * (xy[..., 1] + 0.5)], -1)
        meshes[len(g)], uvs[len(g)] = quad, quv.reshape(2, 6).astype(np.float32)
        named["quad"] = len(g)
        g.append(orc.make_geom(2, 4, (0.5, 5.2, -3.8), (-10, 15, 8), (5.5, 4.5, 1)))
    geoms = np.concatenate(g).view(pt.GEOM_DTYPE)
    n = len(geoms)
    colours = cell_colours()
    textures = [cell_texture(c) for c in colours] + [ramp()]
    gb, scales = np.full(n, -1, np.int32), np.zeros(n, np.float32)
    if bump:
        for k, i in named.items():
            gb[i], scales[i] = 4, BUMP_SCALE[k]
    state = dict(first=0, dof=0, many=int(name.startswith("many")), sweptCubes=int(name.startswith("many")), mesh=int(name.endswith("mesh")),
                 grouped=0, tex=1, bump=int(bump), plain=0)
    return types.SimpleNamespace(geoms=geoms, materials=_materials(pt), camera=cam.camera.copy(), traceDepth=DEPTH, meshes=meshes, mesh_normals={},
                                 mesh_materials={}, mesh_uvs=uvs, textures=textures, geom_textures=(np.arange(n) % 4).astype(np.int32),
                                 geom_bumps=gb, bump_scales=scales, image=np.zeros((H, W, 3), np.float32), cells=colours, named=named, state=state)


def state_bits(state, **over):
    s = dict(state, **over)
    return sum(int(s[k]) << i for i, k in enumerate(STATE))


def twin_renderer(orc, sc, lens):
    """the CPU oracle on the untextured, unbumped twin: the same geometry and materials"""
    ref = orc.Renderer(sc.camera.view(orc.CAMERA_DTYPE), sc.geoms.view(orc.GEOM_DTYPE), sc.materials.view(orc.MATERIAL_DTYPE), DEPTH, meshes=sc.meshes)
    if lens:
        ref.set_extras(**LENS)
    return ref


def specs_of(sc):
    """(textures, 5): every texture's (W, H, cx, cy, margin) -- sc.specs, or SPEC for each of a scene that names none"""
    specs = getattr(sc, "specs", None)
    return np.array([SPEC] * max(len(sc.textures), 1) if specs is None else specs, np.float64).reshape(-1, 5)


def _classify(sc, o, d, white):
    """cast + (u, v) + cell: the unambiguous hits (indices into o), their hit records, texture, cell, texel colour and (u, v).  A scene
    with sc.specs has a spec per texture, and its UNBOUND primitives (texture -1) carry the texel 1 and leave nothing out; a scene
    without takes SPEC for every hit."""
    hit = pr.cast(sc, o, d)
    idx = np.flatnonzero((hit.prim >= 0) & ~hit.ambiguous)
    sub = pr.take(hit, idx)
    u, v, bad = pr.uv(sc, sub)
    tex = sc.geom_textures[sub.prim]
    if getattr(sc, "specs", None) is None:
        ci, border = pr.cell(SPEC, u, v)
        bound = np.ones(len(idx), bool)
    else:
        bound = tex >= 0
        sp = specs_of(sc)[np.maximum(tex, 0)]
        ci, border = pr.cell((sp[:, 0], sp[:, 1], sp[:, 2].astype(int), sp[:, 3].astype(int), sp[:, 4]), u, v)
    texel = np.ones((len(idx), 3), np.float32)
    if not white:
        texel[bound] = sc.cells[tex[bound], ci[bound]]
    return idx, sub, tex, ci, texel, u, v, (bad | border) & bound


def step(sc, prev, cur, white=False):
    """One bounce, k - 1 -> k.  prev, cur = (origin, direction, colour, pixel) of the paths alive after bounces k - 1 and k (pixels sorted).
    Returns the KEPT paths of `cur` (idx) with the colour predicted for them from prev's colours, and what the asserts of both tests read.
    `white`: every texel white (the untextured twin's colours) -- the cells still decide what is left out."""
    o0, d0, c0, p0 = prev
    o1, d1, c1, p1 = cur
    j = np.searchsorted(p0, p1)
    assert len(p1) == 0 or (j.max() < len(p0) and (p0[j] == p1).all()), "a path alive at bounce k was not alive at k - 1"
    idx, sub, tex, ci, texel, u, v, out = _classify(sc, o0[j], d0[j], white)
    Ns, bumped = None, np.zeros(len(idx), bool)
    if (sc.geom_bumps >= 0).any():
        bumped = sc.geom_bumps[sub.prim] >= 0
        Pu, Pv = pr.tangents(sc, sub)
        s = sc.bump_scales[sub.prim].astype(np.float64)
        # every height map a ramp: its slopes (sc.slopes per texture; SLOPE_U, SLOPE_V where the scene names none) and its own W and H
        hmap = np.maximum(sc.geom_bumps[sub.prim], 0)
        slopes = getattr(sc, "slopes", None)
        su, sv = (SLOPE_U, SLOPE_V) if slopes is None else (np.asarray(slopes, np.float64)[hmap, 0], np.asarray(slopes, np.float64)[hmap, 1])
        hw, hh = specs_of(sc)[hmap, 0], specs_of(sc)[hmap, 1]
        # (the tilt starts from the normal the hit is shaded with: a mesh's blended vertex normal where it has them)
        Ns, shaky = pr.tilt(sub.Ns, Pu, Pv, s * su, s * sv, sub.outside, sub.d)
        Ns = np.where(bumped[:, None], Ns, sub.Ns)
        # the ramp's wrap: the central differences reach one texel to each side and the sampler half a texel further; the sphere's seam
        # and poles, where (u, v) is singular
        badb = pr.uv(sc, sub)[2]
        x, y = (u - np.floor(u)) * hw, (v - np.floor(v)) * hh
        wrap = (np.minimum(x, hw - x) < 2.5) | (np.minimum(y, hh - y) < 2.5)
        flat = (s * su == 0) & (s * sv == 0)                               # (a zero scale, a constant map: the hit stays unbumped whatever (u, v))
        out = out | (bumped & ~flat & (shaky | wrap | badb))
    elif sub.blended.any():
        Ns = sub.Ns
    want, mirror, amb, side, off = pr.predict_colour(sc, sub, c0[j][idx], texel, o1[idx], d1[idx], Ns)
    # a half mirror with an exponent samples a lobe about the mirror's direction: its two branches cannot be told apart from the new state
    mats = sc.materials[sub.mat]
    amb = amb | ((mats[mats.dtype.names[1]] > 0) & (mats["hasReflective"] > 0) & (mats["hasRefractive"] == 0))
    keep = ~(out | amb)
    r = pr.take(sub, keep)
    return types.SimpleNamespace(idx=idx[keep], hit=r, col=c0[j][idx][keep], texel=texel[keep], want=want[keep], mirror=mirror[keep], side=side[keep], off=off[keep], tex=tex[keep], cell=ci[keep],
                                 Ns=None if Ns is None else Ns[keep], bumped=bumped[keep], live=len(p1), kept=int(keep.sum()))


def ended_on_light(sc, prev, cur, white=False):
    """The paths alive after bounce k - 1 and gone after bounce k whose float64 cast lands unambiguously on an emitter, clear of the cell
    borders: their pixels, and what each adds to its pixel (from prev's colours)."""
    o0, d0, c0, p0 = prev
    gone = np.flatnonzero(~np.isin(p0, cur[3]))
    idx, sub, tex, ci, texel, u, v, out = _classify(sc, o0[gone], d0[gone], white)
    emit = sc.materials["emittance"][sub.mat] > 0
    keep = emit & ~out
    return p0[gone][idx[keep]], pr.emitted(sc, pr.take(sub, keep), c0[gone][idx[keep]], texel[keep]), tex[keep], ci[keep]


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))
