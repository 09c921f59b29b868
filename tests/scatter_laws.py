"""Float64 LAWS for where a path goes next: the camera ray (L1), the diffuse hemisphere (L2), the REFL mixture (L3), the Phong lobe (L4), the
dielectric (L5), the direct-lighting ray (L6), the new origin (L7), the light's contribution (L8) and an exact furnace (L9) -- each read from
the renderer's own path state after every bounce (tests/test_scatter_laws_cpu.py: the CPU oracle's; tests/test_gpu_scatter_laws.py: the
MI355X's) -- and the denoiser's guide buffers (L10), which are the camera rays' hits.

Mesh attributes and switches.  Where a mesh carries vertex normals, L2 - L6 take the SHADING normal Ns of path_ref.cast (the float64 blend,
turned to its face's side, then to the ray's): the mirror direction and its lobe, Snell and Schlick's cosine, the hemisphere's (d' . Ns)^2,
its azimuth and tangent frame, the direct-lighting cosine.  Which side the ray came from (`outside`, eta) stays geometric; L7 puts the new
origin OFFSET along +-Ns and, with that, on the GEOMETRIC side its branch names.  A glass hit whose Ns faces away from the incoming ray
(Ns . d > -1e-3: Schlick's cosine leaves [0, 1]) is left out of the Fresnel and TIR statistics only -- counted, printed, under the
ambiguity cap -- and stays in the direction residuals.  Where a mesh carries face materials, every lookup goes by the FACE's material: L3's
and L5's branches, L8 (a path ends on a face iff that face's material emits, and adds (col * color) * emittance of that material; a dark
face of an emissive object lets it go on) and L6's emitters (a mesh whose object's material or any face's emits, through the box of all its
vertices).  Under the weighted mixture (PT_FLAG_MIXTURE_WEIGHTED) a REFL hit carries (col * 2) * specColor or (col * 2) * color, bit for
bit (the factor 2 is exact in any order); the share stays 1/2 and every other material carries what it carried.

Plain numpy.  Nothing of the library or the oracle is called: the ray cast is tests/path_ref.py's, and which branch a path took is read
from its new state (its colour, the side of the surface its new origin lies on), never from a random number.  A sampler is held to the
DISTRIBUTION the semantics promise (include/pt_amd.h, README.md): a transform of the new direction that must be uniform on (0, 1), a count
that must be binomial, a residual that must vanish.  What this cannot see: two samplers equal in law (sin and cos swapped in an azimuth).

Bounds.  KS: sqrt(n) D <= 1.95 (Kolmogorov's asymptotic tail 2 exp(-2 x^2) is 1.0e-3 there); z and |r| sqrt(n) <= 3.3 (the two-sided 1e-3
normal quantile).  Geometric tolerances: 1e-4 on directions (path_ref's: it covers the 1e-4 object-space SHORT), 1e-5 on the colour ratio,
1e-3 of slack on the emitter's box, 0.1 OFFSET on new origins; a sphere's hit takes what float32 leaves of its root where that is more (below)."""
import os
import types

import numpy as np

import path_ref as pr
import textured_scenes as ts
from conftest import SCENES

W, H, DEPTH = ts.W, ts.H, ts.DEPTH
KS_MAX, Z_MAX = 1.95, 3.3
DIR_TOL, RATIO_TOL, BOX_SLACK = 1e-4, 1e-5, 1e-3
# A SPHERE's hit is the root of a quadratic the renderer evaluates in float32 from the object-space origin ro (as the reference's
# sphereIntersectionTest does): its radicand is the difference of terms of size |ro|^2, so the root is off by some eps32 (1 + |ro|^2) / |N . d|
# in units of the radius, the normal and the new direction with it, and the new origin by some eps32 (1 + |ro|^2) x scale along N.  Measured on
# the CPU oracle over every case below (a room's sphere of scale 3 has |ro| = 4, one of the 128 of `grouped`, scale 0.6, |ro| = 25):
#   |d' - reference| |N . d| / (eps32 (1 + |ro|^2)) <= 53.6,   |origin residual| / (eps32 (1 + |ro|^2) scale) <= 22.8
# (the worst direction: 7.2e-3 at |N . d| = 0.053 in `grouped`, 3.1e-4 at 0.044 in `few`); cubes and triangles stay under 1.4e-6 and 3.6e-6.
# A sphere hit is allowed twice the measured worst where that exceeds the tolerance every other hit has.
EPS32, SPHERE_DIR, SPHERE_ORIGIN = 2.0 ** -24, 2 * 53.6, 2 * 22.8
# A BLENDED vertex normal is built from barycentrics the renderer evaluates in float32 (a second evaluation of the triangle test).  Measured
# on the CPU oracle over every hit of the cases with vertex normals (vn-smooth, vn-bent), the float32 shading normal against the float64 Ns of
# path_ref.cast: |Ns32 - Ns64| <= MEASURED_BLEND (largest component).  A direction behind such a normal is allowed twice that where it exceeds DIR_TOL.
MEASURED_BLEND = 1.83e-5                                    # (vn-bent; vn-smooth 1.71e-5, over 9531 and 7710 blended hits)
BLEND_TOL = max(DIR_TOL, 2 * MEASURED_BLEND)
SQRT13 = np.sqrt(1.0 / 3.0)
LENS = ts.LENS
FW, FH, FDEPTH, FITERS = 64, 48, 8, 8                       # the furnace (L9)
STATE = ts.STATE

# name: geometry, thin lens, direct lighting, iterations.  (Iteration numbers are fixed inputs: the renderer is deterministic.)
CASES = {
    "few":            dict(geometry="few", iters=(1, 37)),
    "plain":          dict(geometry="few", iters=(1, 37), no_glass=True),
    "many_mesh-lens": dict(geometry="many_mesh", iters=(1, 37), lens=True),
    "grouped":        dict(geometry="grouped", iters=(1, 37)),
    "glass":          dict(geometry="glass", iters=(1, 37, 2)),
    "phong":          dict(geometry="few", iters=(1, 37, 2, 3), specex=20.0),
    "many-direct":    dict(geometry="many", iters=(1, 37, 2), direct=True),
    "mesh-direct2":   dict(geometry="mesh", iters=(1, 37, 2), direct=True, second_emitter=True),
    # vertex normals (PtMesh::normals), face materials (PtMesh::materials), the weighted mixture (PT_FLAG_MIXTURE_WEIGHTED)
    "vn-smooth":       dict(geometry="vn-smooth", iters=(1, 37, 2), guides=True),
    "vn-bent":         dict(geometry="vn-bent", iters=(1, 37, 2), guides=True),
    "faces":           dict(geometry="faces", iters=(1, 37, 2), guides=True),
    "faces-direct":    dict(geometry="faces-direct", iters=(1, 37, 2), direct=True, guides=True),
    "face-light-only": dict(geometry="face-light-only", iters=(1, 37, 2), guides=True),
    "few-weighted":    dict(geometry="few", iters=(1, 37), weighted=True, guides=True),
    "mesh-weighted":   dict(geometry="mesh", iters=(1, 37), weighted=True, guides=True),
}
for _name in ("few", "many_mesh-lens", "grouped"):          # L10, the guide buffers, on three of the older cases too (the lens moves the origins)
    CASES[_name]["guides"] = True
CASES["grouped"]["guide_iters"] = (1,)                      # (the oracle's guides cost a call per pixel and primitive: one iteration of its 134)
FURNACES = ("furnace", "furnace-half")
DIAGONAL = 6                                                # the index of the cube every case adds behind the room's six (see build)


# ---------------------------------------------------------------------------------------------------------------- statistics
def ks(x):
    """the two-sided Kolmogorov statistic sqrt(n) D of a sample against U(0, 1)"""
    x = np.sort(np.asarray(x, np.float64).reshape(-1))
    n = len(x)
    i = np.arange(1, n + 1)
    return float(np.sqrt(n) * max((i / n - x).max(), (x - (i - 1) / n).max()))


def z(successes, probabilities):
    s, p = np.asarray(successes, np.float64), np.asarray(probabilities, np.float64)
    return float((s.sum() - p.sum()) / np.sqrt((p * (1 - p)).sum()))


def rsqrtn(a, b):
    """r sqrt(n) of the paired samples a, b"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.corrcoef(a, b)[0, 1] * np.sqrt(len(a)))


# ---------------------------------------------------------------------------------------------------------------- scenes
def _octahedron():
    """a closed mesh of eight triangles whose bounds are NOT centred on the origin: [-0.3, 0.5] x [-0.5, 0.4] x [-0.4, 0.5]"""
    px, nx, py, ny, pz, nz = (.5, 0, 0), (-.3, 0, 0), (0, .4, 0), (0, -.5, 0), (0, 0, .5), (0, 0, -.4)
    faces = [(px, py, pz), (py, nx, pz), (nx, ny, pz), (ny, px, pz), (py, px, nz), (nx, py, nz), (ny, nx, nz), (px, ny, nz)]
    return np.array(faces, np.float32).reshape(8, 9)


def _attribute_meshes(pt):
    """the small meshes of scenes/: the 80-triangle icosphere with its vertex normals, the 12-triangle cube with the face (0 .. 5: -x, +x, -y,
    +y, -z, +z) of each of its triangles"""
    a = pt.Scene(os.path.join(SCENES, "mesh_attributes.txt"))
    ico, radial, cube = a.meshes[3], a.mesh_normals[3], a.meshes[5]
    t = cube.reshape(-1, 3, 3).astype(np.float64)
    fn = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    axis = np.abs(fn).argmax(1)
    assert len(cube) == 12 and (np.sort(np.abs(fn), 1)[:, :2] == 0).all()
    return ico, radial, cube, 2 * axis + (fn[np.arange(12), axis] > 0)


def _bent(tris, rng):
    """vertex normals bent off the face normal per corner, as tests/test_gpu_fuzz.py draws them (the unit face normal plus a uniform
    vector), by 38.6 degrees at most: |the vector| <= 0.36 sqrt(3) = sin 38.6.  (L7's geometric side needs OFFSET (Ns . N) above the
    SHORT step's share along N, scale x 1e-4 at most: true of every object here up to a bend of 70 degrees, not beyond.)"""
    t = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    fn = pr._unit(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]))
    return pr._unit(fn[:, None, :] + rng.uniform(-0.36, 0.36, t.shape)).reshape(-1, 9).astype(np.float32)


def _attribute_scene(pt, orc, geometry):
    """the room and the meshes of the cases vn-smooth, vn-bent, faces, faces-direct and face-light-only:
    (geoms, materials, meshes, mesh_normals, mesh_materials, the geoms whose vertex normals are radial)"""
    ico, radial, cube, face = _attribute_meshes(pt)
    m = np.zeros(7, pt.MATERIAL_DTYPE)
    m[:6] = ts._materials(pt)
    m[6] = m[0]                                                       # 6: a second, dimmer and coloured emitter
    m["color"][6], m["emittance"][6] = (1.0, 0.8, 0.6), 3.0
    g, meshes, normals, mats, round_ = _room(orc), {}, {}, {}, []

    def add(tris, material, trans, rot, scale, vn=None, fm=None):
        k = len(g)
        meshes[k] = tris
        if vn is not None:
            normals[k] = vn
        if fm is not None:
            mats[k] = np.asarray(fm, np.int32)
        g.append(orc.make_geom(2, material, trans, rot, scale))
        return k

    if geometry in ("vn-smooth", "vn-bent"):
        # three large icospheres near the camera, as `glass` places its objects, under rotated, non-uniform scales: glass, REFL 1, diffuse
        rng = np.random.default_rng(7741)
        where = [(5, (-2.5, 3.6, 3.2), (10, 20, 30), (3.4, 2.8, 3.4)), (4, (2.6, 3.6, 3.4), (25, 35, 15), (3.0, 3.4, 2.6)),
                 (1, (0.2, 7.0, 0.5), (40, 10, 20), (3.2, 2.6, 3.0))]
        for material, trans, rot, scale in where:
            k = add(ico, material, trans, rot, scale, radial if geometry == "vn-smooth" else _bent(ico, rng))
            if geometry == "vn-smooth":
                round_.append(k)
        if geometry == "vn-bent":
            # every normal at the BACK of its face (the blend is turned), on a half mirror; every normal zero (the face normal is kept)
            add(ico, 4, (-3.2, 7.6, -1.6), (0, 30, 10), (2.6, 2.4, 2.6), -radial)
            add(_octahedron(), 1, (3.3, 7.7, -1.2), (20, 30, 0), (2.6, 2.6, 2.6), np.zeros((8, 9), np.float32))
    else:
        light_only = geometry == "face-light-only"
        if light_only:                                                # no ceiling light: its cube turns diffuse
            g[0] = orc.make_geom(1, 1, (0, 10, 0), (0, 0, 0), (4, .3, 4))
            fm = np.array([1, 1, 2, 0, 4, -1])[face]                  # the only emitter of the scene: the +y face of a diffuse cube
            add(cube, 1, (-1.6, 3.2, 2.6), (35, 30, 0), (4.2, 4.2, 4.2), fm=fm)
        else:
            # faces (-x .. +z): REFL 1, emissive, diffuse red, glass, diffuse green, -1 = the object's diffuse white
            add(cube, 1, (-2.4, 3.4, 3.2), (20, 35, 10), (3.0, 3.0, 3.0), fm=np.array([4, 0, 2, 5, 3, -1])[face])
            # ... and an EMISSIVE object (material 6) some of whose faces are not: diffuse white, REFL 1, -1, glass, -1, diffuse green
            add(cube, 6, (2.5, 3.4, 3.4), (-15, -30, 20), (2.8, 2.8, 2.8), fm=np.array([1, 4, -1, 5, -1, 3])[face])
        if geometry == "faces-direct":                                # a diffuse mesh next to the ceiling light whose only emitter is ONE face
            fm = np.full(8, -1)
            fm[3] = 0
            add(_octahedron(), 1, (-3.0, 7.6, -1.0), (20, 30, 0), (2.4, 2.4, 2.4), fm=fm)
    return g, m, meshes, normals, mats, round_


def _room(orc):
    return [orc.make_geom(1, 0, (0, 10, 0), (0, 0, 0), (4, .3, 4)),                   # 0 the light, 1-5 the Cornell walls: as textured_scenes.build
            orc.make_geom(1, 1, (0, 0, 0), (0, 0, 0), (10, .01, 10)),
            orc.make_geom(1, 1, (0, 10, 0), (0, 0, 90), (.01, 10, 10)),
            orc.make_geom(1, 1, (0, 5, -5), (0, 90, 0), (.01, 10, 10)),
            orc.make_geom(1, 2, (-5, 5, 0), (0, 0, 0), (.01, 10, 10)),
            orc.make_geom(1, 3, (5, 5, 0), (0, 0, 0), (.01, 10, 10))]


def _scene(pt, geoms, materials, meshes, state, w=W, h=H, depth=DEPTH, mesh_normals=None, mesh_materials=None):
    cam = pt.Scene(os.path.join(SCENES, "cornell.txt"))
    cam.set_resolution(w, h)
    geoms = np.concatenate(geoms).view(pt.GEOM_DTYPE) if isinstance(geoms, list) else geoms
    n = len(geoms)
    # (mesh_uvs: textured_scenes.ended_on_light asks for a mesh hit's texture cell; every corner sits in the middle of cell 0)
    return types.SimpleNamespace(geoms=geoms, materials=materials, camera=cam.camera.copy(), traceDepth=depth, meshes=meshes, mesh_normals=mesh_normals or {},
                                 mesh_materials=mesh_materials or {}, mesh_uvs={g: np.full((len(t), 6), 0.125, np.float32) for g, t in meshes.items()}, textures=[],
                                 geom_textures=np.full(n, -1, np.int32), geom_bumps=np.full(n, -1, np.int32), bump_scales=np.zeros(n, np.float32),
                                 image=np.zeros((h, w, 3), np.float32), state=state)


def build(pt, orc, name):
    """the scene of case `name` as pathtraceInit reads it, with .extras (pathtraceInit's / set_extras' keywords), .iters and .state"""
    if name in FURNACES:
        return _furnace(pt, orc, name)
    case = CASES[name]
    geometry = case["geometry"]
    state = dict(first=0, dof=int(bool(case.get("lens"))), many=0, sweptCubes=0, mesh=0, grouped=0, tex=0, bump=0, plain=0)
    mesh_normals, mesh_materials, radial = {}, {}, []
    if geometry in ("few", "many", "mesh", "many_mesh"):
        t = ts.build(pt, orc, geometry, False)
        geoms, materials, meshes = t.geoms, t.materials, t.meshes
        state.update(many=t.state["many"], sweptCubes=t.state["sweptCubes"], mesh=t.state["mesh"])
    elif geometry == "grouped":
        # kGroupedMin = 128 swept primitives (csrc/pt_trace.h; pt_init: no mesh, no texture, nswept >= kGroupedMin): the room and 128 spheres
        rng = np.random.default_rng(4128)
        g = _room(orc)
        for i in range(128):
            ix, iy, iz = i % 8, (i // 8) % 4, i // 32
            c = np.array([-4.2 + 1.2 * ix, 1.0 + 2.2 * iy, -4.0 + 2.4 * iz]) + rng.uniform(-.25, .25, 3)
            s = rng.uniform(.5, .8)
            g.append(orc.make_geom(0, (1, 2, 3, 4, 1, 4, 5, 1)[i % 8], tuple(c), tuple(rng.uniform(0, 90, 3)), (s, s * rng.uniform(.8, 1.2), s)))
        geoms, materials, meshes = g, ts._materials(pt), {}
        state.update(many=1, grouped=1)
    elif geometry == "glass":
        # a large glass sphere and a large, rotated glass cube near the camera: rays leave glass from inside at all angles
        g = _room(orc) + [orc.make_geom(0, 5, (-2.2, 3.6, 3.4), (0, 0, 0), (3.6, 3.6, 3.6)),
                          orc.make_geom(1, 5, (2.2, 3.4, 3.6), (25, 35, 15), (3.0, 3.0, 3.0)),
                          orc.make_geom(1, 1, (-0.5, 0.8, -1.5), (0, 30, 0), (1.6, 1.6, 1.6))]
        geoms, materials, meshes = g, ts._materials(pt), {}
    elif geometry in ("vn-smooth", "vn-bent", "faces", "faces-direct", "face-light-only"):
        geoms, materials, meshes, mesh_normals, mesh_materials, radial = _attribute_scene(pt, orc, geometry)
        state.update(mesh=1)
    else:
        raise KeyError(geometry)
    # one more diffuse cube in every scene, turned 45 degrees about z: its upper faces look along (+-1, 1, 0) / sqrt(2), the THIRD tangent
    # frame of the hemisphere sampler (|N.x| and |N.y| both >= sqrt(1/3)), which the other primitives reach with a few dozen hits only
    glist = geoms if isinstance(geoms, list) else [geoms[i:i + 1].view(orc.GEOM_DTYPE) for i in range(len(geoms))]
    meshes, mesh_normals, mesh_materials = ({g + 1 if g >= DIAGONAL else g: t for g, t in d.items()} for d in (meshes, mesh_normals, mesh_materials))
    radial = [g + 1 if g >= DIAGONAL else g for g in radial]
    geoms = glist[:DIAGONAL] + [orc.make_geom(1, 1, (0.3, 1.35, 2.3), (0, 0, 45), (1.8, 1.8, 1.8))] + glist[DIAGONAL:]
    materials = materials.copy()
    if case.get("no_glass"):                                          # the glass sphere turns diffuse: nothing takes the scatter's rarer branches
        materials[5] = materials[1]
    if case.get("specex"):
        materials[materials.dtype.names[1]][4] = case["specex"]
    if case.get("second_emitter"):                                    # an emissive mesh next to the emissive cube
        m = np.zeros(len(materials) + 1, materials.dtype)
        m[:-1] = materials
        m[-1] = materials[0]
        m["emittance"][-1] = 3.0
        materials = m
        glist = list(geoms)
        meshes = dict(meshes)
        meshes[len(glist)] = _octahedron()
        glist.append(orc.make_geom(2, len(m) - 1, (-3.4, 2.0, 1.6), (20, 30, 0), (2.2, 2.2, 2.2)))
        geoms = glist
    refr = (materials["hasRefractive"] > 0).any()
    spex = ((materials["hasReflective"] > 0) & (materials[materials.dtype.names[1]] > 0)).any()
    weighted = bool(case.get("weighted"))
    state["plain"] = int(not case.get("direct") and not refr and not spex and not weighted)
    sc = _scene(pt, geoms, materials, meshes, state, mesh_normals=mesh_normals, mesh_materials=mesh_materials)
    sc.name, sc.iters = name, case["iters"]
    # the weighted mixture is a flag of pathtraceInit (sc.init) and a study variant of the oracle (sc.variant: set_variant, not set_extras)
    sc.weighted, sc.init, sc.variant = weighted, (dict(mixture_weighted=True) if weighted else {}), (dict(mirror_mode=1) if weighted else {})
    sc.guide_iters, sc.radial = (case.get("guide_iters", case["iters"]) if case.get("guides") else ()), radial
    sc.extras = dict(LENS) if case.get("lens") else {}
    sc.lens = bool(case.get("lens"))
    sc.direct = bool(case.get("direct"))
    if sc.direct:
        sc.extras["direct_lighting"] = True
    return sc


def _furnace(pt, orc, name):
    """L9: an emissive cube of scale 40 and emittance 4 around the camera and the `few` objects, no other light; every colour and specular
    colour 1 (`furnace`) or every non-emissive one 1/2 (`furnace-half`)"""
    t = ts.build(pt, orc, "few", False)
    # (the room's walls without its light, the four objects, and the diagonal cube of build)
    glist = [orc.make_geom(1, 0, (0, 5, 0), (0, 0, 0), (40, 40, 40))] + [t.geoms[i:i + 1].view(orc.GEOM_DTYPE) for i in range(1, 10)]
    glist.append(orc.make_geom(1, 1, (0.3, 1.35, 2.3), (0, 0, 45), (1.8, 1.8, 1.8)))
    m = t.materials.copy()
    v = 1.0 if name == "furnace" else 0.5
    m["color"], m[m.dtype.names[2]] = v, v
    m["color"][0], m["emittance"][0] = 1.0, 4.0
    state = dict(first=0, dof=0, many=0, sweptCubes=0, mesh=0, grouped=0, tex=0, bump=0, plain=0)
    sc = _scene(pt, glist, m, {}, state, FW, FH, FDEPTH)
    sc.name, sc.iters, sc.extras, sc.lens, sc.direct, sc.value = name, tuple(range(1, FITERS + 1)), {}, False, False, v
    sc.weighted, sc.init, sc.variant, sc.guide_iters, sc.radial = False, {}, {}, (), []
    return sc


def state_bits(state, **over):
    return ts.state_bits(state, **over)


# ---------------------------------------------------------------------------------------------------------------- one bounce
def _mat(sc, hit):
    """the material record of every hit: the face's own where the mesh names one, else the object's (path_ref.cast's `mat`)"""
    return sc.materials[hit.mat]


def _origin_tol(sc, h, o):
    """(1 + |ro|^2 of the object-space origins, the tolerance of a new origin along the normal: see SPHERE_ORIGIN)"""
    inv = np.array([pr._m(G, "inverseTransform") for G in sc.geoms])[h.prim]
    ro = np.einsum("nij,nj->ni", inv[:, :3, :3], o.astype(np.float64)) + inv[:, :3, 3]
    ro2 = 1 + pr._dot(ro, ro)
    return ro2, np.where(h.kind == 0, np.maximum(0.1 * pr.OFFSET, SPHERE_ORIGIN * EPS32 * ro2 * sc.geoms["scale"][h.prim].max(1)), 0.1 * pr.OFFSET)


def step(sc, prev, cur):
    """One bounce, k - 1 -> k: the paths of `cur` whose float64 cast from `prev` is unambiguous, with the hit, the material (the FACE's), the
    state before and after (float64 directions normalised) and the branch read from the new state: `behind` (the new origin lies beyond the
    GEOMETRIC surface: refracted), `mirror` (the colour is col * specColor, bit for bit), `body` (the colour is col * color, bit for bit);
    under the weighted mixture a REFL material's two colours are (col * 2) * specColor and (col * 2) * color.  `off`: how far the new origin
    sits, along the SHADING normal, from OFFSET to its side of P - short; `off3`: the same as a vector."""
    o0, d0, c0, p0 = prev
    o1, d1, c1, p1 = cur
    j = np.searchsorted(p0, p1)
    assert len(p1) == 0 or (j.max() < len(p0) and (p0[j] == p1).all()), "a path alive at bounce k was not alive at k - 1"
    hit = pr.cast(sc, o0[j], d0[j], inside_cube=True)
    idx = np.flatnonzero((hit.prim >= 0) & ~hit.ambiguous)
    h = pr.take(hit, idx)
    m = _mat(sc, h)
    f = np.float32
    col = c0[j][idx].astype(f)
    refl = (m["hasRefractive"] == 0) & (m["hasReflective"] > 0)
    carried = np.where(refl[:, None], col * f(2), col) if sc.weighted else col       # (the 1 / p weight of either branch: exact)
    spec, body = carried * m[m.dtype.names[2]].astype(f), carried * m["color"].astype(f)
    got = c1[idx].astype(f)
    on = o1[idx].astype(np.float64)
    side = np.where(pr._dot(on - h.P, h.Ng) * np.where(h.outside, 1.0, -1.0) > 0, 1.0, -1.0)      # the GEOMETRIC side the new origin lies on
    ro2, origin_tol = _origin_tol(sc, h, o0[j][idx])
    off3 = on - (h.P - h.short + (side * pr.OFFSET)[:, None] * h.Ns)
    return types.SimpleNamespace(ro2=ro2, origin_tol=origin_tol,
        idx=idx, pix=p1[idx], hit=h, mat=m, col=col, got=got, d=pr._unit(h.d), dn=pr._unit(d1[idx].astype(np.float64)), on=on,
        glass=m["hasRefractive"] > 0, refl=refl, specex=m[m.dtype.names[1]].astype(np.float64),
        mirror=(got.view(np.uint32) == spec.view(np.uint32)).all(1), body=(got.view(np.uint32) == body.view(np.uint32)).all(1),
        behind=side < 0, off=pr._dot(off3, h.Ns), off3=off3, emits=m["emittance"] > 0, live=len(p1), kept=len(idx))


# ---------------------------------------------------------------------------------------------------------------- the laws
def camera_law(sc, rays):
    """L1.  Returns (jx, jy) -- the fractional offsets of every ray inside its pixel -- and for a thin lens ((r / R)^2, angle / 2 pi)."""
    o, d, _, pix = rays
    cam = sc.camera[0] if sc.camera.shape else sc.camera
    eye32 = np.asarray(cam["position"], np.float32)
    eye, view, up = (np.asarray(cam[k], np.float64) for k in ("position", "view", "up"))
    w, h = (int(v) for v in cam["resolution"])
    fx, fy = (np.tan(np.radians(float(v))) for v in cam["fov"])
    right = pr._unit(np.cross(view, up))
    vn = pr._unit(view)
    o, d = o.astype(np.float64), d.astype(np.float64)
    lens = None
    if sc.lens:
        R, fd = sc.extras["lens_radius"], sc.extras["focal_distance"]
        e = o - eye
        assert np.abs(e @ vn).max() < 1e-5, np.abs(e @ vn).max()             # in the plane through the eye normal to `view`
        r = np.linalg.norm(e, axis=1)
        assert r.max() <= R * (1 + 1e-5), r.max()
        lens = ((r / R) ** 2, (np.arctan2(e @ up, e @ right) / (2 * np.pi)) % 1.0)
        t = (fd - e @ vn) / (d @ vn)
        point = o + t[:, None] * d                                           # the ray's point on the focal plane
    else:
        assert ts.same(rays[0], np.broadcast_to(eye32, rays[0].shape)), "a pinhole ray does not start at the eye"
        point = o + d
    # point - eye = s (view - a right - b up): a, b are the screen coordinates in units of tan(fov)
    s = np.linalg.solve(np.stack([view, right, up], 1), (point - eye).T).T
    a, b = -s[:, 1] / s[:, 0], -s[:, 2] / s[:, 0]
    jx = a / (2 * fx / w) + w / 2 - pix % w
    jy = b / (2 * fy / h) + h / 2 - pix // w
    assert jx.min() >= -1e-3 and jx.max() <= 1 + 1e-3 and jy.min() >= -1e-3 and jy.max() <= 1 + 1e-3, (jx.min(), jx.max(), jy.min(), jy.max())
    return np.clip(jx, 0, 1), np.clip(jy, 0, 1), lens


def frame_branch(N):
    """which of the three tangent frames the hemisphere sampler takes for normal N"""
    return np.where(np.abs(N[:, 0]) < SQRT13, 0, np.where(np.abs(N[:, 1]) < SQRT13, 1, 2))


def azimuth(N, v):
    """the azimuth / 2 pi of v about N, in a frame built from N alone (its axis of smallest |component|)"""
    e = np.eye(3)[np.abs(N).argmin(1)]
    t = pr._unit(np.cross(N, e))
    b = np.cross(N, t)
    return (np.arctan2(pr._dot(v, b), pr._dot(v, t)) / (2 * np.pi)) % 1.0


def snell(d, N, ior, outside):
    """(eta, k, refracted direction (NaN where k < 0), Schlick's F with the incident cosine when entering and sqrt(k) when leaving)"""
    eta = np.where(outside, 1.0 / ior, ior)
    c = -pr._dot(N, d)
    k = 1 - eta * eta * (1 - c * c)
    with np.errstate(all="ignore"):
        rk = np.sqrt(k)
        t = eta[:, None] * d + (eta * c - rk)[:, None] * N
        r0 = ((1 - ior) / (1 + ior)) ** 2
        F = r0 + (1 - r0) * (1 - np.where(outside, c, rk)) ** 5
    return eta, k, t, F


def emitters(sc):
    """the direct-lighting bounce's emitters in file order: (geom, object-space centre, extent, rho^2 = |scale x extent|^2 / 4).  A mesh is
    an emitter when its object's material or ANY face's emits; its box is the bounds of ALL its vertices either way."""
    out = []
    for g in range(len(sc.geoms)):
        used = [int(sc.geoms["materialid"][g])]
        if int(sc.geoms["type"][g]) == 2:
            used += [int(k) for k in np.unique(sc.mesh_materials.get(g, [])) if k >= 0]
        if not (sc.materials["emittance"][used] > 0).any():
            continue
        c, e = np.zeros(3), np.ones(3)
        if int(sc.geoms["type"][g]) == 2:
            v = np.asarray(sc.meshes[g], np.float64).reshape(-1, 3)
            c, e = (v.min(0) + v.max(0)) / 2, v.max(0) - v.min(0)
        out.append((g, c, e, ((np.asarray(sc.geoms["scale"][g], np.float64) * e) ** 2).sum() / 4))
    return out


def light_law(sc, s, sel):
    """L6 on the kept diffuse hits `sel` of the last bounce.  Returns (emitter index per aimed point or -1 where the point is not
    recoverable, u + 1/2 (n, 3) in that emitter's box, mask: every corner of that box in front of the surface and the box beyond rho, mask:
    the same of every emitter's box, the number of points that lie in two boxes)."""
    mcol = s.mat["color"][sel].astype(np.float32)
    with np.errstate(all="ignore"):
        ratio = (s.got[sel].astype(np.float64) / (s.col[sel] * mcol).astype(np.float64))
    wgt = ratio.mean(1)
    assert (np.abs(ratio - wgt[:, None]) <= RATIO_TOL * np.abs(wgt)[:, None]).all(), "the three channels carry different weights"
    N, dn, on = s.hit.Ns[sel], s.dn[sel], s.on[sel]                        # (the cosine is the shading normal's)
    cos = pr._dot(N, dn)
    assert (wgt >= 0).all() and (wgt <= np.maximum(cos, 0) * (1 + 1e-5) + 1e-7).all(), "a weight above max(0, N . d')"
    assert (wgt[cos <= -1e-6] == 0).all(), "light from below the surface"
    with np.errstate(all="ignore"):
        cover = wgt / cos
    rec = (cos > 1e-3) & (cover < 0.999)
    n = len(wgt)
    which, uu, clear = np.full(n, -1), np.zeros((n, 3)), np.zeros(n, bool)
    inside = []
    for g, c, e, rho2 in emitters(sc):
        inv, xf = pr._m(sc.geoms[g], "inverseTransform"), pr._m(sc.geoms[g], "transform")
        with np.errstate(all="ignore"):
            target = on + dn * np.sqrt(rho2 / cover)[:, None]
        u = ((target @ inv[:3, :3].T + inv[:3, 3]) - c) / e
        corners = (c + e * (np.array([[i, j, k] for i in (-.5, .5) for j in (-.5, .5) for k in (-.5, .5)]))) @ xf[:3, :3].T + xf[:3, 3]
        front = (np.einsum("cni,ni->cn", corners[:, None, :] - on[None], N) > 0).all(0)
        far = np.linalg.norm(on - (c @ xf[:3, :3].T + xf[:3, 3]), axis=1) > 2.002 * np.sqrt(rho2)
        inside.append((rec & (np.abs(u) <= 0.5 + BOX_SLACK).all(1), u, front & far))
    count = sum(i[0].astype(int) for i in inside)
    assert (count[rec] >= 1).all(), ("an aimed point outside every emitter's box", int((count[rec] == 0).sum()),
                                     [np.abs(i[1][rec & (count == 0)]).max(initial=0) for i in inside])
    for e, (ins, u, ok) in enumerate(inside):
        m = ins & (count == 1)
        which[m], uu[m], clear[m] = e, u[m] + 0.5, ok[m]
    # (where EVERY emitter's box is clear, whichever was chosen shows: the selection no longer depends on the choice)
    return which, uu, clear, np.all([i[2] for i in inside], 0), int((rec & (count > 1)).sum())


def _dir_tol(h, d, ro2):
    """the tolerance of a direction built from the hit's shading normal: DIR_TOL; a sphere's SPHERE_DIR allowance; BLEND_TOL behind a
    blended vertex normal"""
    with np.errstate(all="ignore"):
        sphere = np.maximum(DIR_TOL, SPHERE_DIR * EPS32 * ro2 / np.abs(pr._dot(d, h.N)))
    return np.where(h.kind == 0, sphere, np.where(h.blended, BLEND_TOL, DIR_TOL))


def guide_law(sc, rays, guides, say=print):
    """L10: the denoiser's guide buffers (pos_t, normal, geom) of one iteration against the float64 cast of its camera rays `rays`.  Returns
    (unambiguous hits, misses, the worst position and normal residuals as shares of their tolerances)."""
    o, d, _, pix = rays
    pos_t, nrm, geom = (np.asarray(a) for a in guides)
    assert len(pix) == len(geom) and (pix == np.arange(len(pix))).all()
    hit = pr.cast(sc, o, d)
    miss = hit.prim < 0
    assert (geom[miss] == -1).all() and (pos_t[miss] == np.array([0, 0, 0, -1], np.float32)).all() and (nrm[miss] == 0).all(), "L10: a miss"
    idx = np.flatnonzero(~miss & ~hit.ambiguous)
    h = pr.take(hit, idx)
    assert (~miss).sum() - len(idx) <= (~miss).sum() / 4 and len(idx) >= 200, (len(idx), int((~miss).sum()))         # the ambiguity cap
    assert (geom[idx] == h.prim).all(), ("L10: another primitive", int((geom[idx] != h.prim).sum()))
    ro2, tol = _origin_tol(sc, h, o[idx])
    # (a sphere's allowance is its root's, seen ALONG the normal: the point itself moves along the ray, 1 / |N . d| as far)
    cosi = np.abs(pr._dot(pr._unit(h.d), h.N))
    tol = np.where(h.kind == 0, tol / np.maximum(cosi, 1e-3), tol)
    want = h.P - h.short
    rp = np.abs(pos_t[idx, :3].astype(np.float64) - want).max(1) / tol
    rt = np.abs(pos_t[idx, 3].astype(np.float64) - np.linalg.norm(want - o[idx].astype(np.float64), axis=1)) / tol
    rn = np.abs(nrm[idx].astype(np.float64) - h.Ns).max(1) / _dir_tol(h, pr._unit(h.d), ro2)
    say("%s: L10 %d hits, %d misses, residuals / tolerance: position %.3g, distance %.3g, normal %.3g" % (sc.name, len(idx), int(miss.sum()), rp.max(), rt.max(), rn.max()))
    assert rp.max() < 1 and rt.max() < 1, ("L10: the guide position", rp.max(), rt.max())
    assert rn.max() < 1, ("L10: the guide normal", rn.max(), h.prim[rn.argmax()])
    return len(idx), int(miss.sum()), float(max(rp.max(), rt.max())), float(rn.max())


def _residual(s, m, want):
    """the worst |new direction - want| over the hits m, as a share of its tolerance"""
    if not m.any():
        return 0.0
    return float((np.abs(s.dn[m] - want[m]).max(1) / _dir_tol(s.hit, s.d, s.ro2)[m]).max())


def gone_law(sc, prev, cur):
    """L8's other half: of the paths alive after bounce k - 1 and gone after bounce k, those whose float64 cast lands unambiguously on a
    face -- (how many of them on an emissive one, how many on one that does not emit: a path that ended where it should have gone on, how
    many on an emissive face of a mesh with face materials)"""
    o0, d0, _, p0 = prev
    gone = ~np.isin(p0, cur[3])
    hit = pr.cast(sc, o0[gone], d0[gone], inside_cube=True)
    ok = (hit.prim >= 0) & ~hit.ambiguous
    emits = sc.materials["emittance"][hit.mat] > 0
    return int((ok & emits).sum()), int((ok & ~emits).sum()), int((ok & emits & np.isin(hit.prim, list(sc.mesh_materials))).sum())


def radial_law(sc, h):
    """vn-smooth's second statement: the icosphere's vertex normals are its vertices' directions, so the object-space blend is parallel to
    the hit point ON the triangle -- the shading normal is that point through the inverse transpose, whatever the barycentrics were"""
    m = np.isin(h.prim, sc.radial)
    if not m.any():
        return 0.0
    inv = np.array([pr._m(G, "inverseTransform")[:3, :3] for G in sc.geoms])[h.prim[m]]
    q = h.q[m] + pr.SHORT * pr._unit(np.einsum("nij,nj->ni", inv, h.d[m]))
    w = pr._unit(np.einsum("nji,nj->ni", inv, q))
    w = np.where(h.outside[m, None], w, -w)
    return float(np.abs(w - h.Ns[m]).max())


def run(sc, paths, frame, say=print, guides=None):
    """Every law of the case `sc` on `paths` ({iteration: [(origin, direction, colour, pixel) after k = 0 .. depth bounces]}), `frame`
    (the accumulator after sc.iters[0] alone, (pixels, 3)) and, for L10, `guides` ({iteration: (pos_t, normal, geom)}: the denoiser's guide
    buffers).  Asserts them, and returns the statistics it measured."""
    depth = sc.traceDepth
    jit, lens = [], []
    diff = {b: [] for b in range(3)}                                   # per tangent-frame branch: ((d' . N)^2, azimuth)
    lag_pix, lag_bounce = [], []
    mix = []
    phong = []
    fres = {True: [], False: []}                                       # entering / leaving: (reflected, F)
    tir, worst_dir, worst_off = 0, 0.0, 0.0
    aimed, picks, overlaps = {}, [], 0
    on_light, shares = 0, []
    away_all, ended_lit, ended_dark, own_face, dark_face, worst_radial, g10 = 0, 0, 0, 0, 0, 0.0, []
    objmat = np.asarray(sc.geoms["materialid"], np.int64)
    lit_objects = bool(sc.mesh_materials) and any(sc.materials["emittance"][objmat[g]] > 0 for g in sc.mesh_materials)
    assert sorted(guides or {}) == sorted(sc.guide_iters)
    em = emitters(sc)
    for it in sc.iters:
        P = paths[it]
        assert len(P[0][3]) == W * H and (P[0][2] == 1).all()
        jx, jy, ln = camera_law(sc, P[0])
        jit.append((jx, jy))
        if it in sc.guide_iters:                                       # L10: the denoiser's guides are this iteration's camera rays' hits
            g10.append(guide_law(sc, P[0], guides[it], say))
        if ln is not None:
            lens.append(ln)
        before = None
        for k in range(1, depth + 1):
            s = step(sc, P[k - 1], P[k])
            aiming = sc.direct and k == depth
            N, d, dn = s.hit.Ns, s.d, s.dn                             # N: the SHADING normal (the geometric one but for blended vertex normals)
            # a glass hit whose shading normal faces away from the incoming ray: out of the Fresnel and TIR statistics, under the cap
            away = s.glass & (pr._dot(N, d) > -1e-3)
            away_all += int(away.sum())
            shares.append(1 - (s.kept - int(away.sum())) / max(s.live, 1))
            say("%s it %d bounce %d: live %d kept %d, glass under a normal that faces away %d (left out %.1f %%)" % (sc.name, it, k, s.live, s.kept, away.sum(), 100 * shares[-1]))
            assert s.live - s.kept + away.sum() <= s.live / 4, (it, k, s.live, s.kept, away.sum())        # the ambiguity cap
            assert s.kept >= 200, (it, k, s.kept)
            # L7: the new origin sits OFFSET along +-Ns from P - short -- and with that on the GEOMETRIC side its branch claims (s.behind, below)
            worst_off = max(worst_off, float(np.abs(s.off).max()))
            assert (np.abs(s.off) < s.origin_tol).all(), (it, k, np.abs(s.off).max())
            bl = s.hit.blended
            assert (np.abs(s.off3[bl]).max(1, initial=0) < s.origin_tol[bl]).all(), (it, k, "a new origin off the line along the blended normal")
            worst_radial = max(worst_radial, radial_law(sc, s.hit))
            # L8: no path lives on after an emissive face; none ends on a dark one (the last bounce apart: the renderer need not trace a path
            # that cannot reach an emitter any more, include/pt_amd.h PtCounters::misses)
            assert not s.emits.any(), (it, k, "a path went on from an emissive face", int(s.emits.sum()))
            _, dark, lit = gone_law(sc, P[k - 1], P[k])
            ended_lit += lit
            if k < depth:
                ended_dark += dark
            own_face += int((s.hit.mat != objmat[s.hit.prim]).sum())
            dark_face += int((sc.materials["emittance"][objmat[s.hit.prim]] > 0).sum())
            R = pr.reflect(d, N)
            # ---- the dielectric (L5)
            g = s.glass
            assert not (g & s.behind & ~s.body).any() and not (g & ~s.behind & ~s.mirror).any(), (it, k, "glass: colour and side disagree")
            assert not (~g & s.behind).any(), (it, k, "an opaque surface let a path through")
            ior = s.mat["indexOfRefraction"].astype(np.float64)
            with np.errstate(all="ignore"):
                eta, kk, T, F = snell(d, N, np.where(g, ior, 1.5), s.hit.outside)
            sure = g & (np.abs(kk) >= 1e-4)
            assert not (sure & (kk < 0) & s.behind).any(), (it, k, "refraction beyond the critical angle")
            tir += int((sure & (kk < 0) & ~away).sum())
            worst_dir = max(worst_dir, _residual(s, sure & ~s.behind, R), _residual(s, sure & s.behind, T))
            for entering in (True, False):
                m = sure & (kk > 0) & (s.hit.outside == entering) & ~away
                fres[entering].append((~s.behind[m], F[m]))
            # ---- the REFL mixture (L3) and the Phong lobe (L4)
            r = s.refl
            mirror = r & s.mirror
            if not aiming:
                assert not (r & ~s.mirror & ~s.body).any(), (it, k, "REFL: neither the mirror's colour nor the diffuse one")
            assert not (r & s.mirror & s.body).any()
            mix.append(mirror[r])
            worst_dir = max(worst_dir, _residual(s, mirror & (s.specex == 0), R))
            m = mirror & (s.specex > 0)
            if m.any():
                n1 = s.specex[m] + 1
                amax = np.arccos(1e-3 ** (1 / n1))
                whole = np.arccos(np.clip(pr._dot(R[m], N[m]), -1, 1)) + amax < np.pi / 2
                assert (pr._dot(dn[m], N[m]) > -1e-6).all(), (it, k, "a lobe sample below the surface")
                phong.append((np.clip(pr._dot(dn[m], R[m]), 0, 1) ** n1)[whole])
            # ---- the diffuse branch: the hemisphere (L2) or the ray to a light (L6)
            df = ~g & ~mirror
            if not aiming:
                assert s.body[df].all(), (it, k, "a diffuse path that does not carry col * color")
                cosn = pr._dot(dn[df], N[df])
                assert (cosn > 0).all(), (it, k, cosn.min())
                u1, az, br = cosn ** 2, azimuth(N[df], dn[df]), frame_branch(N[df])
                for b in range(3):
                    diff[b].append((u1[br == b], az[br == b]))
                pix = s.pix[df]
                nb = np.flatnonzero(np.diff(pix) == 1)
                lag_pix.append((u1[nb], u1[nb + 1]))
                if before is not None:
                    _, ia, ib = np.intersect1d(before[0], pix, return_indices=True)
                    lag_bounce.append((before[1][ia], u1[ib]))
                before = (pix, u1)
            else:
                sel = np.flatnonzero(df)
                which, uu, clear, allclear, both = light_law(sc, s, sel)
                overlaps += both
                assert (which[allclear] >= 0).sum() + both >= allclear.sum(), (it, k, "a point aimed at a box in full view was not recovered")
                picks.append(which[(which >= 0) & allclear])
                for e in range(len(em)):
                    aimed.setdefault(e, []).append(uu[(which == e) & clear])
            # ---- L8: a path that ends on the light leaves (col * color) * emittance in its pixel
            if it == sc.iters[0]:
                lp, add, _, _ = ts.ended_on_light(sc, P[k - 1], P[k], white=True)
                assert ts.same(frame[lp], add), (k, len(lp), np.flatnonzero((frame[lp] != add).any(1))[:5])
                on_light += len(lp)
    st = {"left out (worst bounce)": max(shares), "left out (mean)": float(np.mean(shares)), "new origin residual": worst_off, "direction residual / tolerance": worst_dir}

    def bound(name, value, limit):
        st[name] = value
        say("%s: %s = %.3g (limit %.3g)" % (sc.name, name, value, limit))
        assert abs(value) <= limit, (sc.name, name, value, limit)

    def atleast(name, value, floor):
        st[name] = value
        say("%s: %s = %d (at least %d)" % (sc.name, name, value, floor))
        assert value >= floor, (sc.name, name, value, floor)

    assert worst_dir < 1, worst_dir                                     # mirror, reflected and refracted directions (L3, L5)
    assert ended_dark == 0, ("L8: paths that ended on a face that does not emit", ended_dark)
    say("%s: glass hits under a shading normal that faces away from the ray, out of the L5 statistics: %d" % (sc.name, away_all))
    st["glass hits under a normal that faces away"] = away_all
    if sc.radial:
        bound("vn radial normals: |Ns - the hit point's direction|", worst_radial, 1e-5)
    if sc.mesh_materials:
        atleast("L8 hits that scatter by a face's own material", own_face, 300)
        atleast("L8 paths that end on a mesh with face materials", ended_lit, 300)
    if lit_objects:
        atleast("L8 paths that go on from a dark face of an emissive object", dark_face, 300)
    if g10:
        st["L10 hits"], st["L10 misses"] = sum(x[0] for x in g10), sum(x[1] for x in g10)
        st["L10 position residual / tolerance"], st["L10 normal residual / tolerance"] = max(x[2] for x in g10), max(x[3] for x in g10)
    jx, jy = np.concatenate([j[0] for j in jit]), np.concatenate([j[1] for j in jit])
    bound("L1 jitter x KS", ks(jx), KS_MAX)
    bound("L1 jitter y KS", ks(jy), KS_MAX)
    bound("L1 jitter x-y r sqrt(n)", rsqrtn(jx, jy), Z_MAX)
    if lens:
        bound("L1 lens r^2 KS", ks(np.concatenate([l[0] for l in lens])), KS_MAX)
        bound("L1 lens angle KS", ks(np.concatenate([l[1] for l in lens])), KS_MAX)
    for b in range(3):
        u1, az = np.concatenate([x[0] for x in diff[b]]), np.concatenate([x[1] for x in diff[b]])
        atleast("L2 frame %d hits" % b, len(u1), 300)
        bound("L2 frame %d cos^2 KS" % b, ks(u1), KS_MAX)
        bound("L2 frame %d azimuth KS" % b, ks(az), KS_MAX)
    bound("L2 lag-1 pixels r sqrt(n)", rsqrtn(np.concatenate([x[0] for x in lag_pix]), np.concatenate([x[1] for x in lag_pix])), Z_MAX)
    bound("L2 lag-1 bounces r sqrt(n)", rsqrtn(np.concatenate([x[0] for x in lag_bounce]), np.concatenate([x[1] for x in lag_bounce])), Z_MAX)
    mixed = np.concatenate(mix)
    if len(mixed):
        atleast("L3 REFL hits", len(mixed), 300)
        bound("L3 mirror share z", z(mixed, np.full(len(mixed), 0.5)), Z_MAX)
    if phong:
        x = np.concatenate(phong)
        atleast("L4 lobe samples", len(x), 300)
        bound("L4 lobe cos^(n+1) KS", ks(x), KS_MAX + 1e-3 * np.sqrt(len(x)))
    if sc.name == "glass":
        atleast("L5 total internal reflections", tir, 100)
    both = [np.concatenate([x[i] for e in fres for x in fres[e]]) for i in (0, 1)]
    if len(both[0]) >= 300:
        bound("L5 Fresnel z", z(*both), Z_MAX)
    for entering in (True, False):
        refl, F = (np.concatenate([x[i] for x in fres[entering]]) for i in (0, 1))
        if sc.name == "glass":
            atleast("L5 reflected, %s" % ("entering" if entering else "leaving"), int(refl.sum()), 150)
        if refl.sum() >= 150:
            bound("L5 Fresnel z, %s" % ("entering" if entering else "leaving"), z(refl, F), Z_MAX)
    if sc.direct:
        pk = np.concatenate(picks)
        say("%s: L6 aimed points inside two emitters' boxes, left out: %d of %d" % (sc.name, overlaps, len(pk) + overlaps))
        assert overlaps <= len(pk) / 20, (overlaps, len(pk))
        if len(em) > 1:
            atleast("L6 aimed points", len(pk), 300)
            bound("L6 emitter share z", z(pk == 0, np.full(len(pk), 1.0 / len(em))), Z_MAX)
            for e in range(1, len(em) - 1):                             # (with more than two emitters: every one's share)
                bound("L6 emitter %d share z" % e, z(pk == e, np.full(len(pk), 1.0 / len(em))), Z_MAX)
        for e in range(len(em)):
            u = np.concatenate(aimed[e])
            atleast("L6 emitter %d clear points" % e, len(u), 300)
            for a in range(3):
                bound("L6 emitter %d axis %s KS" % (e, "xyz"[a]), ks(np.clip(u[:, a], 0, 1)), KS_MAX)
    atleast("L8 paths that end on the light", on_light, 300)
    return st


# ---------------------------------------------------------------------------------------------------------------- the furnace (L9)
def furnace(sc, paths, frame, misses, say=print):
    """L9, exact.  paths[it][k]: the state after k bounces; frame: the accumulator after all of sc.iters, (pixels, 3)."""
    n = FW * FH
    assert misses == 0, misses
    want = np.zeros(n, np.float64)
    unfinished = 0
    for it in sc.iters:
        P = paths[it]
        assert len(P[0][3]) == n
        for k in range(1, sc.traceDepth + 1):
            gone = P[k - 1][3][~np.isin(P[k - 1][3], P[k][3])]         # finished at bounce k: survived k - 1 bounces, then the light
            assert np.isin(P[k][3], P[k - 1][3]).all()
            np.add.at(want, gone, 4.0 * sc.value ** (k - 1))
        unfinished += len(P[sc.traceDepth][3])
    say("%s: %d unfinished of %d paths" % (sc.name, unfinished, n * len(sc.iters)))
    assert unfinished > 0
    if sc.value == 1.0:                                                 # every pixel 4 (iterations - unfinished), in all three channels
        left = np.zeros(n, np.int64)
        for it in sc.iters:
            np.add.at(left, paths[it][sc.traceDepth][3], 1)
        assert np.array_equal(want, 4.0 * (len(sc.iters) - left))
    want = np.repeat(want.astype(np.float32)[:, None], 3, 1)
    assert ts.same(frame, want), (int((frame != want).any(1).sum()), frame[(frame != want).any(1)][:3], want[(frame != want).any(1)][:3])
    return unfinished
