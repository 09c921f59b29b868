"""Small meshes built on purpose to be hard on the hierarchy walks (ptd::meshIntersectionTest, k_mesh_walk), the CPU copy of the walk, the
hierarchy's invariant checker, and a float64 cast of rays at one mesh.  The generators are seeded, plain numpy; nothing of the library or
the oracle is called in them.  Used by tests/test_adversarial_meshes_cpu.py, tests/test_gpu_adversarial_meshes.py and tests/test_mesh_cpu.py.

Every family is a types.SimpleNamespace(name, tris (n, 9) float32, mats (n,) int32 face materials or None, rays(n) -> (o, d) float64 rays in
OBJECT space (to_world() takes them to a geom's world space), rays64(n): the ray maker of the float64 check, transform = (translation, rotation,
scale) of the geom the per-ray tests put the mesh under):

  lattice       8 x 8 unit squares in z = 0, two right triangles each, integer vertices, shuffled file order, a random first vertex.  Rays
                (0, 0, -1) from z = 4 on the quarter grid: interiors, edges, the diagonal, lattice vertices (six triangles meet).  Every fp32
                operation of the triangle test is exact there, so the answer is known in INTEGER arithmetic (lattice_answers): the closed
                triangles that hold the point, the lowest file index among them.  Pins the tie rule `(t == tbest) & (tri < best)`.
  lattice-dup   + an exact copy of every triangle at index + 128 with another face material (bit-identical arithmetic: every hit ties).
  lattice-flip  + the copies with reversed winding; which of a pair comes first in the file is random: `outside` is the WINNER's winding.
  comb          teeth square to the x axis, positions x_k = 8 ((k + 1) / n)^a, sizes the local spacing: the surface-area splits come out
                lopsided and the stack need large.  COMB_A (4096 teeth, a = 6): natural need 23, the largest found at or below the threshold
                of 24.  The search (one-axis power laws a = 1.5 .. 20 and geometric progressions r = 0.5 .. 0.99 at 64 .. 4096 teeth with sizes
                0.05 .. 20 spacings, and a recursive 1/8 : 7/8 construction) found NO mesh of at most 4096 triangles with a natural need
                above 24 -- the builder refuses splits below an eighth, and the largest need met was 23 --, so the median rebuild is reached
                as before, through PT_AMD_MESH_STACK_MAX: COMB_B (512 teeth, a = 7, natural need 20).  Rays along the axis pass both
                children at every level: they fill a lane's stack to the need.
  soup          8 triangles that span the whole box, 300 small ones, 16 slivers (aspect 1e4), 8 with |det| just under kMeshEps for typical
                rays, 8 degenerate (two or three equal vertices): walks of very unequal length within one wave.
  outlier       200 triangles of size 1e-2 near the origin and one at 3e4: the margin is 0.3, every small box is mostly margin.
  cocentric     65 triangles whose boxes share one centre exactly: no SAH axis, the median fallback is decided by the file index.
  stacked       (scene level: stacked_scene) 24 or 40 mesh geoms, each a 32-triangle lattice patch, concentric, slightly scaled and tilted, two
                pairs exactly coincident with different materials: a quarter tile queues 64 x 24 jobs against a queue of 128, and the
                coincident pairs tie in world distance -- the atomic minimum's low word (file order) decides.

The float64 check (mesh_cast): tolerances per family, TOL = twice the oracle's worst deviation from float64 over the unambiguous hits of the
float64 check's own rays (rays64(1024)) and of the per-ray GPU tests' rays (per_ray_set), measured by
tests/test_adversarial_meshes_cpu.py::test_float64_cast_against_the_oracle (t and the point, relative to max(1, |origin|, t, |point|)):
    family      measured t    measured point   allowed t   allowed point
    comb        9.5e-06       6.4e-06          1.9e-05     1.3e-05        (the worse of comb and comb-b)
    soup        3.4e-06       3.1e-06          6.8e-06     6.2e-06
    outlier     2.3e-05       2.0e-05          4.6e-05     4.0e-05
    cocentric   1.3e-05       9.6e-06          2.6e-05     2.0e-05
Ambiguous rays: at most 25 % of rays64(1024) (comb 5.2 %, comb-b 0.1 %, soup 14.6 %, outlier 22.0 %, cocentric 0.1 %).  The per-ray set is half
rays64 and half the adversarial mix, which the reference may flag wholesale (the comb's axis rays graze every hypotenuse; every hit of one of
the outlier's small triangles lies within the 0.3 margin of an edge, so float64 speaks for its far triangle and the misses only -- the small
ones are held bit for bit by the oracle): PER_RAY_AMBIGUOUS = (0.25 x 512 + 512) / 1024 there, 0.25 where both makers are one.  Measured:
comb 46.7 %, comb-b 40.0 %, soup 16.7 %, outlier 49.5 %, cocentric 0.0 %, with 531, 585, 738, 485 and 923 unambiguous hits.
(The reference models the renderer's hit point as it is defined: 1e-4 short of the surface along the object-space ray, the distance measured
to that point.)
"""
import types

import numpy as np

f32 = np.float32
K_MESH_EPS = 1.1920928955078125e-07
LEAF = 0x80000000
SHORT = 1e-4

# scene materials of the adversarial scenes (materials()): the visible ones have colours that are powers of two in every channel, the two a
# duplicate hides carry a factor 3 -- a path that ever took one has a colour channel whose mantissa is not zero
MAT_LIGHT, MAT_FLOOR, MAT_A, MAT_HIDDEN, MAT_B, MAT_C, MAT_HIDDEN2 = range(7)
HIDDEN = (MAT_HIDDEN, MAT_HIDDEN2)
TOL = {"comb": (1.9e-05, 1.3e-05), "soup": (6.8e-06, 6.2e-06), "outlier": (4.6e-05, 4.0e-05), "cocentric": (2.6e-05, 2.0e-05)}
PER_RAY_AMBIGUOUS = {"comb": 0.625, "soup": 0.25, "outlier": 0.625, "cocentric": 0.25}


def materials(dtype):
    m = np.zeros(7, dtype)
    rows = [((1, 1, 1), 5), ((.5, .5, .5), 0), ((.5, 1, .25), 0), ((.75, .75, .375), 0), ((1, .5, .5), 0), ((.25, .5, 1), 0), ((.375, .75, .75), 0)]
    for i, (col, emit) in enumerate(rows):
        m[i] = (col, 0, (0, 0, 0), 0, 0, 0, emit)
    return m


def carries_hidden_factor(colours):
    """per path: some channel of its colour is no power of two (nor zero): it took a factor 3, i.e. a hidden duplicate's material"""
    c = np.ascontiguousarray(colours, f32)
    return (((c.view(np.uint32) & 0x7fffff) != 0) & (c != 0)).any(-1)


# ---------------------------------------------------------------------------------------------------------------- lattice
def _patch(n, lo):
    """n x n unit squares from (lo, lo), two counter-clockwise right triangles each: (2 n^2, 3, 2) integers"""
    out = []
    for j in range(n):
        for i in range(n):
            x, y = lo + i, lo + j
            a, b, c, d = (x, y), (x + 1, y), (x + 1, y + 1), (x, y + 1)
            out += [(a, b, c), (a, c, d)]
    return np.array(out, np.int64)


def _from_xy(v):
    t = np.zeros((len(v), 3, 3))
    t[:, :, :2] = v
    return t.reshape(-1, 9).astype(f32)


def lattice(variant="", seed=3):
    rng = np.random.default_rng(seed)
    v = _patch(8, -4)
    v = np.stack([np.roll(t, -int(k), 0) for t, k in zip(v, rng.integers(0, 3, len(v)))])      # a random first vertex, same winding
    v = v[rng.permutation(len(v))]
    mats = np.full(len(v), MAT_A, np.int32)
    if variant:
        w = v.copy() if variant == "dup" else v[:, [0, 2, 1]].copy()
        if variant == "flip":
            swap = rng.random(len(v)) < 0.5
            v[swap], w[swap] = w[swap].copy(), v[swap].copy()
        v = np.concatenate([v, w])
        mats = np.concatenate([mats, np.full(len(w), MAT_HIDDEN, np.int32)])
    name = "lattice" + ("-" + variant if variant else "")
    fam = types.SimpleNamespace(name=name, verts=v, tris=_from_xy(v), mats=mats, transform=((3, -5, 2), (0, 0, 0), (2, 0.5, 4)))

    def rays(n, seed=11):
        r = np.random.default_rng(seed)
        q = np.arange(-18, 19)
        pts = np.stack(np.meshgrid(q, q), -1).reshape(-1, 2)                  # quarters
        cnt = lattice_accepting(fam, pts).sum(1)
        six = np.flatnonzero(cnt >= (6 if not variant else 12))
        rest = np.setdiff1d(np.arange(len(pts)), six)
        pick = np.concatenate([six, r.permutation(rest)[:max(n - len(six), 0)]])[:n]
        o = np.concatenate([pts[pick] / 4.0, np.full((len(pick), 1), 4.0)], 1)
        return o, np.tile([0.0, 0.0, -1.0], (len(pick), 1))
    fam.rays = fam.rays64 = rays
    return fam


def lattice_accepting(fam, pts4):
    """(rays, triangles) bool: the CLOSED triangle holds the point; pts4 = 4 x the point (integers): integer edge functions alone"""
    v = 4 * fam.verts[None]                                                 # (1, T, 3, 2)
    p = np.asarray(pts4, np.int64)[:, None, None, :]
    a, b = v, np.roll(v, -1, 2)
    e = (b[..., 0] - a[..., 0]) * (p[..., 1] - a[..., 1]) - (b[..., 1] - a[..., 1]) * (p[..., 0] - a[..., 0])
    return (e >= 0).all(2) | (e <= 0).all(2)


def lattice_answers(fam, o):
    """the known answers for rays (0, 0, -1) from o (z = 4): (triangle or -1, outside, accepting triangles per ray)"""
    p4 = np.round(np.asarray(o)[:, :2] * 4).astype(np.int64)
    assert np.array_equal(p4 / 4.0, np.asarray(o)[:, :2])
    acc = lattice_accepting(fam, p4)
    tri = np.where(acc.any(1), acc.argmax(1), -1)
    v = fam.verts
    area = (v[:, 1, 0] - v[:, 0, 0]) * (v[:, 2, 1] - v[:, 0, 1]) - (v[:, 1, 1] - v[:, 0, 1]) * (v[:, 2, 0] - v[:, 0, 0])
    assert np.all(np.abs(area) == 1)
    return tri, np.where(tri >= 0, area[tri] > 0, True), acc.sum(1)


def lattice_expected(o, transform):
    """World distance and hit point of the lattice rays that hit, under a transform of integers (translation) and powers of two (scale), as
    float32.  Object space: u, v dyadic, t = 4 exactly; the renderer's hit point stops 1e-4 SHORT of the surface along the ray (as the
    reference's getPointOnRay does), z = 4 - fl(4 - fl(1e-4)), exact; the transform rounds once, in P.z = fl(sz z + Tz); the distance is
    sqrt(fl(dz^2)) = |dz| (correctly rounded square root), dz = fl(o.z - P.z)."""
    tr, sc = np.array(transform[0], f32), np.array(transform[2], f32)
    zobj = f32(4.0) - (f32(4.0) - f32(0.0001))
    P = np.zeros((len(o), 3), f32)
    P[:, :2] = np.asarray(o)[:, :2].astype(f32) * sc[:2] + tr[:2]
    P[:, 2] = f32(sc[2] * zobj) + tr[2]
    oz = f32(4.0) * sc[2] + tr[2]
    return np.abs(oz - P[:, 2]).astype(f32), P


# ---------------------------------------------------------------------------------------------------------------- comb
COMB_A = dict(n=4096, a=6.0, c=1.0)          # natural need 23
COMB_B = dict(n=512, a=7.0, c=0.05)          # natural need 20; rebuilt by medians under PT_AMD_MESH_STACK_MAX = 19
COMB_NEED = {"comb": 23, "comb-b": 20}


def comb(n=COMB_A["n"], a=COMB_A["a"], c=COMB_A["c"], name="comb", seed=5):
    rng = np.random.default_rng(seed)
    x = 8.0 * ((np.arange(n) + 1.0) / n) ** a
    s = c * np.diff(np.concatenate([[0.0], x]))
    t = np.zeros((n, 3, 3))
    t[:, :, 0] = x[:, None]
    t[:, 0, 1:], t[:, 1, 1:], t[:, 2, 1:] = np.stack([-s, -s], 1), np.stack([s, -s], 1), np.stack([-s, s], 1)     # the hypotenuse passes the axis
    order = rng.permutation(n)
    tris = t.reshape(n, 9).astype(f32)[order]
    mats = rng.choice([-1, MAT_A, MAT_B, MAT_C], n).astype(np.int32)
    smin = float(s[s > 0].min()) if (s > 0).any() else 1e-6
    fam = types.SimpleNamespace(name=name, tris=tris, mats=mats, transform=((0.5, 1, -2), (20, 35, -10), (1.5, 0.75, 1.25)))

    def rays(n, seed=13):
        """a third along the axis just off it (through every box; on the hypotenuse's far side they miss every tooth), a third grazing at a small
        angle to it, a third aimed at teeth from the side"""
        r = np.random.default_rng(seed)
        o, d = np.zeros((n, 3)), np.zeros((n, 3))
        for i in range(n):
            kind = i % 3
            if kind == 0:
                off = r.uniform(0.02, 0.6, 2) * s[len(s) // 16] * (1 if i % 24 == 0 else -1)      # (one in eight misses every tooth: the longest walk)
                o[i], d[i] = (-1.0, off[0], off[1]), (1, 0, 0)
                if i % 2:
                    o[i, 0], d[i, 0] = 9.5, -1
            elif kind == 1:
                tgt = np.array([r.uniform(0, 8) ** 1.0, 0, 0]) + r.normal(size=3) * [0, 1e-3, 1e-3]
                o[i] = (-r.uniform(0.5, 3), *(r.normal(size=2) * 0.02))
                d[i] = tgt - o[i]
            else:
                k = r.integers(len(x))
                tgt = np.array([x[k], -s[k] * r.uniform(0.1, 0.9), -s[k] * r.uniform(0.1, 0.9)])
                o[i] = tgt + r.normal(size=3) * [1, 0.3, 0.3] * max(4 * s[k], 0.05)
                d[i] = tgt - o[i]
        return o, d
    def rays64(n, seed=15):
        """aimed from the side at the inside of the teeth that are large against the box margin"""
        r = np.random.default_rng(seed)
        bigk = np.flatnonzero(s > 0.25 * s.max())
        k = bigk[r.integers(len(bigk), size=n)]
        tgt = np.stack([x[k], -s[k] * r.uniform(0.2, 0.6, n), -s[k] * r.uniform(0.2, 0.6, n)], 1)
        o = tgt + r.normal(size=(n, 3)) * np.array([1, 0.5, 0.5]) * (3 * s[k])[:, None] + (r.choice([-1, 1], n) * 2 * s[k])[:, None] * [1, 0, 0]
        return o, tgt - o
    fam.rays, fam.rays64 = rays, rays64
    fam.axis_offset = 0.3 * s[len(s) // 4]
    fam.spacing = s
    return fam


def comb_axis_rays(fam, n, seed=27):
    """rays up the comb's axis, just off it on the side the teeth cover: they pass both children's boxes at every level on the way down to the
    first teeth -- a lane's stack fills to the hierarchy's need -- and then hit a tooth, which prunes the rest (half of them tilted by 1e-5)"""
    r = np.random.default_rng(seed)
    off = -r.uniform(0.05, 0.6, (n, 2)) * fam.spacing[len(fam.spacing) // 64]
    o = np.concatenate([np.full((n, 1), -1.0), off], 1)
    d = np.concatenate([np.ones((n, 1)), np.where((np.arange(n) % 2 == 1)[:, None], r.choice([-1e-5, 1e-5], (n, 2)), 0.0)], 1)
    return o, d


# ---------------------------------------------------------------------------------------------------------------- soup, outlier, cocentric
def _aimed(rng, n, targets, spread, dist, centre=(0, 0, 0)):
    tgt = targets[rng.integers(len(targets), size=n)] + rng.normal(size=(n, 3)) * spread
    u = rng.normal(size=(n, 3))
    o = np.asarray(centre, float) + u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(*dist, size=(n, 1))
    return o, tgt - o


def soup(seed=7):
    rng = np.random.default_rng(seed)
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], float)
    big = np.array([corners[[i, 7 - i, (i + 3) % 8 if (i + 3) % 8 not in (i, 7 - i) else (i + 1) % 8]] for i in range(8)])      # each spans the whole box
    c = rng.uniform(-0.85, 0.85, (300, 1, 3))
    small = c + rng.normal(size=(300, 3, 3)) * rng.uniform(0.03, 0.12, (300, 1, 1))
    p = rng.uniform(-0.8, 0.8, (16, 3))
    u, w = rng.normal(size=(16, 3)), rng.normal(size=(16, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    w -= (w * u).sum(1, keepdims=True) * u
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    sliver = np.stack([p, p + u, p + 0.5 * u + 1e-4 * w], 1)                                   # aspect 1e4
    p = rng.uniform(-0.6, 0.6, (8, 3))
    tiny = np.stack([p, p + 3e-4 * u[:8], p + 3e-4 * w[:8]], 1)                               # |det| <= 9e-8 < kMeshEps whatever the ray
    p = rng.uniform(-0.6, 0.6, (8, 3))
    degen = np.stack([p, p, p + rng.normal(size=(8, 3)) * 0.3], 1)
    degen[4:, 2] = degen[4:, 0]                                                               # four with three equal vertices
    t = np.concatenate([big, small, sliver, tiny, degen]).reshape(-1, 9).astype(f32)
    order = rng.permutation(len(t))
    fam = types.SimpleNamespace(name="soup", tris=t[order], mats=rng.choice([-1, MAT_A, MAT_B, MAT_C], len(t)).astype(np.int32),
                                transform=((-1, 2, 0.5), (40, -25, 15), (2, 1.25, 0.75)))
    pts = np.concatenate([small.mean(1), sliver.mean(1), tiny.mean(1), rng.uniform(-0.9, 0.9, (100, 3))])

    def rays(n, seed=17):
        r = np.random.default_rng(seed)
        o, d = _aimed(r, n, pts, 0.02, (1.9, 6.0))
        inside = np.arange(n) % 5 == 4                                                        # origins inside the box: scattered rays
        o[inside] = r.uniform(-0.7, 0.7, (int(inside.sum()), 3))
        d[inside] = r.normal(size=(int(inside.sum()), 3))
        return o, d
    fam.rays = fam.rays64 = rays
    return fam


def outlier(seed=9):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.1, 0.1, (200, 1, 3))
    small = c + rng.normal(size=(200, 3, 3)) * 0.5e-2
    far = np.array([[[3.0e4, 2.6e4, -2.8e4], [3.0e4, 2.9e4, -2.8e4], [2.7e4, 2.75e4, -2.5e4]]])
    t = np.concatenate([small, far]).reshape(-1, 9).astype(f32)
    order = rng.permutation(len(t))
    fam = types.SimpleNamespace(name="outlier", tris=t[order], mats=rng.choice([-1, MAT_A, MAT_B, MAT_C], len(t)).astype(np.int32),
                                transform=((1, 0, -1), (10, 20, 30), (1.5, 1, 2)))
    fc = far[0].mean(0)

    def make(share_far):
        def rays(n, seed=19):
            r = np.random.default_rng(seed)
            o, d = _aimed(r, n, small.mean(1), 2e-3, (0.3, 3.0))
            k = np.flatnonzero(r.random(n) < share_far)
            w = r.dirichlet([2, 2, 2], len(k))
            tgt = np.einsum("ni,ij->nj", w, far[0])
            u = r.normal(size=(len(k), 3))
            o[k] = tgt + u / np.linalg.norm(u, axis=1, keepdims=True) * r.uniform(3e3, 2e4, (len(k), 1))      # (from far off the cluster)
            d[k] = tgt - o[k]
            return o, d
        return rays
    # (the float64 check flags every hit within the box margin, 0.3, of an edge: every hit of a small triangle -- its rays aim mostly at the far one)
    fam.rays, fam.rays64 = make(0.15), make(0.8)
    fam.far_centre = fc
    return fam


def cocentric(k=6, seed=21):
    """2^k + 1 triangles whose BOXES are symmetric about the origin on every axis: the centres the builder bins, 0.5 (lo + hi), are all exactly 0"""
    rng = np.random.default_rng(seed)
    n = 2 ** k + 1
    t = np.zeros((n, 3, 3))
    for i in range(n):
        a, b, c = rng.uniform(0.2, 1.0, 3) * 2.0 ** -rng.integers(0, 4)
        p = rng.uniform(-1, 1, 3)
        sgn = rng.choice([-1, 1], 3)
        t[i] = np.array([[a, b, -c], [-a, p[1] * b, c], [p[0] * a, -b, p[2] * c]]) * sgn
        t[i] = t[i][rng.permutation(3)]
    tris = t.reshape(n, 9).astype(f32)
    v = tris.reshape(n, 3, 3)
    assert np.array_equal(v.min(1), -v.max(1))
    fam = types.SimpleNamespace(name="cocentric", tris=tris, mats=rng.choice([-1, MAT_A, MAT_B, MAT_C], n).astype(np.int32),
                                transform=((0, 1, 0), (-30, 10, 45), (1, 2, 1.5)))

    def rays(n, seed=23):
        r = np.random.default_rng(seed)
        return _aimed(r, n, np.zeros((1, 3)), 0.25, (0.05, 5.0))
    fam.rays = fam.rays64 = rays
    return fam


def families():
    return [lattice(), lattice("dup"), lattice("flip"), comb(), comb(name="comb-b", **COMB_B), soup(), outlier(), cocentric()]


def per_ray_set(fam):
    """the rays of the per-ray GPU tests, object space: at most 1024 -- the family's adversarial mix, the float64 check's, and for the comb the
    stack-filling ones"""
    parts = [fam.rays(448), fam.rays64(512)] + ([comb_axis_rays(fam, 64)] if fam.name.startswith("comb") else [])
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def to_world(geom, o, d, unit_share=0.85, seed=29):
    """object-space rays through a geom's transform (float64, then float32); most directions normalised, some not"""
    m = np.array(geom["transform"], np.float64).reshape(4, 4).T
    ow, dw = o @ m[:3, :3].T + m[:3, 3], d @ m[:3, :3].T
    unit = np.random.default_rng(seed).random(len(o)) < unit_share
    dw = np.where(unit[:, None], dw / np.linalg.norm(dw, axis=1, keepdims=True), dw)
    return np.concatenate([ow, dw], 1).astype(f32)


# ---------------------------------------------------------------------------------------------------------------- scenes
def _camera(pt, scenes_dir, res, eye, look, up=(0, 1, 0), fovy=None):
    import os
    cam = pt.Scene(os.path.join(scenes_dir, "cornell.txt"))
    cam.set_resolution(*res)
    c = cam.camera.copy()
    view = np.asarray(look, float) - np.asarray(eye, float)
    c["position"], c["view"], c["up"] = f32(eye), (view / np.linalg.norm(view)).astype(f32), f32(up)
    if fovy is not None:                                   # (half angles in degrees, x from y as the scene loader derives it)
        c["fov"] = f32([np.degrees(np.arctan(np.tan(np.radians(fovy)) * res[0] / res[1])), fovy])
    return c


def _scene(pt, camera, geoms, meshes, mesh_mats, res):
    return types.SimpleNamespace(geoms=np.concatenate(geoms).view(pt.GEOM_DTYPE), materials=materials(pt.MATERIAL_DTYPE), camera=camera, traceDepth=4,
                                 meshes=meshes, mesh_normals={}, mesh_materials=mesh_mats, image=np.zeros((res[1], res[0], 3), f32))


def family_scene(pt, orc, scenes_dir, fam, res=(64, 48)):
    """One emissive cube, a diffuse one, and the mesh under a plain scale so that it fills the view.  comb: the teeth enlarged
    against the axis, the eye ON the axis (1e-6 off it, on the side the teeth cover) just before the comb's first tooth: every camera ray
    starts inside the boxes of the smallest teeth and widens more slowly than the teeth grow (a tooth's size over its position is a / (k + 1)),
    so it passes both children's boxes at every level -- the stack-filling kind; tests/test_adversarial_meshes_cpu.py counts them.  The light
    stands behind the comb's far end, a wall behind the eye sends the paths back"""
    if fam.name.startswith("comb"):
        k = 2.0 / float(fam.spacing.max())
        off = 1e-6
        geoms = [orc.make_geom(1, MAT_LIGHT, (6, 0, 0), (0, 0, 0), (0.4, 9, 9)),
                 orc.make_geom(2, MAT_B, (0, 0, 0), (0, 0, 0), (0.5, k, k)),
                 orc.make_geom(1, MAT_FLOOR, (-5, 0, 0), (0, 0, 0), (0.2, 14, 14))]
        return _scene(pt, _camera(pt, scenes_dir, res, (-0.001, -off, -off), (4.0, -off, -off), fovy=12.0), geoms, {1: fam.tris}, {1: fam.mats}, res)
    tr = fam.tris.reshape(-1, 3).astype(np.float64)
    if fam.name == "outlier":
        tr = tr[np.abs(tr).max(1) < 1]
    lo, hi = tr.min(0), tr.max(0)
    s = 4.0 / float((hi - lo).max())
    centre = (lo + hi) / 2 * s
    geoms = [orc.make_geom(1, MAT_LIGHT, (centre[0], centre[1] + 6, centre[2]), (0, 0, 0), (6, 0.4, 6)),
             orc.make_geom(2, MAT_B, (0, 0, 0), (0, 0, 0), (s, s, s)),
             orc.make_geom(1, MAT_FLOOR, (centre[0], centre[1] - 3.5, centre[2]), (0, 0, 0), (12, 0.2, 12))]
    eye = centre + ((0.3, 0.6, 3.2) if fam.name.startswith("lattice") else (0.5, 0.8, 3.4))
    return _scene(pt, _camera(pt, scenes_dir, res, eye, centre), geoms, {1: fam.tris}, {1: fam.mats}, res)


def stacked_scene(pt, orc, scenes_dir, nmesh, res=(64, 48), seed=31):
    """nmesh lattice patches (4 x 4 squares, 32 triangles), one centre, scales 3 .. 4 and tilts of a few degrees: every ray is a candidate of nearly
    all of them.  Geoms (3, 4) and (nmesh, nmesh + 1) are exactly coincident pairs: the first of a pair takes a visible material, the second
    a hidden one.  Returns (scene, [(first, second) geom indices])"""
    rng = np.random.default_rng(seed)
    patch = _from_xy(_patch(4, -2) )
    patch = (patch / f32(4.0)).astype(f32)                                                     # [-0.5, 0.5]^2
    geoms = [orc.make_geom(1, MAT_LIGHT, (0, 7, 0), (0, 0, 0), (7, 0.4, 7)), orc.make_geom(1, MAT_FLOOR, (0, -3, 0), (0, 0, 0), (12, 0.2, 12))]
    pairs, meshes, mesh_mats = [], {}, {}
    visible = [MAT_A, MAT_B, MAT_C, MAT_FLOOR]
    k = 0
    while k < nmesh:
        g = len(geoms)
        rot = (float(-90 + rng.uniform(-25, 25)), float(rng.uniform(-25, 25)), float(rng.uniform(-25, 25)))
        sc = float(rng.uniform(3, 4))
        tr = tuple(float(v) for v in rng.uniform(-0.15, 0.15, 3) + (0, 0.5, 0))
        mat = visible[k % 4]
        geoms.append(orc.make_geom(2, mat, tr, rot, (sc, sc, 1)))
        meshes[g] = patch
        k += 1
        if g in (3, nmesh) and k < nmesh:
            geoms.append(orc.make_geom(2, HIDDEN[len(pairs) % 2], tr, rot, (sc, sc, 1)))
            meshes[g + 1] = patch
            mesh_mats[g + 1] = np.full(len(patch), HIDDEN[(len(pairs) + 1) % 2], np.int32)
            pairs.append((g, g + 1))
            k += 1
    return _scene(pt, _camera(pt, scenes_dir, res, (0.3, 2.0, 4.2), (0, 0.5, 0)), geoms, meshes, mesh_mats, res), pairs


# ---------------------------------------------------------------------------------------------------------------- the hierarchy
def check_hierarchy(pt, tris, octant):
    """The properties of the hierarchy pt_init builds (pt.mesh_bvh) that the walk's equivalence with the brute-force rule rests on, for one
    octant copy.  Returns (depth, the copy's own stack need, the need pt_init reserves for all eight)."""
    nt = len(tris)
    recs, nodes, first, need = pt.mesh_bvh(tris, octant)
    assert len(recs) == nt and len(nodes) == max(nt - 1, 1)
    margin = f32(1e-5) * np.abs(tris).max()
    v = tris.reshape(nt, 3, 3)
    neg = np.array([(octant >> a) & 1 for a in range(3)], bool)
    # triangle i, file order: its vertices and the mesh's margin
    assert np.array_equal(recs["v0"], v[:, 0]) and np.array_equal(recs["v1"], v[:, 1]) and np.array_equal(recs["v2"], v[:, 2])
    assert np.all(recs["margin"] == margin)
    box_lo = lambda t: v[t].min(0) - margin                # a triangle's own box, as the kernel derives it
    box_hi = lambda t: v[t].max(0) + margin

    def planes_of(lo, hi):
        # the six halves of a box for this octant: entry planes, exit planes; lo rounded down, hi up (never inwards, and by
        # less than one half-precision step)
        with np.errstate(over="ignore"):
            lo16 = lo.astype(np.float16)
            hi16 = hi.astype(np.float16)
        lo16 = np.where(lo16.astype(f32) > lo, np.nextafter(lo16, np.float16(-np.inf)), lo16)
        hi16 = np.where(hi16.astype(f32) < hi, np.nextafter(hi16, np.float16(np.inf)), hi16)
        return np.concatenate([np.where(neg, hi16, lo16), np.where(neg, lo16, hi16)])

    if nt == 1:
        # a root whose near child is the triangle and whose far child is a box no ray passes (entered at +inf, left at -inf)
        nd = nodes[0]
        assert need == 0 and int(nd["ref"]) == LEAF
        assert np.array_equal(nd["planes"], planes_of(box_lo(0), box_hi(0)))
        fp = nd["far_planes"].astype(f32)
        assert np.all(np.isinf(fp)) and np.all((fp[:3] > 0) != neg) and np.all((fp[3:] < 0) != neg)
        return 0, 0, need
    # walk from the root (inner node 0): every triangle exactly once, every inner node exactly once; a child's box in its
    # parent is the exact union of what lies below it, rounded outwards to half precision and stored as the planes a ray of
    # the octant enters / leaves through; near child first
    seen_tri, seen_node = [], []

    def box_of(ref):
        ref = int(ref)
        if ref & LEAF:
            t = (ref & ~LEAF) // 3
            assert (ref & ~LEAF) % 3 == 0
            seen_tri.append(t)
            return box_lo(t), box_hi(t), 0, 0
        assert (ref - first) % 2 == 0
        k = (ref - first) // 2
        assert 0 <= k < len(nodes)
        seen_node.append(k)
        nd = nodes[k]
        nlo, nhi, nd_, nn = box_of(nd["ref"])
        flo, fhi, fd_, fn = box_of(nd["far_ref"])
        assert np.array_equal(nd["planes"], planes_of(nlo, nhi)) and np.array_equal(nd["far_planes"], planes_of(flo, fhi))
        # the first child is the nearer one for this octant along some axis: its centre does not lie behind the second's
        cl, cr = nlo + nhi, flo + fhi
        assert any((cl[a] >= cr[a]) if (octant >> a) & 1 else (cl[a] <= cr[a]) for a in range(3))
        # depth-first layout: the near child's inner nodes follow their parent directly, the far child's come after them
        if not int(nd["ref"]) & LEAF:
            assert (int(nd["ref"]) - first) // 2 == k + 1
        return np.minimum(nlo, flo), np.maximum(nhi, fhi), 1 + max(nd_, fd_), max(1 + nn, fn)

    _, _, depth, need_here = box_of(first)
    assert sorted(seen_tri) == list(range(nt)) and sorted(seen_node) == list(range(nt - 1))
    # the far children that can wait at once on a lane's stack: this copy's need is within what pt_init reserves for all eight
    assert need_here <= need <= depth
    return depth, need_here, need


def walk(recs, nodes, first, tris, oracle, ro, rd, need, until_deepest=None):
    """The kernel's traversal (ptd::meshIntersectionTest) in numpy fp32 on object-space rays; triangle test by the oracle.
    Returns (winner or -1, its t, records visited, the deepest the stack got).  `until_deepest`: stop as soon as the stack is that deep (the
    question "does this ray fill the stack" is settled on the way down; the winner is then not known)."""
    nt = len(recs)
    up, dn = f32(1.00001), f32(0.99999)
    g = np.where(np.abs(rd) < f32(1e-30), np.copysign(f32(1e-30), rd), rd).astype(f32)
    inv = (f32(1.0) / g).astype(f32)
    c = (-(ro * inv)).astype(f32)
    fma = lambda x: (x.astype(np.float64) * inv.astype(np.float64) + c.astype(np.float64)).astype(f32)   # exact in fp64, rounded once
    best, tbest, visited, deepest = -1, f32(0), 0, 0

    def box_pass(lo, hi):
        with np.errstate(all="ignore"):
            a, b = fma(lo), fma(hi)
            tn = np.max(np.minimum(a, b))
            tf = np.min(np.maximum(a, b))
            tmin = f32(tn * dn)
            return bool(f32(tf * up) >= tmin and tf >= 0 and (best < 0 or not tmin > tbest)), tmin

    def planes_pass(pl):
        with np.errstate(all="ignore"):
            pl = pl.astype(f32)
            tn, tf = np.max(fma(pl[:3])), np.min(fma(pl[3:]))
            tmin = f32(tn * dn)
            return bool(f32(tf * up) >= tmin and tf >= 0 and (best < 0 or not tmin > tbest))

    ref = first
    stack = []
    margin = recs[0]["margin"]
    while True:
        visited += 1
        pop = True
        if ref & LEAF:
            tri = (ref & ~LEAF) // 3
            vv = np.stack([recs[tri]["v0"], recs[tri]["v1"], recs[tri]["v2"]])
            ok, tmin = box_pass(vv.min(0) - margin, vv.max(0) + margin)
            if ok:
                v = tris[tri]
                hit, tuv, front = oracle.mesh_triangle(ro, rd, v[0:3], v[3:6], v[6:9])
                t = f32(tuv[0])
                if hit and t >= tmin and (best < 0 or t < tbest or (t == tbest and tri < best)):
                    best, tbest = tri, t
        else:
            nd = nodes[(int(ref) - first) // 2]
            pn = planes_pass(nd["planes"])
            pf = planes_pass(nd["far_planes"])
            if pn and pf:
                stack.append(int(nd["far_ref"]))
                deepest = max(deepest, len(stack))
                if deepest == until_deepest:
                    break
            if pn or pf:
                ref = int(nd["ref"]) if pn else int(nd["far_ref"])
                pop = False
        if pop:
            if not stack:
                break
            ref = stack.pop()
    assert deepest <= need
    return best, tbest, visited, deepest


def object_ray(oracle, geom, ray):
    """the object-space ray the kernels walk with, in the oracle's fp32: (origin, unit direction, octant)"""
    inv = np.array(geom["inverseTransform"], f32).reshape(-1)[:16]
    ro = oracle.mulmv(inv, (ray[0], ray[1], ray[2], 1.0))
    rd = oracle.normalize(oracle.mulmv(inv, (ray[3], ray[4], ray[5], 0.0)))
    g = np.where(np.abs(rd) < f32(1e-30), np.copysign(f32(1e-30), rd), rd)
    octant = int(np.signbit(g[0])) | int(np.signbit(g[1])) << 1 | int(np.signbit(g[2])) << 2
    return ro, rd, octant


# ---------------------------------------------------------------------------------------------------------------- float64
def mesh_cast(geom, tris, rays, tol, chunk=64):
    """float32 world rays against ONE mesh geom in float64 (path_ref._mesh with the |det| < kMeshEps rule): per ray hit, t (world distance),
    P (world), triangle, and `ambiguous`: the ray crosses the plane of a triangle, at or before its hit, within the mesh's box margin of one of
    that triangle's edges (a near miss included); its two nearest candidates are closer than `tol` (relative); it crosses a triangle whose
    |det| is within a factor 2 of kMeshEps."""
    import path_ref as pr
    tr = np.asarray(tris, np.float64).reshape(-1, 9)
    G = np.asarray(geom).reshape(-1)[0]
    m, inv = pr._m(G, "transform"), pr._m(G, "inverseTransform")
    margin = 1e-5 * np.abs(tr).max()
    v0, v1, v2 = tr[:, 0:3], tr[:, 3:6], tr[:, 6:9]
    e1, e2 = v1 - v0, v2 - v0
    nrm = np.cross(e1, e2)
    out = []
    for c0 in range(0, len(rays), chunk):
        o, d = np.asarray(rays[c0:c0 + chunk, :3], np.float64), np.asarray(rays[c0:c0 + chunk, 3:], np.float64)
        ro, rd = o @ inv[:3, :3].T + inv[:3, 3], pr._unit(d @ inv[:3, :3].T)
        t, k, bary, _ = pr._mesh(ro, rd, tr, eps=K_MESH_EPS)
        hit = np.isfinite(t)
        with np.errstate(all="ignore"):
            p = np.cross(rd[:, None, :], e2[None])
            det = pr._dot(p, e1[None])
            tt = pr._dot(nrm[None], v0[None] - ro[:, None, :]) / pr._dot(nrm[None], rd[:, None, :])
            X = ro[:, None, :] + tt[..., None] * rd[:, None, :]

            def seg(a, b):                                                    # distance of X to the segment a b
                ab = (b - a)[None]
                w = np.nan_to_num(np.clip(pr._dot(X - a[None], ab) / pr._dot(ab, ab), 0, 1))
                return np.linalg.norm(X - (a[None] + w[..., None] * ab), axis=-1)
            edge = np.minimum(np.minimum(seg(v0, v1), seg(v1, v2)), seg(v2, v0))
            s = ro[:, None, :] - v0[None]
            f = 1.0 / det
            bu = f * pr._dot(s, p)
            qv = np.cross(s, e1[None])
            bv = f * pr._dot(qv, rd[:, None, :])
            within = (bu >= -1e-3) & (bv >= -1e-3) & (bu + bv <= 1 + 1e-3)
            tbest = np.where(hit, t, np.inf)[:, None]
            ahead = (tt > -margin) & (tt <= tbest * (1 + tol) + margin)
            amb = (ahead & (edge < margin)).any(1)
            amb |= (ahead & within & (np.abs(det) > K_MESH_EPS / 2) & (np.abs(det) < K_MESH_EPS * 2)).any(1)
            ta = np.where((np.abs(det) >= K_MESH_EPS) & (bu >= 0) & (bv >= 0) & (bu + bv <= 1) & (tt > 0), tt, np.inf)
            ta[np.arange(len(o)), k] = np.inf
            amb |= hit & (ta.min(1) - t < tol * np.maximum(1.0, t))
        # (the renderer's hit point stops 1e-4 short of the surface along the object-space ray, and the distance is measured to THAT point)
        P = (ro + np.where(hit, t - SHORT, 0)[:, None] * rd) @ m[:3, :3].T + m[:3, 3]
        out.append((hit, np.where(hit, np.linalg.norm(P - o, axis=1), -1.0), P, np.where(hit, k, -1), amb))
    cat = [np.concatenate(x) for x in zip(*out)]
    return types.SimpleNamespace(hit=cat[0], t=cat[1], P=cat[2], tri=cat[3], ambiguous=cat[4])
