"""A float64 reference for ONE bounce of a textured / bump-mapped path, in plain numpy: where a ray lands (the primitive, the object-space
point, the cube face or the triangle and its barycentrics), the texture cell there, the colour the path carries afterwards and the normal a
ramp height map tilts the hit to.  Written from the geometry -- the sphere of radius 0.5, the unit cube, Moeller-Trumbore on object-space
triangles, each through the primitive's inverseTransform -- and from the documented semantics; nothing of the library, the oracle or
texture_ref.py is called.  No random numbers, no sampling, no compaction: which branch a path took is read from its new state.

A `scene` is any object with geoms, materials (the renderer's structured arrays), meshes {geom: (ntris, 9)}, mesh_uvs {geom: (ntris, 6)} and,
optionally, mesh_normals {geom: (ntris, 9)} and mesh_materials {geom: (ntris,)}.
A classification float64 cannot settle against a float32 renderer is flagged `ambiguous`, never guessed."""
import types

import numpy as np

OFFSET = 1e-3        # the renderer offsets a new origin by this much along the normal
SHORT = 1e-4         # ... from a hit point it takes this far short of the surface, along the ray in object space (as the reference does)


def _m(g, name):
    return np.array(g[name], np.float64).reshape(4, 4).T             # (column-major in the file and on the device)


def _unit(v):
    with np.errstate(all="ignore"):
        return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _dot(a, b):
    return np.einsum("...i,...i->...", a, b)


def _sphere(ro, rd, tmin):
    a, b, c = _dot(rd, rd), _dot(ro, rd), _dot(ro, ro) - 0.25
    disc = b * b - a * c
    s = np.sqrt(np.maximum(disc, 0))
    t0, t1 = (-b - s) / a, (-b + s) / a
    hit = disc > 0
    t = np.where(hit & (t0 > 0), t0, np.where(hit & (t1 > 0), t1, np.inf))
    inside = hit & (t0 <= 0) & (t1 > 0)
    # the origin's own surface, or a ray that grazes the sphere (the closest approach within 1e-6 of the radius, ahead of the origin -- or
    # within what float32 leaves of the renderer's radicand b^2 / a - (ro . ro - 0.25) from far away: a few ulps of its two terms)
    shaky = (hit & ((np.abs(t0) < tmin) | (np.abs(t1) < tmin))) | ((np.abs(disc) < np.maximum(1e-6 * a, 4e-7 * (b * b + a * _dot(ro, ro)))) & (b < 0))
    return t, inside, shaky


def _cube(ro, rd, tmin):
    rd = np.where(rd == 0, 1e-300, rd)
    ta, tb = (-0.5 - ro) / rd, (0.5 - ro) / rd
    tn, tf = np.minimum(ta, tb).max(1), np.maximum(ta, tb).min(1)
    hit = (tf >= tn) & (tf > 0)
    inside = hit & (tn <= 0)
    t = np.where(hit, np.where(tn > 0, tn, tf), np.inf)
    shaky = hit & ((np.abs(tn) < tmin) | (np.abs(tf) < tmin))
    return t, inside, shaky


def _mesh(ro, rd, tris, tmin=0.0, eps=0.0):
    """nearest two-sided triangle per ray: (t, triangle, (bu, bv)), bu the weight of corner 1 and bv of corner 2.  `eps`: a triangle with
    |det| < eps is not tested (the renderer's rule, glm's epsilon; rd must be a unit vector for it to mean the same)"""
    v0, e1, e2 = tris[:, 0:3], tris[:, 3:6] - tris[:, 0:3], tris[:, 6:9] - tris[:, 0:3]
    p = np.cross(rd[:, None, :], e2[None])
    det = _dot(p, e1[None])
    with np.errstate(all="ignore"):
        f = 1.0 / det
        s = ro[:, None, :] - v0[None]
        bu = f * _dot(s, p)
        qv = np.cross(s, e1[None])
        bv = f * _dot(qv, rd[:, None, :])
        t = f * _dot(qv, e2[None])
    ok = (det != 0) & (np.abs(det) >= eps) & (bu >= 0) & (bv >= 0) & (bu + bv <= 1) & (t > 0)
    traw = t
    t = np.where(ok, t, np.inf)
    k = t.argmin(1)
    i = np.arange(len(ro))
    # (a triangle met within tmin of the origin, before or behind it: float32 may put that root on the other side of zero)
    shaky = ((det != 0) & (bu >= 0) & (bv >= 0) & (bu + bv <= 1) & (np.abs(traw) < tmin)).any(1) if tmin else np.zeros(len(ro), bool)
    return t[i, k], k, np.stack([bu[i, k], bv[i, k]], 1), shaky


def cast(scene, o, d, tmin=1e-4, near=1e-4, edge=2 * OFFSET, inside_cube=False):
    """Rays (o, d) (n, 3) against every primitive.  Returns per ray: prim (-1: nothing), t, gap (the runner-up's distance relative to the
    nearest, (t2 - t1) / t1), P (world), q (object space, SHORT of the surface as the renderer's), axis / sign (a cube's face: the axis of largest |q| and its sign), tri / bary
    (a mesh's triangle and barycentrics), Ng (the outward geometric normal, world), outside, N (Ng turned to the ray's side, as the hit is
    shaded), Ns (the SHADING normal: N, or for a mesh with scene.mesh_normals the blended vertex normal, turned to the face's side, taken to
    world space and turned to the ray's side as N is; `blended` marks those hits), mat (the scene material: scene.mesh_materials' for the
    triangle where that is >= 0, else the object's), short (the world vector by which the renderer's hit point stops short of P) and
    ambiguous: two primitives within `near` of each other, a root within `tmin` of the origin (a triangle's too: a ray that re-enters the
    surface it left), a grazed sphere, a cube hit within `edge` (world units) of an edge, a triangle hit within 1e-4 (barycentric) of an
    edge, a blended normal shorter than 1e-3 or within 1e-3 (cosine) of square to its face, an origin inside a cube (kept with `inside_cube`:
    the hit is the exit face, N the inward normal there)."""
    o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    n, ng = len(o), len(scene.geoms)
    i = np.arange(n)
    T = np.full((ng, n), np.inf)
    inside, shaky = np.zeros((ng, n), bool), np.zeros((ng, n), bool)
    Q = np.zeros((ng, n, 3))
    tri, bary = np.zeros((ng, n), np.int64), np.zeros((ng, n, 2))
    for g in range(ng):
        G = scene.geoms[g]
        inv = _m(G, "inverseTransform")
        ro, rd = o @ inv[:3, :3].T + inv[:3, 3], d @ inv[:3, :3].T
        kind = int(G["type"])
        if kind == 0:
            T[g], inside[g], shaky[g] = _sphere(ro, rd, tmin)
        elif kind == 1:
            T[g], inside[g], shaky[g] = _cube(ro, rd, tmin)
        else:
            T[g], tri[g], bary[g], shaky[g] = _mesh(ro, rd, np.asarray(scene.meshes[g], np.float64).reshape(-1, 9), tmin)
        with np.errstate(all="ignore"):
            Q[g] = ro + np.where(np.isfinite(T[g]), T[g], 0)[:, None] * rd
    order = np.argsort(T, 0)
    prim = order[0]
    t = T[prim, i]
    t2 = T[order[1], i] if ng > 1 else np.full(n, np.inf)
    some = np.isfinite(t)
    with np.errstate(all="ignore"):
        gap = np.where(some, (t2 - t) / t, np.inf)
    q = Q[prim, i]
    kinds = np.array([int(G["type"]) for G in scene.geoms])[prim]
    amb = shaky.any(0) | (gap < near)
    axis = np.abs(q).argmax(1)
    sign = np.where(q[i, axis] > 0, 1, -1)
    # the renderer takes its hit point SHORT of the surface, along the ray in object space: what its sphere normal and its UV maps see
    invs = np.array([_m(G, "inverseTransform")[:3, :3] for G in scene.geoms])[prim]
    q = q - SHORT * _unit(np.einsum("nij,nj->ni", invs, d))
    # the object-space outward normal of the hit
    nobj = q.copy()                                                   # (a sphere's)
    cube = some & (kinds == 1)
    nobj[cube] = 0
    nobj[cube, axis[cube]] = sign[cube]
    scale = np.array([np.array(G["scale"], np.float64) for G in scene.geoms])[prim]
    room = (0.5 - np.abs(q)) * scale                                  # world distance to each pair of faces
    room[i, axis] = np.inf
    amb |= cube & ((room.min(1) < edge) | (inside[prim, i] & (not inside_cube)))
    mesh = some & (kinds == 2)
    ktri, kb = tri[prim, i], bary[prim, i]
    for g in np.unique(prim[mesh]):
        m = mesh & (prim == g)
        tr = np.asarray(scene.meshes[g], np.float64).reshape(-1, 9)[ktri[m]]
        nobj[m] = np.cross(tr[:, 3:6] - tr[:, 0:3], tr[:, 6:9] - tr[:, 0:3])
    amb |= mesh & (np.minimum(np.minimum(kb[:, 0], kb[:, 1]), 1 - kb[:, 0] - kb[:, 1]) < 1e-4)
    Ng = _unit(np.einsum("nji,nj->ni", invs, nobj))                   # (the inverse transpose takes normals to world space)
    outside = np.where(kinds == 2, _dot(Ng, d) < 0, ~inside[prim, i])
    N = np.where(outside[:, None], Ng, -Ng)
    # the shading normal: a mesh with vertex normals blends them with the hit's barycentrics, turns the blend to the side the counter-clockwise
    # face normal points to (a blend of length zero: the face normal) and takes it to world space; which side of the surface the ray is on
    # stays the GEOMETRIC question above (include/pt_amd.h, PtMesh: "everything else as for flat shading")
    Ns, blended = N.copy(), np.zeros(n, bool)
    normals = getattr(scene, "mesh_normals", None) or {}
    for g in np.unique(prim[mesh]):
        if normals.get(g) is None:
            continue
        m = mesh & (prim == g)
        n9 = np.asarray(normals[g], np.float64).reshape(-1, 9)[ktri[m]]
        bu, bv = kb[m, 0:1], kb[m, 1:2]
        blend = n9[:, 0:3] * (1 - bu - bv) + n9[:, 3:6] * bu + n9[:, 6:9] * bv
        face = nobj[m]
        along = _dot(blend, face)
        blend = np.where((along < 0)[:, None], -blend, blend)
        size = np.linalg.norm(blend, axis=1)
        amb[m] |= (size < 1e-3) | (np.abs(along) < 1e-3 * size * np.linalg.norm(face, axis=1))
        blend = np.where((size > 0)[:, None], blend, face)
        w = _unit(np.einsum("nji,nj->ni", invs[m], blend))
        Ns[m] = np.where(outside[m, None], w, -w)
        blended[m] = True
    # the scene material: the face's own (`usemtl`) where it has one, else the object's
    mat = np.array([int(G["materialid"]) for G in scene.geoms])[prim]
    for g, fm in (getattr(scene, "mesh_materials", None) or {}).items():
        m = mesh & (prim == g)
        own = np.asarray(fm, np.int64)[ktri[m]]
        mat[m] = np.where(own >= 0, own, mat[m])
    L = np.array([_m(G, "transform")[:3, :3] for G in scene.geoms])[prim]
    short = SHORT * np.einsum("nij,nj->ni", L, _unit(np.einsum("nij,nj->ni", invs, d)))
    prim = np.where(some, prim, -1)
    return types.SimpleNamespace(short=short, prim=prim, kind=np.where(some, kinds, -1), t=t, gap=gap, P=o + np.where(some, t, 0)[:, None] * d, q=q, axis=axis,
                                 sign=sign, tri=ktri, bary=kb, Ng=Ng, outside=outside, N=N, Ns=Ns, blended=blended & some, mat=np.where(some, mat, -1),
                                 ambiguous=amb & some, d=d)


def take(hit, idx):
    """the hits `idx` (indices or a mask) of a cast's result"""
    return types.SimpleNamespace(**{k: a[idx] for k, a in vars(hit).items()})


def uv(scene, hit):
    """float64 (u, v) per hit (unwrapped) and a mask for the sphere's seam and poles, where the map is singular.  Sphere: longitude and
    latitude of q; cube: q along the two axes after the face's, + 0.5; mesh: the corner UVs blended by the barycentrics."""
    n = len(hit.prim)
    u, v, bad = np.zeros(n), np.zeros(n), np.zeros(n, bool)
    s = hit.kind == 0
    dq = _unit(hit.q[s])
    u[s] = 0.5 + np.arctan2(dq[:, 2], dq[:, 0]) / (2 * np.pi)
    v[s] = 0.5 + np.arcsin(np.clip(dq[:, 1], -1, 1)) / np.pi
    bad[s] = (np.abs(v[s] - 0.5) > 0.45) | (np.abs(u[s] - 0.5) > 0.499)
    c = np.flatnonzero(hit.kind == 1)
    u[c] = hit.q[c, (hit.axis[c] + 1) % 3] + 0.5
    v[c] = hit.q[c, (hit.axis[c] + 2) % 3] + 0.5
    for g in np.unique(hit.prim[hit.kind == 2]):
        m = (hit.kind == 2) & (hit.prim == g)
        c6 = np.asarray(scene.mesh_uvs[g], np.float64).reshape(-1, 6)[hit.tri[m]]
        bu, bv = hit.bary[m, 0], hit.bary[m, 1]
        w = 1 - bu - bv
        u[m] = c6[:, 0] * w + c6[:, 2] * bu + c6[:, 4] * bv
        v[m] = c6[:, 1] * w + c6[:, 3] * bu + c6[:, 5] * bv
    return u, v, bad


def cell(spec, u, v):
    """spec = (W, H, cx, cy, margin in texels) of a cell texture of W x H texels in cx x cy cells (row 0 = the top, v = 0 the bottom,
    repeating); every entry a number or one value per hit, so that each hit may lie on another texture.  Returns the cell's index
    (row * cx + column) and a mask: within `margin` texels of a cell border, where the bilinear sampler may blend two cells (it reads the
    two texels around u * W - 0.5: one cell from half a texel inside the border on).  An axis of ONE cell has no border: the wrap meets
    the same cell."""
    W, H, cx, cy, margin = (np.asarray(s) for s in spec)
    perx, pery = W / cx, H / cy
    x, y = (u - np.floor(u)) * W, (1 - (v - np.floor(v))) * H
    y = np.where(y >= H, y - H, y)
    ix, iy = np.floor(x / perx).astype(int) % cx, np.floor(y / pery).astype(int) % cy
    nearx = (cx > 1) & (np.abs(x / perx - np.round(x / perx)) * perx < margin)
    neary = (cy > 1) & (np.abs(y / pery - np.round(y / pery)) * pery < margin)
    return iy * cx + ix, nearx | neary


def reflect(d, n):
    return d - 2 * _dot(d, n)[:, None] * n


def predict_colour(scene, hit, col, texel, o_new, d_new, Ns=None):
    """The colour after the bounce, in float32 products in the renderer's order: mcol = material.color * texel; a diffuse or refracted
    path carries col * mcol, a mirrored one col * specColor.  The branch is read from the path's new state (o_new, d_new): glass refracted
    exactly when the new origin lies beyond the surface; a REFL material mirrored exactly when the new direction is the reflection about
    Ns (default: N) to 1e-4.  Returns (colour float32 (n, 3), mirror mask, ambiguous mask: a REFL direction within 1e-3 of the mirror's but
    not within 1e-4, the side of the surface the new origin lies on (+1: the ray's), and how far the new origin lies from where this
    reference puts it, along N: it should sit OFFSET to that side of P - short)."""
    f = np.float32
    mats = scene.materials[hit.mat]
    spec = mats[mats.dtype.names[2]].astype(f)
    mcol = mats["color"].astype(f) * np.asarray(texel, f)
    col = np.asarray(col, f)
    Ns = hit.N if Ns is None else Ns
    off = _dot(np.asarray(o_new, np.float64) - hit.P, hit.N)
    glass = mats["hasRefractive"] > 0
    refl = ~glass & (mats["hasReflective"] > 0)
    dev = np.abs(_unit(np.asarray(d_new, np.float64)) - reflect(_unit(hit.d), Ns)).max(1)
    mirror = (glass & (off > 0)) | (refl & (dev < 1e-4))
    amb = refl & (dev >= 1e-4) & (dev < 1e-3)
    side = np.where(off > 0, 1.0, -1.0)
    return np.where(mirror[:, None], col * spec, col * mcol), mirror, amb, side, off - (side * OFFSET - _dot(hit.short, hit.N))


def emitted(scene, hit, col, texel):
    """what a path that ends on an emitter adds to its pixel: (col * (material.color * texel)) * emittance, in float32"""
    f = np.float32
    mats = scene.materials[hit.mat]
    return (np.asarray(col, f) * (mats["color"].astype(f) * np.asarray(texel, f))) * mats["emittance"].astype(f)[:, None]


def tangents(scene, hit):
    """world-space dP/du, dP/dv of the UV maps above at each hit.  Cube: the transform's columns of the two axes after the face's; sphere:
    the derivatives of q = 0.5 (cos lat cos lon, sin lat, cos lat sin lon) by u = lon / 2 pi and v = lat / pi, per unit radius, through the
    transform; mesh: the triangle's edges solved for the UV axes."""
    n = len(hit.prim)
    Tu, Tv = np.zeros((n, 3)), np.zeros((n, 3))
    s = hit.kind == 0
    dq = _unit(hit.q[s])
    rho = np.hypot(dq[:, 0], dq[:, 2])
    with np.errstate(all="ignore"):
        Tu[s] = np.pi * np.stack([-dq[:, 2], 0 * rho, dq[:, 0]], 1)
        Tv[s] = np.pi / 2 * np.stack([-dq[:, 1] * dq[:, 0] / rho, rho, -dq[:, 1] * dq[:, 2] / rho], 1)
    c = np.flatnonzero(hit.kind == 1)
    Tu[c, (hit.axis[c] + 1) % 3] = 1
    Tv[c, (hit.axis[c] + 2) % 3] = 1
    for g in np.unique(hit.prim[hit.kind == 2]):
        m = (hit.kind == 2) & (hit.prim == g)
        tr = np.asarray(scene.meshes[g], np.float64).reshape(-1, 9)[hit.tri[m]]
        c6 = np.asarray(scene.mesh_uvs[g], np.float64).reshape(-1, 6)[hit.tri[m]]
        e1, e2 = tr[:, 3:6] - tr[:, 0:3], tr[:, 6:9] - tr[:, 0:3]
        du1, dv1, du2, dv2 = c6[:, 2] - c6[:, 0], c6[:, 3] - c6[:, 1], c6[:, 4] - c6[:, 0], c6[:, 5] - c6[:, 1]
        det = (du1 * dv2 - du2 * dv1)[:, None]
        Tu[m] = (e1 * dv2[:, None] - e2 * dv1[:, None]) / det
        Tv[m] = (e2 * du1[:, None] - e1 * du2[:, None]) / det
    L = np.array([_m(G, "transform")[:3, :3] for G in scene.geoms])[hit.prim]
    return np.einsum("nij,nj->ni", L, Tu), np.einsum("nij,nj->ni", L, Tv)


def tilt(N, Pu, Pv, hu, hv, outside, d):
    """The shading normal of a height map with gradient (hu, hv): normalize(N - g) seen from outside, normalize(N + g) from inside (N faces
    the ray; g does not turn with it), g = (hu (Pv x N) + hv (N x Pu)) / (N . (Pu x Pv)).  A tilt that would turn the normal away from the ray
    (Ns . d >= 0) is not applied.  Returns (Ns, ambiguous: |Ns . d| < 1e-5, where float32 may decide otherwise)."""
    hu, hv = np.broadcast_to(hu, len(N))[:, None], np.broadcast_to(hv, len(N))[:, None]
    with np.errstate(all="ignore"):
        g = (hu * np.cross(Pv, N) + hv * np.cross(N, Pu)) / _dot(N, np.cross(Pu, Pv))[:, None]
        n = _unit(np.where(np.asarray(outside, bool)[:, None], N - g, N + g))
    c = _dot(n, d)
    ok = np.isfinite(n).all(1) & (c < 0)
    return np.where(ok[:, None], n, N), np.isfinite(c) & (np.abs(c) < 1e-5)
