"""The rays of tests/test_scatter_diet_cpu.py and tests/test_gpu_scatter_diet.py: 2^16 seeded float32 rays of the kind k_bounce's scatter
classes, half of them around cornell.txt's light (the 3 x 0.3 x 3 slab under the ceiling), half around a thin rotated cube.

Origins: on the room's six walls (1e-3 off them, as a scatter leaves), on cornell.txt's sphere (likewise), in the interior, and on the
cube's own faces.  Directions: towards the cube and its shell (grazes of its inflated box), a hemisphere off the surface, any direction;
one ray in eight is exactly axis-parallel, one in eight has one or two components set to +0 or -0.

Also the numpy float32 restatement of the two evaluations of the slab certificate (csrc/pt_device.h): wallCertainMiss -- three reciprocals
formed once, shared with the walls' block -- and wallCertainMissByAxis -- one axis after the other.  v_rcp_f32 is taken as the correctly
rounded quotient; both evaluations take the same reciprocal, so they see the same quotients whichever it is."""
import numpy as np

F = np.float32
N_RAYS = 1 << 16
SEED = 20261020

# (type, material, translation, rotation, scale) for oracle.make_geom
LIGHT = (1, 0, (0, 10, 0), (0, 0, 0), (3, .3, 3))
THIN = (1, 0, (-1.5, 5, 1), (25, 40, -15), (3, .06, 2))
ROOM_LO = np.array([-5.0, 0.0, -5.0])
ROOM_HI = np.array([5.0, 10.0, 5.0])
SPHERE_C = np.array([-1.0, 4.0, -1.0])
SPHERE_R = 1.5


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def rays(g, n, seed):
    """(org, dir), n x 3 float32 each, around the cube g (a 1-element oracle GEOM_DTYPE array)"""
    rng = np.random.default_rng(seed)
    m = np.asarray(g["transform"], np.float64).reshape(-1)
    A = np.array([[m[4 * c + r] for c in range(3)] for r in range(3)])           # world = A obj + t
    t = np.array([m[12], m[13], m[14]])
    k = np.arange(n)
    fam = k % 4
    # --- origins
    org = np.empty((n, 3))
    nrm = _unit(rng.normal(size=(n, 3)))                                          # the surface normal at the origin (interior: any)
    # 0: on a wall of the room, 1e-3 inside
    p = rng.uniform(ROOM_LO, ROOM_HI, (n, 3))
    face = rng.integers(6, size=n)
    ax, hi = face >> 1, (face & 1) == 1
    wn = np.zeros((n, 3))
    wn[k, ax] = np.where(hi, -1.0, 1.0)
    p[k, ax] = np.where(hi, ROOM_HI[ax], ROOM_LO[ax])
    s = fam == 0
    org[s], nrm[s] = (p + 1e-3 * wn)[s], wn[s]
    # 1: on the sphere, 1e-3 outside
    s = fam == 1
    q = _unit(rng.normal(size=(n, 3)))
    org[s], nrm[s] = (SPHERE_C + q * (SPHERE_R + 1e-3))[s], q[s]
    # 2: the interior
    s = fam == 2
    org[s] = rng.uniform(ROOM_LO + 0.01, ROOM_HI - 0.01, (n, 3))[s]
    # 3: on the cube's own faces, 1e-3 off along the world normal (either side: a ray that leaves, a ray that starts behind the face)
    s = fam == 3
    pobj = rng.uniform(-0.5, 0.5, (n, 3))
    cf = rng.integers(6, size=n)
    cax, chi = cf >> 1, np.where((cf & 1) == 1, 1.0, -1.0)
    pobj[k, cax] = 0.5 * chi
    nobj = np.zeros((n, 3))
    nobj[k, cax] = chi
    cn = _unit(nobj @ np.linalg.inv(A))                                           # (A^-T n)
    side = np.where(rng.random(n) < 0.8, 1.0, -1.0)[:, None]
    org[s], nrm[s] = (pobj @ A.T + t + 1e-3 * side * cn)[s], (side * cn)[s]
    # --- directions
    # a target inside the cube, or (half of them) on its shell 0.9 .. 1.2 of the half extents, where the box's inflation decides
    tobj = rng.uniform(-0.5, 0.5, (n, 3))
    onShell = np.nonzero(rng.random(n) < 0.5)[0]
    tobj[onShell, rng.integers(3, size=n)[onShell]] = (rng.choice([-0.5, 0.5], n) * rng.uniform(0.9, 1.2, n))[onShell]
    tgt = tobj @ A.T + t
    aim = _unit(tgt - org)
    hemi = _unit(rng.normal(size=(n, 3)))
    hemi = np.where(((hemi * nrm).sum(1) < 0)[:, None], -hemi, hemi)
    kind = (k // 4) % 8
    d = np.where((kind < 3)[:, None], aim, np.where((kind < 6)[:, None], hemi, _unit(rng.normal(size=(n, 3)))))
    # exactly axis-parallel
    s = kind == 6
    e = np.zeros((n, 3))
    e[k, rng.integers(3, size=n)] = rng.choice([-1.0, 1.0], n)
    d[s] = e[s]
    org32, d32 = org.astype(F), d.astype(F)
    # one or two components +0 / -0 (the others as they are: the direction is only approximately unit, like a scatter's)
    s = np.nonzero(kind == 7)[0]
    z = rng.choice([0.0, -0.0], (n, 3)).astype(F)
    a1, a2 = rng.integers(3, size=n), rng.integers(3, size=n)
    d32[s, a1[s]] = z[s, 0]
    two = s[(k[s] // 32) % 2 == 1]
    d32[two, a2[two]] = z[two, 1]
    return org32, d32


def all_rays(oracle):
    """[(name, geom, org, dir)]: N_RAYS rays in all"""
    out = []
    for i, (name, spec) in enumerate((("cornell's light", LIGHT), ("thin rotated cube", THIN))):
        g = oracle.make_geom(*spec)
        o, d = rays(g, N_RAYS // 2, SEED + i)
        out.append((name, g, o, d))
    return out


def _quotients(lo, hi, org, inv):
    with np.errstate(all="ignore"):
        t1 = ((lo[None, :] - org).astype(F) * inv).astype(F)
        t2 = ((hi[None, :] - org).astype(F) * inv).astype(F)
    return t1, t2


def _decide(tmin, tmax):
    with np.errstate(all="ignore"):
        gap = (tmin - tmax).astype(F) > (F(1e-5) * (np.abs(tmin) + np.abs(tmax)).astype(F)).astype(F)
        return gap | (tmax < 0)


def slab_shared(lo, hi, org, inv):
    """wallCertainMiss(box, org, inv): the nested min / max of the six quotients"""
    t1, t2 = _quotients(lo, hi, org, inv)
    mn, mx = np.fmin(t1, t2), np.fmax(t1, t2)                                    # (v_min_f32 / v_max_f32 drop a NaN)
    tmin = np.fmax(np.fmax(mn[:, 0], mn[:, 1]), mn[:, 2])
    tmax = np.fmin(np.fmin(mx[:, 0], mx[:, 1]), mx[:, 2])
    return _decide(tmin, tmax)


def slab_by_axis(lo, hi, org, d):
    """wallCertainMissByAxis(box, org, dir): each axis forms its reciprocal and folds its quotients into tmin / tmax, from -inf / +inf"""
    n = org.shape[0]
    tmin, tmax = np.full(n, -np.inf, F), np.full(n, np.inf, F)
    for a in range(3):
        with np.errstate(all="ignore"):
            inv = (F(1) / d[:, a]).astype(F)
            t1 = ((lo[a] - org[:, a]).astype(F) * inv).astype(F)
            t2 = ((hi[a] - org[:, a]).astype(F) * inv).astype(F)
        tmin = np.fmax(tmin, np.fmin(t1, t2))
        tmax = np.fmin(tmax, np.fmax(t1, t2))
    return _decide(tmin, tmax)


def l1(org):
    return ((np.abs(org[:, 0]) + np.abs(org[:, 1])).astype(F) + np.abs(org[:, 2])).astype(F)
