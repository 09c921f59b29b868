"""The scatter's second candidacy certificates (k_bounce, class bit 3: a binned primitive is a candidate for the next bounce only if neither
its bounding ball nor a certificate of its kind certifies the miss), on the CPU: tests/candidate_ref.py restates them in numpy float32 --
the slab certificate of a binned CUBE against its inflated world box (wall_box, under its bound on the ray origin) and the half-line form
of the ball's certificate for a binned SPHERE -- beside the oracle's own box and sphere tests (src/intersections.h).

No ray that the oracle hits is certified as missed, over: grazes of the box's edges and faces, origins inside and just outside the balls,
origins on the primitive's own surface leaving it (the scatter's 1e-3 offset), axis-parallel directions, NaN, inf and zero components;
cubes with a 100 : 1 aspect, rotated ones, small ones, and origins near the bound the certificate is issued under.

The test counts the certificates it issued: among the rays AIMED AWAY from the primitive -- leaving its surface, or starting beside it
inside its ball and pointing away from its centre -- either kind must certify at least a tenth, and the parent's rule, the ball against
the LINE, noticeably fewer (under half as many): a certificate that never fires would pass the first half of this file.  Only primitives
that CAN be binned are counted there: a 100 : 1 cube has no finite ball, so the ball certifying nothing of it says nothing about the ball.

The device's own evaluation is swept in tests/test_gpu_candidate_certificates.py."""
import numpy as np
import pytest

import candidate_ref as ref

F = np.float32


def _cubes(oracle):
    S = oracle.make_geom
    return {
        "cornell's light": S(1, 0, (0, 10, 0), (0, 0, 0), (3, .3, 3)),
        "100:1 plate": S(1, 0, (1, 6, -2), (0, 0, 0), (4, .04, 4)),
        "100:1 plate, rotated": S(1, 0, (-2, 5, 1), (25, 40, -15), (5, .05, 3)),
        "rotated block": S(1, 0, (2, 3, -1), (30, 45, 10), (1.5, 1, 2)),
        "small cube at the origin": S(1, 0, (0.02, -0.01, 0.03), (10, 20, 30), (.1, .1, .1)),
        "thin rod": S(1, 0, (-3, 2, 2), (0, 60, 20), (.03, 3, .03)),
    }


def _spheres(oracle):
    S = oracle.make_geom
    return {
        "cornell's sphere": S(0, 4, (-1, 4, -1), (0, 0, 0), (3, 3, 3)),
        "small sphere": S(0, 1, (2, 1, 3), (0, 0, 0), (.5, .5, .5)),
        "unit sphere, rotated": S(0, 1, (-3, 6, -2), (20, 70, -40), (1, 1, 1)),
        "ellipsoid": S(0, 1, (1, 7, 1), (15, -30, 60), (1.2, 1, .9)),
    }


def _unit(v):
    return v / np.linalg.norm(v)


def _to_world(g, p):
    m = np.asarray(g["transform"], np.float64).reshape(-1)
    return np.array([m[0 + r] * p[0] + m[4 + r] * p[1] + m[8 + r] * p[2] + m[12 + r] for r in range(3)])


def _surface_point(g, rng, sphere):
    """a point of the primitive's surface and the direction away from it there (the world normal, by the inverse transpose)"""
    q = _unit(rng.normal(size=3))
    if sphere:
        pobj, nobj = 0.5 * q, q
    else:
        a = int(np.argmax(np.abs(q)))
        pobj = rng.uniform(-0.5, 0.5, 3)
        pobj[a] = 0.5 * np.sign(q[a])
        nobj = np.zeros(3)
        nobj[a] = np.sign(q[a])
    it = np.asarray(g["invTranspose"], np.float64).reshape(-1)
    n = _unit(np.array([it[0 + r] * nobj[0] + it[4 + r] * nobj[1] + it[8 + r] * nobj[2] for r in range(3)]))
    return _to_world(g, pobj), n


def _rays(g, rng, sphere, n):
    """(family, aimed away?, origin, direction) -- float32 rays of the families the docstring lists"""
    centre = ref.ball_of(g[0])[0]
    # (the bounding ball's radius from the corners / the largest axis: a 100 : 1 cube has no finite culling radius -- cullK would be 1)
    c = centre.astype(np.float64)
    R = max(np.linalg.norm(_to_world(g[0], np.array(q) * (0.5 if not sphere else 0.5 / np.sqrt(3))) - c)
            for q in ((1, 1, 1), (1, 1, -1), (1, -1, 1), (-1, 1, 1))) * (1.0 if not sphere else np.sqrt(3))
    box = None if sphere else ref.wall_box(g[0])
    out = []
    for k in range(n):
        fam = k % 6
        away = False
        if fam == 0:                                   # leaving the primitive's own surface, as a scatter does
            P, N = _surface_point(g[0], rng, sphere)
            o = P + 1e-3 * N
            d = _unit(rng.normal(size=3))
            if d @ N < 0:
                d = -d
            away = True
        elif fam == 1:                                 # beside the primitive, inside its ball, pointing away from its centre
            P, N = _surface_point(g[0], rng, sphere)
            o = P + N * rng.uniform(0.002, 0.3) * R
            d = _unit(_unit(o - c) + 0.7 * rng.normal(size=3))
            if d @ N < 0.05:
                d = _unit(d + (0.1 - d @ N) * N)
            away = True
        elif fam == 2:                                 # grazes: aimed at the surface's edges and silhouette from afar and from close
            P, N = _surface_point(g[0], rng, sphere)
            t = _unit(np.cross(N, rng.normal(size=3)))
            o = P + t * np.exp2(rng.uniform(-6, 4)) * R + N * rng.normal() * 1e-4 * R
            d = _unit(P - o)
        elif fam == 3:                                 # origins inside and just outside the ball, any direction
            o = c + _unit(rng.normal(size=3)) * R * rng.uniform(0.97, 1.03)
            d = _unit(rng.normal(size=3)) * np.exp2(rng.uniform(-2, 2) if k % 12 == 3 else 0.0)
        elif fam == 4:                                 # axis-parallel directions, exact zeros
            o = c + rng.uniform(-1.5, 1.5, 3) * R
            d = np.zeros(3)
            d[rng.integers(3)] = rng.choice([-1.0, 1.0])
            if k % 12 == 4:
                d[rng.integers(3)] = rng.choice([-1.0, 1.0])
                d = _unit(d)
        else:                                          # towards / past the primitive from across the scene and near the origin's bound
            far = rng.uniform(1, 12) if box is None else rng.uniform(0.2, 1.0) * float(box[2]) / np.sqrt(3)
            o = c + _unit(rng.normal(size=3)) * far
            d = _unit(c + rng.normal(size=3) * 1.2 * R - o)
        out.append((fam, away, o.astype(F), d.astype(F)))
    return out


def _hits(oracle, g, o, d):
    t = oracle.intersect(g, np.concatenate([o, d]))[0]
    # (the nearest-hit loop takes a hit by `t > 0`: a NaN distance -- an infinite direction component, which no scatter produces -- is none)
    return not (t == F(-1.0) or np.isnan(t))


@pytest.mark.parametrize("sphere", [False, True], ids=["cubes", "spheres"])
def test_no_ray_that_hits_is_certified_and_the_certificates_fire(oracle, sphere):
    rng = np.random.default_rng(20251020 + int(sphere))
    prims = _spheres(oracle) if sphere else _cubes(oracle)
    away_n = away_tight = away_ball = issued = 0
    for name, g in prims.items():
        # (a cube whose ball is infinite -- the 100 : 1 ones: cullK would be 1 -- is never binned: soundness is checked on it like on the others,
        # but it stays out of the comparison with the ball, which could not certify it at all)
        binned = bool(np.isfinite(ref.ball_of(g[0])[1]))
        for fam, away, o, d in _rays(g, rng, sphere, 1500):
            tight = ref.certified(g[0], o, d, True)
            ball = ref.certified(g[0], o, d, False)
            assert tight or not ball, (name, fam)                      # the second condition only ever adds certificates
            if tight:
                issued += 1
                assert not _hits(oracle, g, o, d), (name, fam, o.tolist(), d.tolist())
            if away and binned:
                away_n += 1
                away_tight += tight
                away_ball += ball
    print("%s: %d certificates; aimed away %d, certified %d, by the ball alone %d" % ("spheres" if sphere else "cubes", issued, away_n, away_tight, away_ball))
    assert away_tight * 10 >= away_n
    assert away_ball * 2 < away_tight


def test_nan_inf_and_zero_components_are_never_certified_against_a_hit(oracle):
    rng = np.random.default_rng(5)
    bad = [np.nan, np.inf, -np.inf, 0.0]
    for prims, sphere in ((_cubes(oracle), False), (_spheres(oracle), True)):
        for name, g in prims.items():
            c = ref.ball_of(g[0])[0].astype(np.float64)
            for k in range(120):
                o = (c + rng.normal(size=3) * 2).astype(F)
                d = _unit(c + rng.normal(size=3) * 0.3 - o).astype(F)
                v = (o, d)[k % 2]
                v[rng.integers(3)] = bad[(k // 2) % 4]
                if k % 7 == 0:
                    v[rng.integers(3)] = bad[(k // 3) % 4]
                if ref.certified(g[0], o, d, True):
                    assert not _hits(oracle, g, o, d), (name, o.tolist(), d.tolist())
            # a zero direction and a NaN origin certify nothing
            assert not ref.certified(g[0], c.astype(F), np.zeros(3, F), True)
            assert not ref.certified(g[0], np.full(3, np.nan, F), np.array([0, 1, 0], F), True)


def test_the_slab_certificate_is_issued_only_inside_its_bound_on_the_origin(oracle):
    g = _cubes(oracle)["small cube at the origin"]
    lo, hi, omax = ref.wall_box(g[0])
    assert 0.5 < float(omax) < 1.5                                      # (a turned cube of extent 0.1 at the origin: S = 0.26, omax = 5 S - big = 1.23)
    d = np.array([0, 1, 0], F)
    inside = np.array([0.3, 0.2, 0.1], F)                               # beside the cube, pointing past it
    outside = np.array([0.8, 0.4, 0.3], F)
    assert ref.box_miss((lo, hi, omax), inside, d)
    assert not ref.box_miss((lo, hi, omax), outside, d)                 # the same miss, beyond the bound: the ball alone decides
    assert ref.certified(g[0], outside, d, True) == ref.certified(g[0], outside, d, False)
