"""The scatter's slab certificate for a binned cube, once from shared reciprocals and alone (k_bounce, class bit 3, the PLAIN forms), on the
CPU: tests/scatter_diet_rays.py restates both evaluations in numpy float32 -- ptd::wallCertainMiss from three reciprocals formed once for
the cube and the walls, and ptd::wallCertainMissByAxis, which the other forms keep -- and generates the 2^16 rays (around cornell.txt's
light and around a thin rotated cube; origins on the walls, on the sphere, in the interior and on the cube itself; exactly axis-parallel
directions and components of +-0 among them).

The two evaluations decide alike on every ray.

The cube's rule without the bounding ball -- certified iff the slab certifies and |o|_1 <= the box's bound -- certifies no ray that the
oracle's box test hits, certifies every ray the parent's rule (ball or slab, tests/candidate_ref.py) certified except ones the ball alone
did, and those are few: the inflated box lies inside the inflated ball, so the ball adds only lines whose half-line the slab does not
see as missing -- counted and printed.

The device's own evaluation is swept over the same rays in tests/test_gpu_scatter_diet.py."""
import numpy as np
import pytest

import candidate_ref as ref
import scatter_diet_rays as sdr

F = np.float32


@pytest.fixture(scope="module")
def cases(oracle):
    return sdr.all_rays(oracle)


def test_the_ray_set_is_what_the_docstring_says(cases):
    n = sum(o.shape[0] for _, _, o, _ in cases)
    assert n == sdr.N_RAYS
    for _, _, o, d in cases:
        assert o.dtype == F and d.dtype == F and np.isfinite(o).all() and np.isfinite(d).all()
        nz = (d == 0).sum(1)
        assert ((nz == 2) & (np.abs(d).max(1) == 1)).sum() >= o.shape[0] // 16          # exactly axis-parallel
        assert np.signbit(d[d == 0]).any() and (~np.signbit(d[d == 0])).any()           # -0 and +0
        assert (nz == 1).sum() > 0


def test_shared_reciprocals_and_by_axis_decide_alike(cases):
    for name, g, o, d in cases:
        lo, hi, omax = ref.wall_box(g[0])
        with np.errstate(all="ignore"):
            inv = (F(1) / d).astype(F)
        shared = sdr.slab_shared(lo, hi, o, inv)
        by_axis = sdr.slab_by_axis(lo, hi, o, d)
        print("%s: %d of %d rays certified by the slab" % (name, int(shared.sum()), o.shape[0]))
        assert np.array_equal(shared, by_axis), name
        assert 0 < shared.sum() < o.shape[0]
        # ... and the vector form is the scalar restatement the other tests use (a sample: that one is a Python loop)
        for i in range(0, o.shape[0], 97):
            assert bool(shared[i] and sdr.l1(o[i:i + 1])[0] <= omax) == ref.box_miss((lo, hi, omax), o[i], d[i]), (name, i)


def test_the_slab_alone_never_certifies_a_hit_and_loses_few_certificates(oracle, cases):
    for name, g, o, d in cases:
        lo, hi, omax = ref.wall_box(g[0])
        with np.errstate(all="ignore"):
            inv = (F(1) / d).astype(F)
        rule = sdr.slab_shared(lo, hi, o, inv) & (sdr.l1(o) <= omax)
        hits = 0
        for i in np.nonzero(rule)[0]:
            t = oracle.intersect(g, np.concatenate([o[i], d[i]]))[0]
            hits += not (t == F(-1.0) or np.isnan(t))
        # the certificates the parent's rule issued through the ball alone (a sample of the rays: ball_miss is a Python loop)
        ball = ref.ball_of(g[0])
        sample = range(0, o.shape[0], 16)
        ball_only = sum(1 for i in sample if not rule[i] and ref.ball_miss(ball, o[i], d[i], False))
        print("%s: %d of %d rays certified by the slab alone, %d of them hit; of %d sampled rays the ball alone certified %d more" % (
            name, int(rule.sum()), o.shape[0], hits, len(sample), ball_only))
        assert rule.sum() > 0
        assert hits == 0
