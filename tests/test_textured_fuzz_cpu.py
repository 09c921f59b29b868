"""The ledger of the TEXTURED family (tests/textured_fuzz_scenes.py), without a GPU: conditions on the INPUTS of tests/test_gpu_textured_fuzz.py,
read off the host-only plan (pt_test_scene_plan after the scene's textures, height maps and meshes are registered), the CPU oracle and the
float64 reference (tests/path_ref.py).  Where one fails the generator changes, never the condition.

  * every seed's state is the plan's: {few, many} x {no mesh, mesh} x {pinhole, lens} x {tex, tex|bump}, each of the 16 three times or more,
    and through them all 24 TEX forms of k_bounce (pt_test_bounce_form);
  * counts per kind, and of everything the four hand-built scenes never had: a non-square texture on a sphere, a cube and a mesh, a non-square
    height map, an unbound primitive of every kind beside a bound one, a textured mesh behind an untextured one, a mesh bumped but not
    textured and the reverse, vertex normals under a texture and under a bump, a face material under a texture, a textured emitter, direct
    lighting, a plane wall, the frames of 1 x 1 and 130 x 5, the identity seeds;
  * the crowd: the scene of CROWD_ASKED primitives is refused for LDS with plan_lds' message, the lowered one plans many|sweptCubes|tex|bump;
  * the reference on every seed without a tilt, against the oracle on the untextured twin: with every texel white it gives the oracle's
    colours bit for bit at the checked bounces of both iterations, the paths that end on an emitter leave the oracle's pixel, and where 800
    paths or more are alive it leaves out a quarter at the most and keeps 200 (print-out: the share per seed);
  * E of the affine tolerance, measured on those very paths, equals the generator's E_MEASURED to the digits shown, and the largest
    tolerance that follows is printed;
  * every constant twin's material table: a copy per (material, texture) pair that occurs, its colour float32(colour * c_t), all else the
    material's."""
import collections
import ctypes as C
import time

import numpy as np
import pytest

import path_ref as pr
import textured_fuzz_scenes as tf
import textured_scenes as ts
from test_kernel_select_cpu import FORM, STATE, names

SEEDS = range(tf.N_SEEDS)
GRAZING = 0.05


@pytest.fixture(scope="module")
def family(pt, oracle):
    """[(seed, scene, plan)] of every seed"""
    return [(seed, sc, pt.scene_plan(sc, **tf.plan_options(pt, sc.extras))) for seed in SEEDS for sc in [tf.textured_scene(pt, oracle, seed)]]


def state_of(plan):
    s = {n: bool((plan.state_bits >> i) & 1) for i, n in enumerate(STATE)}
    return ("many" if s["many"] else "few", "mesh" if s["mesh"] else "no mesh", "lens" if s["dof"] else "pinhole", "tex|bump" if s["bump"] else "tex")


def test_every_state_three_times_and_all_24_forms(pt, family):
    T = pt.test_lib()
    states, forms = collections.Counter(), set()
    for seed, sc, plan in family:
        s = {n: bool((plan.state_bits >> i) & 1) for i, n in enumerate(STATE)}
        assert s["tex"] and not s["grouped"] and not s["plain"] and not s["first"], (seed, names(plan.state_bits, STATE))
        assert (s["many"], s["mesh"], s["dof"], s["bump"]) == tuple(sc.wants[k] for k in ("many", "mesh", "lens", "bump")), (seed, names(plan.state_bits, STATE), sc.wants)
        assert s["dof"] == ("lens_radius" in sc.extras) and s["mesh"] == bool(sc.meshes) and s["bump"] == bool((sc.geom_bumps >= 0).any()), seed
        states[state_of(plan)] += 1
        for first in (0, 1):
            got = C.c_uint32(0xffffffff)
            assert T.pt_test_bounce_form(plan.state_bits | first, C.byref(got)) == 0, T.pt_last_error()
            forms.add(got.value)
    print("states:", {"|".join(k): v for k, v in sorted(states.items())})
    print("forms:", sorted(names(f, FORM) for f in forms))
    assert len(states) == 16 and min(states.values()) >= 3, states
    bit = {n: 1 << i for i, n in enumerate(FORM)}
    want = {bit["TEX"] | b | f | g for b in (0, bit["BUMP"]) for f in (0, bit["FIRST"], bit["FIRST"] | bit["DOF"])
            for g in (0, bit["MANY"] | bit["CUBES"], bit["MESH"], bit["MANY"] | bit["CUBES"] | bit["MESH"])}
    assert len(want) == 24 and forms == want


def _square(sc, t):
    return sc.specs[t, 0] == sc.specs[t, 1]


def tally(sc):
    """what the seed holds of the list above"""
    n = collections.Counter()
    gt, gb, kinds = sc.geom_textures, sc.geom_bumps, sc.kinds
    for kind in ("sphere", "cube", "mesh"):
        of = kinds == kind
        n["non-square texture on a " + kind] = any(gt[g] >= 0 and not _square(sc, gt[g]) for g in np.flatnonzero(of))
        n["unbound %s beside a bound one" % kind] = bool((gt[of] < 0).any() and (gt[of] >= 0).any())
    n["non-square height map"] = any(not _square(sc, t) for t in gb[gb >= 0])
    meshes = sorted(sc.meshes)
    n["textured mesh behind an untextured one"] = any(gt[a] < 0 and gt[b] >= 0 for i, a in enumerate(meshes) for b in meshes[i + 1:])
    n["mesh bumped, not textured"] = any(gb[g] >= 0 and gt[g] < 0 for g in meshes)
    n["mesh textured, not bumped (a bump seed)"] = sc.bump and any(gb[g] < 0 and gt[g] >= 0 for g in meshes)
    n["mesh textured and bumped"] = any(gb[g] >= 0 and gt[g] >= 0 for g in meshes)
    n["bump rows apart from texture rows"] = any(gb[g] >= 0 and sum(len(sc.meshes[a]) for a in meshes if a < g and gb[a] >= 0) !=
                                                 sum(len(sc.meshes[a]) for a in meshes if a < g and gt[a] >= 0) for g in meshes if gt[g] >= 0)
    n["vertex normals under a texture"] = any(gt[g] >= 0 for g in sc.mesh_normals)
    n["vertex normals under a bump"] = any(gb[g] >= 0 for g in sc.mesh_normals)
    n["face materials under a texture"] = any(gt[g] >= 0 for g in sc.mesh_materials)
    emits = sc.materials["emittance"][sc.geoms["materialid"]] > 0
    n["textured emitter"] = bool((emits & (gt >= 0)).any())
    n["untextured emitter"] = bool((emits & (gt < 0)).any())
    n["direct lighting"] = bool(sc.extras.get("direct_lighting"))
    n["plane wall"] = "turned wall" in sc.cases
    n["UVs outside [0, 1]"] = "UVs outside [0, 1]" in sc.cases
    n["scale below zero"] = bool((sc.bump_scales < 0).any())
    n["scale above zero"] = bool((sc.bump_scales > 0).any())
    if sc.identity:
        n["identity: " + sc.identity] = True
    if sc.res in ((1, 1), (130, 5)):
        n["frame %d x %d" % sc.res] = True
    n["depth %d" % sc.traceDepth] = True
    n["kind " + sc.kind] = True
    return n


def test_counts(family):
    n = collections.Counter()
    for seed, sc, plan in family:
        assert 2 <= sc.ntex <= 7 and 1 <= sc.traceDepth <= 6 and sc.iters[0] == 1 and 2 <= sc.iters[1] < 100, seed
        assert all(tuple(int(v) for v in sc.specs[t, :2]) in tf.SIZES for t in range(sc.ntex)), seed
        assert all(sc.specs[t, 0] / sc.specs[t, 2] >= 8 and sc.specs[t, 1] / sc.specs[t, 3] >= 8 for t in range(sc.ntex) if sc.specs[t, 2] * sc.specs[t, 3] > 1), seed
        assert (37 <= sc.res[0] <= 96 and 23 <= sc.res[1] <= 72) or sc.res in ((1, 1), (130, 5)), seed
        assert int((sc.materials["emittance"][sc.geoms["materialid"]] > 0).sum()) <= tf.EMIT_MAX, seed
        n.update({k: int(v) for k, v in tally(sc).items()})
    print("seeds holding each case:")
    for k, v in sorted(n.items()):
        print("    %-45s %d" % (k, v))
    assert tf.N_SEEDS >= 56 and n["kind mixed"] == tf.N_MIXED and n["kind affine"] == tf.N_AFFINE >= 6 and n["kind crowd"] == tf.N_CROWD
    for k in ["non-square texture on a sphere", "non-square texture on a cube", "non-square texture on a mesh", "non-square height map",
              "unbound sphere beside a bound one", "unbound cube beside a bound one", "unbound mesh beside a bound one",
              "textured mesh behind an untextured one", "mesh bumped, not textured", "mesh textured, not bumped (a bump seed)", "mesh textured and bumped",
              "bump rows apart from texture rows", "vertex normals under a texture", "vertex normals under a bump", "face materials under a texture",
              "textured emitter", "untextured emitter", "plane wall", "UVs outside [0, 1]", "scale below zero", "scale above zero",
              "identity: zero scale", "identity: constant map", "frame 1 x 1", "frame 130 x 5"] + ["depth %d" % d for d in range(1, 7)]:
        assert n[k] >= 1, k
    assert 7 <= n["direct lighting"] <= 9


def test_the_crowd(pt, family):
    for seed, sc, plan in family:
        if sc.kind != "crowd":
            continue
        swept = int(((sc.kinds == "sphere") | (sc.kinds == "cube")).sum())
        bound = sc.geom_textures[(sc.kinds == "sphere") | (sc.kinds == "cube")] >= 0
        print("crowd seed %d: %d spheres and cubes, %d of them textured, nSphCull %d, LDS %d B, refused: %s" % (seed, swept, bound.sum(), plan.nSphCull, plan.ldsBytes, sc.refused))
        assert names(plan.state_bits, STATE) == ("many|sweptCubes|tex|bump" if sc.bump else "many|sweptCubes|tex") and plan.nSphGroups == 0, seed
        assert sc.res == (48, 36) and swept >= 130 and plan.nSphCull >= 128 and 0.25 < bound.mean() < 0.42, seed
        if seed % 2:                                                # the scene of CROWD_ASKED primitives: PT_ERR_INVALID, plan_lds' message
            count, message = sc.refused
            head, tail = "pt_amd error -1: pt_init: scene does not fit the 160 KiB LDS (", " B)"
            assert count >= tf.CROWD_ASKED and message.startswith(head) and message.endswith(tail) and int(message[len(head):-len(tail)]) > 160 * 1024, sc.refused
            assert plan.ldsBytes <= 160 * 1024
        else:
            assert sc.refused is None and 130 <= swept <= 200, seed


def test_constant_twins_material_tables(pt, oracle, family):
    for seed, sc, plan in family:
        if tf.tilted(sc):
            continue
        const, twin, pairs = tf.constant_twin(sc)
        nm = len(sc.materials)
        assert len(twin.materials) == nm + len(pairs) and np.array_equal(twin.materials[:nm].view(np.uint8), sc.materials.view(np.uint8)), seed
        assert sorted(pairs.values()) == list(range(nm, nm + len(pairs))), seed
        for (m, t), i in pairs.items():
            a, b = sc.materials[m], twin.materials[i]
            assert ts.same(b["color"], a["color"].astype(np.float32) * const.consts[t]), (seed, m, t)
            assert all(np.array_equal(a[f], b[f]) for f in a.dtype.names if f != "color"), (seed, m, t)
        occur = set()
        for g in np.flatnonzero(sc.geom_textures >= 0):
            t = int(sc.geom_textures[g])
            fm = np.asarray(sc.mesh_materials.get(g, [-1]))
            occur |= {(int(f), t) for f in fm if f >= 0}
            if (fm < 0).any():
                occur.add((int(sc.geoms["materialid"][g]), t))
                assert twin.geoms["materialid"][g] == pairs[(int(sc.geoms["materialid"][g]), t)], (seed, g)
        assert occur == set(pairs), seed
        unbound = sc.geom_textures < 0
        assert np.array_equal(twin.geoms["materialid"][unbound], sc.geoms["materialid"][unbound]), seed
        assert all((const.textures[t] == const.consts[t]).all() and const.textures[t].shape == sc.textures[t].shape for t in range(sc.ntex)), seed
        assert not twin.textures and (twin.geom_textures < 0).all() and len({tuple(c) for c in const.consts}) == sc.ntex, seed


def reference_bounce(sc, paths, it, k, white=True):
    """textured_scenes.step from bounce k - 1 to k of `paths`[it], with the distance of every kept path's new origin from where the float64
    reference puts it: OFFSET along the normal the hit is shaded with (a mesh's blended vertex normal where it has them, else the geometric
    one), to the side the path went, from the hit point taken SHORT of the surface"""
    s = ts.step(sc, paths[it][k - 1], paths[it][k], white=white)
    want = s.hit.P - s.hit.short + (s.side * pr.OFFSET)[:, None] * s.hit.Ns
    s.origin_error = np.linalg.norm(paths[it][k][0][s.idx].astype(np.float64) - want, axis=1)
    # (a ray that meets its surface at a grazing angle: what fp32 leaves of the distance to the surface moves the hit point ALONG the
    # surface by that over the cosine -- such hits are left out of E and of hold (d), and count as left out)
    s.grazing = np.abs(pr._dot(s.hit.N, pr._unit(s.hit.d))) < GRAZING
    return s


def affine_tolerance(sc, s, E):
    """hold (d): per kept hit and channel M (|b| / |Pu| + |c| / |Pv|) E + 2^-20 |texel| (textured_fuzz_scenes' docstring), with the float64
    texel and the mask of the hits within a texel of the wrap"""
    u, v, _ = pr.uv(sc, s.hit)
    texel, wrap = tf.affine_texel(sc, s.tex, u, v)
    Pu, Pv = pr.tangents(sc, s.hit)
    k = sc.affine[np.maximum(s.tex, 0)]
    with np.errstate(all="ignore"):
        slack = tf.M_TOL * (np.abs(k[:, :, 1]) / np.linalg.norm(Pu, axis=1)[:, None] + np.abs(k[:, :, 2]) / np.linalg.norm(Pv, axis=1)[:, None]) * E
    slack = np.where((s.tex >= 0)[:, None], slack, 0.0)
    return texel, slack + 2.0 ** -20 * np.abs(texel), wrap


def test_reference_reproduces_the_untextured_twin(pt, oracle, family):
    t0 = time.time()
    E, worst_tol, all_tol, on_light, shares = 0.0, 0.0, [], collections.Counter(), {}
    for seed, sc, plan in family:
        if tf.tilted(sc):
            continue
        ref = tf.oracle_renderer(oracle, tf.untextured_twin(sc))
        W, H = sc.res
        for it in sc.iters:
            need = sorted({0} | {k for b in sc.coloured for k in (b - 1, b)})
            paths = {it: {k: tuple(a.copy() for a in ref.dump_paths(it, k)) for k in need}}
            assert len(paths[it][0][3]) == W * H and (paths[it][0][2] == 1).all(), seed
            for k in sc.coloured:
                s = reference_bounce(sc, paths, it, k)
                got = paths[it][k][2][s.idx]
                bad = (got.view(np.uint32) != s.want.view(np.uint32)).any(1)
                assert not bad.any(), (seed, it, k, int(bad.sum()), s.hit.prim[bad][:5], s.hit.mat[bad][:5], got[bad][:3], s.want[bad][:3])
                # the new origins sit where this reference puts them
                assert (np.abs(s.off[~s.hit.blended]) < 0.1 * pr.OFFSET).all() and (s.origin_error[~s.grazing] < 0.5 * pr.OFFSET).all(), (seed, it, k)
                shares[(seed, it, k)] = (s.live, s.kept)
                if s.live >= 800:
                    assert s.live - s.kept <= s.live / 4, (seed, it, k, s.live, s.kept)
                    assert s.kept >= 200, (seed, it, k, s.kept)
                if (~s.grazing).any():
                    E = max(E, float(s.origin_error[~s.grazing].max()))
                if sc.kind == "affine" and s.kept:
                    texel, tol, wrap = affine_tolerance(sc, s, tf.E_MEASURED)
                    out = wrap | s.grazing
                    worst_tol = max(worst_tol, float((tol / np.abs(texel))[~out].max()))
                    all_tol.append((tol / np.abs(texel))[~out & (s.tex >= 0)].max(1))
                    if s.live >= 800:
                        assert s.live - (~out).sum() <= s.live / 4 and (~out).sum() >= 200, (seed, it, k, s.live, int((~out).sum()))
                if it == 1:                                        # the paths that end on an emitter, against the oracle's own frame
                    if k == sc.coloured[0]:
                        frame = np.zeros(W * H * 3, np.float32)
                        ref.iterate(1, frame)
                        frame = frame.reshape(-1, 3)
                    pix, add, _, _ = ts.ended_on_light(sc, paths[it][k - 1], paths[it][k], white=True)
                    assert ts.same(frame[pix], add), (seed, k, len(pix))
                    on_light[sc.kind] += len(pix)
    for seed in sorted({s for s, _, _ in shares}):
        rows = [(k, v) for k, v in shares.items() if k[0] == seed]
        print("seed %2d left out per checked bounce (iteration, bounce: live, kept): %s" % (seed, "  ".join("%d,%d: %d, %d (%.0f %%)" % (it, k, l, kp, 100 * (1 - kp / max(l, 1))) for (_, it, k), (l, kp) in rows)))
    print("paths that ended on an emitter:", dict(on_light))
    print("E = %.3g (largest distance between the oracle's new origin and the float64 reference's); affine tolerance relative to its texel: largest %.3g, median over the bound hits %.3g" % (E, worst_tol, np.median(np.concatenate(all_tol))))
    print("CPU time of the reference over the family: %.1f s" % (time.time() - t0))
    assert float("%.1e" % E) == tf.E_MEASURED, E
