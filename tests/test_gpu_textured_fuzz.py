"""The TEXTURED family on the MI355X: the seeded scenes of tests/textured_fuzz_scenes.py, which take all 24 TEX / TEX|BUMP forms of k_bounce with
non-square textures at offsets of their own, unbound primitives, meshes textured only / bumped only / both, vertex normals and face materials
under a texture, textured emitters, plane walls, a lens, direct lighting and a crowd of up to 900 swept primitives.  The CPU oracle knows
neither textures nor height maps; four holds, each an existing idea generalised (tests/test_textured_fuzz_cpu.py is the ledger of the inputs
and validates the reference on the CPU):

(a) geometry, exact.  Every seed without a tilt (texture-only seeds and the two identity seeds: a zero scale, a constant map): the state bits
    are the plan's; the paths alive after bounce 0, after every checked bounce (1, a drawn one, the last) and after the bounce before each,
    their origins, directions and pixels, in both iterations, and the `live` tallies of iteration 1, are the oracle's on the untextured twin
    (same geometry, vertex normals, face materials, lens, direct lighting), bit for bit.  Nothing is left out.
(b) colours through cell textures, exact.  The colour of every kept path after a checked bounce is the float64 reference's prediction from
    the GPU's own colour one bounce earlier, bit for bit: (face or object material) x (the cell's colour, 1 for an unbound primitive); a kept
    path that ends on an emitter, textured or not, leaves (col * (colour * texel)) * emittance in its pixel, bit for bit, in iteration 1.
(c) whole frames, exact: test_constant_twin.  Every texture replaced by one colour c_t of its size, rendered through the PRODUCT library
    under a drawn schedule (1 .. 3 shards, batches of 1, 3 or 8, 1 .. 3 in flight, a third traced ahead, 2 .. 6 iterations): the accumulator
    and the tallies are the oracle's on the twin whose material table holds float32(colour * c_t) per (material, texture) pair.
(d) the bilinear blend, to a derived tolerance: the `affine` seeds, whose texel centres sample a + b u + c v.  Per kept hit and channel
    |colour - col * (material * (a + b u + c v))| <= col * material * (M (|b| / |Pu| + |c| / |Pv|) E + 2^-20 |texel|), E and M from the
    generator's docstring; hits within a texel of the wrap or at a grazing angle are left out.
Bump seeds keep the laws of tests/test_gpu_textured_paths.py with its tolerances: a path that carries the mirror's colour left along
reflect(d, Ns) about the TILTED normal (1e-4), under 1 % about the flat one where the two differ, and every path leaves towards the side its
origin was offset to (-1e-5; about the renderer's N, a mesh's blended vertex normal where it has them, and where the tilt was applied or
the hit is flat-shaded: an untilted hit with vertex normals is the untextured renderer's, which has no such rule).  The tilt is float64's
(path_ref.tangents / tilt) with the gradient of a non-square ramp, from the blended vertex normal where the mesh has them.

Left out of (b) and (d): what tests/path_ref.py cannot settle, the lobe of a half mirror with an exponent, and under direct lighting the
last bounce (its diffuse colour carries the light sample's weight; (a) and (c) hold it).  Where 800 paths or more are alive at most a quarter
is left out and 200 are kept -- asserted.

Mutations, each built apart and run once against this file and the 16 cases of tests/test_gpu_textured_paths.py: see MUTATIONS below."""
import collections
import ctypes as C

import numpy as np
import pytest

import path_ref as pr
import textured_fuzz_scenes as tf
import textured_scenes as ts
from test_textured_fuzz_cpu import affine_tolerance, reference_bounce

pytestmark = pytest.mark.gpu

MUTATIONS = """Mutations of csrc/pt_trace.h / csrc/pt_device.h, each built apart (both libraries) and run once against the 89 cases of this file (56 of paths, 33 constant twins) and the 16
cases of tests/test_gpu_textured_paths.py.  The 16 existing cases passed under every one of them: their textures are square, their
meshes have neither face materials nor differing rows.
  * td.y / td.z swapped in the texture fetch (textureSample(texels, td.x, td.z, td.y, u, v); in bounds: the last texel read is
    (W - 1) H + H - 1): 54 of the 56 path cases failed, 48 on a colour that is no cell of the texture at bounce 1 of iteration 1 (seed 0:
    905 paths) and the 6 affine seeds beyond their tolerance.  Seeds 20 (one pixel) and 38 passed, and every constant twin: a texture of
    one colour reads the same with W and H swapped.
  * the same swap in the height fetch (bumpGradient): the 22 tilted mixed seeds and the bumped crowd failed hold (b) at bounce 1 -- a wrong
    tilt sends the mirror's paths off the predicted direction, so the reference takes them for diffuse ones and predicts another colour
    (seed 11: 208 paths).  The two identity seeds passed, as they must.
  * fh replaced by fw in bumpGradient: seeds 24 and 46 failed, on 2 paths and 1.  The hold is weak here and says why: on a RAMP the central
    difference over 2 / W times W / 2 is the slope whatever W is, so only the hits whose v - 1 / W and v - 1 / H fall into different texels
    next to the wrap margin differ.  A height map that is not linear in v would hold it; the family has none.
  * the face's material replaced by the object's in the colour product (`MESH && faceMat != 0` made false in the few-primitive forms): 9
    path cases (seeds 2, 6, 10, 14, 18, 26, 30, 46, 50: the few|mesh states with face materials) failed hold (b), hold (d) (seed 50) or the
    emission hold (a face that emits), and 5 constant twins (2, 6, 18, 38, 50) differed from the oracle's frame.
Described, not run -- each reads outside a table:
  * the bump rows read at TexGeom::uvBase (`bg.z` -> `tg.z`): a mesh textured and bumped behind a textured-only mesh has tg.z = that
    mesh's triangle count and bg.z = 0, so its rows would be read past the end of bumpUV / bumpTan (seeds of "bump rows apart from
    texture rows" in the ledger);
  * the `tg.x >= 0` test dropped: texDesc[-1] for every unbound primitive;
  * triBase zeroed (`tg.w` -> 0): a textured mesh behind an untextured one would read UV rows past the table, as the docstring of
    tests/test_gpu_textured_paths.py says of its second mesh."""
__doc__ += "\n\n" + MUTATIONS
SEEDS = list(range(tf.N_SEEDS))
UNTILTED = [s for s in SEEDS if not ((s < tf.N_MIXED and s % 16 >= 8 and s not in (tf.ZERO_SCALE, tf.CONSTANT_MAP)) or s == tf.N_SEEDS - 1)]
TALLY = collections.Counter()


@pytest.fixture(scope="module")
def gpu(pt):
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return pt


_SCENES = {}


def _scene(gpu, oracle, seed):
    if seed not in _SCENES:
        _SCENES[seed] = tf.textured_scene(gpu, oracle, seed)
    return _SCENES[seed]


def _need(sc):
    return sorted({0} | {k for b in sc.checked for k in (b - 1, b)})


def _trace(gpu, sc):
    """in the test library's own renderer: its state bits, iteration 1's frame and tallies, the paths behind the bounces the holds read"""
    n = sc.res[0] * sc.res[1]
    gpu.pathtraceFree()
    with gpu.renderer_from_test_library():
        gpu.pathtraceInit(sc, **sc.extras)
        bits = C.c_uint32(0xffffffff)
        assert gpu.test_lib().pt_test_renderer_state(C.byref(bits)) == 0, gpu.test_lib().pt_last_error()
        gpu.counters_reset()
        gpu.pathtrace(None, 0, 1, readback=False)
        frame = gpu.readback(n).reshape(-1, 3)
        live = [int(v) for v in gpu.counters().live]
        paths = {it: {k: tuple(a.copy() for a in gpu.debug_trace_paths(it, k, n)) for k in _need(sc)} for it in sc.iters}
        gpu.pathtraceFree()
    return bits.value, frame, live, paths


def _cell_of(sc, s, got, i):
    """which cell of its texture path i's colour says it read (-1: none of them)"""
    if s.tex[i] < 0:
        return -1
    mcol = sc.materials["color"][s.hit.mat[i]].astype(np.float32) * sc.cells[s.tex[i]]
    same = (s.col[i] * mcol == got[i]).all(1)
    return int(np.argmax(same)) if same.any() else -1


def _bump_laws(sc, s, got, d, it, k):
    """the laws of tests/test_gpu_textured_paths.py on the kept paths of one bounce; -> the mirrored bumped paths counted"""
    dk = pr._unit(d[s.idx].astype(np.float64))
    # the side rule, about the normal the renderer offsets the new origin along (a mesh's blended vertex normal where it has them): the
    # renderer ends a TILTED path that breaks it, and a flat-shaded hit keeps it by itself; a hit with vertex normals whose tilt was not
    # applied (no height map; a blended normal that faces away from the ray already: pt_device.h, "unbumped") is the untextured
    # renderer's, which has no such rule
    law = (np.abs(s.Ns - s.hit.Ns).max(1) > 0) | ~s.hit.blended
    assert (s.side * pr._dot(dk, s.hit.Ns) > -1e-5)[law].all(), (sc.seed, it, k)
    mats = sc.materials[s.hit.mat]
    refl = (mats["hasReflective"] > 0) & (mats["hasRefractive"] == 0)
    m = s.bumped & refl
    if not m.any():
        return 0
    specular = (got[m].view(np.uint32) == (s.col[m] * mats["specularColor"][m].astype(np.float32)).view(np.uint32)).all(1)
    assert np.array_equal(specular, s.mirror[m]), (sc.seed, it, k, int(specular.sum()), int(s.mirror[m].sum()))
    m &= np.abs(s.Ns - s.hit.Ns).max(1) > 1e-3
    if m.any():
        flat = np.abs(dk[m] - pr.reflect(pr._unit(s.hit.d[m]), s.hit.Ns[m])).max(1) < 1e-4
        assert flat.mean() < 0.01, (sc.seed, it, k, flat.mean())
    return int(s.mirror[m].sum())


@pytest.mark.parametrize("seed", SEEDS)
def test_paths_of_the_family(gpu, oracle, seed):
    sc = _scene(gpu, oracle, seed)
    W, H = sc.res
    plan = gpu.scene_plan(sc, **tf.plan_options(gpu, sc.extras))
    state, frame, live, paths = _trace(gpu, sc)
    assert state == plan.state_bits, (seed, state, plan.state_bits)
    assert (seed in UNTILTED) == (not tf.tilted(sc))
    if not tf.tilted(sc):                                           # (a) the oracle's paths on the untextured twin, bit for bit
        twin = tf.oracle_renderer(oracle, tf.untextured_twin(sc))
        for it in sc.iters:
            for k in _need(sc):
                o, d, c, pix = paths[it][k]
                wo, wd, _, wpix = twin.dump_paths(it, k)
                assert np.array_equal(pix, wpix), (seed, it, k, len(pix), len(wpix))
                assert ts.same(o, wo) and ts.same(d, wd), (seed, it, k)
        want = np.zeros(W * H * 3, np.float32)
        nd = sc.traceDepth + (1 if sc.extras.get("direct_lighting") else 0)
        assert live[1:nd + 2] == [int(v) for v in twin.iterate(1, want).live[1:nd + 2]], seed
    for it in sc.iters:
        o, d, c, pix = paths[it][0]
        assert len(pix) == W * H and (c == 1).all(), seed
        for k in sc.coloured:
            o, d, c, pix = paths[it][k]
            s = reference_bounce(sc, paths, it, k, white=sc.kind == "affine")
            got = c[s.idx]
            out = np.zeros(s.kept, bool)
            if sc.kind == "affine":                                 # (d)
                texel, tol, wrap = affine_tolerance(sc, s, tf.E_MEASURED)
                out = wrap | s.grazing
                mcol = sc.materials["color"][s.hit.mat].astype(np.float64) * s.col
                want = np.where(s.mirror[:, None], s.want, mcol * texel)
                err = np.abs(got - want) - mcol * tol
                bad = np.flatnonzero(((err > 0).any(1) | ((got.view(np.uint32) != s.want.view(np.uint32)).any(1) & (s.mirror | (s.tex < 0)))) & ~out)
                assert len(bad) == 0, (seed, it, k, len(bad), [dict(prim=int(s.hit.prim[i]), tex=int(s.tex[i]), got=got[i].tolist(), want=want[i].tolist(), tol=(mcol * tol)[i].tolist()) for i in bad[:4]])
            else:                                                   # (b)
                bad = np.flatnonzero((got.view(np.uint32) != s.want.view(np.uint32)).any(1))
                assert len(bad) == 0, (seed, it, k, len(bad), [dict(prim=int(s.hit.prim[i]), bounce=k, pixel=int(pix[s.idx[i]]), mirror=bool(s.mirror[i]), tex=int(s.tex[i]),
                                                                     cell_got=_cell_of(sc, s, got, i), cell_wanted=int(s.cell[i])) for i in bad[:6]])
            assert (np.abs(s.off[~s.hit.blended]) < 0.1 * pr.OFFSET).all(), (seed, it, k)
            kept = int((~out).sum())
            print("seed %d %s it %d bounce %d: live %d kept %d (left out %.1f %%)" % (seed, sc.kind, it, k, s.live, kept, 100 * (1 - kept / max(s.live, 1))))
            if s.live >= 800:
                assert s.live - kept <= s.live / 4, (seed, it, k, s.live, kept)
                assert kept >= 200, (seed, it, k, kept)
            TALLY["kept, " + sc.kind] += kept
            TALLY["kept on a bound primitive"] += int((s.tex[~out] >= 0).sum())
            TALLY["kept on an unbound primitive"] += int((s.tex[~out] < 0).sum())
            if tf.tilted(sc):
                TALLY["mirrored bumped paths"] += _bump_laws(sc, s, got, d, it, k)
            if it == 1:                                             # the paths that end on an emitter
                lp, add, tex, _ = ts.ended_on_light(sc, paths[it][k - 1], paths[it][k], white=sc.kind == "affine")
                if sc.kind != "affine":
                    assert ts.same(frame[lp], add), (seed, k, len(lp), np.flatnonzero((frame[lp] != add).any(1))[:5])
                else:
                    assert ts.same(frame[lp][tex < 0], add[tex < 0]), (seed, k)
                TALLY["ended on a textured emitter"] += int((tex >= 0).sum())
                TALLY["ended on an untextured emitter"] += int((tex < 0).sum())
    print("tallies so far:", dict(TALLY))


def _schedule(rng, sc):
    """how a constant twin is rendered: (shards, this shard, batch, iterations, batches in flight, traced ahead)"""
    world = 1 if sc.res[1] < 3 else int(rng.choice([1, 1, 2, 3]))
    return world, int(rng.integers(0, world)), int(rng.choice([1, 3, 8])), int(rng.integers(2, 7)), int(rng.choice([1, 2, 3])), bool(rng.random() < 0.33)


@pytest.mark.parametrize("seed", UNTILTED)
def test_constant_twin(gpu, oracle, seed):
    """(c): the frame of the scene under constant textures, through the product library, against the oracle on the material twin"""
    sc = _scene(gpu, oracle, seed)
    const, twin, pairs = tf.constant_twin(sc)
    W, H = sc.res
    world, rank, batch, iters, pipeline, ahead = _schedule(np.random.default_rng(tf.SEED0 + 900 + seed), sc)
    ref = tf.oracle_renderer(oracle, twin)
    want, live = np.zeros(W * H * 3, np.float32), np.zeros(64, np.int64)
    gpu.pathtraceFree()
    gpu.pathtraceInit(const, traceDepth=sc.traceDepth, max_batch=batch, pipeline_depth=pipeline, shard_rank=rank, shard_count=world, trace_ahead=ahead, **sc.extras)
    it = 1
    while it <= iters:
        n = 1 if ahead else min(batch, iters - it + 1)
        gpu.pathtrace_batch(None, 0, it, n)
        it += n
    for k in range(1, iters + 1):
        live += np.array(ref.iterate(k, want, rank, world).live[:64])
    got = gpu.readback(W * H)
    cnt = gpu.counters()
    gpu.pathtraceFree()
    nd = sc.traceDepth + (1 if sc.extras.get("direct_lighting") else 0)
    if not (ahead and batch > 1):                                   # (the tallies also cover iterations traced ahead)
        assert [int(cnt.live[d]) for d in range(1, nd + 2)] == live[1:nd + 2].tolist(), seed
    assert cnt.iterations == iters
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, (seed, len(bad), len(pairs), (world, rank, batch, iters, pipeline, ahead), got[bad][:4], want[bad][:4])
    assert len(pairs) == 0 or (want != 0).any() or W * H < 10, seed
