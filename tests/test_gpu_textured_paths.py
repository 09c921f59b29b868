"""Textured and bump-mapped paths on the MI355X at EVERY bounce, against the float64 reference (tests/path_ref.py): 16 cases -- four scenes
(few / many small primitives, without / with two UV-mapped meshes) x thin lens off / on x bump off / on -- that together take all 24 TEX
forms of k_bounce (tests/test_textured_paths_cpu.py checks that, and validates the reference and the scenes on the CPU).

Texture-only cases: the paths alive after every bounce, their origins and directions are the CPU oracle's on the untextured twin, bit for
bit.  Every case: the colour of every kept path after bounce k is the reference's prediction from the GPU's own colour after bounce k - 1,
bit for bit, the texel being the colour of the cell the float64 cast lands in; a path that ends on the textured light leaves
(colour * (light colour * cell)) * emittance in its pixel, bit for bit.  Bump cases: mirror paths leave about the tilted normal (1e-4, and
under 1 % about the flat one where the two differ, the tolerances of tests/test_gpu_bump.py), every path leaves towards the side its
origin was offset to.  Each step starts from the GPU's own state after the bounce before, so it stands alone.

What the float64 classification cannot settle is left out (tests/path_ref.py, tests/textured_scenes.py: near-ties between primitives,
cube edges, cell borders, the sphere's seam and poles, the ramp's wrap, a direction between 1e-4 and 1e-3 of the mirror's): at most a
quarter of the live paths at any bounce, and at least 200 kept -- asserted, about 12 % measured.

Mutations of csrc/pt_trace.h this test was seen to catch (each built apart and run once): texBary.x / .y swapped in the meshUV calls --
`mesh` fails at bounce 1, 14 paths on the quad in another cell; `face` forced to 0 in the texture's cubeUV call -- `few` fails at bounce 1,
815 paths; Pu / Pv swapped in the sphere's bump branch -- `few-bump` fails at bounce 1, 26 mirror paths off the predicted direction (a
ramp of EQUAL slopes let this one pass: swapping the tangents then swaps two equal gradients, hence SLOPE_U != SLOPE_V).  tg.w replaced
by 0 moves the second mesh's rows 128 rows on, past the UV table: every `mesh` case would read other corners for each quad hit; it was
not run, being a build that reads out of bounds."""
import ctypes as C

import numpy as np
import pytest

import path_ref as pr
import textured_scenes as ts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(pt):
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return pt


def _trace(gpu, sc, extras):
    """in the test library's own renderer: its state bits, iteration 1's frame, the paths after every bounce of both iterations"""
    n = ts.W * ts.H
    gpu.pathtraceFree()
    with gpu.renderer_from_test_library():
        gpu.pathtraceInit(sc, **extras)
        bits = C.c_uint32(0xffffffff)
        assert gpu.test_lib().pt_test_renderer_state(C.byref(bits)) == 0, gpu.test_lib().pt_last_error()
        gpu.pathtrace(None, 0, 1, readback=False)
        frame = gpu.readback(n).reshape(-1, 3)
        paths = {it: [tuple(a.copy() for a in gpu.debug_trace_paths(it, k, n)) for k in range(ts.DEPTH + 1)] for it in ts.ITERS}
        gpu.pathtraceFree()
    return bits.value, frame, paths


def _cell_of(sc, s, got, i):
    """which cell of its texture path i's colour says it read (-1: none of them)"""
    mcol = sc.materials["color"][sc.geoms["materialid"][s.hit.prim[i]]].astype(np.float32) * sc.cells[s.tex[i]]
    return int(np.argmax((s.col[i] * mcol == got[i]).all(1))) if (s.col[i] * mcol == got[i]).all(1).any() else -1


@pytest.mark.parametrize("name,lens,bump", ts.CASES, ids=ts.CASE_IDS)
def test_every_bounce_against_the_float64_reference(gpu, oracle, name, lens, bump):
    sc = ts.build(gpu, oracle, name, bump)
    state, frame, paths = _trace(gpu, sc, ts.LENS if lens else {})
    assert state == ts.state_bits(sc.state, dof=int(lens)), ([k for i, k in enumerate(ts.STATE) if (state >> i) & 1], sc.state)
    mats = sc.materials[sc.geoms["materialid"]]
    refl = (mats["hasReflective"] > 0) & (mats["hasRefractive"] == 0)
    spec = mats["specularColor"].astype(np.float32)
    on_light, mirrors = 0, {int(sc.geoms["type"][g]): 0 for g in np.flatnonzero(sc.geom_bumps >= 0) if refl[g]}
    twin = None if bump else ts.twin_renderer(oracle, sc, lens)
    for it in ts.ITERS:
        for k in range(ts.DEPTH + 1):
            o, d, c, pix = paths[it][k]
            if twin is not None:                                   # a texture changes colours only: the twin's paths, bit for bit
                wo, wd, _, wpix = twin.dump_paths(it, k)
                assert np.array_equal(pix, wpix), (it, k, len(pix), len(wpix))
                assert ts.same(o, wo) and ts.same(d, wd), (it, k)
            if k == 0:
                assert len(pix) == ts.W * ts.H and (c == 1).all()
                continue
            s = ts.step(sc, paths[it][k - 1], paths[it][k])
            print("%s lens %d bump %d it %d bounce %d: live %d kept %d (left out %.1f %%)"
                  % (name, lens, bump, it, k, s.live, s.kept, 100 * (1 - s.kept / max(s.live, 1))))
            got = c[s.idx]
            bad = np.flatnonzero((got.view(np.uint32) != s.want.view(np.uint32)).any(1))
            assert len(bad) == 0, (it, k, len(bad), [dict(prim=int(s.hit.prim[i]), bounce=k, pixel=int(pix[s.idx[i]]), mirror=bool(s.mirror[i]),
                                                           cell_got=_cell_of(sc, s, got, i), cell_wanted=int(s.cell[i])) for i in bad[:6]])
            assert (np.abs(s.off) < 0.1 * pr.OFFSET).all(), (it, k)         # the new origins sit where the reference puts them
            assert s.live - s.kept <= s.live / 4, (it, k, s.live, s.kept)
            assert s.kept >= 200, (it, k, s.kept)
            if bump:
                dk = pr._unit(d[s.idx].astype(np.float64))
                # the geometric side rule: every path leaves towards the side its origin was offset to (the slack of test_gpu_bump.py)
                assert (s.side * pr._dot(dk, s.hit.N) > -1e-5).all(), (it, k)
                for kind in mirrors:
                    m = s.bumped & refl[s.hit.prim] & (s.hit.kind == kind)
                    if not m.any():
                        continue
                    # a path that carries the mirror's colour left along reflect(d, Ns), Ns the tilted normal
                    specular = (got[m].view(np.uint32) == (s.col[m] * spec[s.hit.prim[m]]).view(np.uint32)).all(1)
                    assert np.array_equal(specular, s.mirror[m]), (it, k, kind, int(specular.sum()), int(s.mirror[m].sum()))
                    # ... and next to none about the flat normal -- where the two differ: a tilt that would turn the normal away from the
                    # ray is not applied (pt_device.h, "unbumped"), Ns is N there, as on a face seen at a grazing angle
                    m &= np.abs(s.Ns - s.hit.N).max(1) > 1e-3
                    if not m.any():
                        continue
                    flat = np.abs(dk[m] - pr.reflect(pr._unit(s.hit.d[m]), s.hit.N[m])).max(1) < 1e-4
                    assert flat.mean() < 0.01, (it, k, kind, flat.mean())
                    if k >= 2:
                        mirrors[kind] += int(s.mirror[m].sum())
            if it == 1:                                            # the paths that end on the textured light
                lp, add, _, _ = ts.ended_on_light(sc, paths[it][k - 1], paths[it][k])
                assert ts.same(frame[lp], add), (k, len(lp), np.flatnonzero((frame[lp] != add).any(1))[:5])
                on_light += len(lp)
    assert on_light >= 300, on_light
    assert all(v > 0 for v in mirrors.values()), mirrors              # every bumped kind mirrored kept paths at a bounce >= 2
