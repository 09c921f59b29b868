"""The float64 path reference (tests/path_ref.py) and the scenes of tests/test_gpu_textured_paths.py, validated without a GPU.

A texture changes a path's colour and nothing else, so the paths of every texture-only GPU case are the CPU oracle's paths of the
untextured twin.  On those very paths, bounce by bounce: the reference, with every texel white, must give the oracle's own colours bit for
bit (it picks the hit, the branch and the product order the renderer does); the share of paths it leaves out as ambiguous stays under the
cap; every cell of every texture and both meshes are reached at a bounce >= 2; enough paths end on the textured light.  The 16 cases
together reach all 24 TEX forms of k_bounce, and the tilt's conventions agree with the fp32 restatement of the kernel's (tests/bump_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import bump_ref as br
import path_ref as pr
import textured_scenes as ts

TEXTURE_ONLY = [(s, l) for s, l, b in ts.CASES if not b]
FORM = ("FIRST", "MANY", "DOF", "MESH", "PLAIN", "CUBES", "GROUPS", "TEX", "BUMP")              # bit i of pt_test_bounce_form's form_bits


@pytest.mark.parametrize("name,lens", TEXTURE_ONLY, ids=[i for i, c in zip(ts.CASE_IDS, ts.CASES) if not c[2]])
def test_reference_reproduces_the_untextured_twin(pt, oracle, name, lens):
    sc = ts.build(pt, oracle, name, False)
    ref = ts.twin_renderer(oracle, sc, lens)
    reached, meshes_hit, on_light = set(), set(), 0
    for it in ts.ITERS:
        paths = [tuple(a.copy() for a in ref.dump_paths(it, k)) for k in range(ts.DEPTH + 1)]
        assert len(paths[0][3]) == ts.W * ts.H and (paths[0][2] == 1).all()
        for k in range(1, ts.DEPTH + 1):
            s = ts.step(sc, paths[k - 1], paths[k], white=True)
            print("%s lens %d it %d bounce %d: live %d kept %d (left out %.1f %%)" % (name, lens, it, k, s.live, s.kept, 100 * (1 - s.kept / max(s.live, 1))))
            got = paths[k][2][s.idx]
            bad = (got.view(np.uint32) != s.want.view(np.uint32)).any(1)
            assert not bad.any(), (it, k, int(bad.sum()), s.hit.prim[bad][:5], got[bad][:3], s.want[bad][:3])
            assert (np.abs(s.off) < 0.1 * pr.OFFSET).all()                # the new origins sit where this reference puts them
            assert s.live - s.kept <= s.live / 4, (it, k, s.live, s.kept)
            assert s.kept >= 200, (it, k, s.kept)
            if k >= 2:
                reached |= set(zip(s.tex.tolist(), s.cell.tolist()))
                meshes_hit |= set(s.hit.prim[s.hit.kind == 2].tolist())
            if it == 1:                                            # the paths that end on the light, against the oracle's own frame
                if k == 1:
                    frame = np.zeros(ts.W * ts.H * 3, np.float32)
                    ref.iterate(1, frame)
                    frame = frame.reshape(-1, 3)
                pix, add, _, _ = ts.ended_on_light(sc, paths[k - 1], paths[k], white=True)
                assert ts.same(frame[pix], add), (k, len(pix))
                on_light += len(pix)
    assert reached == {(t, c) for t in range(4) for c in range(16)}, sorted({(t, c) for t in range(4) for c in range(16)} - reached)
    assert meshes_hit == set(sc.meshes), (meshes_hit, set(sc.meshes))
    assert on_light >= 300, on_light


def test_the_cases_reach_every_textured_form(pt, oracle):
    T = pt.test_lib()
    assert "pt_test_renderer_state" in pt.TEST_ABI_SYMBOLS and hasattr(T, "pt_test_renderer_state") and not hasattr(pt.lib(), "pt_test_renderer_state")
    bits = C.c_uint32(0)
    T.pt_free()
    assert T.pt_test_renderer_state(C.byref(bits)) != 0 and T.pt_test_renderer_state(None) != 0      # (no renderer yet; no result pointer)
    forms = set()
    for name, lens, bump in ts.CASES:
        state = ts.build(pt, oracle, name, bump).state
        for first in (0, 1):
            got = C.c_uint32(0xffffffff)
            assert T.pt_test_bounce_form(ts.state_bits(state, dof=int(lens), first=first), C.byref(got)) == 0, T.pt_last_error()
            forms.add(got.value)
    bit = {n: 1 << i for i, n in enumerate(FORM)}
    want = {bit["TEX"] | b | f | g for b in (0, bit["BUMP"]) for f in (0, bit["FIRST"], bit["FIRST"] | bit["DOF"])
            for g in (0, bit["MANY"] | bit["CUBES"], bit["MESH"], bit["MANY"] | bit["CUBES"] | bit["MESH"])}
    assert len(want) == 24 and forms == want


def test_tilt_and_tangents_agree_with_the_kernels_restatement(pt, oracle):
    """random rays into the bumped mesh scene: (u, v), the tangents and the tilted normal of the float64 reference against
    bump_ref.evaluate (the kernel's fp32 arithmetic, fed the reference's own hits)"""
    sc = ts.build(pt, oracle, "mesh", True)
    rng = np.random.default_rng(812)
    o = rng.uniform(-4, 4, (20000, 3)) + [0, 5, 0]
    d = rng.normal(size=(20000, 3))
    hit = pr.cast(sc, o, d / np.linalg.norm(d, axis=1, keepdims=True))
    hit = pr.take(hit, (hit.prim >= 0) & ~hit.ambiguous & (sc.geom_bumps[hit.prim] >= 0))
    assert {int(k) for k in np.unique(hit.kind)} == {0, 1, 2} and len(hit.prim) > 2000
    u, v, bad = pr.uv(sc, hit)
    n = len(u)
    e = np.zeros((n, 40), np.float32)
    e[:, 0], e[:, 1], e[:, 2:5], e[:, 5:8] = sc.bump_scales[hit.prim], hit.outside, hit.N, hit.d
    e[:, 8:20] = sc.geoms["transform"][hit.prim].reshape(n, 4, 4)[:, :, :3].reshape(n, 12)      # (column-major: the columns' first three rows)
    e[:, 20:23] = hit.q
    e[hit.kind == 1, 23] = (hit.axis * 2 + (hit.sign > 0))[hit.kind == 1]
    for g in sc.meshes:
        m = hit.prim == g
        e[m, 20:22], e[m, 22:28], e[m, 28:37] = hit.bary[m], sc.mesh_uvs[g][hit.tri[m]], sc.meshes[g][hit.tri[m]]
    out = br.evaluate(ts.ramp()[:, :, 0], hit.kind, e)
    assert np.abs(out[:, 12] - u).max() < 1e-5 and np.abs(out[:, 13] - v).max() < 1e-5
    x, y = (u - np.floor(u)) * ts.SPEC[0], (v - np.floor(v)) * ts.SPEC[0]
    clear = ~bad & (np.minimum(x, ts.SPEC[0] - x) > 2.5) & (np.minimum(y, ts.SPEC[0] - y) > 2.5)
    assert clear.mean() > 0.7
    s = sc.bump_scales[hit.prim].astype(np.float64)
    su, sv = s * ts.SLOPE_U, s * ts.SLOPE_V                           # the ramp's gradient away from its wrap
    assert np.abs(out[clear, 0] - su[clear]).max() < 1e-4 and np.abs(out[clear, 1] - sv[clear]).max() < 1e-4
    Pu, Pv = pr.tangents(sc, hit)
    scale = np.abs(out[:, 2:8]).max(1, keepdims=True)
    assert (np.abs(out[clear, 2:5] - Pu[clear]) < 1e-5 * scale[clear]).all() and (np.abs(out[clear, 5:8] - Pv[clear]) < 1e-5 * scale[clear]).all()
    Ns, shaky = pr.tilt(hit.N, Pu, Pv, su, sv, hit.outside, hit.d)
    ok = clear & ~shaky
    assert np.abs(out[ok, 8:11] - Ns[ok]).max() < 1e-5
    assert (out[ok, 11] == 1).mean() > 0.8                          # (most of them tilted, the rest turned away from the ray and left flat)
    assert (np.abs(out[ok, 8:11] - hit.N[ok]).max(1) > 1e-2).mean() > 0.8
