"""Object history (PT_FLAG_OBJECT_HISTORY) on the MI355X, every comparison bit for bit against the numpy restatement
(tests/temporal_motion_ref.py): all fourteen instantiations of k_temporal over synthetic arrays whose branches
tests/test_temporal_motion_cpu.py counts; the rendered cases of tests/object_motion_scenes.py at 1, 2 and 4 new samples -- the captured
history, the motion table, pt_denoise_var in every level form, the display's bytes --; a chain of views; that nothing moved is
PT_FLAG_TEMPORAL; every drop rule alone; the unflagged renderer; the refusals; pt_render --history-move; PT_FLAG_KEEP_RENDERER."""
import os
import subprocess

import numpy as np
import pytest

import demod_ref as dm
import denoise_ref as dr
import denoise_var_ref as dv
import object_motion_scenes as oms
import spatial_var_ref as sv
import temporal_demod_ref as td
import temporal_motion_ref as tm
import temporal_ref as tr
from conftest import ROOT, SCENES
from test_gpu_temporal import _same_but_nans

pytestmark = pytest.mark.gpu
F = np.float32
SIGMAS = (4.0, 0.35, 2.0)
W, H, DEPTH = oms.W, oms.H, oms.DEPTH
OLD = 16
EXE = os.path.join(ROOT, "project3-cuda-path-tracer_amd", "host", "pt_render")
HIST_KEYS = ("hc", "hn", "hpos_t", "hnrm_id", "cam")


@pytest.fixture(scope="module")
def gpu(pt):
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return pt


def _bits(a):
    return np.ascontiguousarray(a, F).reshape(-1).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---- 1: the kernel, all fourteen instantiations ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(37, 23), (70, 5)])
def test_all_fourteen_forms_on_synthetic_arrays(gpu, w, h):
    """851 and 350 pixels -- the last block is partial -- under a table that mixes states 0, 1 and 2: a translation, a rotation, a non-uniform
    scale, all three at once and a singular G.  The MOTION = false forms go through the entry points they had and give what they gave."""
    n = 3
    S, Q, pos_t, nrm_id, hc, hn, hpos, hnrm_id, cam, rows = tm.synthetic(w, h, 11 * w + h)
    rng = np.random.default_rng(w)
    special = np.array([np.nan, np.inf, 0.0, -0.0, 1e-40, 3e38], F)
    ha = rng.uniform(0, 1, (h, w, 4)).astype(F)
    m = rng.uniform(0, 1, ha.shape) < 0.05
    ha[m] = rng.choice(special, int(m.sum()))
    asum = (rng.uniform(0, 1, (h, w, 4)) * n).astype(F)
    m = rng.uniform(0, 1, asum.shape) < 0.08
    asum[m] = rng.choice(np.array([0.0, np.nan, 1e-3, np.inf], F), int(m.sum()))
    hist5, hist6 = (hc, hn, hpos, hnrm_id, cam), (hc, hn, hpos, hnrm_id, cam, ha)
    cap = float(tm.object_cap())
    assert float(tm.history_cap(rows)) == cap
    args = (w, h, n, S, Q, pos_t, nrm_id, hc, hn, hpos, hnrm_id, cam)
    # MOTION = true, ALBEDO = false: filter, capture, moments
    want_c, want_v = tm.filter_form(S, Q, n, pos_t, nrm_id, hist5, rows)
    out, _, _ = gpu.test_temporal_motion(0, False, True, *args, rows=rows, hist_cap=cap)
    assert _same_but_nans(out[:, :3], want_c) and _same_but_nans(out[:, 3], want_v)
    plain_c, plain_v = tr.filter_form(S, Q, n, pos_t, nrm_id, *hist5)
    assert not _same_but_nans(want_c, plain_c)                                   # (the table matters)
    want_hc, want_hn = tm.capture_form(S, Q, n, pos_t, nrm_id, hist5, rows)
    out, out_n, _ = gpu.test_temporal_motion(1, False, True, *args, rows=rows, hist_cap=cap)
    assert _same_but_nans(out, want_hc) and _same_but_nans(out_n, want_hn)
    want_m, want_n = tm.moments_form(S, Q, n, pos_t, nrm_id, hist5, rows)
    out, out_n, _ = gpu.test_temporal_motion(2, False, True, *args, rows=rows, hist_cap=cap)
    assert _same_but_nans(out, want_m) and _same_but_nans(out_n, want_n)
    # MOTION = true, ALBEDO = true: filter, capture, moments and the fused demodulating filter
    want_a = tm.albedo_form(asum, n, pos_t, nrm_id, hist6, rows)
    for form, (wa, wb) in ((0, (np.concatenate([want_c, want_v[..., None]], 2), None)), (1, (want_hc, want_hn)), (2, (want_m, want_n))):
        out, out_n, out_a = gpu.test_temporal_motion(form, True, True, *args, rows=rows, hist_cap=cap, asum=asum, ha=ha)
        assert _same_but_nans(out, wa) and _same_but_nans(out_a, want_a) and (wb is None or _same_but_nans(out_n, wb)), form
    cd, vd = dm.demodulate(want_c, want_v, want_a, 1, dm.MIN_ALBEDO)
    out, _, out_a = gpu.test_temporal_motion(3, True, True, *args, rows=rows, hist_cap=cap, asum=asum, ha=ha)
    assert _same_but_nans(out[:, :3], cd) and _same_but_nans(out[:, 3], vd) and _same_but_nans(out_a, want_a)
    # another cap is another result; a table of unmoved rows under MOTION = true is the MOTION = false kernel's result
    out32, _, _ = gpu.test_temporal_motion(0, False, True, *args, rows=rows, hist_cap=32.0)
    assert _same_but_nans(out32[:, :3], tm.filter_form(S, Q, n, pos_t, nrm_id, hist5, rows, cap=32.0)[0]) and not _same_but_nans(out32[:, :3], want_c)
    still = np.stack([tm.row_of(tm._affine(), tm.UNMOVED)] * len(rows))
    out0, _, _ = gpu.test_temporal_motion(0, False, True, *args, rows=still, hist_cap=32.0)
    assert _same_but_nans(out0[:, :3], plain_c) and _same_but_nans(out0[:, 3], plain_v)
    # MOTION = false: the seven forms through the old entry points, and through the new one, are temporal_ref's / temporal_demod_ref's
    old = gpu.test_temporal(False, *args)
    assert _same_but_nans(old[:, :3], plain_c) and _same_but_nans(old[:, 3], plain_v)
    assert _same_but_nans(gpu.test_temporal_motion(0, False, False, *args)[0], old)
    o, on = gpu.test_temporal(True, *args)
    phc, phn = tr.capture_form(S, Q, n, pos_t, nrm_id, *hist5)
    assert _same_but_nans(o, phc) and _same_but_nans(on, phn)
    o, on = gpu.test_temporal(2, *args)
    pm, pn = sv.moments_form(S, Q, n, pos_t, nrm_id, hist5)
    assert _same_but_nans(o, pm) and _same_but_nans(on, pn)
    pa = td.albedo_form(asum, n, pos_t, nrm_id, hist6)
    common = (w, h, n, S, Q, pos_t, nrm_id, asum, hc, hn, ha, hpos, hnrm_id, cam)
    for form, wa in ((0, np.concatenate([plain_c, plain_v[..., None]], 2)), (1, phc), (2, pm)):
        o, _, oa = gpu.test_temporal_albedo(form, *common)
        assert _same_but_nans(o, wa) and _same_but_nans(oa, pa), form
    fused, _, fa = gpu.test_temporal_albedo(0, *common, front=1)
    assert _same_but_nans(fused, td.demodulated_front(S, Q, asum, n, pos_t, nrm_id, hist6, SIGMAS[1], SIGMAS[2])[0]) and _same_but_nans(fa, pa)
    assert _same_but_nans(gpu.test_temporal_motion(3, True, False, *args, asum=asum, ha=ha)[0], fused)


# ---- the rendered cases -------------------------------------------------------------------------------------------------------------------
def _kind(case, **over):
    k = dict(temporal=True, object_history=True, spatial_variance=True, max_batch=16)
    if case["demod"]:
        k.update(demodulate=True, demod_history=True)
    k.update(over)
    return k


def _init(pt, case, new, free=False, geoms=None, eye=None, **over):
    sc = case["scene"]
    sc.geoms = np.ascontiguousarray(case["new_geoms"] if new else case["old_geoms"]) if geoms is None else np.ascontiguousarray(geoms)
    sc.camera["position"][0] = (case["eye1"] if new else case["eye0"]) if eye is None else eye
    if free:
        pt.pathtraceFree()
    pt.pathtraceInit(sc, traceDepth=DEPTH, moments=True, **_kind(case, **over))


def _state(pt, case=None):
    """(S, Q, pos_t, nrm_id[, asum]) of the current renderer, the guides of iteration 1 as the device holds them"""
    out = (pt.readback(W * H).reshape(H, W, 3), pt.readback_moments().reshape(H, W)) + tr.pack_guides(*pt.gbuffer(1), H, W)
    return out + ((pt.test_albedo().reshape(H, W, 4),) if case is not None and case["demod"] else (None,))


def _empty(case):
    return td.empty_history(H, W) if case["demod"] else tr.empty_history(H, W)


def _case(pt, orc, name):
    c = oms.build(pt, orc, name)
    c["old_geoms"] = np.array(c["scene"].geoms, copy=True)
    return c


def _history_is(got, hist, rows, ha=None):
    if got is None or not all(_same(got[k], hist[i]) for i, k in enumerate(HIST_KEYS)):
        return False
    if rows is None:
        return got["motion"] is None and got["cap"] == float(tr.constants()[0])
    return got["motion"] is not None and _same(got["motion"], rows) and got["cap"] == float(tm.object_cap()) and (ha is None or _same(ha, hist[5]))


@pytest.fixture(scope="module")
def rendered(gpu, oracle):
    """Per case, by the test library's renderer (the product's kernels, its own instance): 16 iterations of the old view, the
    re-initialisation with the new geoms, then 1, 2 and 4 iterations there.  Computed once; the tests below read it."""
    out = {}
    with gpu.renderer_from_test_library():
        for name in oms.NAMES:
            c = _case(gpu, oracle, name)
            _init(gpu, c, False, free=True)
            cam0 = gpu.test_temporal_camera(c["scene"].camera)
            gpu.pathtrace_batch(None, 0, 1, OLD)
            S0, Q0, p0, n0, a0 = _state(gpu, c)
            _init(gpu, c, True)
            rec = dict(case=c, hist=tm.capture(S0, Q0, OLD, p0, n0, cam0, _empty(c), None, a0), got=gpu.test_history(),
                       got_ha=gpu.test_history_albedo() if c["demod"] else None, rows=tm.motion_table(c["old_geoms"], c["new_geoms"])[0], at={})
            done = 0
            for n in (1, 2, 4):
                gpu.pathtrace_batch(None, 0, OLD + done + 1, n - done)
                done = n
                S, Q, pos_t, nrm_id, asum = _state(gpu, c)
                rec["at"][n] = dict(S=S, Q=Q, g=(pos_t, nrm_id), asum=asum, dv=gpu.denoise_var(n, 5, *SIGMAS, with_variance=True),
                                    forms=[gpu.test_denoise_var(n, form, 5, *SIGMAS) for form in (0, 1, 2, 3)], rgba=gpu.denoise_var_rgba8(n, 5, *SIGMAS))
            out[name] = rec
        gpu.pathtraceFree()
    return out


@pytest.mark.parametrize("name", oms.NAMES)
def test_a_moved_object_keeps_its_history(gpu, rendered, name):
    """the captured history, the table as the device holds it, pt_denoise_var in every level form and the display's bytes at 1 (under
    PT_FLAG_SPATIAL_VARIANCE), 2 and 4 new samples"""
    rec = rendered[name]
    c, hist, rows = rec["case"], rec["hist"], rec["rows"]
    assert _history_is(rec["got"], hist, rows, rec["got_ha"])
    st = tm.states(rows)
    assert all(st[g] != 0 for g in c["moved"]) and (st != 0).sum() == len(c["moved"])
    for n in (1, 2, 4):
        at = rec["at"][n]
        want, wantv = tm.denoise_var(at["S"], at["Q"], n, *at["g"], hist, rows, 5, *SIGMAS, asum=at["asum"])
        assert np.isfinite(want).all()
        assert _same(at["dv"][0], want) and _same(at["dv"][1], wantv), n
        assert np.array_equal(at["rgba"], dr.to_rgba8(want)), n
        for form, (o, v) in enumerate(at["forms"]):
            assert _same(o, want) and _same(v, wantv), (n, form)
        # the moved primitive's pixels do find history, and neither the unflagged reading nor a dropped history gives this frame
        ids = np.ascontiguousarray(at["g"][1][..., 3]).view(np.int32)
        Nh = tm.reproject(*at["g"], *hist[:5], rows=rows)[1]
        follows = [g for g in c["moved"] if st[g] == tm.MOVED]
        assert all(((ids == g) & (Nh > 0)).sum() >= 100 and ((ids == g) & (Nh == 0)).sum() >= 20 for g in follows), n
        assert all(not ((ids == g) & (Nh > 0)).any() for g in c["moved"] if st[g] == tm.NO_HISTORY)
        assert Nh.max() <= float(tm.object_cap())
        assert not _same(want, tm.denoise_var(at["S"], at["Q"], n, *at["g"], hist, None, 5, *SIGMAS, asum=at["asum"])[0])


def _pbo():
    import torch
    t = torch.full((W * H, 4), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def test_the_display_path_follows_the_object_and_allocates_nothing(gpu, oracle):
    """PT_FLAG_DISPLAY_FILTER: the bytes pt_iterate writes at 1 and 2 samples are the restatement's, and nothing is allocated after pt_init --
    the table is pt_init's upload"""
    c = _case(gpu, oracle, "sphere")
    live = gpu.test_lib().pt_test_live_device_buffers
    pbo = _pbo()
    try:
        with gpu.renderer_from_test_library():
            _init(gpu, c, False, free=True, display_filter=True)
            cam0 = gpu.test_temporal_camera(c["scene"].camera)
            gpu.pathtrace_batch(None, 0, 1, OLD)
            S0, Q0, p0, n0, _ = _state(gpu, c)
            _init(gpu, c, True, display_filter=True)
            hist, rows = tm.capture(S0, Q0, OLD, p0, n0, cam0, _empty(c)), tm.motion_table(c["old_geoms"], c["new_geoms"])[0]
            before = live()
            for n in (1, 2):
                gpu.pathtrace(pbo.data_ptr(), 0, n, readback=False)
                gpu.sync()
                assert live() == before
                shown = pbo.cpu().numpy()
                S, Q, pos_t, nrm_id, _ = _state(gpu, c)
                want = tm.display_bytes(S, Q, n, pos_t, nrm_id, hist, rows, 5, *SIGMAS)
                assert np.array_equal(shown, want) and np.array_equal(gpu.readback_rgba8(n, W * H), want), n
            gpu.pathtraceFree()
            assert live() == 0
    finally:
        del pbo


# ---- chains ---------------------------------------------------------------------------------------------------------------------------------
def test_a_chain_of_views_each_with_another_object_moved_then_a_same_scene_move(gpu, oracle):
    """View 0 -> 1: the sphere moves.  1 -> 2: the left wall moves (and the sphere stays where view 1 put it).  2 -> 3: the right wall.  The
    capture at a view's pt_init reprojects the going view's samples with the table that view got at ITS pt_init; only then is the table for
    the coming view made.  View 3 commits nothing, so 3 -> 4 (the sphere again) captures nothing and its table reaches two moves back.
    Last, pt_init's same-scene form: no table, and the results are PT_FLAG_TEMPORAL's (the restatement without a table)."""
    c = _case(gpu, oracle, "sphere")
    g0, g1 = c["old_geoms"], c["new_geoms"]
    g2 = tm.moved_geoms(oracle, g1, {4: ((-4.6, 5.0, 0.0), None, None)})
    with gpu.renderer_from_test_library():
        _init(gpu, c, False, free=True)
        cams = [gpu.test_temporal_camera(c["scene"].camera)]
        gpu.pathtrace_batch(None, 0, 1, 8)
        s0 = _state(gpu)
        _init(gpu, c, True)
        hist1, rows01 = tm.capture(s0[0], s0[1], 8, s0[2], s0[3], cams[0], _empty(c)), tm.motion_table(g0, g1)[0]
        assert _history_is(gpu.test_history(), hist1, rows01)
        gpu.pathtrace_batch(None, 0, 9, 4)
        s1 = _state(gpu)
        _init(gpu, c, True, geoms=g2, eye=(-0.3, 4.4, 2.5))
        cam1 = cams[0]                                       # (view 1 kept view 0's eye)
        hist2, rows12 = tm.capture(s1[0], s1[1], 4, s1[2], s1[3], cam1, hist1, rows01), tm.motion_table(g1, g2)[0]
        assert tm.states(rows01).tolist() == [0, 0, 0, 0, 0, 0, 1] and tm.states(rows12).tolist() == [0, 0, 0, 0, 1, 0, 0]
        assert _history_is(gpu.test_history(), hist2, rows12)
        assert not _same(hist2[0], tm.capture(s1[0], s1[1], 4, s1[2], s1[3], cam1, hist1, None)[0])      # (the capture did go through rows01)
        cam2 = gpu.test_temporal_camera(c["scene"].camera)
        gpu.pathtrace_batch(None, 0, 13, 2)
        s2 = _state(gpu)
        want, wantv = tm.denoise_var(s2[0], s2[1], 2, s2[2], s2[3], hist2, rows12, 5, *SIGMAS)
        got, gotv = gpu.denoise_var(2, 5, *SIGMAS, with_variance=True)
        assert _same(got, want) and _same(gotv, wantv)
        # 2 -> 3: a third object, the right wall
        g3 = tm.moved_geoms(oracle, g2, {5: ((4.7, 5.0, 0.0), None, None)})
        _init(gpu, c, True, geoms=g3, eye=(-0.2, 4.35, 2.55))
        hist3, rows23 = tm.capture(s2[0], s2[1], 2, s2[2], s2[3], cam2, hist2, rows12), tm.motion_table(g2, g3)[0]
        assert tm.states(rows23).tolist() == [0, 0, 0, 0, 0, 1, 0] and _history_is(gpu.test_history(), hist3, rows23)
        # 3 -> 4 with nothing committed in view 3: no capture is due, the history stays view 2's -- its samples, guides and camera, in view 2's
        # poses -- and the table for view 4 spans BOTH moves since: the wall's of view 3 and the sphere's of view 4
        g4 = tm.moved_geoms(oracle, g3, {6: ((0.4, 4.1, -0.9), None, None)})
        _init(gpu, c, True, geoms=g4, eye=(-0.2, 4.35, 2.55))
        rows24 = tm.motion_table(g2, g4)[0]
        assert tm.states(rows24).tolist() == [0, 0, 0, 0, 0, 1, 1] and tm.states(tm.motion_table(g3, g4)[0]).tolist() == [0, 0, 0, 0, 0, 0, 1]
        assert _history_is(gpu.test_history(), hist3, rows24)
        cam4 = gpu.test_temporal_camera(c["scene"].camera)
        gpu.pathtrace_batch(None, 0, 15, 2)
        s4 = _state(gpu)
        want, wantv = tm.denoise_var(s4[0], s4[1], 2, s4[2], s4[3], hist3, rows24, 5, *SIGMAS)
        got, gotv = gpu.denoise_var(2, 5, *SIGMAS, with_variance=True)
        assert _same(got, want) and _same(gotv, wantv)
        # the same-scene form
        cam = c["scene"].camera.copy()
        cam["position"][0] = (-0.1, 4.3, 2.6)
        gpu.pathtraceSetCamera(cam)
        assert gpu.camera_move_info()["fast"] is True
        hist5 = tm.capture(s4[0], s4[1], 2, s4[2], s4[3], cam4, hist3, rows24)
        assert _history_is(gpu.test_history(), hist5, None)
        gpu.pathtrace_batch(None, 0, 17, 2)
        s5 = _state(gpu)
        want, wantv = tr.denoise_var_temporal(s5[0], s5[1], 2, s5[2], s5[3], hist5, 5, *SIGMAS)
        got, gotv = gpu.denoise_var(2, 5, *SIGMAS, with_variance=True)
        assert _same(got, want) and _same(gotv, wantv)
        gpu.pathtraceFree()


def test_nothing_moved_is_the_temporal_renderer_in_every_output(gpu, oracle):
    """a flagged renderer re-initialised with identical geoms (and another eye) against the PT_FLAG_TEMPORAL renderer: no table, the same bits"""
    c = _case(gpu, oracle, "camera")
    res = {}
    with gpu.renderer_from_test_library():
        for flagged in (False, True):
            _init(gpu, c, False, free=True, object_history=flagged)
            gpu.pathtrace_batch(None, 0, 1, 8)
            _init(gpu, c, False, eye=c["eye1"], object_history=flagged)
            h = gpu.test_history()
            assert h["motion"] is None and h["cap"] == 32.0
            out = {k: h[k] for k in HIST_KEYS}
            for n in (1, 2):
                gpu.pathtrace_batch(None, 0, 8 + n, 1)
                dvn = gpu.denoise_var(n, 5, *SIGMAS, with_variance=True)
                out.update({"S%d" % n: gpu.readback(W * H), "Q%d" % n: gpu.readback_moments(), "dv%d" % n: dvn[0], "var%d" % n: dvn[1],
                            "rgba%d" % n: gpu.denoise_var_rgba8(n).view(F), "plain%d" % n: gpu.denoise(n)})
            out["variance"] = gpu.variance(2)
            res[flagged] = out
        gpu.pathtraceFree()
    diff = [k for k in res[False] if not _same(res[False][k], res[True][k])]
    assert not diff, diff


# ---- drop rules, each alone ----------------------------------------------------------------------------------------------------------------
def _no_history_frame(gpu, case, n=2):
    """the renderer's pt_denoise_var against the restatement of a renderer WITHOUT history, bit for bit"""
    S, Q, pos_t, nrm_id, asum = _state(gpu, case)
    geom = np.ascontiguousarray(nrm_id[..., 3]).view(np.int32)
    if case["demod"]:
        want = dm.denoise_var_demod(S, Q, asum, n, pos_t[..., :3], nrm_id[..., :3], geom, 5, *SIGMAS)[0]
    else:
        want = dv.denoise_var(S, Q, n, pos_t[..., :3], nrm_id[..., :3], geom, 5, *SIGMAS)[0]
    return _same(gpu.denoise_var(n, 5, *SIGMAS), want)


def _drop(gpu, case, change, **new_kind):
    """old view, 2 iterations; `change` edits the scene; the re-initialisation; 2 iterations: no history, and a frame made without one"""
    _init(gpu, case, False, free=True)
    gpu.pathtrace_batch(None, 0, 1, 2)
    change(case["scene"])
    sc = case["scene"]
    gpu.pathtraceInit(sc, traceDepth=DEPTH, moments=True, **_kind(case, **new_kind))
    assert gpu.test_history() is None
    gpu.pathtrace_batch(None, 0, 3, 2)
    assert _no_history_frame(gpu, case)


def test_every_other_difference_drops_the_history(gpu, oracle):
    with gpu.renderer_from_test_library():
        def plain():
            return _case(gpu, oracle, "sphere")

        def textured():
            return _case(gpu, oracle, "mesh")
        # control: the same calls with nothing but the pose changed keep it
        c = plain()
        _init(gpu, c, False, free=True)
        gpu.pathtrace_batch(None, 0, 1, 2)
        _init(gpu, c, True)
        assert gpu.test_history() is not None and gpu.test_history()["motion"] is not None
        # another ngeoms
        extra = np.asarray(oracle.make_geom(0, 2, (2.2, 3.0, -0.5), (0, 0, 0), (1, 1, 1))).view(c["old_geoms"].dtype)
        _drop(gpu, plain(), lambda sc: setattr(sc, "geoms", np.concatenate([sc.geoms, extra])))
        # a type (the sphere becomes a cube), a materialid

        def retype(sc):
            sc.geoms = sc.geoms.copy()
            sc.geoms["type"][6] = 1

        def rematerial(sc):
            sc.geoms = sc.geoms.copy()
            sc.geoms["materialid"][6] = 1

        def recolour(sc):                                    # one material byte
            sc.materials = sc.materials.copy()
            b = sc.materials.view(np.uint8).reshape(-1)
            b[4 * 11] ^= 1                                   # (the lowest mantissa bit of material 1's red)
        _drop(gpu, plain(), retype)
        _drop(gpu, plain(), rematerial)
        _drop(gpu, plain(), recolour)
        # one texel, one triangle (the registrations; the textured scene, under PT_FLAG_DEMOD_HISTORY)

        def retexel(sc):
            sc.textures = [t.copy() for t in sc.textures]
            sc.textures[0][0, 0, 0] = np.nextafter(sc.textures[0][0, 0, 0], F(2))

        def retriangle(sc):
            q = sc.named["quad"]
            sc.meshes = dict(sc.meshes)
            sc.meshes[q] = sc.meshes[q].copy()
            sc.meshes[q][0, 0] = np.nextafter(sc.meshes[q][0, 0], F(-2))
        _drop(gpu, textured(), retexel)
        _drop(gpu, textured(), retriangle)
        # the flag on one side only, either side
        _drop(gpu, plain(), lambda sc: None, object_history=False)
        c = plain()
        _init(gpu, c, False, free=True, object_history=False)
        gpu.pathtrace_batch(None, 0, 1, 2)
        _init(gpu, c, True)
        assert gpu.test_history() is None
        gpu.pathtraceFree()


def test_a_refused_call_leaves_the_history_and_the_renderer(gpu, oracle):
    c = _case(gpu, oracle, "sphere")
    with gpu.renderer_from_test_library():
        _init(gpu, c, False, free=True)
        gpu.pathtrace_batch(None, 0, 1, 4)
        _init(gpu, c, True)
        gpu.pathtrace_batch(None, 0, 5, 2)
        before, S = gpu.test_history(), gpu.readback(W * H)
        assert before["motion"] is not None
        sc = c["scene"]
        for bad, msg in ((dict(temporal=True, object_history=True, lens_radius=0.1, focal_distance=5.0), "PT_FLAG_TEMPORAL"),
                         (dict(object_history=True), "PT_FLAG_OBJECT_HISTORY"), (dict(temporal=True, object_history=True, trace_ahead=True), "PT_FLAG_TEMPORAL")):
            with pytest.raises(gpu.PtError, match="pt_amd error -1.*" + msg):
                gpu.pathtraceInit(sc, traceDepth=DEPTH, moments=True, **bad)
        with pytest.raises(gpu.PtError, match="pt_amd error -1.*PT_FLAG_MOMENTS"):                 # (PT_FLAG_TEMPORAL's own refusal comes first)
            gpu.pathtraceInit(sc, traceDepth=DEPTH, temporal=True, object_history=True)
        after = gpu.test_history()
        assert all(_same(before[k], after[k]) for k in HIST_KEYS) and _same(before["motion"], after["motion"]) and before["cap"] == after["cap"]
        assert _same(gpu.readback(W * H), S)
        gpu.pathtraceFree()
        assert gpu.test_history() is None and gpu.test_lib().pt_test_live_device_buffers() == 0


def test_a_group_refuses_the_flag(gpu):
    sc = gpu.Scene(os.path.join(SCENES, "cornell.txt"))
    sc.set_resolution(W, H)
    g = gpu.Group(2, devices=[0, 0])
    try:
        with pytest.raises(gpu.PtError, match="error -1.*PT_FLAG_OBJECT_HISTORY"):
            g.init(sc, traceDepth=3, flags=gpu.PT_FLAG_OBJECT_HISTORY)
        g.init(sc, traceDepth=3)                         # (and is as usable as before)
    finally:
        g.destroy()


# ---- the unflagged renderer ------------------------------------------------------------------------------------------------------------------
def test_without_the_flag_a_moved_object_is_reprojected_as_before(gpu, oracle):
    """PT_FLAG_TEMPORAL alone, the promise broken: the history is kept, no table is made, and pt_denoise_var is temporal_ref's"""
    c = _case(gpu, oracle, "sphere")
    with gpu.renderer_from_test_library():
        _init(gpu, c, False, free=True, object_history=False)
        cam0 = gpu.test_temporal_camera(c["scene"].camera)
        gpu.pathtrace_batch(None, 0, 1, 8)
        s0 = _state(gpu)
        _init(gpu, c, True, object_history=False)
        hist = tm.capture(s0[0], s0[1], 8, s0[2], s0[3], cam0, _empty(c))
        assert _history_is(gpu.test_history(), hist, None)
        gpu.pathtrace_batch(None, 0, 9, 2)
        s1 = _state(gpu)
        want, wantv = tr.denoise_var_temporal(s1[0], s1[1], 2, s1[2], s1[3], hist, 5, *SIGMAS)
        got, gotv = gpu.denoise_var(2, 5, *SIGMAS, with_variance=True)
        assert _same(got, want) and _same(gotv, wantv)
        gpu.pathtraceFree()


# ---- PT_FLAG_KEEP_RENDERER ------------------------------------------------------------------------------------------------------------------
def test_keep_renderer_with_changed_geoms_takes_the_full_call_and_captures_with_motion(gpu, oracle):
    c = _case(gpu, oracle, "sphere")
    with gpu.renderer_from_test_library():
        _init(gpu, c, False, free=True, keep=True)
        cam0 = gpu.test_temporal_camera(c["scene"].camera)
        gpu.pathtrace_batch(None, 0, 1, 4)
        s0 = _state(gpu)
        _init(gpu, c, True, keep=True)
        assert gpu.camera_move_info()["fast"] is None and gpu.keep_mismatch() == "geoms"
        hist1, rows = tm.capture(s0[0], s0[1], 4, s0[2], s0[3], cam0, _empty(c)), tm.motion_table(c["old_geoms"], c["new_geoms"])[0]
        assert _history_is(gpu.test_history(), hist1, rows)
        gpu.pathtrace_batch(None, 0, 5, 2)
        s1 = _state(gpu)
        # the same call again with another eye: the move in place -- and its capture goes through the table
        _init(gpu, c, True, keep=True, eye=(-0.2, 4.3, 2.5))
        assert gpu.camera_move_info()["fast"] is True
        hist2 = tm.capture(s1[0], s1[1], 2, s1[2], s1[3], cam0, hist1, rows)
        assert _history_is(gpu.test_history(), hist2, None)
        gpu.pathtraceFree()


# ---- the headless driver ------------------------------------------------------------------------------------------------------------------
def test_pt_render_history_move(gpu, oracle, tmp_path):
    """--history-move 6 0.9 0.1 0.4 0 25 0: the history view shows the sphere displaced (and turned) from the file's pose, the final view
    the file's; against the Python path, byte for byte"""
    from test_host import _decode_png
    w, h = 64, 48
    scene = os.path.join(SCENES, "cornell.txt")
    args = [EXE, scene, "--res", str(w), str(h), "--iterations", "2", "--depth", "4", "--denoise-var", "5", "4.0", "0.35", "2.0",
            "--history-from", "0.3", "5.0", "10.5", "6"]
    move = ["--history-move", "6", "0.9", "0.1", "0.4", "0", "25", "0"]
    for name, extra in (("t", []), ("m", move)):
        r = subprocess.run(args + extra + ["--out", str(tmp_path / name)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (name, r.stderr[-2000:])
    r = subprocess.run(args[:-5] + move, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--history-move needs" in r.stderr
    sc = gpu.Scene(scene)
    sc.set_resolution(w, h)
    home = tuple(float(v) for v in sc.camera["position"][0])
    now = np.array(sc.geoms, copy=True)
    t = tuple(float(a) + b for a, b in zip(now["translation"][6], (0.9, 0.1, 0.4)))
    r_ = tuple(float(a) + b for a, b in zip(now["rotation"][6], (0.0, 25.0, 0.0)))
    then = tm.moved_geoms(oracle, now, {6: (t, r_, None)})
    ns = lambda geoms: __import__("types").SimpleNamespace(geoms=geoms, materials=sc.materials, camera=sc.camera, traceDepth=4, meshes={}, mesh_normals={},
                                                           mesh_materials={}, image=np.zeros((h, w, 3), F))
    try:
        sc.camera["position"][0] = (0.3, 5.0, 10.5)
        gpu.pathtraceFree()
        gpu.pathtraceInit(ns(then), traceDepth=4, moments=True, temporal=True, object_history=True, max_batch=8)
        gpu.pathtrace_batch(None, 0, 1, 6)
        sc.camera["position"][0] = home
        gpu.pathtraceInit(ns(now), traceDepth=4, moments=True, temporal=True, object_history=True, max_batch=8)
        gpu.pathtrace_batch(None, 0, 7, 2)
        frame = gpu.readback(w * h).reshape(h, w, 3) / F(2)
        mean = gpu.denoise_var(2, 5, 4.0, 0.35, 2.0).reshape(h, w, 3)
    finally:
        gpu.pathtraceFree()
    conv = lambda m: (np.clip(m, 0, 1) * F(255)).astype(np.uint8)[:, ::-1]          # the driver's PNG conversion, X mirrored
    got = _decode_png(str(tmp_path / "m.denoised.png"))
    assert np.array_equal(_decode_png(str(tmp_path / "m.png")), conv(frame))
    assert np.array_equal(got, conv(mean))
    assert not np.array_equal(got, _decode_png(str(tmp_path / "t.denoised.png")))
