"""Object history (PT_FLAG_OBJECT_HISTORY) on the host (no GPU): the flag and its refusals; that the numpy restatement
(tests/temporal_motion_ref.py) under a table of unmoved primitives is temporal_ref's bit for bit; the host's motion table against the
restatement's; an outside check of the reprojection that never forms the motion matrix; the ledger of the branches the GPU test's inputs take;
and the study on the CPU oracle that chooses PT_OBJECT_HISTORY_MAX and gives the README's numbers."""
import os
import re

import numpy as np
import pytest

import denoise_var_ref as dv
import object_motion_scenes as oms
import spatial_var_ref as sv
import temporal_demod_ref as td
import temporal_motion_ref as tm
import temporal_ref as tr
from conftest import ROOT, SCENES
from test_temporal_cpu import H, LEVELS, NEW, OLD, SIGMA_LUM, SIGMA_NORMAL, SIGMA_POSITION, W, _cornell, _rmse, _sphere_before_a_wall, _view

F = np.float32
EPS = 2.0 ** -24


def _bits(a):
    return np.ascontiguousarray(a, F).reshape(-1).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---- (a) the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_flag_value_entry_points_and_refusals(pt):
    hdr = open(os.path.join(ROOT, "include", "pt_amd.h")).read()
    thdr = open(os.path.join(ROOT, "include", "pt_amd_test.h")).read()
    assert re.search(r"PT_FLAG_OBJECT_HISTORY = 4096\b", hdr) and pt.PT_FLAG_OBJECT_HISTORY == 4096
    assert float(tm.object_cap()) == pt.PT_OBJECT_HISTORY_MAX and pt.PT_OBJECT_HISTORY_MAX in tm.CANDIDATE_CAPS
    assert pt.lib().pt_abi_version() == 7 and re.search(r"#define PT_AMD_ABI_VERSION 7\b", hdr)       # a flag: no function, no struct
    assert len(pt.ABI_SYMBOLS) == 47
    for s in ("pt_test_motion_table", "pt_test_history_motion", "pt_test_temporal_motion"):
        assert re.search(r"\bint %s\(" % s, thdr) and s in pt.TEST_ABI_SYMBOLS and hasattr(pt.test_lib(), s) and not hasattr(pt.lib(), s)
    sc = pt.Scene(os.path.join(SCENES, "cornell.txt"))
    sc.set_resolution(32, 24)
    O, T, M = pt.PT_FLAG_OBJECT_HISTORY, pt.PT_FLAG_TEMPORAL, pt.PT_FLAG_MOMENTS
    for bad in (dict(flags=O), dict(flags=O | M), dict(flags=O | T)):
        with pytest.raises(pt.PtError, match="pt_amd error -1"):
            pt.scene_plan(sc, **bad)
    with pytest.raises(pt.PtError, match="PT_FLAG_OBJECT_HISTORY"):
        pt.scene_plan(sc, flags=O | M)
    # every refusal of PT_FLAG_TEMPORAL stands
    for bad in (dict(flags=O | T | M | pt.PT_FLAG_TRACE_AHEAD, max_batch=4), dict(flags=O | T | M, lens_radius=0.1, focal_distance=5.0),
                dict(flags=O | T | M, shard_count=2)):
        with pytest.raises(pt.PtError, match="pt_amd error -1"):
            pt.scene_plan(sc, **bad)
    # what goes with it is planned, and the plan itself does not know of the flag
    D = pt.PT_FLAG_DEMODULATE | pt.PT_FLAG_DEMOD_HISTORY
    for extra in (0, D, pt.PT_FLAG_DISPLAY_FILTER, pt.PT_FLAG_SPATIAL_VARIANCE, pt.PT_FLAG_KEEP_RENDERER, pt.PT_FLAG_DIRECT_LIGHTING):
        assert bytes(pt.scene_plan(sc, flags=O | T | M | extra)) == bytes(pt.scene_plan(sc, flags=M | (extra & pt.PT_FLAG_DIRECT_LIGHTING)))


# ---- (b) nothing moved: temporal_ref's bits -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(37, 23), (70, 5)])
def test_a_table_of_unmoved_rows_is_temporal_ref_bit_for_bit(w, h):
    from test_gpu_temporal import _same_but_nans, _synthetic
    n = 3
    S, Q, pos_t, nrm_id, hc, hn, hpos, hnrm_id, cam = _synthetic(w, h, 11 * w + h)
    hist = (hc, hn, hpos, hnrm_id, cam)
    rng = np.random.default_rng(w)
    ha, asum = rng.uniform(0, 1, (h, w, 4)).astype(F), (rng.uniform(0, 1, (h, w, 4)) * n).astype(F)
    rows = np.stack([tm.row_of(tm._affine(), tm.UNMOVED)] * 3)
    assert float(tm.history_cap(rows)) == float(tr.constants()[0]) and float(tm.history_cap(None)) == float(tr.constants()[0])
    for table in (rows, None):
        assert all(_same_but_nans(a, b) for a, b in zip(tm.filter_form(S, Q, n, pos_t, nrm_id, hist, table), tr.filter_form(S, Q, n, pos_t, nrm_id, *hist)))
        assert all(_same_but_nans(a, b) for a, b in zip(tm.capture_form(S, Q, n, pos_t, nrm_id, hist, table), tr.capture_form(S, Q, n, pos_t, nrm_id, *hist)))
        assert all(_same_but_nans(a, b) for a, b in zip(tm.moments_form(S, Q, n, pos_t, nrm_id, hist, table), sv.moments_form(S, Q, n, pos_t, nrm_id, hist)))
        assert _same_but_nans(tm.albedo_form(asum, n, pos_t, nrm_id, hist + (ha,), table), td.albedo_form(asum, n, pos_t, nrm_id, hist + (ha,)))
    # ... and a row of another state takes the other cap
    rows[1] = tm.row_of(tm._affine(trans=(1, 0, 0)))
    assert float(tm.history_cap(rows)) == float(tm.object_cap())


# ---- the host's table ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases(pt, oracle):
    """per rendered case: the case, the oracle's guides of the old and the new view, the old camera and the restatement's table"""
    out = {}
    for name in oms.NAMES:
        c = oms.build(pt, oracle, name)
        (p0, n0), cam0 = oms.oracle_guides(oracle, c, False)
        (p1, n1), _ = oms.oracle_guides(oracle, c, True)
        out[name] = dict(case=c, old=(p0, n0), new=(p1, n1), cam0=cam0, rows=tm.motion_table(c["scene"].geoms, c["new_geoms"])[0])
    return out


def test_the_library_makes_the_restatements_table(pt, oracle, cases):
    """pt_init's function (host only) against float64 numpy, bit for bit: translations, a rotation with a non-uniform scale, a mesh, a zero
    scale (state 2: the inverse transpose is not finite), and identical geoms (no table kept)."""
    for name, rec in cases.items():
        c = rec["case"]
        rows, kept = pt.test_motion_table(c["scene"].geoms, c["new_geoms"])
        assert kept and _same(rows, rec["rows"]), name
        st = tm.states(rows)
        assert all(st[g] != 0 for g in c["moved"]) and (st != 0).sum() == len(c["moved"]), name
        same, kept = pt.test_motion_table(c["scene"].geoms, c["scene"].geoms.copy())
        assert not kept and (tm.states(same) == 0).all() and _same(same, tm.motion_table(c["scene"].geoms, c["scene"].geoms)[0])
    st = tm.states(cases["two"]["rows"])
    assert st[6] == tm.MOVED and st[7] == tm.NO_HISTORY and not np.isfinite(cases["two"]["rows"][7]).all()
    # the reverse of "two" -- a primitive that loses its extent -- is state 2 as well: the new inverse is not finite
    c = cases["two"]["case"]
    assert tm.states(pt.test_motion_table(c["new_geoms"], c["scene"].geoms)[0])[7] == tm.NO_HISTORY


# ---- (c) an outside check that never forms A ---------------------------------------------------------------------------------------------
def _f64_projection(P, geom_then, geom_now, camera):
    """(s, u, v) in float64: the new hit to object space by the new inverse, to the old world by the old transform, into the old camera by
    solving [view | -right | -up] (s, s a, s b) = P_old - e with the camera's fp32 constants taken as exact"""
    Ti, T = tm._mat(geom_now, "inverseTransform"), tm._mat(geom_then, "transform")
    P4 = np.concatenate([np.asarray(P, np.float64), np.ones(P.shape[:-1] + (1,))], axis=-1)
    obj = P4 @ Ti.T
    old = (obj @ T.T)[..., :3]
    view, up, right, e, plx, ply, hw, hh = (np.asarray(x, np.float64) for x in tr.camera_constants(camera))
    sol = np.linalg.solve(np.stack([view, -right, -up], axis=1), (old - e).T).T
    s = sol[..., 0]
    return s, sol[..., 1] / s / plx + hw - 0.5, sol[..., 2] / s / ply + hh - 0.5


@pytest.mark.parametrize("name", ["camera", "cube"])
def test_reprojection_agrees_with_a_float64_composition(cases, name):
    """The restatement's (u, v) of the moved primitive's pixels against float64 that reads the two matrices separately.  The bound, per pixel,
    to first order in eps = 2^-24 and doubled for the second order:
      P'.k   three products, three sums, and the row's entries rounded once: 7 eps M_k,  M_k = sum_j |m_kj| |P_j| + |m_k3|
      d = P' - e: one more rounding, eps |d_k|
      a dot with a row of the camera's inverse (its entries rounded once, three products, two sums): sum_i |r_i| dd_i + 6 eps sum_i |r_i| |d_i|
      a = num / s: (dnum + |a| ds) / s + eps |a|;  u = (a / pixLen + halfW) - 0.5: da / pixLen + 3 eps (|a| / pixLen + halfW + 1)
    The magnitudes |P|, 1 / s and 1 / pixLen enter as they are in the case."""
    rec = cases[name]
    c = rec["case"]
    (p1, n1), rows = rec["new"], rec["rows"]
    ids = np.ascontiguousarray(n1[..., 3]).view(np.int32)
    cam_old = c["scene"].camera.copy()
    cam_old["position"][0] = c["eye0"]
    cam16 = rec["cam0"].astype(np.float64)
    worst = (0.0, 0.0)
    for g in c["moved"]:
        mask = ids == g
        assert mask.sum() >= 100
        P = p1[..., :3][mask]
        pf, _ = tm.follow(p1, n1, rows)
        s32, u32, v32 = tr.project(pf[..., :3][mask], rec["cam0"])
        s64, u64, v64 = _f64_projection(P, c["scene"].geoms[g], c["new_geoms"][g], cam_old)
        assert (s32 > 0).all() and (s64 > 0).all()
        m = np.abs(rows[g, :12].astype(np.float64).reshape(3, 4))
        M = np.abs(P.astype(np.float64)) @ m[:, :3].T + m[:, 3]
        d = np.abs(pf[..., :3][mask].astype(np.float64) - cam16[0:3])
        dd = 7 * EPS * M + EPS * d
        r0, r1, r2 = np.abs(cam16[7:10]), np.abs(cam16[10:13]), np.abs(cam16[13:16])
        ddot = lambda r: dd @ r + 6 * EPS * (d @ r)
        for r, pix_len, half, got, want in ((r1, cam16[3], cam16[5], u32, u64), (r2, cam16[4], cam16[6], v32, v64)):
            a = np.abs((want + 0.5 - half) * pix_len)
            da = (ddot(r) + a * ddot(r0)) / s64 + EPS * a
            bound = 2 * (da / pix_len + 3 * EPS * (a / pix_len + half + 1))
            err = np.abs(got.astype(np.float64) - want)
            worst = max(worst, (float(err.max()), float(bound[np.argmax(err)])))
            assert (err <= bound).all()
    print("%s: largest error of (u, v) against the float64 composition %.3g px, its bound %.3g px" % ((name,) + worst))
    assert worst[1] < 1e-3          # (the bound itself is far below anything a bilinear weight notices)


# ---- (d) the ledger: what the GPU test's inputs exercise ---------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(37, 23), (70, 5)])
def test_ledger_the_synthetic_arrays_take_every_branch(w, h):
    a = tm.synthetic(w, h, 11 * w + h)
    L = tm.ledger(*a[2:])
    print({k: v for k, v in L.items() if k != "valid"}, "pixels with history:", int(L["valid"].sum()))
    assert L["state0"] > 0 and L["state1"] > 0 and L["state2"] > 0 and L["no_length"] > 0 and L["behind"] > 0 and L["outside"] > 0
    assert min(L["rejected_id"], L["rejected_normal"], L["rejected_plane"]) >= 20
    st = tm.states(a[9])
    assert set(st.tolist()) == {0, 1, 2}
    ids = np.ascontiguousarray(a[3][..., 3]).view(np.int32)
    moved = (ids >= 0) & (st[np.clip(ids, 0, len(st) - 1)] == tm.MOVED)
    assert (L["valid"] & moved).sum() >= 20 and (L["valid"] & ~moved).sum() >= 5           # history is found on both sides of step 1' (70 x 5 holds 70 unmoved pixels)
    # the four motions: a translation, a rotation, a non-uniform scale, a singular G
    lin = [np.asarray(A)[:, :3] for A in tm.MOTIONS[1:]]
    assert np.allclose(lin[0], np.eye(3)) and np.allclose(lin[1] @ lin[1].T, np.eye(3)) and not np.allclose(lin[1], np.eye(3))
    assert np.allclose(lin[2], np.diag(np.diag(lin[2]))) and len(set(np.diag(lin[2]))) == 3
    assert (a[9][13, 12:15] == 0).all() and st[13] == tm.MOVED and st[14] == tm.NO_HISTORY


@pytest.mark.parametrize("name", oms.NAMES)
def test_ledger_every_rendered_case_shows_a_moved_primitive_with_and_without_history(cases, name):
    """on the oracle's guides, under a history that is full everywhere: at least 100 pixels of a moved primitive find it, at least 20 do not"""
    rec = cases[name]
    hist = (np.ones((oms.H, oms.W, 4), F), np.full((oms.H, oms.W), 16, F)) + rec["old"] + (rec["cam0"],)
    L = tm.ledger(*rec["new"], *hist, rec["rows"])
    ids = np.ascontiguousarray(rec["new"][1][..., 3]).view(np.int32)
    st = tm.states(rec["rows"])
    per = {g: (int(((ids == g) & L["valid"]).sum()), int(((ids == g) & ~L["valid"]).sum())) for g in rec["case"]["moved"]}
    print(name, "pixels of the moved primitives (with history, without):", per)
    one = [g for g in rec["case"]["moved"] if st[g] == tm.MOVED]
    assert one and all(per[g][0] >= 100 and per[g][1] >= 20 for g in one)
    for g in rec["case"]["moved"]:
        if st[g] == tm.NO_HISTORY:
            assert per[g][0] == 0 and per[g][1] >= 100


# ---- (e) the study: the CPU oracle chooses PT_OBJECT_HISTORY_MAX -----------------------------------------------------------------------
def _lum64(c):
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def _study_scenes(oracle):
    """(name, camera, materials, old geoms, new geoms, old eye, new eye, the moved primitive)"""
    cam, geoms, mats, e0, e1 = _cornell(oracle)
    g = geoms[6]
    to = (float(g["translation"][0]) + 0.5, float(g["translation"][1]), float(g["translation"][2]))
    new = tm.moved_geoms(oracle, geoms, {6: (to, None, None)})
    yield "cornell", cam, mats, geoms, new, e0, e0, 6
    yield "cornell+camera", cam, mats, geoms, new, e0, e1, 6
    cam, geoms, mats, e0, _ = _sphere_before_a_wall(oracle)
    g = geoms[3]
    to = (float(g["translation"][0]) + 0.5 * float(g["scale"][0]), float(g["translation"][1]), float(g["translation"][2]))
    yield "sphere", cam, mats, geoms, tm.moved_geoms(oracle, geoms, {3: (to, None, None)}), e0, e0, 3


COLUMNS = ("dropped", "kept") + tm.CANDIDATE_CAPS
REGIONS = ("frame", "object", "band")


@pytest.fixture(scope="module")
def study(oracle):
    """Per scene: 16 iterations of the OLD scene from the old eye, captured; iterations 17 .. of the NEW scene from the new eye after 2 and 4
    of them, and their mean over 2048 as the reference; the mean of 2048 iterations of the OLD scene from the new eye, for the band: the pixels
    whose converged luminance differs between the two scenes by more than 10 % of the larger.  Per column and count the RMSE of the filtered
    frame (the shipped filter setting) over the frame, the moved object's pixels and the band."""
    out = {}
    for name, cam, mats, old, new, e0, e1, prim in _study_scenes(oracle):
        at0, _, g0, cam0 = _view(oracle, cam, old, mats, e0, 1, (OLD,))
        at1, conv, g1, _ = _view(oracle, cam, new, mats, e1, OLD + 1, NEW, nref=2048)
        before = _view(oracle, cam, old, mats, e1, 3001, (1,), nref=2048, guides=False)[1]
        hist = tr.capture_form(*at0[OLD], OLD, *g0, *tr.empty_history(H, W)) + (g0[0], g0[1], cam0)
        rows, kept = tm.motion_table(old, new)
        assert kept
        ids1 = np.ascontiguousarray(g1[1][..., 3]).view(np.int32)
        la, lb = _lum64(conv), _lum64(before)
        masks = dict(frame=np.ones((H, W), bool), object=ids1 == prim, band=np.abs(la - lb) > 0.1 * np.maximum(la, lb))
        out[(name, "pixels")] = {k: int(m.sum()) for k, m in masks.items()}
        for n in NEW:
            S, Q = at1[n]
            img = dict(dropped=dv.denoise_var(S, Q, n, g1[0][..., :3], g1[1][..., :3], ids1, LEVELS, SIGMA_LUM, SIGMA_NORMAL, SIGMA_POSITION)[0],
                       kept=tr.denoise_var_temporal(S, Q, n, *g1, hist, LEVELS, SIGMA_LUM, SIGMA_NORMAL, SIGMA_POSITION)[0])
            for cap in tm.CANDIDATE_CAPS:
                img[cap] = tm.denoise_var(S, Q, n, *g1, hist, rows, LEVELS, SIGMA_LUM, SIGMA_NORMAL, SIGMA_POSITION, cap=cap)[0]
            for col, im in img.items():
                out[(name, n, col)] = {k: _rmse(im, conv, m) for k, m in masks.items()}
    return out


def _cells(study):
    return [(s, n) for s in ("cornell", "cornell+camera", "sphere") for n in NEW]


def _admitted(study, cap):
    return all(study[(s, n, cap)]["frame"] < study[(s, n, "dropped")]["frame"] for s, n in _cells(study))


def _score(study, cap, region):
    return float(np.mean([study[(s, n, cap)][region] / study[(s, n, "dropped")][region] for s, n in _cells(study)]))


def choose_cap(study):
    """The rule: a candidate is admitted only if its frame RMSE beats "history dropped" on every scene at both counts; among the admitted the
    lowest mean of band RMSE / dropped-history band RMSE ships.  No candidate admitted: the one that loses least, the lowest mean of frame
    RMSE / dropped-history frame RMSE.  Equal scores (16 and 32 are one column here: a history of 16 samples reaches neither cap): the smaller
    cap, which washes stale light out faster in the longer chains this study does not run."""
    admitted = [c for c in tm.CANDIDATE_CAPS if _admitted(study, c)]
    if admitted:
        return min(admitted, key=lambda c: (_score(study, c, "band"), c)), admitted
    return min(tm.CANDIDATE_CAPS, key=lambda c: (_score(study, c, "frame"), c)), admitted


def test_study_the_table_and_the_rule_for_the_cap(study):
    """RMSE against 2048 samples of the new scene, 72 x 40, depth 8, filter at (5 levels, sigma_lum 4, 0.35, 2.0); 16 old samples, 2 and 4 new.
    The figures are in the README ("Object history")."""
    for s in ("cornell", "cornell+camera", "sphere"):
        print("%s: pixels %s" % (s, study[(s, "pixels")]))
        assert study[(s, "pixels")]["object"] >= 10 and study[(s, "pixels")]["band"] >= 10
        for n in NEW:
            for col in COLUMNS:
                r = study[(s, n, col)]
                print("  n = %d  %-8s frame %.5f  object %.5f  band %.5f" % ((n, "cap %g" % col if not isinstance(col, str) else col) + tuple(r[k] for k in REGIONS)))
    shipped, admitted = choose_cap(study)
    for c in tm.CANDIDATE_CAPS:
        print("cap %-3g %s  mean frame ratio %.4f  mean object ratio %.4f  mean band ratio %.4f" %
              (c, "admitted" if c in admitted else "refused ", _score(study, c, "frame"), _score(study, c, "object"), _score(study, c, "band")))
    print("kept without the flag: mean frame ratio %.4f  mean object ratio %.4f  mean band ratio %.4f" % tuple(_score(study, "kept", k) for k in REGIONS))
    print("the rule ships cap %g (admitted: %s)" % (shipped, admitted))
    assert float(tm.object_cap()) == shipped


def test_study_following_the_object_beats_the_broken_promise_on_the_object(study):
    """on the moved object's own pixels the flag (at the shipped cap) is better than history kept without it, on every scene at both counts:
    without the flag those pixels either lose their history to the tests or blend the wrong place"""
    cap = float(tm.object_cap())
    for s, n in _cells(study):
        assert study[(s, n, cap)]["object"] < study[(s, n, "kept")]["object"], (s, n)
