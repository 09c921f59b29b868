"""Demodulated history (PT_FLAG_DEMOD_HISTORY) on the host (no GPU): the flag and its constant in the header and in Python, the frozen ABI, the
planner's refusals and acceptances, pt_render's refusals; the exact properties of the numpy float32 restatement
(tests/temporal_demod_ref.py); the study that shows why history has to carry albedo and that chooses PT_DEMOD_HISTORY_MIN_OWN; and Cornell
on the CPU oracle."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import demod_ref as dm
import denoise_ref as dr
import denoise_var_ref as dv
import spatial_var_ref as sv
import temporal_demod_ref as td
import temporal_ref as tr
from conftest import ROOT, SCENES

F = np.float32
# the shipped setting of the filter (PT_DISPLAY_*)
LEVELS, SIGMA_LUM, SIGMA_NORMAL, SIGMA_POSITION = 5, 4.0, 0.35, 2.0
SETTING = (LEVELS, SIGMA_LUM, SIGMA_NORMAL, SIGMA_POSITION)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _rmse(a, ref, mask):
    return float(np.sqrt(np.mean(((np.asarray(a, np.float64) - ref) ** 2)[mask])))


# ---- the flag and the refusals -----------------------------------------------------------------------------------------------------------
def test_flag_constant_and_the_frozen_abi(pt):
    hdr = open(os.path.join(ROOT, "include", "pt_amd.h")).read()
    thdr = open(os.path.join(ROOT, "include", "pt_amd_test.h")).read()
    assert re.search(r"PT_FLAG_DEMOD_HISTORY = 1024\b", hdr) and pt.PT_FLAG_DEMOD_HISTORY == 1024
    others = [v for k, v in vars(pt).items() if k.startswith("PT_FLAG_") and k != "PT_FLAG_DEMOD_HISTORY"]
    assert others and not any(v & 1024 for v in others)
    assert td.min_own() == pt.PT_DEMOD_HISTORY_MIN_OWN
    # no new product function, no struct change
    assert len(pt.ABI_SYMBOLS) == 47 and pt.lib().pt_abi_version() == 7 and pt.PT_AMD_ABI_VERSION == 7
    assert C.sizeof(pt.PtDenoiseVarParams) == 20 and C.sizeof(pt.PtOptions) == 48
    for name in ("pt_test_temporal_albedo", "pt_test_history_albedo"):
        assert re.search(r"\bint %s\(" % name, thdr) and name in pt.TEST_ABI_SYMBOLS
        assert hasattr(pt.test_lib(), name) and not hasattr(pt.lib(), name)
    sig = inspect.signature(pt.pathtraceInit).parameters
    assert "demod_history" in sig and sig["demod_history"].default is False
    pt.test_lib().pt_free()
    assert pt.test_history_albedo() is None                 # before pt_init the context holds no history


def test_the_planner_refuses_and_plans(pt):
    sc = pt.Scene(os.path.join(SCENES, "cornell.txt"))
    sc.set_resolution(32, 24)
    D, M, T, A = pt.PT_FLAG_DEMODULATE, pt.PT_FLAG_MOMENTS, pt.PT_FLAG_TEMPORAL, pt.PT_FLAG_DEMOD_HISTORY
    # the flag without all three of the others
    for bad in (dict(flags=A), dict(flags=A | M), dict(flags=A | M | T), dict(flags=A | M | D), dict(flags=A | T | D)):
        with pytest.raises(pt.PtError, match="pt_amd error -1"):
            pt.scene_plan(sc, **bad)
    for bad in (dict(flags=A | M), dict(flags=A | M | T), dict(flags=A | M | D)):
        with pytest.raises(pt.PtError, match="pt_amd error -1.*PT_FLAG_DEMOD_HISTORY"):
            pt.scene_plan(sc, **bad)
    # without it the two still refuse each other, in today's words
    with pytest.raises(pt.PtError, match=r"pt_amd error -1.*PT_FLAG_DEMODULATE is not for PT_FLAG_TEMPORAL renderers \(history carries no albedo\)"):
        pt.scene_plan(sc, flags=D | M | T)
    # every other refusal of either flag stands under it
    all4 = A | M | T | D
    for bad in (dict(flags=all4 | pt.PT_FLAG_TRACE_AHEAD, max_batch=4), dict(flags=all4 | pt.PT_FLAG_TRACE_AHEAD, max_batch=1),
                dict(flags=all4, lens_radius=0.1, focal_distance=5.0), dict(flags=all4, shard_count=2), dict(flags=all4 | pt.PT_FLAG_ACCUM_SHARD_ROWS)):
        with pytest.raises(pt.PtError, match="pt_amd error -1"):
            pt.scene_plan(sc, **bad)
    # with it they are planned together -- direct lighting, the display filter and the spatial estimate too -- and the plan does not record it
    for extra in (0, pt.PT_FLAG_DIRECT_LIGHTING, pt.PT_FLAG_DISPLAY_FILTER, pt.PT_FLAG_SPATIAL_VARIANCE, pt.PT_FLAG_DISPLAY_FILTER | pt.PT_FLAG_SPATIAL_VARIANCE):
        assert bytes(pt.scene_plan(sc, flags=all4 | extra)) == bytes(pt.scene_plan(sc, flags=M | extra))
    for name in ("mesh_small.txt", "cornell_textured.txt", "cornell_bump.txt"):
        s2 = pt.Scene(os.path.join(SCENES, name))
        s2.set_resolution(32, 24)
        assert bytes(pt.scene_plan(s2, flags=all4)) == bytes(pt.scene_plan(s2, flags=M))


def test_pt_render_refuses_before_a_device(built, tmp_path):
    exe = os.path.join(ROOT, "project3-cuda-path-tracer_amd", "host", "pt_render")
    base = [exe, os.path.join(SCENES, "cornell.txt"), "--res", "16", "16", "--iterations", "2", "--out", str(tmp_path / "no")]
    dvar, hist = ["--denoise-var", "5", "4", "0.35", "2"], ["--history-from", "0", "5", "9", "2"]
    for args in (["--history-albedo"], ["--history-albedo"] + dvar, ["--history-albedo"] + hist):
        r = subprocess.run(base + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "--history-albedo needs --denoise-var and --history-from" in r.stderr, args
    # --demodulate with --history-from stays refused with today's words
    r = subprocess.run(base + ["--demodulate"] + dvar + hist, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--demodulate needs --denoise-var and does not go with --history-from" in r.stderr
    assert os.listdir(tmp_path) == []


# ---- exact properties of the restatement ---------------------------------------------------------------------------------------------
def _wall_view(eye, w, h, pixlen):
    """The guides of a camera at `eye` looking down -z (up +y, right +x) at the wall z = 0 -- pixel centres -- and its 16 constants"""
    yy, xx = np.mgrid[0:h, 0:w]
    a = pixlen * (xx + 0.5 - w / 2)
    b = pixlen * (yy + 0.5 - h / 2)
    pos_t = np.zeros((h, w, 4), F)
    pos_t[..., 0] = eye[0] - a * eye[2]
    pos_t[..., 1] = eye[1] - b * eye[2]
    pos_t[..., 3] = eye[2] * np.sqrt(a * a + b * b + 1)
    nrm = np.zeros((h, w, 3), F)
    nrm[..., 2] = 1
    _, nrm_id = tr.pack_guides(pos_t, nrm, np.zeros((h, w), np.int32), h, w)
    return pos_t, nrm_id, tr.temporal_camera((0, 0, -1), (0, 1, 0), (1, 0, 0), eye, pixlen, pixlen, F(w) * F(0.5), F(h) * F(0.5))


def _random_sums(rng, h, w, n):
    S = rng.uniform(0, 3 * n, (h, w, 3)).astype(F)
    S[rng.uniform(0, 1, (h, w)) < 0.15] = 0
    Q = (dv.lum(S / F(n)) ** 2 * F(n) * rng.uniform(1.0, 3.0, (h, w))).astype(F)
    asum = dm.accumulate([rng.uniform(0, 1, (h, w, 3)).astype(F) for _ in range(n)])
    return S, Q, asum


@pytest.mark.parametrize("n", [1, 2, 5])
def test_without_history_the_blended_albedo_is_the_mean_albedo_to_the_bit(n):
    """Ab = (0 * 0 + Asum) / (0 + n) = Asum / n: the bits demodAlbedo forms before its floor, so without history the whole filter is
    PT_FLAG_DEMODULATE's."""
    rng = np.random.default_rng(4)
    h, w = 23, 37
    S, Q, asum = _random_sums(rng, h, w, n)
    asum[0, 0, :3] = (0, np.nan, 1e-4)
    pos_t, nrm_id, _ = _wall_view((0.25, 0.0, 4.0), w, h, 0.125)
    behind = (np.full((h, w, 4), 7, F), np.full((h, w), 9, F), pos_t, nrm_id, _wall_view((0.0, 0.0, -4.0), w, h, 0.125)[2], np.full((h, w, 4), 0.3, F))
    geom = np.zeros((h, w), np.int32)
    for hist in (td.empty_history(h, w), behind):
        ab = td.albedo_form(asum, n, pos_t, nrm_id, hist)
        with np.errstate(all="ignore"):
            assert _same(ab[..., :3], asum[..., :3] / F(n)) and (ab[..., 3] == n).all()
        assert _same(dm.floored_albedo(ab, 1), dm.floored_albedo(asum, n))
        hc, hn, ha = td.capture_form(S, Q, asum, n, pos_t, nrm_id, hist)
        assert _same(ha, ab) and (hn == n).all()
        if n >= 2:
            want = dm.denoise_var_demod(S, Q, asum, n, pos_t[..., :3], nrm_id[..., :3], geom, *SETTING)
        else:
            c, v, _ = sv.spatial_variance(*sv.moments_form(S, Q, n), pos_t[..., :3], nrm_id[..., :3], geom, sv.constants()[1], SIGMA_NORMAL, SIGMA_POSITION)
            want = dm.atrous_demod(c, v, asum, n, pos_t[..., :3], nrm_id[..., :3], geom, *SETTING)
        for own_from in (1, 2, 4, td.NEVER):            # whichever is multiplied back: the same bits
            got = td.denoise_var_demod_history(S, Q, asum, n, pos_t, nrm_id, hist, *SETTING, own_from=own_from)
            assert _same(got[0], want[0]) and _same(got[1], want[1])


@pytest.mark.parametrize("n", [1, 2, 5])
def test_an_albedo_of_one_everywhere_is_the_temporal_filter_to_the_bit(n):
    """Ha = (1, 1, 1) and Asum = n (1, 1, 1): sumA = sumW to the bit (1 * w is w, added in the same order), ha = sumW / sumW = 1,
    Ab = (Nh + n) / (Nh + n) = 1 (1 * Nh is Nh; the sum is tot's own), c / 1 and c * 1 are exact and rho = L / L = 1."""
    rng = np.random.default_rng(6)
    w, h = 41, 19
    old = _wall_view((0.0, 0.0, 4.0), w, h, 0.125)
    new = _wall_view((-0.171875, 0.09375, 4.5), w, h, 0.125)
    S0, Q0, _ = _random_sums(rng, h, w, 8)
    ones = lambda k: dm.accumulate([np.ones((h, w, 3), F)] * k)
    hist = td.capture(S0, Q0, ones(8), 8, old[0], old[1], old[2], td.empty_history(h, w))
    assert (hist[5][..., :3] == 1).all() and (hist[5][..., 3] == 8).all()
    S, Q, _ = _random_sums(rng, h, w, n)
    _, Nh = tr.reproject(new[0], new[1], *hist[:5])
    assert 0.5 < (Nh > 0).mean() < 1.0
    ab = td.albedo_form(ones(n), n, new[0], new[1], hist)
    assert (ab[..., :3] == 1).all() and _same(ab[..., 3], Nh + F(n))
    if n >= 2:
        want = tr.denoise_var_temporal(S, Q, n, new[0], new[1], hist[:5], *SETTING)
    else:
        want = sv.denoise_var_spatial(S, Q, n, new[0], new[1], *SETTING, history=hist[:5])
    for own_from in (1, td.NEVER):
        got = td.denoise_var_demod_history(S, Q, ones(n), n, new[0], new[1], hist, *SETTING, own_from=own_from)
        assert _same(got[0], want[0]) and _same(got[1], want[1])
    # ... and the captured albedo is recursive: Ha' = Ab, with the uncapped count behind it
    hist2 = td.capture(S, Q, ones(n), n, new[0], new[1], new[2], hist)
    assert _same(hist2[5], ab) and hist2[1].max() <= tr.constants()[0]


# ---- the study ----------------------------------------------------------------------------------------------------------------------------
W, H = 64, 48
OLD, COUNTS = 16, (1, 2, 4, 16)
CANDIDATES = (1, 2, 4, 8, td.NEVER)       # PT_DEMOD_HISTORY_MIN_OWN: 1 = always the new samples' albedo, NEVER = always the blend
PIXLEN, EYE_Z = 0.0125, 4.0               # 0.05 world units per pixel: the spacing of tests/test_demod_cpu.py's planar guides
BOARDS = {"6.5 px 0.25 / 0.75": (6.5, 0.25, 0.75, (3.37, 1.61)), "6.5 px 0.02 / 0.9": (6.5, 0.02, 0.9, (3.37, 1.61)),
          "8 px aligned 0.25 / 0.75": (8.0, 0.25, 0.75, (2.5, 0.5))}
MAIN, DARK = "6.5 px 0.25 / 0.75", "6.5 px 0.02 / 0.9"


def _even_measure(t, cell):
    """the measure of {s in [0, t]: floor(s / cell) is even}"""
    t = np.asarray(t, np.float64)
    return np.floor(t / (2 * cell)) * cell + np.minimum(t % (2 * cell), cell)


def _samples(rng, cell, lo, hi, shift, count):
    """`count` samples per pixel of a view whose pixel (x, y) covers the board's [x + shift.x, +1) x [y + shift.y, +1), as
    tests/test_demod_cpu.py::_board draws them (grey): the albedo at the sample's own jittered position, times uniform(0, 2); per sample the
    jitters drawn before the factor"""
    yy, xx = np.mgrid[0:H, 0:W]
    albedos, samples = [], []
    for _ in range(count):
        j = rng.uniform(0, 1, (H, W, 2))
        parity = (np.floor((xx + shift[0] + j[..., 0]) / cell) + np.floor((yy + shift[1] + j[..., 1]) / cell)) % 2
        a = np.repeat(np.where(parity == 0, lo, hi)[..., None], 3, axis=2).astype(F)
        albedos.append(a)
        samples.append(a * rng.uniform(0, 2, (H, W, 1)).astype(F))
    return albedos, samples


def _sums(albedos, samples, n):
    S = np.zeros((H, W, 3), F)
    for s in samples[:n]:
        S = S + s
    return S, dv.moments(samples[:n]), dm.accumulate(albedos[:n])


def _board(cell, lo, hi, shift):
    """One board: a checkerboard albedo of `cell`-pixel cells on the wall z = 0.  The old view, `shift` pixels aside, takes OLD samples and is
    captured; the new view takes n of COUNTS.  Truth: the new view's box-filtered albedo.  RMSE over the pixels WITH history of: "temporal"
    (today's PT_FLAG_TEMPORAL filter), "demod" (PT_FLAG_DEMODULATE without history), "naive" (blended colour over the new samples' albedo),
    "blend" / "own" (the flagged pipeline multiplying Ab / the new samples' mean albedo back).  Returns {n: {...}}."""
    yy, xx = np.mgrid[0:H, 0:W]
    fx = _even_measure(xx + 1.0, cell) - _even_measure(xx, cell)
    fy = _even_measure(yy + 1.0, cell) - _even_measure(yy, cell)
    even = fx * fy + (1 - fx) * (1 - fy)
    truth = np.repeat((lo * even + hi * (1 - even))[..., None], 3, axis=2)
    px = PIXLEN * EYE_Z
    new = _wall_view((0.0, 0.0, EYE_Z), W, H, PIXLEN)
    old = _wall_view((-shift[0] * px, -shift[1] * px, EYE_Z), W, H, PIXLEN)       # (pos.x falls with x: a pixel of the old view lies `shift` further on)
    a0, s0 = _samples(np.random.default_rng(11), cell, lo, hi, shift, OLD)
    hist = td.capture(*_sums(a0, s0, OLD), OLD, *old, td.empty_history(H, W))
    albedos, samples = _samples(np.random.default_rng(7), cell, lo, hi, (0.0, 0.0), max(COUNTS))
    pos, nrm, geom = new[0][..., :3], new[1][..., :3], np.zeros((H, W), np.int32)
    _, Nh = tr.reproject(new[0], new[1], *hist[:5])
    mask = Nh > 0
    assert 0.8 < mask.mean() < 1.0
    # the reprojection lands where the board says: the old view's albedo, reprojected, is the truth up to its own noise and the bilinear blur
    assert _rmse(td.reproject_albedo(new[0], new[1], hist)[0], truth, mask) < 0.6 * (hi - lo) / 2
    rows = {}
    for n in COUNTS:
        S, Q, asum = _sums(albedos, samples, n)
        row = {}
        if n >= 2:
            row["temporal"] = tr.denoise_var_temporal(S, Q, n, new[0], new[1], hist[:5], *SETTING)[0]
            row["demod"] = dm.denoise_var_demod(S, Q, asum, n, pos, nrm, geom, *SETTING)[0]
        else:
            row["temporal"] = sv.denoise_var_spatial(S, Q, n, new[0], new[1], *SETTING, history=hist[:5])[0]
            c, v, _ = sv.spatial_variance(*sv.moments_form(S, Q, n), pos, nrm, geom, sv.constants()[1], SIGMA_NORMAL, SIGMA_POSITION)
            row["demod"] = dm.atrous_demod(c, v, asum, n, pos, nrm, geom, *SETTING)[0]
        row["naive"] = td.denoise_var_naive(S, Q, asum, n, new[0], new[1], hist, *SETTING)[0]
        co, vo, ab = td.filtered(S, Q, asum, n, new[0], new[1], hist, *SETTING)
        row["blend"] = td.remodulate(co, vo, ab, asum, n, td.NEVER)[0]
        row["own"] = td.remodulate(co, vo, ab, asum, n, 1)[0]
        rows[n] = {k: _rmse(v, truth, mask) for k, v in row.items()}
    return rows


def _of(rows, n, own_from):
    """the flagged pipeline's RMSE at n samples under PT_DEMOD_HISTORY_MIN_OWN = own_from"""
    return rows[n]["blend" if n < own_from else "own"]


@pytest.fixture(scope="module")
def study():
    out = {name: _board(*spec) for name, spec in BOARDS.items()}
    for name, rows in out.items():
        for n, r in rows.items():
            print("%-26s n = %2d: temporal only %.4f  demodulated, no history %.4f  naive %.4f  flagged: blended albedo back %.4f, own albedo back %.4f" % (
                name, n, r["temporal"], r["demod"], r["naive"], r["blend"], r["own"]))
    return out


def _score(study, own_from):
    return float(np.mean([_of(study[b], n, own_from) / study[b][n]["temporal"] for b in BOARDS for n in COUNTS]))


def _admitted(study, own_from):
    return all(_of(study[MAIN], n, own_from) < study[MAIN][n]["temporal"] for n in COUNTS)


def test_study_the_rule_chooses_the_albedo_multiplied_back(study, pt):
    """PT_DEMOD_HISTORY_MIN_OWN, the smallest sample count from which the renderer's own mean albedo is multiplied back.  The rule: a candidate
    of 1, 2, 4, 8, never is admitted only if on the 6.5-px 0.25 / 0.75 board the pipeline beats today's temporal-only filter at every count of
    1, 2, 4, 16; among the admitted the lowest mean, over the three boards and four counts, of RMSE / temporal-only RMSE is shipped.
    Measured (64 x 48, the shipped setting, 16 old samples, pixels with history; RMSE against the box-filtered albedo at n = 1 / 2 / 4 / 16):
                                     temporal only                       blended albedo back                 own albedo back
        6.5 px 0.25 / 0.75           0.0787 / 0.0742 / 0.0667 / 0.0398   0.0587 / 0.0558 / 0.0508 / 0.0336   0.1007 / 0.0713 / 0.0485 / 0.0250
        6.5 px 0.02 / 0.9            0.1154 / 0.1070 / 0.0931 / 0.0490   0.1031 / 0.0981 / 0.0892 / 0.0590   0.1774 / 0.1254 / 0.0849 / 0.0436
        8 px aligned 0.25 / 0.75     0.0935 / 0.0876 / 0.0773 / 0.0388   0.0838 / 0.0792 / 0.0712 / 0.0446   0.0035 / 0.0043 / 0.0041 / 0.0034
    Mean ratio: 1: 0.6943 (not admitted: it loses at one sample), 2: 0.6678, 4: 0.7004, 8: 0.7795, never: 0.9121 -- 2 ships.  The known cost
    of 2: the dark board at 2 samples (0.1254 against the temporal-only 0.1070) and the aligned board at one sample (0.0838 against 0.0282
    for demodulation without history).
    (the module prints the table it measures; README, "Demodulated history", quotes it)."""
    scores = {c: _score(study, c) for c in CANDIDATES}
    admitted = [c for c in CANDIDATES if _admitted(study, c)]
    print("mean RMSE / temporal-only RMSE: " + "  ".join("%s: %.4f%s" % (c, scores[c], "" if c in admitted else " (not admitted)") for c in CANDIDATES))
    assert admitted
    best = min(admitted, key=lambda c: scores[c])
    print("the rule ships PT_DEMOD_HISTORY_MIN_OWN = %s; the header has %d" % (best, pt.PT_DEMOD_HISTORY_MIN_OWN))
    assert best != td.NEVER or pt.PT_DEMOD_HISTORY_MIN_OWN > 1 << 20
    assert best == td.NEVER or pt.PT_DEMOD_HISTORY_MIN_OWN == best
    assert td.min_own() == pt.PT_DEMOD_HISTORY_MIN_OWN


def test_study_history_has_to_carry_albedo(study, pt):
    """The naive combination -- the blended colour over the new samples' albedo alone, what lifting the refusal would compute -- divides old
    light that a dark texel reflected by a bright new albedo and the other way round: on the dark board it is worse than the shipped pipeline
    at 1, 2 and 4 samples."""
    for n in (1, 2, 4):
        assert study[DARK][n]["naive"] > _of(study[DARK], n, pt.PT_DEMOD_HISTORY_MIN_OWN)


# ---- Cornell on the CPU oracle ---------------------------------------------------------------------------------------------------------------
def test_cornell_is_neutral(oracle):
    """A flat-coloured scene has nothing to gain: 72 x 40, depth 8, the sidestep of tests/test_temporal_cpu.py (0.3 to the right), 16 old samples,
    2 and 4 new against 2048 of the new view.  Flagged RMSE at most 1.03 x the temporal-only filter's: the margin
    tests/test_demod_cpu.py::test_cornell_is_neutral allows PT_FLAG_DEMODULATE -- the same mechanism, an albedo constant per primitive."""
    w, h = 72, 40
    sc = oracle.Scene(os.path.join(SCENES, "cornell.txt"))
    sc.set_resolution(w, h)
    mats = sc.materials

    def view(eye, first, counts, nref):
        cam = sc.camera.copy()
        cam["position"][0] = eye
        ref = oracle.Renderer(cam, sc.geoms, mats, 8)
        acc, singles, albedos, at, guides = np.zeros(w * h * 3, F), [], [], {}, None
        for k in range(1, max(max(counts), nref) + 1):
            if k <= max(counts):
                one = np.zeros(w * h * 3, F)
                ref.iterate(first + k - 1, one)
                singles.append(one.reshape(h, w, 3))
                pos_t, nrm, geom = dr.oracle_guides(oracle, ref, first + k - 1)
                m = mats[sc.geoms["materialid"][np.maximum(geom, 0)]]
                albedos.append(dm.albedo_of_hit(geom >= 0, m["emittance"], m["hasReflective"], m["hasRefractive"], m["color"]).reshape(h, w, 3))
            ref.iterate(first + k - 1, acc)
            if k in counts:
                at[k] = (acc.reshape(h, w, 3).copy(), dv.moments(singles), dm.accumulate(albedos))
        conv = (acc / F(nref)).reshape(h, w, 3).astype(np.float64) if nref else None
        return at, conv, tr.pack_guides(*dr.oracle_guides(oracle, ref, 1), h, w), tr.camera16(cam)

    at0, _, g0, cam0 = view((0.0, 5.0, 10.5), 1, (OLD,), 0)
    at1, truth, g1, _ = view((0.3, 5.0, 10.5), OLD + 1, (2, 4), 2048)
    hist = td.capture(*at0[OLD], OLD, *g0, cam0, td.empty_history(h, w))
    everywhere = np.ones((h, w), bool)
    for n in (2, 4):
        S, Q, asum = at1[n]
        temporal = _rmse(tr.denoise_var_temporal(S, Q, n, *g1, hist[:5], *SETTING)[0], truth, everywhere)
        flagged = _rmse(td.denoise_var_demod_history(S, Q, asum, n, *g1, hist, *SETTING)[0], truth, everywhere)
        print("Cornell n = %d: temporal only %.5f  flagged %.5f  (x %.3f)" % (n, temporal, flagged, flagged / temporal))
        assert flagged <= 1.03 * temporal
