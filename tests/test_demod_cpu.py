"""Albedo demodulation (PT_FLAG_DEMODULATE) on the host (no GPU): the flag and its constant in the header and in Python, the frozen ABI, the
refusals of the planner; the exact properties of the numpy float32 restatement (tests/demod_ref.py); the study that shows why the demodulator
is the MEAN albedo of the pixel's own samples and not one sample's, and that chooses PT_DEMOD_MIN_ALBEDO; and Cornell on the CPU oracle."""
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
from conftest import ROOT, SCENES

F = np.float32
# the shipped setting of the filter (PT_DISPLAY_*)
LEVELS, SIGMA_LUM, SIGMA_NORMAL, SIGMA_POSITION = 5, 4.0, 0.35, 2.0
SETTING = (LEVELS, SIGMA_LUM, SIGMA_NORMAL, SIGMA_POSITION)
COUNTS = (2, 4, 16, 64)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _rmse(a, ref):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - ref) ** 2)))


# ---- the flag and the refusals -----------------------------------------------------------------------------------------------------------
def test_flag_constant_and_the_frozen_abi(pt):
    hdr = open(os.path.join(ROOT, "include", "pt_amd.h")).read()
    thdr = open(os.path.join(ROOT, "include", "pt_amd_test.h")).read()
    assert re.search(r"PT_FLAG_DEMODULATE = 512\b", hdr) and pt.PT_FLAG_DEMODULATE == 512
    others = [v for k, v in vars(pt).items() if k.startswith("PT_FLAG_") and k != "PT_FLAG_DEMODULATE"]
    assert others and not any(v & 512 for v in others)
    m = re.search(r"^#define PT_DEMOD_MIN_ALBEDO ([0-9.]+)f$", hdr, re.M)
    assert m and F(m.group(1)) == F(pt.PT_DEMOD_MIN_ALBEDO) == dm.MIN_ALBEDO and dm.MIN_ALBEDO in dm.CANDIDATES
    # no new product function, no struct change
    assert len(pt.ABI_SYMBOLS) == 47 and pt.lib().pt_abi_version() == 7 and pt.PT_AMD_ABI_VERSION == 7
    assert C.sizeof(pt.PtDenoiseVarParams) == 20 and C.sizeof(pt.PtOptions) == 48
    for name in ("pt_test_albedo", "pt_test_demodulate"):
        assert re.search(r"\bint %s\(" % name, thdr) and name in pt.TEST_ABI_SYMBOLS
        assert hasattr(pt.test_lib(), name) and not hasattr(pt.lib(), name)
    sig = inspect.signature(pt.pathtraceInit).parameters
    assert "demodulate" in sig and sig["demodulate"].default is False


def test_the_planner_refuses_and_plans(pt):
    sc = pt.Scene(os.path.join(SCENES, "cornell.txt"))
    sc.set_resolution(32, 24)
    D, M = pt.PT_FLAG_DEMODULATE, pt.PT_FLAG_MOMENTS
    for bad in (dict(flags=D),                                                   # without PT_FLAG_MOMENTS
                dict(flags=D | pt.PT_FLAG_DISPLAY_FILTER),
                dict(flags=D | M | pt.PT_FLAG_TEMPORAL),
                dict(flags=D | M | pt.PT_FLAG_TRACE_AHEAD, max_batch=4),
                dict(flags=D | M | pt.PT_FLAG_TRACE_AHEAD, max_batch=1)):         # judged on the caller's flags: max_batch 1 strips it from the plan's
        with pytest.raises(pt.PtError, match="pt_amd error -1.*PT_FLAG_(DEMODULATE|DISPLAY_FILTER)"):
            pt.scene_plan(sc, **bad)
    for bad in (dict(flags=D), dict(flags=D | M | pt.PT_FLAG_TEMPORAL), dict(flags=D | M | pt.PT_FLAG_TRACE_AHEAD, max_batch=4)):
        with pytest.raises(pt.PtError, match="pt_amd error -1.*PT_FLAG_DEMODULATE"):
            pt.scene_plan(sc, **bad)
    # row shards refuse PT_FLAG_MOMENTS, hence the flag
    for bad in (dict(flags=D | M, shard_count=2), dict(flags=D | M | pt.PT_FLAG_ACCUM_SHARD_ROWS)):
        with pytest.raises(pt.PtError, match="pt_amd error -1"):
            pt.scene_plan(sc, **bad)
    # a thin lens, direct lighting, the display filter and the spatial variance estimate go with it; the plan does not record the flag
    for ok in (dict(), dict(lens_radius=0.1, focal_distance=5.0), dict(flags=pt.PT_FLAG_DIRECT_LIGHTING), dict(flags=pt.PT_FLAG_DISPLAY_FILTER),
               dict(flags=pt.PT_FLAG_SPATIAL_VARIANCE), dict(flags=pt.PT_FLAG_DISPLAY_FILTER | pt.PT_FLAG_SPATIAL_VARIANCE, max_batch=8)):
        base = dict(ok)
        base["flags"] = base.get("flags", 0) | M
        flagged = dict(base)
        flagged["flags"] |= D
        assert bytes(pt.scene_plan(sc, **flagged)) == bytes(pt.scene_plan(sc, **base))
    # a mesh scene whose hierarchy fits k_gbuffer's stacks -- k_albedo's too -- is planned, textured and bump-mapped scenes as well.  (No mesh
    # reaches the refusal: a hierarchy that needs more than 24 levels is rebuilt by median splits, and the stacks hold 64.  It stands next to
    # PT_FLAG_DISPLAY_FILTER's in the planner, with the flag named.)
    for name in ("mesh_small.txt", "cornell_textured.txt", "cornell_bump.txt"):
        s2 = pt.Scene(os.path.join(SCENES, name))
        s2.set_resolution(32, 24)
        assert bytes(pt.scene_plan(s2, flags=D | M)) == bytes(pt.scene_plan(s2, flags=M))
    plan_src = open(os.path.join(ROOT, "project3-cuda-path-tracer_amd", "csrc", "pt_scene_plan.h")).read()
    assert re.search(r'PT_FLAG_DEMODULATE\) && guideStackBytes\(true, p\.meshStackNeed\) > 64 \* 1024\)\s*return fail\(PT_ERR_INVALID, "pt_init: PT_FLAG_DEMODULATE: guide buffers',
                     plan_src)


def test_pt_render_and_the_shim_refuse_before_a_device(built, tmp_path):
    exe = os.path.join(ROOT, "project3-cuda-path-tracer_amd", "host", "pt_render")
    base = [exe, os.path.join(SCENES, "cornell.txt"), "--res", "16", "16", "--iterations", "2", "--out", str(tmp_path / "no")]
    r = subprocess.run(base + ["--demodulate"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--demodulate needs --denoise-var" in r.stderr
    r = subprocess.run(base + ["--demodulate", "--denoise-var", "5", "4", "0.35", "2", "--history-from", "0", "5", "9", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--demodulate needs --denoise-var and does not go with --history-from" in r.stderr
    env = dict(os.environ, PT_AMD_DEMODULATE="1", PT_AMD_DEVICES="2")
    r = subprocess.run(base, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 1 and "PT_AMD_DEVICES" in r.stderr and "demodulation" in r.stderr and "pathtraceInit" in r.stderr
    assert os.listdir(tmp_path) == []


# ---- exact properties of the restatement ---------------------------------------------------------------------------------------------
def _random_frame(rng, h, w, n):
    S = rng.uniform(0, 3 * n, (h, w, 3)).astype(F)
    S[rng.uniform(0, 1, (h, w)) < 0.15] = 0
    Q = (dv.lum(S / F(n)) ** 2 * F(n) * rng.uniform(1.0, 3.0, (h, w))).astype(F)
    pos = rng.normal(0, 3, (h, w, 3)).astype(F)
    nrm = rng.normal(0, 1, (h, w, 3)).astype(F)
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True).astype(F)
    geom = rng.integers(-1, 4, (h, w)).astype(np.int32)
    pos[geom < 0] = 0
    nrm[geom < 0] = 0
    return S, Q, pos, nrm, geom


@pytest.mark.parametrize("n", [2, 5, 16])
def test_an_albedo_of_one_is_the_unflagged_filter_to_the_bit(n):
    """Asum = n (1, 1, 1): a frame of misses, lights and mirrors.  a = n / n = 1 exactly, c / 1 and c * 1 are exact, rho = L / L = 1."""
    rng = np.random.default_rng(3)
    h, w = 23, 37
    S, Q, pos, nrm, geom = _random_frame(rng, h, w, n)
    asum = dm.accumulate([dm.albedo_of_hit(np.zeros((h, w), bool), np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w, 3)))] * n)
    assert (asum == F(n)).all()
    c, v = dv.mean_and_variance(S, Q, n)
    cd, vd = dm.demodulate(c, v, asum, n)
    assert _same(cd, c) and _same(vd, v)
    want_c, want_v = dv.atrous_var(c, v, pos, nrm, geom, *SETTING)
    got_c, got_v = dm.denoise_var_demod(S, Q, asum, n, pos, nrm, geom, *SETTING)
    assert _same(got_c, want_c) and _same(got_v, want_v)


@pytest.mark.parametrize("k", [1, 2, 4])
def test_a_constant_grey_power_of_two_albedo_changes_nothing(k):
    """g = 2^-k >= eps: division by and multiplication with a power of two are exact (no value here leaves the normal range), so c' = c / g,
    lum(c') = lum(c) / g and rho = 1 / g to the bit, and every level's sums scale by the same power of two -- the output is the unflagged
    filter's to the bit.  One term does not scale: the 1e-8 in the colour term's scale 1 / (sl2 g_v + 1e-8).  The frame is bright enough (a
    variance of the order of 10^5) that it lies below half an ulp of sl2 g_v with and without g wherever g_v > 0; where g_v = 0 the scale is
    1e8 either way and a tap of another luminance has a weight of 0 in both.  With the colour term off (sigma_lum = +inf) any frame does."""
    rng = np.random.default_rng(5)
    h, w, n = 19, 41, 4
    S, Q, pos, nrm, geom = _random_frame(rng, h, w, n)
    g = F(2.0 ** -k)
    assert g >= dm.MIN_ALBEDO
    asum = dm.accumulate([np.full((h, w, 3), g, F)] * n)
    inv = F(1.0) / g
    for scale, sigma_lum in ((F(1.0), np.inf), (F(1024.0), SIGMA_LUM)):
        Ss, Qs = S * scale, Q * (scale * scale)
        c, v = dv.mean_and_variance(Ss, Qs, n)
        cd, vd = dm.demodulate(c, v, asum, n)
        assert _same(cd, c * inv) and _same(vd, np.where(dv.lum(c) > 0, v * (inv * inv), v))
        want_c, want_v = dv.atrous_var(c, v, pos, nrm, geom, LEVELS, sigma_lum, SIGMA_NORMAL, SIGMA_POSITION)
        got_c, got_v = dm.denoise_var_demod(Ss, Qs, asum, n, pos, nrm, geom, LEVELS, sigma_lum, SIGMA_NORMAL, SIGMA_POSITION)
        assert _same(got_c, want_c)
        lit = dv.lum(want_c) > 0
        assert lit.mean() > 0.9 and _same(got_v[lit], want_v[lit])


def test_a_nan_or_zero_sum_takes_the_floor_and_a_black_pixel_keeps_its_variance():
    asum = np.array([[0, 0, 0, 4], [np.nan, np.nan, np.nan, 4], [4, 2, 1e-3, 4], [-1, 0.5, np.inf, 4]], F)
    al = dm.floored_albedo(asum, 4)
    e = dm.MIN_ALBEDO
    assert _same(al, np.array([[e, e, e], [e, e, e], [1, 0.5, e], [e, 0.125, np.inf]], F))
    for eps in dm.CANDIDATES:
        assert _same(dm.floored_albedo(asum[:2], 4, eps), np.full((2, 3), eps, F))
    # L = 0 (and a negative or NaN luminance) leaves v untouched
    c = np.array([[0, 0, 0], [0.5, 0.25, 1], [-1, 0, 0], [np.nan, 1, 1]], F)
    v = np.array([0.25, 0.5, 0.75, 1.0], F)
    s4 = np.array([[2, 2, 2, 4]] * 4, F)
    cd, vd = dm.demodulate(c, v, s4, 4)
    assert _same(cd[:3], c[:3] / F(0.5)) and _same(vd, np.array([0.25, 0.5 * 4, 0.75, 1.0], F))
    out, var = dm.remodulate(c, v, s4, 4)
    assert _same(out[:3], c[:3] * F(0.5)) and _same(var, np.array([0.25, 0.5 * 0.25, 0.75, 1.0], F))


def test_the_rule_of_a_single_albedo_and_the_accumulation():
    col = np.array([[0.5, 0.25, 1.0]] * 6, F)
    tex = np.array([[0.3, 0.7, 0.11]] * 6, F)
    hit = np.array([0, 1, 1, 1, 1, 1], bool)
    emit = np.array([0, 0, 5, 0, 0, 0], F)
    refl = np.array([0, 0, 0, 1, 0, 0], F)
    refr = np.array([0, 0, 0, 0, 1, 0], F)
    a = dm.albedo_of_hit(hit, emit, refl, refr, col, tex)
    one = np.ones(3, F)
    assert _same(a, np.stack([one, col[1] * tex[1], one, one, one, col[5] * tex[5]]))
    assert _same(dm.albedo_of_hit(hit, emit, refl, refr, col)[1], col[1])
    # a batch equals its single calls: the sums are a chain of fp32 additions in iteration order
    rng = np.random.default_rng(9)
    As = [rng.uniform(0, 1, (7, 3)).astype(F) for _ in range(5)]
    whole = dm.accumulate(As)
    parts = dm.accumulate(As[3:], dm.accumulate(As[1:3], dm.accumulate(As[:1])))
    assert _same(whole, parts) and (whole[:, 3] == 5).all()
    chain = np.zeros((7, 3), F)
    for a in As:
        chain = chain + a
    assert _same(whole[:, :3], chain)


# ---- the study ----------------------------------------------------------------------------------------------------------------------------
W, H = 64, 48


def _even_measure(t, cell):
    """the measure of {s in [0, t]: floor(s / cell) is even}"""
    t = np.asarray(t, np.float64)
    return np.floor(t / (2 * cell)) * cell + np.minimum(t % (2 * cell), cell)


def _board(cell, lo, hi, grey, ns=COUNTS, eps_list=(dm.MIN_ALBEDO,)):
    """One board of the study: a checkerboard albedo of `cell`-pixel cells, `lo` where the cell's parity is even and `hi` where odd -- RGB
    (a, a / 2, 1 - a) as tests/test_denoise_var_cpu.py has it, or grey (a, a, a) -- under planar guides.  Sample i of a pixel takes the albedo
    at its own jittered position times uniform(0, 2); default_rng(7), per sample the jitters drawn before the factor.  Truth: the box-filtered
    albedo.  Returns {n: {"raw", "guided", "one", ("mean", eps)...}} RMSE."""
    rgb = (lambda a: np.stack([a, a, a], axis=-1)) if grey else (lambda a: np.stack([a, a / 2, 1 - a], axis=-1))
    yy, xx = np.mgrid[0:H, 0:W]
    fx = _even_measure(xx + 1.0, cell) - _even_measure(xx, cell)
    fy = _even_measure(yy + 1.0, cell) - _even_measure(yy, cell)
    even = fx * fy + (1 - fx) * (1 - fy)
    truth = rgb(lo * even + hi * (1 - even))
    pos = np.stack([xx * 0.05, yy * 0.05, np.zeros((H, W))], axis=2).astype(F)
    nrm = np.broadcast_to(np.array([0, 0, 1], F), (H, W, 3)).copy()
    geom = np.zeros((H, W), np.int32)
    rng = np.random.default_rng(7)
    albedos, samples = [], []
    for _ in range(max(ns)):
        j = rng.uniform(0, 1, (H, W, 2))
        parity = (np.floor((xx + j[..., 0]) / cell) + np.floor((yy + j[..., 1]) / cell)) % 2
        a = rgb(np.where(parity == 0, lo, hi)).astype(F)
        albedos.append(a)
        samples.append(a * rng.uniform(0, 2, (H, W, 1)).astype(F))
    rows = {}
    for n in ns:
        S = np.zeros((H, W, 3), F)
        for s in samples[:n]:
            S = S + s
        Q = dv.moments(samples[:n])
        row = {"raw": _rmse(S / F(n), truth), "guided": _rmse(dv.denoise_var(S, Q, n, pos, nrm, geom, *SETTING)[0], truth)}
        one = dm.accumulate([albedos[0]] * n)                       # the demodulator a single guide iteration would give
        mean = dm.accumulate(albedos[:n])
        row["one"] = _rmse(dm.denoise_var_demod(S, Q, one, n, pos, nrm, geom, *SETTING)[0], truth)
        for eps in eps_list:
            row[("mean", eps)] = _rmse(dm.denoise_var_demod(S, Q, mean, n, pos, nrm, geom, *SETTING, eps=eps)[0], truth)
        rows[n] = row
    return rows


def _print(name, rows, eps_list=(dm.MIN_ALBEDO,)):
    for n, r in rows.items():
        print("%-20s n = %2d: unfiltered %.4f  guided %.4f  one-sample albedo %.4f  mean albedo %s" % (
            name, n, r["raw"], r["guided"], r["one"], "  ".join("%.4f (eps 1/%d, x%.2f)" % (r[("mean", e)], round(1 / e), r[("mean", e)] / r["guided"]) for e in eps_list)))


@pytest.fixture(scope="module")
def study():
    out = {"aligned": _board(8.0, 0.25, 0.75, False), "jittered": _board(6.5, 0.25, 0.75, False),
           "black": _board(6.5, 0.0, 0.75, True, eps_list=dm.CANDIDATES), "dark": _board(6.5, 0.02, 0.9, True, eps_list=dm.CANDIDATES)}
    _print("aligned 0.25 / 0.75", out["aligned"])
    _print("6.5 px 0.25 / 0.75", out["jittered"])
    _print("6.5 px 0 / 0.75", out["black"], dm.CANDIDATES)
    _print("6.5 px 0.02 / 0.9", out["dark"], dm.CANDIDATES)
    return out


def _ratio(rows, n, eps=dm.MIN_ALBEDO):
    return rows[n][("mean", eps)] / rows[n]["guided"]


def test_study_the_mean_albedo_halves_the_error_on_textures(study):
    """Measured (RMSE against the box-filtered albedo; 64 x 48, the shipped setting):
        6.5-px cells, 0.25 / 0.75     n    unfiltered  guided  one-sample albedo  mean albedo
                                      2    0.2072      0.1323  0.0911             0.0642   (x 0.48)
                                      4    0.1459      0.0986  0.0912             0.0434   (x 0.44)
                                      16   0.0716      0.0448  0.0818             0.0218   (x 0.49)
                                      64   0.0369      0.0199  0.0606             0.0111   (x 0.56)
        8-px cells (aligned)          2 / 4 / 16 / 64: guided 0.1139 / 0.0804 / 0.0271 / 0.0049, mean albedo 0.0213 / 0.0136 / 0.0055 / 0.0023
    (the module prints the tables it measures; DESIGN.md, "Demodulation", quotes them)."""
    for n in COUNTS:
        assert _ratio(study["jittered"], n) <= 0.7
    for n in (2, 4, 16):
        assert _ratio(study["aligned"], n) <= 0.5
    assert _ratio(study["aligned"], 64) < 1.0


def test_study_a_one_sample_albedo_loses_to_no_demodulation(study):
    """Why k_albedo follows every committed iteration: the albedo of ONE camera sample -- the guide iteration's -- is the wrong demodulator for
    the other samples of a pixel on a texel border; c / A is an outlier there that no sample count averages away."""
    for n in (16, 64):
        assert study["jittered"][n]["one"] > study["jittered"][n]["guided"]
    for n in COUNTS:
        assert study["jittered"][n][("mean", dm.MIN_ALBEDO)] < study["jittered"][n]["one"]


def test_study_dark_texels_and_the_floor_follows_the_rule(study, pt):
    """A black (0 / 0.75) and a dark (0.02 / 0.9) texel, grey, 6.5-px cells.  The known cost: at 64 samples the floor makes the demodulated filter
    lose to the plain one (at most 1.3 x); below it is at most 1.05 x.  The rule for PT_DEMOD_MIN_ALBEDO: of 1/256, 1/64, 1/16 the lowest mean
    RMSE over {black, dark} x {4, 16} samples.  Measured, demodulated over guided at 2 / 4 / 16 / 64 samples with the shipped floor: black
    1.05 / 1.01 / 0.85 / 1.16, dark 0.77 / 0.73 / 0.73 / 1.10; the rule's mean RMSE: 0.0674 at 1/256 and at 1/64 (1/64 ahead in the sixth
    digit: the floor only matters where a pixel's every sample hit the black texel), 0.0787 at 1/16."""
    for board in ("black", "dark"):
        for n in (2, 4, 16):
            assert _ratio(study[board], n) <= 1.05
        assert _ratio(study[board], 64) <= 1.3
    score = {e: np.mean([study[b][n][("mean", e)] for b in ("black", "dark") for n in (4, 16)]) for e in dm.CANDIDATES}
    best = min(dm.CANDIDATES, key=lambda e: score[e])
    print("mean RMSE over {black, dark} x {4, 16}: " + "  ".join("1/%d: %.6f" % (round(1 / e), score[e]) for e in dm.CANDIDATES) +
          "; shipped PT_DEMOD_MIN_ALBEDO 1/%d" % round(1 / pt.PT_DEMOD_MIN_ALBEDO))
    assert F(pt.PT_DEMOD_MIN_ALBEDO) == best == dm.MIN_ALBEDO


# ---- Cornell on the CPU oracle ---------------------------------------------------------------------------------------------------------------
def test_cornell_is_neutral(oracle):
    """A flat-coloured scene has nothing to gain: 72 x 40, depth 8, against 2048 samples; A from the guides' primitive of each of the samples' own
    iterations and the scene's materials.  Demodulated RMSE at most 1.03 x the guided filter's at 2 / 4 / 16 / 64 samples."""
    w, h = 72, 40
    sc = oracle.Scene(os.path.join(SCENES, "cornell.txt"))
    sc.set_resolution(w, h)
    ref = oracle.Renderer(sc.camera, sc.geoms, sc.materials, 8)
    acc = np.zeros(w * h * 3, F)
    singles = []
    for it in range(1, 2049):
        if it <= 64:
            one = np.zeros(w * h * 3, F)
            ref.iterate(it, one)
            singles.append(one.reshape(h, w, 3))
        ref.iterate(it, acc)
    truth = (acc / F(2048)).reshape(h, w, 3).astype(np.float64)
    mats = sc.materials
    albedos = []
    guides = None
    for it in range(1, 65):
        pos_t, nrm, geom = dr.oracle_guides(oracle, ref, it)
        if it == 1:
            guides = (pos_t[:, :3].reshape(h, w, 3), nrm.reshape(h, w, 3), geom.reshape(h, w))
        m = mats[sc.geoms["materialid"][np.maximum(geom, 0)]]
        albedos.append(dm.albedo_of_hit(geom >= 0, m["emittance"], m["hasReflective"], m["hasRefractive"], m["color"]).reshape(h, w, 3))
    pos, nrm, geom = guides
    S = np.zeros((h, w, 3), F)
    for n in range(1, 65):
        S = S + singles[n - 1]
        if n not in COUNTS:
            continue
        Q = dv.moments(singles[:n])
        guided = _rmse(dv.denoise_var(S, Q, n, pos, nrm, geom, *SETTING)[0], truth)
        demod = _rmse(dm.denoise_var_demod(S, Q, dm.accumulate(albedos[:n]), n, pos, nrm, geom, *SETTING)[0], truth)
        print("Cornell n = %2d: guided %.5f  demodulated %.5f  (x %.3f)" % (n, guided, demod, demod / guided))
        assert demod <= 1.03 * guided
