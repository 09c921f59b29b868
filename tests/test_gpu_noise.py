"""The noise statistics and the render-until loop on the MI355X, every comparison bit for bit: k_noise_stats over host arrays
(pt_test_noise_stats) and over rendered frames (pt_noise_stats) against the numpy restatement (tests/noise_ref.py), pt_iterate_until's
sample counts against the stopping rule applied to the CPU oracle's frames and its accumulators against a plain pt_iterate_batch run of the
same length, the refusals, and the headless driver's --noise-threshold.  Frames: one pixel, one full tile, a row of 17 (two tiles, the second
one pixel wide), 33 x 17 (partial tiles on both edges, 3 x 2 tiles: one workgroup, its last wave idle), 72 x 40 (5 x 3 tiles: two
workgroups)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_var_ref as dv
import noise_ref as nr
from conftest import ROOT, SCENES
from test_noise_cpu import special_frame

pytestmark = pytest.mark.gpu
F = np.float32
FLOOR = 0.05
FIELDS = ("samples", "tiles_x", "tiles_y", "tiles", "unconverged", "converged")


@pytest.fixture(scope="module")
def gpu(pt):
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return pt


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(a, b):
    """the same bits, whatever the arrays' shapes"""
    return np.array_equal(_bits(a).reshape(-1), _bits(b).reshape(-1))


def _equal(got, want, tile_map=True):
    """a result of the library against noise_ref.stats, field by field"""
    for f in FIELDS:
        assert got[f] == want[f], (f, got[f], want[f])
    assert _bits(got["max_rel_var"]) == _bits(want["max_rel_var"]) and _bits(got["thr2"]) == _bits(want["thr2"])
    if tile_map:
        assert got["tile_rel_var"].shape == want["tile_rel_var"].shape and _same(got["tile_rel_var"], want["tile_rel_var"])


# ---- 1: the kernel over host arrays -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (16, 16), (17, 1), (33, 17), (72, 40)])
def test_kernel_equals_the_restatement_on_random_frames(gpu, w, h):
    rng = np.random.default_rng(1000 * w + h)
    n = 5
    S = (rng.uniform(0, 4, (h, w, 3)) * 2.0 ** rng.integers(-6, 3, (h, w, 1))).astype(F)       # magnitudes apart: the order of the sums shows
    Q = (rng.uniform(0, 6, (h, w)) * 2.0 ** rng.integers(-6, 6, (h, w))).astype(F)
    r = nr.tile_rel_var(S, Q, n, FLOOR)
    assert np.isfinite(r).all() and (r > 0).any()
    for thr in (float(np.sqrt(np.median(r))), 1e-3, 1e3):          # some tiles flagged, all of them, none
        want = nr.stats(S, Q, n, thr, FLOOR)
        _equal(gpu.test_noise_stats(S, Q, w, h, n, thr, FLOOR), want)
    assert nr.stats(S, Q, n, 1e-3, FLOOR)["unconverged"] == r.size and nr.stats(S, Q, n, 1e3, FLOOR)["converged"]
    # a wave of the grid may take any number of tiles (the library's choice is 2): the same bits, the last wave's share cut at the frame's end
    want = nr.stats(S, Q, n, float(np.sqrt(np.median(r))), FLOOR)
    for tpw in (1, 2, 3, 4, 7):
        _equal(gpu.test_noise_stats(S, Q, w, h, n, float(np.sqrt(np.median(r))), FLOOR, tiles_per_wave=tpw), want)
    # another floor, another sample count
    _equal(gpu.test_noise_stats(S, Q, w, h, 2, 0.7, 2.0), nr.stats(S, Q, 2, 0.7, 2.0))


def test_kernel_equals_the_restatement_on_special_values(gpu):
    """NaN, +-inf and denormals in S and Q (test_noise_cpu.special_frame says what each tile holds), and the NaN ratio of an infinite variance
    in a tile of infinite luminance: neither flagged nor the maximum."""
    S, Q = special_frame()
    want = nr.stats(S, Q, 2, 1.0, FLOOR)
    assert want["unconverged"] == 2 and np.isposinf(want["max_rel_var"]) and 0 < want["tile_rel_var"][0, 2] < 1e-35
    _equal(gpu.test_noise_stats(S, Q, 48, 16, 2, 1.0, FLOOR), want)
    S[:, 16:32] = 0
    S[3, 21] = (np.inf, np.inf, np.inf)
    want = nr.stats(S, Q, 2, 1.0, FLOOR)
    assert np.isnan(want["tile_rel_var"][0, 1]) and want["unconverged"] == 1 and np.isfinite(want["max_rel_var"])
    _equal(gpu.test_noise_stats(S, Q, 48, 16, 2, 1.0, FLOOR), want)


# ---- 2: pt_noise_stats over rendered frames ------------------------------------------------------------------------------------------------
def _init(pt, scene, w, h, depth=8, moments=True, **opts):
    sc = pt.Scene(os.path.join(SCENES, scene))
    sc.set_resolution(w, h)
    pt.pathtraceFree()
    pt.pathtraceInit(sc, traceDepth=depth, moments=moments, **opts)
    return sc


def _render(pt, schedule):
    """seven iterations"""
    if schedule == "iterate":
        for it in range(1, 8):
            pt.pathtrace(None, 0, it, readback=False)
    elif schedule == "batch7":
        pt.pathtrace_batch(None, 0, 1, 7)
    else:
        pt.pathtrace_batch(None, 0, 1, 3)
        pt.pathtrace_batch(None, 0, 4, 4)


def _check_against_own_readback(pt, w, h, n):
    S, Q = pt.readback(w * h).reshape(h, w, 3), pt.readback_moments().reshape(h, w)
    r = nr.tile_rel_var(S, Q, n, FLOOR)
    thr = float(np.sqrt(np.median(r[r > 0]))) if (r > 0).any() else 1.0
    for t in (thr, 1e-3):
        want = nr.stats(S, Q, n, t, FLOOR)
        _equal(pt.noise_stats(n, t, FLOOR, tile_map=True), want)
        got = pt.noise_stats(n, t, FLOOR)                       # no tile map asked for: the same frame words
        assert "tile_rel_var" not in got
        _equal(got, want, tile_map=False)
    assert _same(pt.readback(w * h), S.reshape(-1)) and _same(pt.readback_moments(), Q.reshape(-1))          # both accumulators untouched
    return r


@pytest.mark.parametrize("scene", ["cornell.txt", "sphere.txt"])
@pytest.mark.parametrize("w,h", [(72, 40), (8, 8)])
def test_noise_stats_equals_the_restatement_on_rendered_frames(gpu, scene, w, h):
    _init(gpu, scene, w, h, max_batch=7)
    try:
        _render(gpu, "batch7")
        r = _check_against_own_readback(gpu, w, h, 7)
        _equal(gpu.noise_stats(2, 0.9, 0.5), nr.stats(gpu.readback(w * h).reshape(h, w, 3), gpu.readback_moments().reshape(h, w), 2, 0.9, 0.5),
               tile_map=False)
        if scene == "sphere.txt" and w == 72:
            assert (r == 0).any() and (r > 0).any()             # tiles of misses: V = M = 0, r = 0 / floor^2 = 0, converged
    finally:
        gpu.pathtraceFree()


@pytest.mark.parametrize("schedule,opts", [("iterate", {}), ("batch3+4", dict(max_batch=4)), ("batch7", dict(max_batch=7))])
def test_noise_stats_under_every_commit_schedule(gpu, schedule, opts):
    ref = None
    _init(gpu, "cornell.txt", 72, 40, **opts)
    try:
        _render(gpu, schedule)
        r = _check_against_own_readback(gpu, 72, 40, 7)
    finally:
        gpu.pathtraceFree()
    _init(gpu, "cornell.txt", 72, 40, max_batch=7)
    try:
        _render(gpu, "batch7")
        ref = gpu.noise_stats(7, 1.0, FLOOR, tile_map=True)["tile_rel_var"]
    finally:
        gpu.pathtraceFree()
    assert _same(r, ref)


def test_noise_stats_with_a_caller_owned_accumulator(gpu):
    import torch
    w, h = 72, 40
    acc = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    _init(gpu, "cornell.txt", w, h, max_batch=4, accum_dev=acc.data_ptr())
    try:
        _render(gpu, "batch3+4")
        _check_against_own_readback(gpu, w, h, 7)
        gpu.sync()
        assert _same(acc.cpu().numpy(), gpu.readback(w * h))
        st, done = gpu.iterate_until(8, 1.5, 24, check_every=8, lookahead=0)          # ... and the loop adds to the caller's buffer
        assert done in (15, 23, 24) and _same(acc.cpu().numpy(), gpu.readback(w * h))
    finally:
        gpu.pathtraceFree()


# ---- 3: pt_iterate_until -------------------------------------------------------------------------------------------------------------------
W, H, CAP, EVERY = 72, 40, 96, 8


@pytest.fixture(scope="module")
def cornell(gpu, oracle):
    """Cornell 72 x 40, depth 8, on the CPU oracle: S and Q after 8, 16, ..., 96 iterations"""
    sc = gpu.Scene(os.path.join(SCENES, "cornell.txt"))
    sc.set_resolution(W, H)
    ref = oracle.Renderer(sc.camera.view(oracle.CAMERA_DTYPE), sc.geoms.view(oracle.GEOM_DTYPE), sc.materials.view(oracle.MATERIAL_DTYPE), 8)
    acc = np.zeros(W * H * 3, F)
    Q = np.zeros((H, W), F)
    at = {}
    for it in range(1, CAP + 1):
        one = np.zeros(W * H * 3, F)
        ref.iterate(it, one)
        l = dv.lum(one.reshape(H, W, 3))
        Q = Q + l * l
        ref.iterate(it, acc)
        if it % EVERY == 0:
            at[it] = (acc.reshape(H, W, 3).copy(), Q.copy())
    return at


_plain = {}


def _plain_run(pt, n):
    """S and Q of pt_iterate_batch over iterations 1 .. n in batches of 8 (computed once per length)"""
    if n not in _plain:
        _init(pt, "cornell.txt", W, H, max_batch=8)
        try:
            for first in range(1, n + 1, 8):
                pt.pathtrace_batch(None, 0, first, min(8, n - first + 1))
            _plain[n] = (pt.readback(W * H), pt.readback_moments())
        finally:
            pt.pathtraceFree()
    return _plain[n]


def _rule(at, thr, lookahead, fraction=0.0, min_samples=2, cap=CAP):
    return nr.samples_done(lambda s: nr.stats(*at[s], s, thr, FLOOR, fraction)["converged"], 1, min_samples, cap, EVERY, lookahead)


@pytest.mark.parametrize("lookahead", [0, 1])
@pytest.mark.parametrize("thr,max_batch", [(1.5, 8), (0.75, 3)])
def test_iterate_until_stops_where_the_rule_says(gpu, cornell, thr, max_batch, lookahead):
    """Expected: 24 and 64 samples with lookahead 0, 32 and 72 with lookahead 1 (a round of 8 is split into batches of 3, 3, 2 at max_batch 3)."""
    want_done, want_conv = _rule(cornell, thr, lookahead)
    assert want_conv and want_done == {(1.5, 0): 24, (0.75, 0): 64, (1.5, 1): 32, (0.75, 1): 72}[(thr, lookahead)]
    _init(gpu, "cornell.txt", W, H, max_batch=max_batch)
    try:
        st, done = gpu.iterate_until(1, thr, CAP, lum_floor=FLOOR, check_every=EVERY, lookahead=lookahead)
        S, Q = gpu.readback(W * H), gpu.readback_moments()
        print("threshold %g lookahead %d: %d samples, %s" % (thr, lookahead, done, st))
        assert done == want_done and st["converged"] and st["samples"] == done
        # `out` is the statistics of the final accumulator
        final = nr.stats(S.reshape(H, W, 3), Q.reshape(H, W), done, thr, FLOOR)
        for f in ("tiles_x", "tiles_y", "tiles", "unconverged"):
            assert st[f] == final[f]
        assert _bits(st["max_rel_var"]) == _bits(final["max_rel_var"]) and _bits(st["thr2"]) == _bits(final["thr2"])
        _equal(gpu.noise_stats(done, thr, FLOOR), final, tile_map=False)
        # rendering goes on correctly after the call
        gpu.pathtrace_batch(None, 0, done + 1, min(8, max_batch))
        S2, Q2 = gpu.readback(W * H), gpu.readback_moments()
    finally:
        gpu.pathtraceFree()
    ps, pq = _plain_run(gpu, done)
    assert _same(S, ps) and _same(Q, pq)
    assert _same(S, cornell[done][0]) and _same(Q, cornell[done][1])          # ... which are the oracle's
    if max_batch == 8:
        ps, pq = _plain_run(gpu, done + 8)
        assert _same(S2, ps) and _same(Q2, pq)


def test_iterate_until_ends_at_the_cap_when_the_threshold_is_out_of_reach(gpu, cornell):
    _init(gpu, "cornell.txt", W, H, max_batch=8)
    try:
        for lookahead, cap in ((0, 24), (1, 24), (1, 21)):          # (21: the last round is cut to 5 iterations)
            st, done = gpu.iterate_until(1, 0.01, cap, check_every=EVERY, lookahead=lookahead)
            assert done == cap and not st["converged"] and st["samples"] == cap and st["unconverged"] > 0
            S, Q = gpu.readback(W * H), gpu.readback_moments()
            ps, pq = _plain_run(gpu, cap)
            _init(gpu, "cornell.txt", W, H, max_batch=8)
            assert _same(S, ps) and _same(Q, pq)
        # continuing a frame: first_iter - 1 samples are in the accumulator, the rounds count from there
        gpu.pathtrace_batch(None, 0, 1, 8)
        st, done = gpu.iterate_until(9, 1.5, CAP, check_every=EVERY, lookahead=0)
        assert done == 24 and st["converged"]
        assert _same(gpu.readback(W * H), cornell[24][0])
    finally:
        gpu.pathtraceFree()


def test_min_samples_delays_the_stop_and_a_fraction_brings_it_forward(gpu, cornell):
    assert _rule(cornell, 1.5, 0) == (24, True)
    late = _rule(cornell, 1.5, 0, min_samples=37)
    assert late == (40, True)
    early = _rule(cornell, 0.75, 0, fraction=0.5)
    assert early[1] and early[0] < _rule(cornell, 0.75, 0)[0]
    _init(gpu, "cornell.txt", W, H, max_batch=8)
    try:
        st, done = gpu.iterate_until(1, 1.5, CAP, check_every=EVERY, lookahead=0, min_samples=37)
        assert (done, st["converged"]) == late
        _init(gpu, "cornell.txt", W, H, max_batch=8)
        st, done = gpu.iterate_until(1, 0.75, CAP, check_every=EVERY, lookahead=0, max_unconverged_fraction=0.5)
        assert (done, st["converged"]) == early and 0 < st["unconverged"] <= 7          # floor(0.5 * 15) tiles may stay above
        assert _same(gpu.readback(W * H), cornell[done][0])
        # the Python companion: pathtrace_batch(until=...) renders at most `count` iterations
        _init(gpu, "cornell.txt", W, H, max_batch=8)
        st, done = gpu.pathtrace_batch(None, 0, 1, CAP, until=dict(threshold=1.5, check_every=EVERY, lookahead=0))
        assert done == 24 and st["converged"]
    finally:
        gpu.pathtraceFree()


# ---- 4: refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    w, h = 16, 16
    L = gpu.lib()
    tm = np.full(4, 7, F)
    nan, inf = float("nan"), float("inf")

    def stats(samples=2, thr=1.0, floor=FLOOR, size=None, out=True):
        st = gpu.PtNoiseStats()
        st.tiles = -9
        tm[:] = 7
        rc = L.pt_noise_stats(samples, thr, floor, C.byref(st) if out else None, C.sizeof(st) if size is None else size, tm.ctypes.data_as(C.c_void_p))
        assert rc == 0 or (st.tiles == -9 and (tm == 7).all())
        return rc

    def until(first=1, thr=1.0, floor=FLOOR, frac=0.0, mn=2, mx=8, every=4, look=1, size=None, out=True, target=True):
        tgt, st, done = gpu.PtNoiseTarget(thr, floor, frac, mn, mx, every, look), gpu.PtNoiseStats(), C.c_int32(-5)
        st.tiles = -9
        rc = L.pt_iterate_until(0, first, C.byref(tgt) if target else None, C.sizeof(tgt) if size is None else size, C.byref(st) if out else None,
                                C.byref(done))
        assert rc == 0 or (st.tiles == -9 and done.value == -5)
        return rc

    _init(gpu, "cornell.txt", w, h, depth=4, max_batch=4)
    try:
        gpu.pathtrace_batch(None, 0, 1, 2)
        before, q = gpu.readback(w * h), gpu.readback_moments()
        for bad in (dict(samples=1), dict(samples=0), dict(samples=-2), dict(thr=0.0), dict(thr=-1.0), dict(thr=nan), dict(thr=inf), dict(floor=0.0),
                    dict(floor=-0.05), dict(floor=nan), dict(floor=inf), dict(size=36), dict(size=48), dict(out=False)):
            assert stats(**bad) == -1, bad                      # PT_ERR_INVALID
        for bad in (dict(mn=1), dict(mn=0), dict(thr=0.0), dict(thr=-1.0), dict(thr=nan), dict(thr=inf), dict(floor=0.0), dict(floor=nan),
                    dict(floor=inf), dict(floor=-1.0), dict(frac=-0.1), dict(frac=1.5), dict(frac=nan), dict(every=0), dict(every=-3),
                    dict(first=9, mx=8), dict(first=0), dict(first=-1), dict(look=2), dict(look=-1), dict(size=24), dict(size=32), dict(out=False),
                    dict(target=False), dict(mx=1)):
            assert until(**bad) == -1, bad
        assert _same(gpu.readback(w * h), before) and _same(gpu.readback_moments(), q)          # a refused call enqueues nothing
        assert stats() == 0 and until(first=3) == 0             # ... and the renderer is usable afterwards
    finally:
        gpu.pathtraceFree()
    # PT_FLAG_TRACE_AHEAD: the statistics are there, the loop is not
    _init(gpu, "cornell.txt", w, h, depth=4, max_batch=4, trace_ahead=True)
    try:
        gpu.pathtrace(None, 0, 1, readback=False)
        gpu.pathtrace(None, 0, 2, readback=False)
        assert stats() == 0
        assert until(first=3) == -1 and b"PT_FLAG_TRACE_AHEAD" in L.pt_last_error()
    finally:
        gpu.pathtraceFree()
    # without the flag
    _init(gpu, "cornell.txt", w, h, depth=4, moments=False)
    try:
        gpu.pathtrace(None, 0, 1, readback=False)
        gpu.pathtrace(None, 0, 2, readback=False)
        assert stats() == -1 and b"PT_FLAG_MOMENTS" in L.pt_last_error()
        assert until(first=3) == -1 and b"PT_FLAG_MOMENTS" in L.pt_last_error()
    finally:
        gpu.pathtraceFree()
    assert stats() == -2 and until() == -2                      # PT_ERR_NOT_INIT after pt_free


# ---- 5: the headless driver ----------------------------------------------------------------------------------------------------------------
def test_pt_render_noise_threshold(gpu, cornell, tmp_path):
    from test_host import _decode_png
    exe = os.path.join(ROOT, "project3-cuda-path-tracer_amd", "host", "pt_render")
    args = [exe, os.path.join(SCENES, "cornell.txt"), "--res", str(W), str(H), "--iterations", str(CAP), "--depth", "8", "--batch", "8"]
    r = subprocess.run(args + ["--out", str(tmp_path / "nt"), "--noise-threshold", "1.5", "--check-every", "8"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["nt.png"]
    done = _rule(cornell, 1.5, 1)[0]
    assert done == 32
    S, Q = cornell[done]
    want = nr.stats(S, Q, done, 1.5, FLOOR)
    m = re.search(r"noise threshold 1\.5: (\d+) samples, converged (yes|no), (\d+) of (\d+) tiles above it, largest relative standard error ([0-9.]+)",
                  r.stdout)
    assert m, r.stdout
    assert (int(m.group(1)), m.group(2), int(m.group(3)), int(m.group(4))) == (done, "yes", want["unconverged"], 15)
    assert abs(float(m.group(5)) - float(np.sqrt(np.float64(want["max_rel_var"])))) < 1e-4
    assert re.search(r"^%d iterations of %dx%d" % (done, W, H), r.stdout, re.M)
    conv = lambda mean: (np.clip(mean, 0, 1) * F(255)).astype(np.uint8)[:, ::-1]          # the driver's PNG conversion, X mirrored
    assert np.array_equal(_decode_png(str(tmp_path / "nt.png")), conv(S / F(done)))      # normalised by the samples actually taken
    # a fraction, and a threshold out of reach: the cap
    r = subprocess.run(args[:6] + ["16", "--depth", "8", "--out", str(tmp_path / "cap"), "--noise-threshold", "0.01", "--noise-fraction", "0.25"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert re.search(r"noise threshold 0\.01: 16 samples, converged no, ", r.stdout), r.stdout
    assert np.array_equal(_decode_png(str(tmp_path / "cap.png")), conv(cornell[16][0] / F(16)))
