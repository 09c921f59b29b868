"""What temporal reprojection costs on one MI355X, Cornell, against its yardsticks from the same build and the same run: k_temporal in both
forms (pt_test_temporal over the device's own accumulators, guides and captured history: HIP events) next to one tiled level of k_atrous_tiled<AtrousGuided>
and k_gbuffer (pt_test_denoise_var's per-kernel times) on the same frame, the three alternating, at 1280x720 and 1920x1080; and the wall time
of a pt_init over a live renderer with PT_FLAG_TEMPORAL (the capture: k_temporal<true>, the guides' hand-over, one stream synchronisation)
against the same call without the flag, the two alternating.  Prints the first part of profiles/temporal_cost.txt (the bench.py comparison
behind it was run and added by hand: the file gives the command).

    python profiles/temporal_cost.py

Stops at the first failure (an exception ends it); nothing is retried."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
FRAMES = [(1280, 720), (1920, 1080)]
REPS, ROUNDS, OLD, NEW, LEVELS = 7, 5, 16, 4, 5
HBM_PEAK_GBS = 8000.0          # bench.py: HBM_PEAK_GBS
EYES = [(0.0, 5.0, 10.5), (0.4, 5.1, 10.3)]


def _package(w, h):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pt = ge.load_package()
    if pt.device_count() < 1:
        raise SystemExit("no HIP device")
    sc = pt.Scene(os.path.join(ROOT, "scenes", "cornell.txt"))
    sc.set_resolution(w, h)
    return pt, sc


def _init(pt, sc, eye, temporal):
    sc.camera["position"][0] = eye
    pt.pathtraceInit(sc, max_batch=8, moments=True, temporal=temporal)


def _fmt(v):
    v = np.sort(np.asarray(v, np.float64))
    return "%.4f (%.4f, %.4f)" % (v[0], v[len(v) // 2], v[-1])


def frame(w, h):
    import temporal_ref as tr
    pt, sc = _package(w, h)
    lines = []
    with pt.renderer_from_test_library():
        _init(pt, sc, EYES[0], True)
        pt.pathtrace_batch(None, 0, 1, 8)
        pt.pathtrace_batch(None, 0, 9, OLD - 8)
        _init(pt, sc, EYES[1], True)
        pt.pathtrace_batch(None, 0, OLD + 1, NEW)
        pt.sync()
        hist = pt.test_history()
        S, Q = pt.readback(w * h).reshape(h, w, 3), pt.readback_moments().reshape(h, w)
        g = tr.pack_guides(*pt.gbuffer(1), h, w)
        args = (w, h, NEW, S, Q, g[0], g[1], hist["hc"], hist["hn"], hist["hpos_t"], hist["hnrm_id"], hist["cam"])
        _, Nh = tr.reproject(g[0], g[1], hist["hc"], hist["hn"], hist["hpos_t"], hist["hnrm_id"], hist["cam"])
        pt.test_denoise_var(NEW, 0, LEVELS)                 # warm-up
        t_filter, t_capture, t_level, t_gbuf = [], [], [], []
        calls = 0
        for rep in range(ROUNDS):
            t_filter += list(pt.test_temporal(False, *args, timing_reps=REPS)[1])
            t_capture += list(pt.test_temporal(True, *args, timing_reps=REPS)[1])
            for k in range(REPS):
                calls += 1
                _, _, ms = pt.test_denoise_var(NEW, 0, LEVELS, guide_iter=1 + (calls & 1), timing=True)      # (another guide_iter every call: k_gbuffer runs)
                t_gbuf.append(ms[0])
                t_level.append(ms[1])
    px = w * h
    lines.append("%dx%d after %d + %d Cornell iterations, depth 8, eye %s -> %s; %.1f %% of the pixels find history; HIP events, %d rounds x %d launches,"
                 % (w, h, OLD, NEW, EYES[0], EYES[1], 100.0 * float((Nh > 0).mean()), ROUNDS, REPS))
    lines.append("the kernels alternating: ms best (median, worst).  These are WARM-cache times: the launches repeat over the same %.0f MB of buffers, which"
                 % (120 * px / 1e6))
    lines.append("fit or nearly fit the 256 MB Infinity Cache.  For scale only: a pixel's own streams (60 B read, 16 / 20 written; the four taps' 52 B each NOT")
    lines.append("counted) are %.1f MB = %.4f ms at the %g GB/s HBM peak -- a floor for a cold launch, not a bound on these numbers."
                 % (76 * px / 1e6, 76 * px / (HBM_PEAK_GBS * 1e6), HBM_PEAK_GBS))
    lines.append("  k_temporal<false> (filter form)                  %s" % _fmt(t_filter))
    lines.append("  k_temporal<true>  (capture form)                 %s" % _fmt(t_capture))
    lines.append("  k_atrous_tiled<AtrousGuided>, level 0 (step 1, 64x8)  %s" % _fmt(t_level))
    lines.append("  k_gbuffer                                        %s" % _fmt(t_gbuf))
    lines.append("  k_temporal<false> / one filter level: %.2f (best over best), %.2f (median over median)"
                 % (min(t_filter) / min(t_level), float(np.median(t_filter)) / float(np.median(t_level))))
    return lines


def reinit(w, h):
    pt, sc = _package(w, h)
    wall = {True: [], False: []}
    try:
        for rnd in range(ROUNDS + 1):
            for flag in (True, False):
                pt.pathtraceFree()
                _init(pt, sc, EYES[0], flag)
                pt.pathtrace_batch(None, 0, 1, 8)
                pt.sync()
                t0 = time.perf_counter()
                _init(pt, sc, EYES[1], flag)                # over the live renderer
                dt = (time.perf_counter() - t0) * 1e3
                if rnd:                                     # (the first round warms up)
                    wall[flag].append(dt)
    finally:
        pt.pathtraceFree()
    f, u = np.sort(wall[True]), np.sort(wall[False])
    return ["%dx%d: pt_init over a live renderer of 8 committed iterations, wall ms best (median, worst) of %d, the two alternating:" % (w, h, ROUNDS),
            "  with PT_FLAG_TEMPORAL (captures)   %s" % _fmt(f),
            "  without                            %s" % _fmt(u),
            "  extra: %.3f ms (best - best), %.3f ms (median - median)" % (f[0] - u[0], f[len(f) // 2] - u[len(u) // 2])]


if __name__ == "__main__":
    out = []
    for w, h in FRAMES:
        out += frame(w, h) + [""]
    for w, h in FRAMES:
        out += reinit(w, h) + [""]
    print("\n".join(out[:-1]))
