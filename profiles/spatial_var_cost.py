"""What the spatial variance estimate (PT_FLAG_SPATIAL_VARIANCE) costs on one MI355X, Cornell, at 1280x720 and 1920x1080, against its
yardsticks from the same build and the same run:

  1. stage A (k_temporal<kTemporalMoments>, pt_test_temporal's capture 2) and stage B (k_spatial_variance_*<PT_SPATIAL_RADIUS>,
     pt_test_spatial_variance) over the device's own one-sample accumulators and guides, next to one tiled level of the guided filter at step 1
     (pt_test_denoise_var's per-kernel times) on the same frame -- HIP events, the kernels alternating;
  2. stage B in its two forms, the LDS tiles against the plain gather, on that frame (every pixel takes the estimate) and on the same frame
     with the counts of a view that has history (17 everywhere but a band of one in sixteen columns, as a disocclusion leaves them: the
     tiled form's early-out), and the rule of the issue: the faster form at 1280x720 is the product's, and within the run-to-run spread
     (the gather's best-to-median) the simpler gather stays;
  3. the first displayed frame, pt_iterate(0, 1, rgba8_dev) right after a pt_init, with the flag against without it (the raw conversion)
     and against pt_iterate(0, 1, NULL): wall time of the call plus the wait for the renderer's stream, a fresh renderer for every
     measurement, the three alternating.

Prints the first part of profiles/spatial_var_cost.txt.

    python profiles/spatial_var_cost.py

Stops at the first failure (an exception ends it); nothing is retried."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
FRAMES = [(1280, 720), (1920, 1080)]
ROUNDS, REPS, FIRST_FRAMES = 5, 7, 15


def _package(w, h):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pt = ge.load_package()
    if pt.device_count() < 1:
        raise SystemExit("no HIP device")
    sc = pt.Scene(os.path.join(ROOT, "scenes", "cornell.txt"))
    sc.set_resolution(w, h)
    return pt, sc


def _fmt(v):
    v = np.sort(np.asarray(v, np.float64))
    return "%.4f (%.4f, %.4f)" % (v[0], v[len(v) // 2], v[-1])


def _med(v):
    return float(np.median(np.asarray(v, np.float64)))


def kernels(w, h):
    import spatial_var_ref as sv
    import temporal_ref as tr
    pt, sc = _package(w, h)
    R = pt.PT_SPATIAL_RADIUS
    with pt.renderer_from_test_library():
        pt.pathtraceInit(sc, max_batch=2, moments=True, spatial_variance=True)
        pt.pathtrace_batch(None, 0, 1, 1)
        pt.sync()
        S, Q = pt.readback(w * h).reshape(h, w, 3), pt.readback_moments().reshape(h, w)
        g = tr.pack_guides(*pt.gbuffer(1), h, w)
        M, N = sv.moments_form(S, Q, 1)
        with_history = np.full((h, w), 17.0, np.float32)
        with_history[:, (np.arange(w) % 256) < 16] = 1.0
        frac = float((with_history < 2).mean())
        stage_a = (2, w, h, 1, S, Q, g[0], g[1]) + tr.empty_history(h, w)
        pt.pathtrace_batch(None, 0, 2, 1)                        # (the filter's own level needs two samples)
        pt.test_denoise_var(2, 0, pt.PT_DISPLAY_LEVELS)          # warm-up
        t = {k: [] for k in ("a", "gather", "tiled", "gather_h", "tiled_h", "level")}
        for rnd in range(ROUNDS):
            t["a"] += list(pt.test_temporal(*stage_a, timing_reps=REPS)[1])
            for form, name in ((0, "gather"), (1, "tiled")):
                t[name] += list(pt.test_spatial_variance(R, form, w, h, M, N, g[0], g[1], timing_reps=REPS)[1])
                t[name + "_h"] += list(pt.test_spatial_variance(R, form, w, h, M, with_history, g[0], g[1], timing_reps=REPS)[1])
            for k in range(REPS):
                t["level"].append(pt.test_denoise_var(2, 0, pt.PT_DISPLAY_LEVELS, timing=True)[2][1])
    shipped = "gather" if min(t["gather"]) <= min(t["tiled"]) else "tiled"
    spread = _med(t["gather"]) - min(t["gather"])
    diff = min(t["tiled"]) - min(t["gather"])
    lines = ["%dx%d, one Cornell sample, depth 8, radius %d; HIP events, %d rounds x %d launches, the kernels alternating: ms best (median, worst)."
             % (w, h, R, ROUNDS, REPS),
             "WARM-cache times: the launches repeat over the same buffers.",
             "  stage A  k_temporal<kTemporalMoments>, no history             %s" % _fmt(t["a"]),
             "  stage B  k_spatial_variance_gather<%d>, every pixel estimates  %s" % (R, _fmt(t["gather"])),
             "  stage B  k_spatial_variance_tiled<%d>,  every pixel estimates  %s" % (R, _fmt(t["tiled"])),
             "  stage B  gather, %4.1f %% of the pixels estimate (history)      %s" % (100 * frac, _fmt(t["gather_h"])),
             "  stage B  tiled,  %4.1f %% of the pixels estimate (history)      %s" % (100 * frac, _fmt(t["tiled_h"])),
             "  k_atrous_tiled<AtrousGuided>, level 0 (step 1, 64x8)          %s" % _fmt(t["level"]),
             "  stage A / one filter level: %.2f (best over best);  stage B (gather) / one filter level: %.2f;  (tiled): %.2f"
             % (min(t["a"]) / min(t["level"]), min(t["gather"]) / min(t["level"]), min(t["tiled"]) / min(t["level"])),
             "  tiled - gather: %+.4f ms (best - best), %+.4f ms (median - median); the gather's best-to-median spread: %.4f ms -> %s"
             % (diff, _med(t["tiled"]) - _med(t["gather"]), spread,
                "within the spread: the gather stays" if abs(diff) <= spread else "the faster form is the %s" % shipped)]
    return lines


def first_frame(w, h):
    import torch
    pt, sc = _package(w, h)
    L = pt.lib()
    pbo = torch.zeros((w * h, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    wall = {"null": [], "raw": [], "flag": []}
    try:
        for rnd in range(FIRST_FRAMES + 2):
            for name in wall:
                pt.pathtraceFree()
                pt.pathtraceInit(sc, moments=True, display_filter=True, spatial_variance=name == "flag")
                pt.sync()
                t0 = time.perf_counter()
                rc = L.pt_iterate(0, 1, None if name == "null" else pbo.data_ptr())
                pt.sync()
                dt = (time.perf_counter() - t0) * 1e3
                if rc:
                    raise RuntimeError(L.pt_last_error().decode())
                if rnd >= 2:                                     # (the first two rounds warm up)
                    wall[name].append(dt)
    finally:
        pt.pathtraceFree()
    return ["%dx%d: the first frame after a pt_init (moments + display filter), pt_iterate(0, 1, .) and the wait for the stream: wall ms best (median, worst)"
            % (w, h),
            "of %d, a fresh renderer each, the three alternating:" % FIRST_FRAMES,
            "  pt_iterate(0, 1, NULL)                                       %s" % _fmt(wall["null"]),
            "  pt_iterate(0, 1, rgba8_dev), unflagged: the raw conversion   %s" % _fmt(wall["raw"]),
            "  pt_iterate(0, 1, rgba8_dev) under PT_FLAG_SPATIAL_VARIANCE   %s" % _fmt(wall["flag"]),
            "  the flagged first frame on top of the unflagged one: %.4f ms (best - best), %.4f ms (median - median) -- k_gbuffer, stages A and B and"
            % (min(wall["flag"]) - min(wall["raw"]), _med(wall["flag"]) - _med(wall["raw"])),
            "  the five levels, in place of one k_to_rgba8"]


if __name__ == "__main__":
    out = []
    for w, h in FRAMES:
        out += kernels(w, h) + [""]
    for w, h in FRAMES:
        out += first_frame(w, h) + [""]
    print("\n".join(out[:-1]), flush=True)
