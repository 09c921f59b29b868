"""What demodulated history (PT_FLAG_DEMOD_HISTORY) costs on one MI355X, on scenes/cornell_textured.txt at 1280x720 and 1920x1080, HIP events,
best (median) of 35, the things compared alternating within one run of one build:

  forms     the six instantiations of k_temporal -- filter, capture and moments form, each without and with ALBEDO -- over the device's own
            frame after a camera move (pt_test_temporal / pt_test_temporal_albedo), and the front at two samples and more as ONE launch
            (k_temporal<kTemporalFilterDemod, true>) against the TWO it fuses (k_temporal<kTemporalFilter, true>, k_demodulate<true>).
            The fused form becomes the product's only if it is ahead by more than the two-launch form's own best-to-median spread.
  display   the displayed frame, pt_iterate_batch(.., rgba8_dev) at batch 1 under PT_FLAG_DISPLAY_FILTER in a context that holds history, of a
            flagged renderer against a PT_FLAG_TEMPORAL one, ms per call

Every step runs in a child process of its own under a time limit; the first failure ends the run, nothing is retried.

    python profiles/demod_history_cost.py

Prints profiles/demod_history_cost.txt."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
FRAMES = [(1280, 720), (1920, 1080)]
SCENE = "cornell_textured.txt"
N, REPS = 35, 5         # N measurements per figure, REPS per call: N / REPS alternating rounds
STEP_LIMIT = 240        # seconds per child
E0 = (0.4, 5.1, 10.3)


def _package(w, h):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pt = ge.load_package()
    if pt.device_count() < 1:
        raise SystemExit("no HIP device")
    sc = pt.Scene(os.path.join(ROOT, "scenes", SCENE))
    sc.set_resolution(w, h)
    return pt, sc


def _fmt(v):
    v = np.sort(np.asarray(v, np.float64))
    return "%.4f (%.4f)" % (v[0], v[len(v) // 2])


def _move(pt, sc, flagged, old, **opts):
    """`old` iterations from E0, then the re-initialisation at the scene's camera with no free: a context with history"""
    kw = dict(moments=True, temporal=True, spatial_variance=True, demodulate=flagged, demod_history=flagged, **opts)
    home = tuple(float(v) for v in sc.camera["position"][0])
    sc.camera["position"][0] = E0
    pt.pathtraceInit(sc, **kw)
    pt.pathtrace_batch(None, 0, 1, old)
    sc.camera["position"][0] = home
    pt.pathtraceInit(sc, **kw)


def forms(w, h):
    import temporal_ref as tr
    pt, sc = _package(w, h)
    with pt.renderer_from_test_library():
        _move(pt, sc, True, 4, max_batch=4)
        pt.pathtrace_batch(None, 0, 5, 2)
        S, Q, A = pt.readback(w * h), pt.readback_moments(), pt.test_albedo()
        g = tr.pack_guides(*pt.gbuffer(1), h, w)
        hs, ha = pt.test_history(), pt.test_history_albedo()
        pt.pathtraceFree()
    plain = (w, h, 2, S, Q, g[0], g[1], hs["hc"], hs["hn"], hs["hpos_t"], hs["hnrm_id"], hs["cam"])
    alb = (w, h, 2, S, Q, g[0], g[1], A, hs["hc"], hs["hn"], ha, hs["hpos_t"], hs["hnrm_id"], hs["cam"])
    runs = {}
    for form, name in enumerate(("filter", "capture", "moments")):
        runs["%s" % name] = lambda form=form: pt.test_temporal(form, *plain, timing_reps=REPS)[1]
        runs["%s, ALBEDO" % name] = lambda form=form: pt.test_temporal_albedo(form, *alb, timing_reps=REPS)[1]
    runs["front, fused (1 launch)"] = lambda: pt.test_temporal_albedo(0, *alb, front=1, timing_reps=REPS)[1]
    runs["front, 2 launches"] = lambda: pt.test_temporal_albedo(0, *alb, front=2, timing_reps=REPS)[1]
    t = {k: [] for k in runs}
    for rnd in range(N // REPS + 1):
        for k, fn in runs.items():
            ms = fn()
            if rnd:                                              # (the first round warms up)
                t[k] += list(ms)
    lines = ["  k_temporal<%-16s>  %s" % (k, _fmt(v)) for k, v in t.items() if not k.startswith("front")]
    one, two = np.sort(t["front, fused (1 launch)"]), np.sort(t["front, 2 launches"])
    spread = two[len(two) // 2] - two[0]
    lines.append("  the front at >= 2 samples: fused %s  two launches %s  fused ahead by %.4f; the two-launch form's best-to-median spread %.4f: %s"
                 % (_fmt(one), _fmt(two), two[0] - one[0], spread, "the fused form is ahead by more" if two[0] - one[0] > spread else "not ahead by more"))
    return lines


def display(w, h):
    import torch
    pt, sc = _package(w, h)
    pbo = torch.zeros((w * h, 4), dtype=torch.uint8, device="cuda")
    ctx = {f: pt.Context() for f in (False, True)}
    t = {False: [], True: []}
    nxt = {False: 1, True: 1}          # (the count the bytes are made with is the call's `iter`: the new view counts from 1)
    try:
        for f, c in ctx.items():
            with c:
                _move(pt, sc, f, 4, max_batch=4, display_filter=True)
        for rnd in range(N + 3):
            for f, c in ctx.items():
                with c:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    pt.pathtrace_batch(pbo.data_ptr(), 0, nxt[f], 1)
                    e1.record()
                    e1.synchronize()
                    nxt[f] += 1
                    if rnd >= 3:                                  # (the first three rounds warm up: the guides, and the one-sample frame's other launches)
                        t[f].append(e0.elapsed_time(e1))
    finally:
        for c in ctx.values():
            with c:
                pt.pathtraceFree()
            c.destroy()
    return ["  displayed frame with history, pt_iterate_batch(.., rgba8_dev) at batch 1, ms per call: PT_FLAG_TEMPORAL %s  + PT_FLAG_DEMOD_HISTORY %s  +%.4f (+%.4f)"
            % (_fmt(t[False]), _fmt(t[True]), min(t[True]) - min(t[False]), np.median(t[True]) - np.median(t[False]))]


STEPS = {"forms": forms, "display": display}

if __name__ == "__main__":
    if len(sys.argv) == 4:
        print("\n".join(STEPS[sys.argv[1]](int(sys.argv[2]), int(sys.argv[3]))), flush=True)
        raise SystemExit(0)
    print("ms, best (median) of %d; %s." % (N, SCENE), flush=True)
    for w, h in FRAMES:
        print("%dx%d" % (w, h), flush=True)
        for step in STEPS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), step, str(w), str(h)], timeout=STEP_LIMIT)
            if r.returncode:
                raise SystemExit("step %s failed with %d: stopping" % (step, r.returncode))
