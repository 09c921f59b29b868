"""What the display filter (PT_FLAG_DISPLAY_FILTER) costs on one MI355X, Cornell from 16 samples on, at 1280x720 and 1920x1080, everything of a
frame size alternating in one run, HIP events, best and median of 35:

  1. per displayed frame, what a host does today for the filtered preview -- pt_denoise_var_rgba8 into page-locked host memory (it synchronises)
     and the upload of those bytes into the device buffer it displays from -- against the flagged pt_iterate(..., rgba8_dev), both next to the
     pt_iterate(..., NULL) they come on top of (events on the renderer's stream around each call; every timed pt_iterate adds one sample);
  2. the last level that writes the bytes itself against the two launches it replaces -- the parent's k_atrous_*<AtrousGuided, false, true> and
     k_to_rgba8, which this build holds instruction for instruction (profiles/display_resource_usage.txt) -- through pt_test_display's
     per-kernel times at exactly 16 samples, and the rule of the issue: the fused level stays only if it is not slower than the pair by more than
     the pair's own best-to-median spread.

Prints the first part of profiles/display_cost.txt (the bench.py comparison behind it was run and added by hand: the file gives the command).

    python profiles/display_cost.py

Stops at the first failure (an exception ends it); nothing is retried."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = [(1280, 720), (1920, 1080)]
REPS, SAMPLES = 35, 16


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


def host_against_device(w, h):
    import torch
    pt, sc = _package(w, h)
    L = pt.lib()
    stream = torch.cuda.Stream()
    pbo = torch.zeros((w * h, 4), dtype=torch.uint8, device="cuda")
    shown = torch.zeros((w * h, 4), dtype=torch.uint8, device="cuda")
    pinned = torch.zeros((w * h, 4), dtype=torch.uint8).pin_memory()
    prm = pt.PtDenoiseVarParams(pt.PT_DISPLAY_LEVELS, pt.PT_DISPLAY_GUIDE_ITER, pt.PT_DISPLAY_SIGMA_LUM, pt.PT_DISPLAY_SIGMA_NORMAL, pt.PT_DISPLAY_SIGMA_POSITION)
    torch.cuda.synchronize()
    t = {"null": [], "flag": [], "host": []}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        ev[0].record(stream)
        fn()
        ev[1].record(stream)
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1])

    def check(rc):
        if rc:
            raise RuntimeError(L.pt_last_error().decode())

    it = [SAMPLES]

    def iterate(ptr):
        it[0] += 1
        check(L.pt_iterate(0, it[0], ptr))

    def host_path():
        # (the filter's bytes to the host, synchronised, and back up into the buffer the display reads)
        check(L.pt_denoise_var_rgba8(it[0], C.byref(prm), C.sizeof(prm), pinned.data_ptr()))
        with torch.cuda.stream(stream):
            shown.copy_(pinned, non_blocking=True)

    try:
        pt.pathtraceFree()
        pt.pathtraceInit(sc, max_batch=8, moments=True, display_filter=True, stream=stream.cuda_stream)
        pt.pathtrace_batch(None, 0, 1, 8)
        pt.pathtrace_batch(None, 0, 9, SAMPLES - 8)
        for _ in range(3):                                       # warm-up of every timed shape
            iterate(None)
            iterate(pbo.data_ptr())
            host_path()
        stream.synchronize()
        same = bool(torch.equal(pbo, shown))                     # (the host path ran behind the flagged call at the same count)
        for _ in range(REPS):
            t["null"].append(timed(lambda: iterate(None)))
            t["flag"].append(timed(lambda: iterate(pbo.data_ptr())))
            t["host"].append(timed(host_path))
        pt.sync()
    finally:
        pt.pathtraceFree()
    if not same:
        raise SystemExit("the device path's bytes differ from the host path's")
    dflag = (min(t["flag"]) - min(t["null"]), _med(t["flag"]) - _med(t["null"]))
    return ["%dx%d, Cornell, depth 8, from %d samples on (every timed pt_iterate adds one); HIP events on the renderer's stream around each call, the three"
            % (w, h, SAMPLES),
            "alternating, %d each: ms best (median, worst).  The two paths' bytes are equal." % REPS,
            "  pt_iterate(iter, NULL)                                      %s" % _fmt(t["null"]),
            "  pt_iterate(iter, rgba8_dev) under PT_FLAG_DISPLAY_FILTER    %s" % _fmt(t["flag"]),
            "  today: pt_denoise_var_rgba8 -> page-locked host, + upload   %s" % _fmt(t["host"]),
            "  the display on top of pt_iterate(iter, NULL): flagged %.4f ms (best - best), %.4f ms (median - median); today's host path %.4f ms"
            % (dflag[0], dflag[1], min(t["host"])),
            "  (best), %.4f ms (median): %.2f x / %.2f x the flagged path's" % (_med(t["host"]), min(t["host"]) / dflag[0], _med(t["host"]) / dflag[1])]


def fused_against_pair(w, h):
    import torch
    pt, sc = _package(w, h)
    pbo = torch.zeros((w * h, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    last = {True: [], False: []}
    whole = {True: [], False: []}
    with pt.renderer_from_test_library():
        pt.pathtraceInit(sc, max_batch=8, moments=True)
        pt.pathtrace_batch(None, 0, 1, 8)
        pt.pathtrace_batch(None, 0, 9, SAMPLES - 8)
        for fused in (True, False):
            pt.test_display(SAMPLES, 0, pbo.data_ptr(), fused=fused, timing=True)
        for _ in range(REPS):
            for fused in (True, False):
                ms = pt.test_display(SAMPLES, 0, pbo.data_ptr(), fused=fused, timing=True)
                last[fused].append(ms[pt.PT_DISPLAY_LEVELS])
                whole[fused].append(float(ms[1:].sum()))
    pair = np.sort(np.asarray(last[False], np.float64))
    spread = pair[len(pair) // 2] - pair[0]
    slower = min(last[True]) - pair[0]
    keep = slower <= spread
    return ["%dx%d, Cornell at %d samples: the last of the %d levels (step 16, the gather), HIP events, %d each, the two alternating: ms best (median, worst)"
            % (w, h, SAMPLES, pt.PT_DISPLAY_LEVELS, REPS),
            "  fused: k_atrous_gather<AtrousGuided, false, true, true> writes the bytes  %s" % _fmt(last[True]),
            "  pair:  k_atrous_gather<AtrousGuided, false, true>, then k_to_rgba8        %s" % _fmt(last[False]),
            "  the five levels together: fused %s, pair %s" % (_fmt(whole[True]), _fmt(whole[False])),
            "  fused - pair: %+.4f ms (best - best), %+.4f ms (median - median); the pair's best-to-median spread: %.4f ms -> the fused level %s"
            % (slower, _med(last[True]) - _med(last[False]), spread, "stays" if keep else "GOES: keep the two launches")]


if __name__ == "__main__":
    out = []
    for w, h in FRAMES:
        out += host_against_device(w, h) + [""]
    for w, h in FRAMES:
        out += fused_against_pair(w, h) + [""]
    print("\n".join(out[:-1]), flush=True)
