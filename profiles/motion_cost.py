"""What motion blur (PT_FLAG_MOTION) costs on one MI355X, on scenes/cornell_motion.txt, each figure against its baseline from the same build and
the same process, the two alternating, best (median) of N >= 11:

  init      pathtraceInit with the flag (16 poses planned, their tables uploaded) against the unflagged call on step 0's scene, at 1280x720
            and 1920x1080, batch 8, wall-clock ms around the call (the renderer before it freed outside the clock) -- the flagged call twice:
            with the work list's face certificates evaluated on the device (k_camera_faces: the product) and on the host
            (PT_AMD_MOTION_HOST_FACES=1, a switch for this measurement)
  iterate   a flagged renderer against an unflagged one of step 0's scene (two contexts, each continuing its own sequence of iterations), at
            batch 8 and batch 64, 1280x720: ms per iteration over one cycle of 128 iterations, wall clock from the first call to pt_sync
  memory    the scene tables each of the two holds on the device, in bytes as pt_init allocates them (pt_test_pose_tables, from the plans), at
            1280x720 and 1920x1080

Every step runs in a child process of its own under a time limit; the first failure ends the run, nothing is retried.

    python profiles/motion_cost.py

Prints the three sections of profiles/motion_cost.txt (the benchmark against the parent's build is run beside it: bench.py twice each,
alternating, with --dump-frame for the frames' checksums)."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
N = 11
STEP_LIMIT = 240        # seconds per child


def _package(w, h):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    import motion_scenes as ms
    pt = ge.load_package()
    if pt.device_count() < 1:
        raise SystemExit("no HIP device")
    sc = pt.Scene(os.path.join(ROOT, "scenes", "cornell_motion.txt"))
    sc.set_resolution(w, h)
    return pt, sc, ms.StaticScene(sc, sc.step_geoms[0])


def _fmt(v):
    v = np.sort(np.asarray(v, np.float64))
    return "%9.4f (%9.4f)" % (v[0], v[len(v) // 2])


def init(w, h):
    pt, sc, static = _package(w, h)
    t = {"static": [], "device": [], "host": []}
    for rep in range(N + 1):
        for how in ("static", "device", "host"):
            pt.pathtraceFree()
            os.environ["PT_AMD_MOTION_HOST_FACES"] = "1" if how == "host" else "0"
            t0 = time.perf_counter()
            pt.pathtraceInit(static if how == "static" else sc, motion=how != "static", max_batch=8)
            dt = (time.perf_counter() - t0) * 1e3
            if rep:                                         # (the first round loads the code object)
                t[how].append(dt)
    pt.pathtraceFree()
    a, b, c = (np.min(t[k]) for k in ("static", "device", "host"))
    print("  %4dx%-4d  unflagged, step 0's scene %s ms   flagged, 16 poses: certificates on the device %s ms (adds %8.3f ms = %5.2f x the unflagged "
          "call), on the host %s ms (adds %8.3f ms = %5.2f x)" % (w, h, _fmt(t["static"]), _fmt(t["device"]), b - a, b / a, _fmt(t["host"]), c - a, c / a))


def iterate(w, h, batch):
    pt, sc, static = _package(w, h)
    ctx = {False: pt.Context(), True: pt.Context()}
    nxt = {False: 1, True: 1}
    for motion in (False, True):
        with ctx[motion]:
            pt.pathtraceInit(sc if motion else static, motion=motion, max_batch=batch)
    t = {False: [], True: []}

    def cycle(motion):
        with ctx[motion]:
            pt.sync()
            t0 = time.perf_counter()
            for _ in range(128 // batch):
                pt.pathtrace_batch(None, 0, nxt[motion], batch)
                nxt[motion] += batch
            pt.sync()
            return (time.perf_counter() - t0) * 1e3 / 128

    for rep in range(N + 2):
        for motion in (False, True):
            dt = cycle(motion)
            if rep >= 2:
                t[motion].append(dt)
    frames = {}
    for motion in (False, True):
        with ctx[motion]:
            frames[motion] = pt.readback(w * h)
            pt.pathtraceFree()
        ctx[motion].destroy()
    s = np.sort(t[False])
    spread = s[len(s) // 2] - s[0]
    d = np.min(t[True]) - np.min(t[False])
    print("  %4dx%-4d batch %2d  static %s ms / iteration   motion-blurred %s   difference %+8.4f ms = %+5.1f x the static side's best-to-median "
          "spread of %.4f   (the frames differ: %s)" % (w, h, batch, _fmt(t[False]), _fmt(t[True]), d, d / spread if spread > 0 else float("inf"), spread,
                                                      not np.array_equal(frames[False], frames[True])))


def memory(w, h):
    pt, sc, static = _package(w, h)
    out = {}
    with pt.renderer_from_test_library():
        for motion in (False, True):
            pt.pathtraceFree()
            pt.pathtraceInit(sc if motion else static, motion=motion, max_batch=8)
            t = pt.pose_tables()
            out[motion] = (t["shared_bytes"] + t["all_own_bytes"], t)
            pt.pathtraceFree()
    t = out[True][1]
    print("  %4dx%-4d  unflagged %10d bytes of scene tables   flagged %10d bytes in %d poses of %d tables each (step 0's: %d bytes) and %d held once "
          "(%d bytes)   the 16 poses add %d bytes = %.2f MB" % (w, h, out[False][0], out[True][0], t["poses"], t["own_buffers"], t["own_bytes"],
                                                             t["shared_buffers"], t["shared_bytes"], out[True][0] - out[False][0],
                                                             (out[True][0] - out[False][0]) / 1e6))


def _child(*args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(a) for a in args], timeout=STEP_LIMIT)
    if r.returncode:
        raise SystemExit("motion_cost.py %s ended with %d" % (" ".join(str(a) for a in args), r.returncode))


def main():
    if len(sys.argv) > 1:
        {"init": init, "iterate": iterate, "memory": memory}[sys.argv[1]](*[int(v) for v in sys.argv[2:]])
        return
    print("1. pathtraceInit, wall-clock ms, best (median) of %d, the two alternating" % N, flush=True)
    for w, h in ((1280, 720), (1920, 1080)):
        _child("init", w, h)
    print("2. ms per iteration over a cycle of 128 iterations, best (median) of %d, the two alternating" % N, flush=True)
    for batch in (8, 64):
        _child("iterate", 1280, 720, batch)
    print("3. scene tables on the device, bytes as allocated", flush=True)
    for w, h in ((1280, 720), (1920, 1080)):
        _child("memory", w, h)


if __name__ == "__main__":
    main()
