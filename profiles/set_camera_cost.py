"""What a camera move costs on one MI355X: pt_init's same-scene form (PT_SAME_SCENE: the renderer's buffers kept, the work list's face
certificates on the device, only the tables that differ uploaded) against the full pt_init over the live renderer, which is what a move
cost before.  Wall time of
the call by the host's clock -- both end in a synchronise, so the next pt_iterate can be enqueued when they return.

  reinit    the full re-initialisation alone, split by the host's clock inside pt_init (PT_AMD_INIT_PHASES=1: each phase ended by a device
            synchronise of its own): host planning; the drain and the free; streams, events and every allocation with its zeroing; the
            tables' uploads; launch sizing and the final synchronise.  Per phase best (median) of N calls over the live renderer of 8
            committed iterations, max_batch 8 and 64.
  move      scenes/cornell.txt and scenes/cornell_textured.txt at 1280x720 and 1920x1080, max_batch 8 and 64, a live renderer of 8 committed
            iterations, without and with PT_FLAG_TEMPORAL (PT_FLAG_MOMENTS with it): the two calls alternating in one process between two
            eyes, best (median, worst) of N each; the re-initialisation's own best-to-median spread beside it; the tables and bytes the
            fast path uploaded.
  faces     k_camera_faces for Cornell's one-cube groups by HIP events (pt_test_camera_resolved_device), against the host's time for the
            same certificates: pt_test_camera_resolved less pt_test_camera_list, the same list without them.

The renderer is the test library's (libpt_amd_test.so: the product's source with the test entry points), whose pt_test_last_camera_move
says which way a move went.  Every step runs in a child process of its own under a time limit; the first failure ends the run, nothing
is retried.

    python profiles/set_camera_cost.py

Prints profiles/set_camera_cost.txt."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = [(1280, 720), (1920, 1080)]
SCENES = ["cornell.txt", "cornell_textured.txt"]
N = 11                  # measurements per figure
STEP_LIMIT = 240        # seconds per child
EYES = ((0.0, 5.0, 10.5), (0.4, 5.1, 10.3))


def _package(scene, w, h):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pt = ge.load_package()
    if pt.device_count() < 1:
        raise SystemExit("no HIP device")
    sc = pt.Scene(os.path.join(ROOT, "scenes", scene))
    sc.set_resolution(w, h)
    return pt, sc


def _fmt(v):
    v = np.sort(np.asarray(v, np.float64))
    return "%8.3f (%8.3f, %8.3f)" % (v[0], v[len(v) // 2], v[-1])


def move(scene, w, h, batch, temporal):
    pt, sc = _package(scene, w, h)
    kw = dict(max_batch=batch, moments=temporal, temporal=temporal)
    cams = []
    for e in EYES:
        c = np.array(sc.camera, copy=True)
        c["position"][0] = e
        cams.append(c)
    t_init, t_set, t_plan, info = [], [], [], None
    with pt.renderer_from_test_library():
        sc.camera[:] = cams[0]
        pt.pathtraceInit(sc, **kw)
        for k in range(2 * N + 2):
            pt.pathtrace_batch(None, 0, 1, 8)
            pt.sync()
            cam = cams[(k + 1) % 2]
            if k % 2 == 0:
                sc.camera[:] = cam
                t0 = time.perf_counter()
                pt.pathtraceInit(sc, **kw)
                dt = time.perf_counter() - t0
                if k >= 2:
                    t_init.append(dt * 1e3)
            else:
                t0 = time.perf_counter()
                pt.pathtraceSetCamera(cam)
                dt = time.perf_counter() - t0
                info = pt.camera_move_info()
                if info["fast"] is not True:
                    raise SystemExit("the move took the slow path")
                if k >= 2:
                    t_set.append(dt * 1e3)
        pt.pathtraceFree()
        for k in range(N):      # the host planning alone (no device)
            sc.camera[:] = cams[k % 2]
            t0 = time.perf_counter()
            pt.scene_plan(sc, max_batch=batch, flags=(pt.PT_FLAG_MOMENTS | pt.PT_FLAG_TEMPORAL) if temporal else 0)
            t_plan.append((time.perf_counter() - t0) * 1e3)
    a, b = np.sort(t_init), np.sort(t_set)
    spread = a[len(a) // 2] - a[0]
    print("%-20s %4dx%-4d batch %2d %-8s  full pt_init over the live renderer %s ms [host planning %6.2f, the rest %6.2f]   same-scene form %s ms   "
          "ahead by %7.3f ms = %5.1f x the re-initialisation's best-to-median spread of %.3f; %d tables, %d bytes uploaded"
          % (scene, w, h, batch, "temporal" if temporal else "plain", _fmt(t_init), min(t_plan), a[0] - min(t_plan), _fmt(t_set), a[0] - b[0],
             (a[0] - b[0]) / max(spread, 1e-9), spread, info["tables_uploaded"], info["bytes_uploaded"]))


def reinit(scene, w, h, batch):
    """(child, PT_AMD_INIT_PHASES=1 in its environment) N + 1 full calls over the live renderer; the library prints the phases to stderr"""
    pt, sc = _package(scene, w, h)
    for k in range(N + 2):
        sc.camera["position"][0] = EYES[k % 2]
        pt.pathtraceInit(sc, max_batch=batch)
        pt.pathtrace_batch(None, 0, 1, 8)
        pt.sync()
    pt.pathtraceFree()


def reinit_report(step, stderr):
    rows = [[float(v) for v in line.split()[4::2]] for line in stderr.splitlines() if line.startswith("pt_init phases ms:")][1:]      # (the first call had no renderer to free)
    v = np.sort(np.asarray(rows, np.float64), axis=0)
    tot = np.sort(np.asarray(rows, np.float64).sum(axis=1))
    names = ("plan", "free", "allocate", "upload", "size+sync")
    print("%-20s %4sx%-4s batch %2s  full pt_init over the live renderer, %d calls, best (median) ms per phase: %s; sum %.3f (%.3f)"
          % (step[1], step[2], step[3], step[4], len(rows), ", ".join("%s %.3f (%.3f)" % (n, v[0][i], v[len(v) // 2][i]) for i, n in enumerate(names)),
             tot[0], tot[len(tot) // 2]))


def faces(w, h):
    pt, sc = _package("cornell.txt", w, h)
    cam, geoms = sc.camera.view(pt.CAMERA_DTYPE), sc.geoms.view(pt.GEOM_DTYPE)
    dev, host_all, host_list = [], [], []
    for k in range(N):
        _, ms = pt.camera_resolved_device(cam, geoms, with_ms=True)
        dev.append(ms)
        t0 = time.perf_counter()
        got = pt.camera_resolved(cam, geoms)
        host_all.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        pt.camera_list(cam, geoms)
        host_list.append((time.perf_counter() - t0) * 1e3)
    lanes = got[0].reshape(-1, 64)
    print("cornell.txt %4dx%-4d  %d listed pixels: k_camera_faces %s ms by HIP events; the host's certificates %.3f ms "
          "(pt_test_camera_resolved %.3f less pt_test_camera_list %.3f, best of %d, each called twice: sizes, then arrays)"
          % (w, h, int((lanes != 0xFFFFFFFF).sum()), _fmt(dev), (min(host_all) - min(host_list)) / 2, min(host_all), min(host_list), N))


def main():
    if len(sys.argv) > 1:
        what = sys.argv[1]
        if what == "reinit":
            reinit(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
        elif what == "move":
            move(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), sys.argv[6] == "1")
        else:
            faces(int(sys.argv[2]), int(sys.argv[3]))
        return
    print("camera move on one MI355X: wall ms of the call, best (median, worst) of %d, the two calls alternating in one process" % N)
    steps = [("reinit", s, str(w), str(h), str(b)) for s in SCENES for w, h in FRAMES for b in (8, 64)]
    steps += [("faces", str(w), str(h)) for w, h in FRAMES]
    steps += [("move", s, str(w), str(h), str(b), t) for s in SCENES for w, h in FRAMES for b in (8, 64) for t in ("0", "1")]
    for step in steps:
        sys.stdout.flush()
        env = dict(os.environ, PT_AMD_INIT_PHASES="1") if step[0] == "reinit" else os.environ
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(step), timeout=STEP_LIMIT, stderr=subprocess.PIPE, text=True, env=env)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit("step %r failed with status %d: the run ends here" % (step, r.returncode))
        if step[0] == "reinit":
            reinit_report(step, r.stderr)


if __name__ == "__main__":
    main()
