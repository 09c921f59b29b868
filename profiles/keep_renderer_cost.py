"""What PT_FLAG_KEEP_RENDERER and the shim's keep switch buy a host on the reference's three symbols, on one MI355X.

  protocol  the camera move as the reference's host makes it -- pathtraceFree(); pathtraceInit(scene); through host/pathtrace_shim.cpp -- by
            the host's clock, over a renderer that has rendered 8 iterations: with the keep switch off (Free frees, Init builds: what every
            such host paid so far) and on (Free parks, Init sets the flag, the library moves in place), the two alternating in ONE process
            (profiles/keep_renderer_host.cpp), best (median, worst) of N.  scenes/cornell.txt and cornell_textured.txt at 1280x720 and
            1920x1080, PT_AMD_TRACE_AHEAD 8 and 64 (the shim's max_batch).  "parent": the same host built against the PARENT commit's shim
            and library (PT_AMD_PARENT names a checkout of it with both built), in the same run: the baseline for "before".
  flag      the full-argument pt_init with the flag -- the scene registered again in front of it (pt_set_meshes, pt_set_textures,
            pt_set_bump_maps), as the shim and pathtraceInit do -- next to pt_init's same-scene form, both called through ctypes with
            arguments made beforehand, in turns in one process over the same eight rows: what the flag adds to the move is the registration's
            copies and the comparison, reported against the same-scene form's own best-to-median spread.
  rate      the steady-state price of PT_AMD_TEMPORAL under the shim, which traces nothing ahead with it: pathtrace calls per second on
            scenes/cornell.txt at 1280x720, with and without, and the ratio.

Every step runs in a child process of its own under a time limit; the first failure ends the run, nothing is retried.

    python profiles/keep_renderer_cost.py [--build-only]

Prints profiles/keep_renderer_cost.txt."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "project3-cuda-path-tracer_amd")
OUT = os.path.join(ROOT, "profiles", "out")
FRAMES = [(1280, 720), (1920, 1080)]
SCENES = ["cornell.txt", "cornell_textured.txt"]
N = 11
STEP_LIMIT = 300
EYES = ((0.0, 5.0, 10.5), (0.4, 5.1, 10.3))
PARENT = os.environ.get("PT_AMD_PARENT")


def _fmt(v):
    v = np.sort(np.asarray(v, np.float64))
    return "%8.3f (%8.3f, %8.3f)" % (v[0], v[len(v) // 2], v[-1])


def _host(tree, name, defs=()):
    """the measuring host linked against the shim and libraries of `tree`; -> (binary, the directories its libraries lie in)"""
    pkg = os.path.join(tree, "project3-cuda-path-tracer_amd")
    exe = os.path.join(OUT, name)
    src = os.path.join(ROOT, "profiles", "keep_renderer_host.cpp")
    deps = [src, os.path.join(pkg, "host", "pathtrace_shim.cpp"), os.path.join(pkg, "host", "pathtrace.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        os.makedirs(OUT, exist_ok=True)
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fno-fast-math"] + list(defs) +
                              ["-I" + os.path.join(pkg, "host"), "-I" + os.path.join(tree, "include"), "-o", exe, src,
                               os.path.join(pkg, "host", "pathtrace_shim.cpp"), "-L" + os.path.join(pkg, "host"), "-lpt_host",
                               "-L" + os.path.join(pkg, "csrc"), "-lpt_amd"])
    return exe, [os.path.join(pkg, "host"), os.path.join(pkg, "csrc")]


def _run_host(host, args):
    exe, libs = host
    env = dict(os.environ, LD_LIBRARY_PATH=":".join(libs + [os.environ.get("LD_LIBRARY_PATH", "")]))
    for k in ("PT_AMD_KEEP_RENDERER", "PT_AMD_TEMPORAL", "PT_AMD_DEVICES", "PT_AMD_DEMODULATE", "PT_AMD_DISPLAY_FILTER", "PT_AMD_SPATIAL_VARIANCE"):
        env.pop(k, None)
    r = subprocess.run([exe] + [str(a) for a in args], timeout=STEP_LIMIT, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit("%s %r failed with status %d: the run ends here" % (os.path.basename(exe), args, r.returncode))
    return {line.split()[0]: line.split()[1:] for line in r.stdout.splitlines() if line.strip()}


def protocol(here, parent):
    for scene in SCENES:
        for w, h in FRAMES:
            for ahead in (8, 64):
                got = _run_host(here, ["move", os.path.join(ROOT, "scenes", scene), w, h, ahead, N])
                off, on = [float(v) for v in got["without"]], [float(v) for v in got["keep"]]
                line = "%-20s %4dx%-4d ahead %2d  Free + Init: switch off %s ms   PT_AMD_KEEP_RENDERER %s ms   %5.1f x" % (
                    scene, w, h, ahead, _fmt(off), _fmt(on), min(off) / min(on))
                if parent:
                    got = _run_host(parent, ["move", os.path.join(ROOT, "scenes", scene), w, h, ahead, N])
                    line += "   parent's shim and library %s ms" % _fmt([float(v) for v in got["without"]])
                print(line)
                sys.stdout.flush()


def rate(here):
    res = {0: [], 1: []}
    for temporal in (0, 1) * 3:
        got = _run_host(here, ["rate", os.path.join(ROOT, "scenes", "cornell.txt"), 1280, 720, temporal, 3000])
        res[temporal].append(float(got["rate"][4]))
    plain, temp = float(np.median(res[0])), float(np.median(res[1]))
    print("cornell.txt 1280x720, pathtrace calls per second through the shim (3000 calls after 40; three runs each, in turns; the median): "
          "default (32 iterations traced ahead) %.1f %r   PT_AMD_TEMPORAL=1 (nothing traced ahead) %.1f %r   ratio %.3f"
          % (plain, res[0], temp, res[1], temp / plain))


def flag(scene, w, h, batch):
    """(child) pathtraceInit(keep=True) and pathtraceSetCamera over one live renderer, in turns of two moves each -- the eye alternates
    between two places with every move, so each kind of call makes the move in both directions (the work list's length, and with it the
    host's planning and the bytes uploaded, depends on the pose)"""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pt = ge.load_package()
    if pt.device_count() < 1:
        raise SystemExit("no HIP device")
    sc = pt.Scene(os.path.join(ROOT, "scenes", scene))
    sc.set_resolution(w, h)
    kw = dict(max_batch=batch, keep=True)
    cams = []
    for e in EYES:
        c = np.array(sc.camera, copy=True)
        c["position"][0] = e
        cams.append(c)
    t_flag, t_set = [], []
    import ctypes as C
    geoms, mats = np.ascontiguousarray(sc.geoms), np.ascontiguousarray(sc.materials)
    gp, mp = geoms.ctypes.data_as(C.c_void_p), mats.ctypes.data_as(C.c_void_p)
    opt = pt.PtOptions(0, 1, -1, pt.PT_FLAG_KEEP_RENDERER, 0, batch, None, None, 0.0, 0.0)     # (what pathtraceInit(sc, **kw) passes)
    with pt.renderer_from_test_library():
        L = pt.lib()
        sc.camera[:] = cams[0]
        pt.pathtraceInit(sc, **kw)
        for k in range(4 * ((N + 1) // 2) + 4):
            pt.pathtrace_batch(None, 0, 1, 8)
            pt.sync()
            cam = np.ascontiguousarray(cams[(k + 1) % 2])
            cp = cam.ctypes.data_as(C.c_void_p)
            flagged = (k // 2) % 2 == 0
            t0 = time.perf_counter()
            if flagged:
                pt.set_meshes(sc.meshes, sc.mesh_normals, sc.mesh_materials)
                pt.set_textures(sc.textures, sc.geom_textures, sc.mesh_uvs)
                pt.set_bump_maps(sc.geom_bumps, sc.bump_scales, sc.mesh_uvs)
                rc = L.pt_init(cp, gp, len(geoms), mp, len(mats), sc.traceDepth, C.byref(opt))
            else:
                rc = L.pt_init(cp, None, 0, None, 0, pt.PT_SAME_SCENE, None)
            dt = (time.perf_counter() - t0) * 1e3
            if rc:
                raise SystemExit("call %d failed: %s" % (k, L.pt_last_error().decode()))
            if pt.camera_move_info()["fast"] is not True:
                raise SystemExit("call %d did not move in place: %r" % (k, pt.keep_mismatch()))
            if k >= 4:
                (t_flag if flagged else t_set).append(dt)
        # the registration alone: what pathtraceInit does in front of pt_init (pt_set_meshes, pt_set_textures, pt_set_bump_maps copy the scene's arrays)
        t_reg = []
        for k in range(N):
            t0 = time.perf_counter()
            pt.set_meshes(sc.meshes, sc.mesh_normals, sc.mesh_materials)
            pt.set_textures(sc.textures, sc.geom_textures, sc.mesh_uvs)
            pt.set_bump_maps(sc.geom_bumps, sc.bump_scales, sc.mesh_uvs)
            t_reg.append((time.perf_counter() - t0) * 1e3)
        pt.pathtraceFree()
    a, b = np.sort(t_flag), np.sort(t_set)
    spread = b[len(b) // 2] - b[0]
    print("%-20s %4dx%-4d batch %2d  pt_init with the flag (registration included) %s ms   same-scene form %s ms   the flag adds %7.3f ms "
          "(registering the scene again alone: %.3f) = %5.1f x the same-scene form's best-to-median spread of %.3f"
          % (scene, w, h, batch, _fmt(t_flag), _fmt(t_set), a[0] - b[0], min(t_reg), (a[0] - b[0]) / max(spread, 1e-9), spread))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "flag":
        flag(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
        return
    here = _host(ROOT, "keep_renderer_host")
    parent = _host(PARENT, "keep_renderer_host_parent", ["-DPT_PARENT_SHIM"]) if PARENT else None
    if len(sys.argv) > 1 and sys.argv[1] == "--build-only":
        return
    print("the camera move of a host on the reference's three symbols, one MI355X: wall ms of pathtraceFree(); pathtraceInit(scene);, best (median, worst) of %d" % N)
    if not parent:
        print("(PT_AMD_PARENT not set: no parent column)")
    sys.stdout.flush()
    protocol(here, parent)
    print("the full-argument pt_init with PT_FLAG_KEEP_RENDERER against pt_init's same-scene form, in turns in one process, best (median, worst) of %d" % (2 * ((N + 1) // 2)))
    for scene in SCENES:
        for w, h in FRAMES:
            for b in (8, 64):
                sys.stdout.flush()
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "flag", scene, str(w), str(h), str(b)], timeout=STEP_LIMIT,
                                   stderr=subprocess.PIPE, text=True)
                if r.returncode != 0:
                    sys.stderr.write(r.stderr[-4000:])
                    raise SystemExit("step flag %s %dx%d %d failed with status %d: the run ends here" % (scene, w, h, b, r.returncode))
    sys.stdout.flush()
    rate(here)


if __name__ == "__main__":
    main()
