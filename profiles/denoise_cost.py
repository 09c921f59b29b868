"""What the denoiser costs on one MI355X: k_gbuffer once and each of five k_atrous levels at 1280x720 after 8 Cornell iterations, by HIP
events (pt_test_denoise), for the plain gather and the two LDS-tiled forms of every level; against the bytes a level must move (64 B per
pixel: three 16-byte streams in, one out) at the HBM rate bench.py prices its roofline with, and against a Cornell iteration of the same
frame.  Writes profiles/denoise_cost.txt.

    python profiles/denoise_cost.py            # the measurement runs in a child process under its own timeout

The child stops at the first failure (an exception ends it); nothing is retried."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, LEVELS, REPS = 1280, 720, 5, 5
HBM_PEAK_GBS = 8000.0          # bench.py: HBM_PEAK_GBS
FORMS = [(1, "gather"), (2, "tiled 64x4"), (3, "tiled 64x8")]


def child(out_path):
    sys.path.insert(0, ROOT)
    import numpy as np
    import __graft_entry__ as ge
    pt = ge.load_package()
    if pt.device_count() < 1:
        raise SystemExit("no HIP device")
    sc = pt.Scene(os.path.join(ROOT, "scenes", "cornell.txt"))
    sc.set_resolution(W, H)
    lines = []
    with pt.renderer_from_test_library():
        pt.pathtraceInit(sc, max_batch=8)
        pt.pathtrace_batch(None, 0, 1, 8)
        pt.sync()
        t0 = time.perf_counter()                       # a Cornell iteration of this frame: 64 more, 8 per batch
        for b in range(8):
            pt.pathtrace_batch(None, 0, 9 + 8 * b, 8)
        pt.sync()
        iter_ms = (time.perf_counter() - t0) * 1e3 / 64
        ms_g = []
        best = {}
        ref = None
        for rep in range(REPS):
            for form, name in FORMS:
                out, ms = pt.test_denoise(72, form, LEVELS, guide_iter=1 + rep * len(FORMS) + form, timing=True)   # a fresh guide_iter: k_gbuffer runs
                ms_g.append(float(ms[0]))
                best[form] = np.minimum(best.get(form, np.full(LEVELS, np.inf)), ms[1:])
        for form, name in FORMS:                        # ... and every form gives the same bits
            out = pt.test_denoise(72, form, LEVELS, guide_iter=1)
            if ref is None:
                ref = out
            if not np.array_equal(ref.view(np.uint32), out.view(np.uint32)):
                raise SystemExit("form %s differs from the gather" % name)
        auto, ms_auto = pt.test_denoise(72, 0, LEVELS, guide_iter=1, timing=True)
        if not np.array_equal(ref.view(np.uint32), auto.view(np.uint32)):
            raise SystemExit("the product's choice differs from the gather")
        pt.pathtraceFree()
    floor_ms = W * H * 64 / (HBM_PEAK_GBS * 1e9) * 1e3
    lines.append("Denoiser cost, one MI355X, %dx%d after 8 (+64 timed) Cornell iterations, depth 8; HIP events, best of %d runs per form." % (W, H, REPS))
    lines.append("A level must move 64 B per pixel = %.1f MB: %.4f ms at the %.0f GB/s of HBM bench.py --full prices its roofline with." % (W * H * 64 / 1e6, floor_ms, HBM_PEAK_GBS))
    lines.append("")
    lines.append("k_gbuffer (8 primitives, brute force): %.4f ms (best of %d; worst %.4f)" % (min(ms_g), len(ms_g), max(ms_g)))
    lines.append("")
    lines.append("k_atrous, ms per level        " + "".join("%-14s" % n for _, n in FORMS) + "fastest       x HBM floor")
    total = 0.0
    for i in range(LEVELS):
        row = [float(best[f][i]) for f, _ in FORMS]
        k = int(np.argmin(row))
        total += row[k]
        lines.append("  level %d (step %2d)           " % (i, 1 << i) + "".join("%-14.4f" % v for v in row) + "%-14s%.1f" % (FORMS[k][1], row[k] / floor_ms))
    lines.append("(level 0's gather forms the mean, sum / samples, again for each of its 24 neighbour taps -- 72 divisions per pixel the tiled forms do once per")
    lines.append(" staged entry: its level-0 time is biased against it; from level 1 on every form reads the same float4 colours.)")
    lines.append("")
    lines.append("five levels, fastest form each: %.4f ms; as pt_denoise launches them (its choice per level): %.4f ms" % (total, float(ms_auto[1:].sum())))
    lines.append("one Cornell iteration of this frame (64 iterations, 8 per batch, wall): %.4f ms" % iter_ms)
    lines.append("k_gbuffer + five levels = %.4f ms = %.2f Cornell iterations" % (min(ms_g) + float(ms_auto[1:].sum()), (min(ms_g) + float(ms_auto[1:].sum())) / iter_ms))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "denoise_cost.txt")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], timeout=240)
        sys.exit(r.returncode)
