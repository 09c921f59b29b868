"""Albedo demodulation (PT_FLAG_DEMODULATE) on the GPU's own frames of a textured scene at product resolution: scenes/cornell_textured.txt at
1280x720, depth 8, pt_denoise_var with the shipped setting at 1, 2, 4, 16 and 64 samples (one sample: under PT_FLAG_SPATIAL_VARIANCE) of a
flagged and of an unflagged renderer -- the same iterations, so the same accumulators, bit for bit -- against the mean of the GPU's iterations
1 .. 2048.  The filtering is the device's (tests/test_gpu_demod.py holds it to the numpy restatement bit for bit).

    python profiles/demod_study.py [SCENE]

Prints profiles/demod_study.txt.  Stops at the first failure (an exception ends it); nothing is retried."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, CONVERGED, BATCH = 1280, 720, 2048, 64
COUNTS = (1, 2, 4, 16, 64)
F = np.float32


def _rmse(a, ref):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - ref) ** 2)))


def render(pt, sc, flagged, converge):
    out = {}
    pt.pathtraceFree()
    pt.pathtraceInit(sc, traceDepth=8, max_batch=BATCH, moments=True, spatial_variance=True, demodulate=flagged)
    done = 0
    for n in COUNTS:
        pt.pathtrace_batch(None, 0, done + 1, n - done)
        done = n
        out[n] = pt.denoise_var(n).reshape(H, W, 3).copy()
        out["raw%d" % n] = (pt.readback(W * H).reshape(H, W, 3) / F(n)).astype(F)
    if converge:
        while done < CONVERGED:
            k = min(BATCH, CONVERGED - done)
            pt.pathtrace_batch(None, 0, done + 1, k)
            done += k
        out["ref"] = (pt.readback(W * H).reshape(H, W, 3) / F(CONVERGED)).astype(np.float64)
        out["geom"] = pt.gbuffer(1)[2].reshape(H, W).copy()
    pt.pathtraceFree()
    return out


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pt = ge.load_package()
    if pt.device_count() < 1:
        raise SystemExit("no HIP device")
    name = sys.argv[1] if len(sys.argv) > 1 else "cornell_textured.txt"
    sc = pt.Scene(os.path.join(ROOT, "scenes", name))
    sc.set_resolution(W, H)
    off = render(pt, sc, False, True)
    on = render(pt, sc, True, False)
    ref = off["ref"]
    tex = np.isin(off["geom"], np.flatnonzero(np.asarray(sc.geom_textures) >= 0))
    print("%s at %dx%d, depth 8: pt_denoise_var (%d levels, sigma_lum %g, sigma_normal %g, sigma_position %g) of the GPU's first n iterations against the"
          % (name, W, H, pt.PT_DISPLAY_LEVELS, pt.PT_DISPLAY_SIGMA_LUM, pt.PT_DISPLAY_SIGMA_NORMAL, pt.PT_DISPLAY_SIGMA_POSITION))
    print("mean of its iterations 1 .. %d; n = 1 under PT_FLAG_SPATIAL_VARIANCE.  RMSE over the frame, and over the %.1f %% of its pixels whose first hit"
          % (CONVERGED, 100.0 * tex.mean()))
    print("(iteration 1) is a textured primitive.  The unfiltered frames of the two renderers are identical: %s."
          % all(np.array_equal(off["raw%d" % n], on["raw%d" % n]) for n in COUNTS))
    print("   n   unfiltered  guided   demodulated  ratio  | textured: unfiltered  guided   demodulated  ratio")
    for n in COUNTS:
        r = [_rmse(x, ref) for x in (off["raw%d" % n], off[n], on[n])]
        t = [_rmse(x[tex], ref[tex]) for x in (off["raw%d" % n], off[n], on[n])]
        print("  %2d   %.4f      %.4f   %.4f       %.3f  |           %.4f      %.4f   %.4f       %.3f" % (n, r[0], r[1], r[2], r[2] / r[1], t[0], t[1], t[2], t[2] / t[1]),
              flush=True)
