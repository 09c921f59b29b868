"""The study of tests/test_spatial_var_cpu.py -- which PT_SPATIAL_RADIUS, and why the estimate is used below two samples only -- repeated at
product resolution, 1280x720, where five filter levels no longer span the image: Cornell, depth 8, rendered on the GPU (one, two and three
samples and the mean of iterations 1 .. 2048 as the converged reference, the GPU's own), and the checkerboard of the CPU study at that size.
The frames are filtered by the numpy restatements (tests/spatial_var_ref.py, denoise_var_ref.py, denoise_ref.py: bit for bit what the
kernels compute, which is what tests/test_gpu_spatial_var.py holds them to) because the product instantiates the shipped radius only.

    python profiles/spatial_var_study.py                    render and filter
    python profiles/spatial_var_study.py --dump FILE.npz    render only: the accumulators, the reference and the guides, compressed
    python profiles/spatial_var_study.py --load FILE.npz    filter only (needs no GPU)

Prints profiles/spatial_var_study.txt.  Stops at the first failure (an exception ends it); nothing is retried."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
W, H, CONVERGED = 1280, 720, 2048
F = np.float32
LEVELS, SIGMA_LUM, SIGMA_NORMAL, SIGMA_POSITION = 5, 4.0, 0.35, 2.0
PLAIN = (2.0, 0.35, 2.0)
RADII = (1, 2, 3)


def render():
    import temporal_ref as tr
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pt = ge.load_package()
    if pt.device_count() < 1:
        raise SystemExit("no HIP device")
    sc = pt.Scene(os.path.join(ROOT, "scenes", "cornell.txt"))
    sc.set_resolution(W, H)
    out = {}
    try:
        pt.pathtraceFree()
        pt.pathtraceInit(sc, traceDepth=8, max_batch=16, moments=True)
        for n in (1, 2, 3):
            pt.pathtrace_batch(None, 0, n, 1)
            out["S%d" % n] = pt.readback(W * H).reshape(H, W, 3).copy()
            out["Q%d" % n] = pt.readback_moments().reshape(H, W).copy()
        for first in range(4, CONVERGED + 1, 16):
            pt.pathtrace_batch(None, 0, first, min(16, CONVERGED + 1 - first))
        out["ref"] = (pt.readback(W * H).reshape(H, W, 3) / F(CONVERGED)).astype(F)
        out["pos_t"], out["nrm_id"] = tr.pack_guides(*pt.gbuffer(1), H, W)
    finally:
        pt.pathtraceFree()
    return out


def _rmse(a, ref):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - ref) ** 2)))


def rows(name, sums, ref, pos_t, nrm_id):
    """sums: {n: (S, Q)} for n = 1, 2, 3"""
    import denoise_ref as dr
    import denoise_var_ref as dv
    import spatial_var_ref as sv
    pos, nrm = pos_t[..., :3], nrm_id[..., :3]
    geom = np.ascontiguousarray(nrm_id[..., 3]).view(np.int32)
    ref = ref.astype(np.float64)
    lines, one = [], {}
    for n in (1, 2, 3):
        S, Q = sums[n]
        raw = _rmse(S / F(n), ref)
        plain = _rmse(dr.denoise(S, n, pos, nrm, geom, LEVELS, *PLAIN), ref)
        today = "refused" if n < 2 else "%.4f " % _rmse(dv.denoise_var(S, Q, n, pos, nrm, geom, LEVELS, SIGMA_LUM, SIGMA_NORMAL, SIGMA_POSITION)[0], ref)
        sp = {r: _rmse(sv.denoise_var_spatial(S, Q, n, pos_t, nrm_id, LEVELS, SIGMA_LUM, SIGMA_NORMAL, SIGMA_POSITION, radius=r, min_count=np.inf)[0], ref)
              for r in RADII}
        lines.append("%-8s %d   %.4f      %.4f      %s   %.4f   %.4f   %.4f" % (name, n, raw, plain, today, sp[1], sp[2], sp[3]))
        if n == 1:
            one = dict(sp, raw=raw, plain=plain)
            M, N = sv.moments_form(S, Q, 1)
            lref = (0.2126 * ref[..., 0] + 0.7152 * ref[..., 1]) + 0.0722 * ref[..., 2]
            mse = float(((dv.lum(S).astype(np.float64) - lref) ** 2).mean())
            cal = [float(sv.spatial_variance(M, N, pos, nrm, geom, r, SIGMA_NORMAL, SIGMA_POSITION)[1].astype(np.float64).mean()) / mse for r in RADII]
        print(lines[-1], file=sys.stderr, flush=True)
    lines.append("%-8s n = 1: mean estimated variance / mean squared luminance error of the one-sample frame: 3x3 %.3f  5x5 %.3f  7x7 %.3f" % ((name,) + tuple(cal)))
    return lines, one


def checkerboard():
    import denoise_var_ref as dv
    import temporal_ref as tr
    yy, xx = np.mgrid[0:H, 0:W]
    a = np.where(((xx // 8) + (yy // 8)) % 2 == 0, 0.25, 0.75)
    albedo = np.stack([a, a / 2, 1 - a], axis=2).astype(F)
    rng = np.random.default_rng(7)
    samples = [albedo * rng.uniform(0, 2, (H, W, 1)).astype(F) for _ in range(3)]
    pos_t = np.stack([xx * 0.05, yy * 0.05, np.zeros((H, W)), np.ones((H, W))], axis=2).astype(F)
    nrm = np.broadcast_to(np.array([0, 0, 1], F), (H, W, 3)).copy()
    pos_t, nrm_id = tr.pack_guides(pos_t, nrm, np.zeros((H, W), np.int32), H, W)
    sums, S = {}, np.zeros((H, W, 3), F)
    for n in (1, 2, 3):
        S = S + samples[n - 1]
        sums[n] = (S, dv.moments(samples[:n]))
    return sums, albedo, pos_t, nrm_id


if __name__ == "__main__":
    if "--load" in sys.argv:
        z = np.load(sys.argv[sys.argv.index("--load") + 1])
        data = {k: z[k] for k in z.files}
    else:
        data = render()
    if "--dump" in sys.argv:
        np.savez_compressed(sys.argv[sys.argv.index("--dump") + 1], **data)
        raise SystemExit(0)
    shipped = int(__import__("re").search(r"#define PT_SPATIAL_RADIUS ([0-9]+)", open(os.path.join(ROOT, "include", "pt_amd.h")).read()).group(1))
    out = ["%dx%d; Cornell: depth 8, the GPU's iterations 1, 2, 3 against the mean of its iterations 1 .. %d; checker: 8-pixel cells against the albedo." % (W, H, CONVERGED),
           "Frame RMSE; the shipped setting (%d levels, sigma_lum %g, sigma_normal %g, sigma_position %g), pt_denoise at (%g, %g, %g); the spatial columns"
           % ((LEVELS, SIGMA_LUM, SIGMA_NORMAL, SIGMA_POSITION) + PLAIN),
           "force the estimate on for every pixel (at n = 2, 3 against the pixel's own variance: `today`).",
           "scene    n   unfiltered  pt_denoise  today     3x3      5x5      7x7"]
    sums = {n: (data["S%d" % n], data["Q%d" % n]) for n in (1, 2, 3)}
    lines, cornell = rows("Cornell", sums, data["ref"], data["pos_t"], data["nrm_id"])
    out += lines
    csums, albedo, cpos, cnrm = checkerboard()
    lines, checker = rows("checker", csums, albedo, cpos, cnrm)
    out += lines
    eligible = [r for r in RADII if all(o[r] < o["raw"] and o[r] < o["plain"] for o in (cornell, checker))]
    best = min(eligible, key=lambda r: cornell[r]) if eligible else None
    out.append("The rule (the lowest Cornell RMSE among the radii that beat the unfiltered frame and pt_denoise on both scenes at n = 1): eligible %s, radius %s"
               % (eligible, best))
    out.append("here; the CPU study at 64x48, which is the reproducible one and decides, ships radius %d: %s." % (shipped, "they agree" if best == shipped else "THEY DISAGREE"))
    print("\n".join(out), flush=True)
