"""What the noise statistics and the render-until loop cost on one MI355X, against their yardsticks from the same build:
  (a) k_noise_stats against k_variance over the same arrays -- both read 16 B per pixel; k_variance writes 4 B per pixel, k_noise_stats one
      float per 256 -- at 1280x720 and 1920x1080 (HIP events round each kernel, the two alternating: pt_test_noise_stats), and both against
      16 B per pixel at the 8 TB/s the roofline is priced with;
  (b) pt_iterate_until with a threshold out of reach against the plain pt_iterate_batch loop, Cornell 1280x720, batches of 32, a check every 32
      iterations, 512 iterations (HIP events on the caller's stream round the calls, the three loops alternating): lookahead 1 should cost
      nothing, lookahead 0 drains the GPU at every check.
Writes profiles/noise_cost.txt.

    python profiles/noise_cost.py        # each measurement runs in a child process under its own timeout

A child stops at the first failure (an exception ends it); nothing is retried."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK_GBS = 8000.0          # bench.py: HBM_PEAK_GBS
KERNEL_FRAMES = [(1280, 720), (1920, 1080)]
KERNEL_REPS, KERNEL_ROUNDS = 20, 3
TILES_PER_WAVE, LIBRARY_TPW = (1, 2, 4), 2          # csrc/pt_noise.h: kNoiseTilesPerWave
W, H, BATCH, EVERY, CAP, ROUNDS = 1280, 720, 32, 32, 512, 4


def _package():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pt = ge.load_package()
    if pt.device_count() < 1:
        raise SystemExit("no HIP device")
    return pt


def child_kernel(out_path):
    import numpy as np
    pt = _package()
    lines = ["k_noise_stats against k_variance over the same arrays, one MI355X; HIP events round each kernel, the two alternating, %d rounds of %d"
             % (KERNEL_ROUNDS, KERNEL_REPS),
             "pairs: us, best (median) [worst].  Both read 16 B per pixel (S 12, Q 4); k_variance also writes 4 B per pixel.  All tiles flagged: every",
             "workgroup issues both its atomics.", ""]
    rng = np.random.default_rng(1)
    for w, h in KERNEL_FRAMES:
        S = rng.uniform(0, 64, (h, w, 3)).astype(np.float32)
        Q = rng.uniform(0, 400, (h, w)).astype(np.float32)
        floor_us = w * h * 16 / (HBM_PEAK_GBS * 1e9) * 1e6
        lines.append("  %dx%d (%.1f MB read, %.2f us at %.0f GB/s):" % (w, h, w * h * 16 / 1e6, floor_us, HBM_PEAK_GBS))
        for tpw in TILES_PER_WAVE:
            ms = []
            for _ in range(KERNEL_ROUNDS):
                _, m = pt.test_noise_stats(S, Q, w, h, 16, 0.5, tiles_per_wave=tpw, timing_reps=KERNEL_REPS)
                ms.append(m)
            ms = np.concatenate(ms).astype(np.float64) * 1e3
            a, b = ms[:, 0], ms[:, 1]
            lines.append("    k_noise_stats, %d tile(s) per wave%s  %.2f (%.2f) [%.2f]   x HBM floor %.1f   / k_variance: best %.3f, medians %.3f" % (
                tpw, " (the library's)" if tpw == LIBRARY_TPW else "                ", a.min(), np.median(a), a.max(), a.min() / floor_us,
                a.min() / b.min(), np.median(a) / np.median(b)))
            lines.append("    k_variance beside it                            %.2f (%.2f) [%.2f]   x HBM floor %.1f" % (b.min(), np.median(b), b.max(),
                                                                                                                       b.min() / floor_us))
    return lines


def child_loop(out_path):
    import numpy as np
    import torch
    pt = _package()
    sc = pt.Scene(os.path.join(ROOT, "scenes", "cornell.txt"))
    sc.set_resolution(W, H)
    kinds = ["pt_iterate_batch", "pt_iterate_until lookahead 1", "pt_iterate_until lookahead 0"]
    ms = {k: [] for k in kinds}
    frames = {}
    for rnd in range(ROUNDS):
        for kind in kinds:
            pt.pathtraceFree()
            pt.pathtraceInit(sc, max_batch=BATCH, moments=True)
            for b in range(2):                                          # warm-up
                pt.pathtrace_batch(None, 0, 1 + b * BATCH, BATCH)
            pt.sync()
            first = 2 * BATCH + 1
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if kind == "pt_iterate_batch":
                for b in range(CAP // BATCH):
                    pt.pathtrace_batch(None, 0, first + b * BATCH, BATCH)
            else:
                st, done = pt.iterate_until(first, 1e-4, first + CAP - 1, check_every=EVERY, lookahead=int(kind[-1]))
                if done != first + CAP - 1 or st["converged"]:
                    raise SystemExit("%s stopped at %d" % (kind, done))
            e1.record()
            e1.synchronize()
            pt.sync()
            ms[kind].append(e0.elapsed_time(e1) / CAP)
            if rnd == 0:
                frames[kind] = (pt.readback(W * H), pt.readback_moments())
    pt.pathtraceFree()
    for kind in kinds[1:]:
        if not all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(frames[kinds[0]], frames[kind])):
            raise SystemExit("%s: another frame than the plain loop's" % kind)
    lines = ["The render-until loop against the plain loop, same build, Cornell %dx%d depth 8 with PT_FLAG_MOMENTS, batches of %d, a check every %d"
             % (W, H, BATCH, EVERY),
             "iterations, %d iterations with a threshold out of reach (%d checks); HIP events on the caller's stream round the calls, the three loops"
             % (CAP, CAP // EVERY),
             "alternating, %d windows each: ms per iteration, best (median) [worst].  The three leave the same accumulators, bit for bit." % ROUNDS]
    base = np.array(ms[kinds[0]])
    for kind in kinds:
        a = np.array(ms[kind])
        lines.append("  %-30s %.5f (%.5f) [%.5f]   / plain: best %.4f, medians %.4f" % (kind, a.min(), np.median(a), a.max(), a.min() / base.min(),
                                                                                        np.median(a) / np.median(base)))
    lines.append("  the plain loop's own spread, worst / best: %.4f" % (base.max() / base.min()))
    return lines


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--child":
        lines = {"kernel": child_kernel, "loop": child_loop}[sys.argv[2]](sys.argv[3])
        with open(sys.argv[3], "w") as f:
            f.write("\n".join(lines) + "\n")
        sys.exit(0)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "noise_cost.txt")
    me = os.path.abspath(__file__)
    text = []
    with tempfile.TemporaryDirectory() as tmp:
        for part in ("kernel", "loop"):
            piece = os.path.join(tmp, part + ".txt")
            r = subprocess.run([sys.executable, me, "--child", part, piece], timeout=240)
            if r.returncode:
                sys.exit(r.returncode)
            text += open(piece).read().splitlines() + [""]
    body = "\n".join(text[:-1]) + "\n"
    sys.stdout.write(body)
    with open(out, "w") as f:
        f.write(body)
