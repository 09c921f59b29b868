"""What the second moments and the variance-guided filter cost on one MI355X, Cornell, against their yardsticks from the same build: each
level of each form of k_atrous_*<AtrousGuided> against the plain filter's same level and the five levels as the library launches them (HIP events:
pt_test_denoise_var / pt_test_denoise, the two alternating; at 1280x720 and once more at 1920x1080, so that the tiled / gather thresholds
do not rest on one frame size), the iteration rate of a renderer with PT_FLAG_MOMENTS against one without (1280x720; HIP events on the
caller's stream around batches of 1 and of 32, the two alternating), and the commit kernels themselves -- k_commit_one / k_commit, <false>
and <true> -- from a run of their own under rocprofv3 --kernel-trace --stats (skipped, and said so, where rocprofv3 is missing).  Writes
profiles/denoise_var_cost.txt.

    python profiles/denoise_var_cost.py        # each measurement runs in a child process under its own timeout

A child stops at the first failure (an exception ends it); nothing is retried."""
import csv
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, LEVELS, REPS, SAMPLES = 1280, 720, 5, 7, 72
HBM_PEAK_GBS = 8000.0          # bench.py: HBM_PEAK_GBS
FORMS = [(1, "gather"), (2, "tiled 64x4"), (3, "tiled 64x8")]
FILTER_FRAMES = [(1280, 720), (1920, 1080)]
RATE_ROUNDS, RATE_ITERS = 4, {1: 640, 32: 1920}


def thresholds():
    """(kAtrousTiledMaxStep, kAtrousVarTiledMaxStep) of this tree's csrc/pt_denoise.h: the largest step each filter's product path tiles"""
    src = open(os.path.join(ROOT, "project3-cuda-path-tracer_amd", "csrc", "pt_denoise.h")).read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % n, src).group(1)) for n in ("kAtrousTiledMaxStep", "kAtrousVarTiledMaxStep"))


def _package(w=W, h=H):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pt = ge.load_package()
    if pt.device_count() < 1:
        raise SystemExit("no HIP device")
    sc = pt.Scene(os.path.join(ROOT, "scenes", "cornell.txt"))
    sc.set_resolution(w, h)
    return pt, sc


def _render(pt, batch, first, iters):
    for b in range(iters // batch):
        if batch == 1:
            pt.pathtrace(None, 0, first + b, readback=False)
        else:
            pt.pathtrace_batch(None, 0, first + b * batch, batch)
    return first + iters


def child_filter(out_path):
    lines = []
    for w, h in FILTER_FRAMES:
        lines += filter_frame(w, h) + [""]
    return lines[:-1]


def filter_frame(w, h):
    import numpy as np
    pt, sc = _package(w, h)
    lines = []
    with pt.renderer_from_test_library():
        pt.pathtraceInit(sc, max_batch=8, moments=True)
        _render(pt, 8, 1, SAMPLES)
        pt.sync()
        plain, var, auto_p, auto_v = {}, {}, [], []
        for form, _ in [(0, "")] + FORMS:               # warm-up: every kernel of every form once, guides cached
            pt.test_denoise(SAMPLES, form, LEVELS)
            pt.test_denoise_var(SAMPLES, form, LEVELS)
        for rep in range(REPS):
            for form, _ in FORMS:
                _, ms = pt.test_denoise(SAMPLES, form, LEVELS, timing=True)
                plain.setdefault(form, []).append(ms[1:].copy())
                _, _, ms = pt.test_denoise_var(SAMPLES, form, LEVELS, timing=True)
                var.setdefault(form, []).append(ms[1:].copy())
            _, ms = pt.test_denoise(SAMPLES, 0, LEVELS, timing=True)            # ... and the five levels as the library launches them
            auto_p.append(float(ms[1:].sum()))
            _, _, ms = pt.test_denoise_var(SAMPLES, 0, LEVELS, timing=True)
            auto_v.append(float(ms[1:].sum()))
        ref = None
        for form, name in [(0, "the product's choice")] + FORMS:      # ... and every form gives the same bits
            out = pt.test_denoise_var(SAMPLES, form, LEVELS)
            ref = ref or out
            if not all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(ref, out)):
                raise SystemExit("form %s differs" % name)
        pt.pathtraceFree()
    floor_ms = w * h * 64 / (HBM_PEAK_GBS * 1e9) * 1e3
    lines.append("Variance-guided filter against the plain one, one MI355X, %dx%d after %d Cornell iterations, depth 8; HIP events per level," % (w, h, SAMPLES))
    lines.append("the two filters alternating, %d runs per form: best (median).  A level of either moves 64 B per pixel = %.1f MB: %.4f ms at %.0f GB/s." % (
        REPS, w * h * 64 / 1e6, floor_ms, HBM_PEAK_GBS))
    lines.append("")
    lines.append("ms per level           form          plain best (median)   guided best (median)   guided / plain   guided x HBM floor")
    for i in range(LEVELS):
        for form, name in FORMS:
            p = np.array([m[i] for m in plain[form]], np.float64)
            v = np.array([m[i] for m in var[form]], np.float64)
            lines.append("  level %d (step %2d)    %-12s  %.4f (%.4f)       %.4f (%.4f)        %.2f             %.1f" % (
                i, 1 << i, name, p.min(), np.median(p), v.min(), np.median(v), v.min() / p.min(), v.min() / floor_ms))
    tp, tv = thresholds()
    lines.append("")
    lines.append("five levels as the library launches them, timed as one sequence, best (median) of %d:" % REPS)
    lines.append("  plain   (tiled 64x8 up to step %d -- kAtrousTiledMaxStep --, the gather above):     %.4f (%.4f) ms" % (tp, min(auto_p), float(np.median(auto_p))))
    lines.append("  guided  (tiled 64x8 up to step %d -- kAtrousVarTiledMaxStep --, the gather above):  %.4f (%.4f) ms" % (tv, min(auto_v), float(np.median(auto_v))))
    return lines


def child_rate(out_path):
    import torch
    pt, sc = _package()
    lines = ["Iteration rate with and without PT_FLAG_MOMENTS, same build, Cornell %dx%d depth 8; HIP events on the caller's stream around the calls," % (W, H),
             "the two renderers alternating, %d windows each: ms per iteration, best (median)." % RATE_ROUNDS]
    import numpy as np
    for batch in (1, 32):
        ms = {False: [], True: []}
        for rnd in range(RATE_ROUNDS):
            for flag in (False, True):
                pt.pathtraceFree()
                pt.pathtraceInit(sc, max_batch=batch, moments=flag)
                nxt = _render(pt, batch, 1, 2 * batch if batch > 1 else 16)       # warm-up
                pt.sync()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _render(pt, batch, nxt, RATE_ITERS[batch])
                e1.record()
                e1.synchronize()
                pt.sync()
                ms[flag].append(e0.elapsed_time(e1) / RATE_ITERS[batch])
        a, b = np.array(ms[False]), np.array(ms[True])
        lines.append("  batches of %-2d (%d iterations per window):  without %.5f (%.5f)   with %.5f (%.5f)   with / without %.3f (medians %.3f)" % (
            batch, RATE_ITERS[batch], a.min(), np.median(a), b.min(), np.median(b), b.min() / a.min(), np.median(b) / np.median(a)))
    pt.pathtraceFree()
    return lines


def child_commit(out_path):
    """the work rocprofv3 traces: both renderers, batches of 1 (k_commit_one) and of 32 (k_commit)"""
    pt, sc = _package()
    for batch in (1, 32):
        for flag in (False, True):
            pt.pathtraceFree()
            pt.pathtraceInit(sc, max_batch=batch, moments=flag, pipeline_depth=1)
            _render(pt, batch, 1, 8 * batch if batch > 1 else 64)
            pt.sync()
    pt.pathtraceFree()
    return []


def commit_rows(trace_dir):
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True), key=os.path.getmtime)
    if not files:
        return ["  (rocprofv3 wrote no kernel_stats.csv)"]
    rows = []
    for r in csv.DictReader(open(files[-1])):
        name = r.get("Name") or r.get("KernelName") or ""
        if "k_commit" not in name:
            continue
        calls = r.get("Calls", "?")
        avg = float(r.get("AverageNs") or r.get("Average") or 0) / 1e3
        mn = float(r.get("MinNs") or r.get("Min") or 0) / 1e3
        mx = float(r.get("MaxNs") or r.get("Max") or 0) / 1e3
        rows.append("  %-44s calls %-5s  us: average %.2f  min %.2f  max %.2f" % (name.split("(")[0][:44], calls, avg, mn, mx))
    return sorted(rows) or ["  (no k_commit row in %s)" % os.path.basename(files[-1])]


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--child":
        lines = {"filter": child_filter, "rate": child_rate, "commit": child_commit}[sys.argv[2]](sys.argv[3])
        with open(sys.argv[3], "w") as f:
            f.write("\n".join(lines) + "\n")
        sys.exit(0)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "denoise_var_cost.txt")
    me = os.path.abspath(__file__)
    text = []
    with tempfile.TemporaryDirectory() as tmp:
        for part in ("filter", "rate"):
            piece = os.path.join(tmp, part + ".txt")
            r = subprocess.run([sys.executable, me, "--child", part, piece], timeout=240)
            if r.returncode:
                sys.exit(r.returncode)
            text += open(piece).read().splitlines() + [""]
        text.append("The commit kernels, rocprofv3 --kernel-trace --stats over a run of their own (one batch in flight; 64 calls of one iteration, 8 batches of 32):")
        text.append("<false> is the kernel every renderer launched before the flag existed (same ISA), <true> also reads and writes 4 B of moments per lit pixel")
        text.append("and squares each entry's luminance.")
        prof = shutil.which("rocprofv3")
        if not prof:
            text.append("  not measured: rocprofv3 is not on the PATH")
        else:
            trace = os.path.join(tmp, "trace")
            r = subprocess.run([prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace, "--", sys.executable, me, "--child", "commit",
                                os.path.join(tmp, "commit.txt")], timeout=240, stdout=subprocess.DEVNULL)
            if r.returncode:
                sys.exit(r.returncode)
            text += commit_rows(trace)
    body = "\n".join(text) + "\n"
    sys.stdout.write(body)
    with open(out, "w") as f:
        f.write(body)
