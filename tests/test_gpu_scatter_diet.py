"""The scatter's candidacy of a binned cube on the device (k_bounce, class bit 3): the slab certificate evaluated from the reciprocals the
walls' block shares (the PLAIN forms) and standing alone, without the bounding ball beside it (every form that bins a cube).
tests/test_scatter_diet_cpu.py restates both on the CPU over the same rays.

(a) pt_test_slab_decisions over the 2^16 rays of tests/scatter_diet_rays.py: the evaluation from shared reciprocals (ptd::wallCertainMiss)
    and the one axis by axis (ptd::wallCertainMissByAxis) decide alike on every ray, and no ray the rule certifies -- slab and |o|_1 within
    the box's bound -- is hit by the device's full box test.  The device's box is the one tests/candidate_ref.py computes.
(b) Frames at 96x64, depth 8, 4 iterations of cornell.txt, cornell_glass.txt, a textured scene (tests/textured_scenes.py's `few`, every
    texel white: the textured forms, the untextured twin's frame) and a scene whose binned cube -- a small light near the world origin --
    lies beyond its certificate's bound for most origins (the guard fails: those scatters are candidates): each equal to the oracle's bit
    for bit, equal under PT_AMD_NO_TIGHT_CANDIDATES=1, and a batch equal to its single calls.  Every render is a process of its own.
(d) The tally on Cornell at 96x64, 8 iterations: the lanes of candidate tiles that hit a binned primitive are the ones of the ball's
    classes (none was classed away); the rule in force leaves at least the candidates that the ball beside it would ([6] >= [7]), and
    on Cornell far fewer than the ball alone ([6] < [5]).

There is no (c): the camera list that carries utilhash(pixel) beside each pixel word was built, tested the same way and counted; the
camera-ray launch issued MORE vector instructions with it, so the code and its tests were taken out (profiles/scatter_diet.txt, 4)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import candidate_ref as ref
import scatter_diet_rays as sdr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = "PT_AMD_NO_TIGHT_CANDIDATES"
W, H, DEPTH, ITERS = 96, 64, 8, 4

# (name, base scene file or "textured", {object index: (TRANS, ROTAT, SCALE)} to rewrite)
SCENES = [
    ("cornell", "cornell.txt", {}),
    ("glass", "cornell_glass.txt", {}),
    ("textured", "textured", {}),
    ("light beyond its bound", "cornell.txt", {0: ("0.02 0.5 0.03", "10 20 30", ".4 .4 .4")}),
]


@pytest.fixture(scope="module")
def gpu(pt):
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return pt


def _scene_file(tmp_path, base, edits):
    """the base scene's text with the named objects' TRANS / ROTAT / SCALE rewritten"""
    if base == "textured":
        return base
    src = os.path.join(ROOT, "scenes", base)
    if not edits:
        return src
    out, obj = [], None
    for line in open(src).read().splitlines():
        w = line.split()
        if w and w[0] == "OBJECT":
            obj = int(w[1])
        if w and obj in edits and w[0] in ("TRANS", "ROTAT", "SCALE"):
            line = "%s %s" % (w[0], edits[obj][("TRANS", "ROTAT", "SCALE").index(w[0])])
        out.append(line)
    path = str(tmp_path / "scene.txt")
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")
    return path


def _child(tmp_path, scene_path, w, h, iters, off):
    out = str(tmp_path / ("out_%d.npz" % int(off)))
    env = dict(os.environ)
    env.pop(SWITCH, None)
    if off:
        env[SWITCH] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "scatter_diet_child.py"), scene_path, str(w), str(h), str(DEPTH), str(iters), out],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(out)
    return z["batch"], z["single"], z["light"], z["cand"]


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32), np.ascontiguousarray(b, np.float32).reshape(-1).view(np.uint32))


def test_both_evaluations_decide_alike_and_the_rule_rejects_no_hit(gpu, oracle):
    total = 0
    for name, g, o, d in sdr.all_rays(oracle):
        flags, lo, hi, omax = gpu.test_slab_decisions(g.view(gpu.GEOM_DTYPE), o, d)
        rlo, rhi, romax = ref.wall_box(g[0])
        assert _same(lo, rlo) and _same(hi, rhi), (name, lo, rlo, hi, rhi)
        shared, by_axis, inside, hit = (flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0, (flags & 8) != 0
        rule = shared & inside
        print("%s: %d rays, bound %.4g (reference %.4g); slab certifies %d, within the bound %d, the rule %d; hits %d; disagreements %d, violations %d" % (
            name, len(flags), omax, romax, int(shared.sum()), int(inside.sum()), int(rule.sum()), int(hit.sum()),
            int((shared != by_axis).sum()), int((rule & hit).sum())))
        assert np.array_equal(shared, by_axis), (name, np.flatnonzero(shared != by_axis)[:8])
        assert not (rule & hit).any(), (name, np.flatnonzero(rule & hit)[:8])
        assert not ((by_axis & inside) & hit).any()
        assert rule.sum() > len(flags) // 20 and hit.sum() > len(flags) // 20
        # the CPU restatement takes the correctly rounded reciprocal for v_rcp_f32 (one ulp): decisions may differ on a handful of grazes, no more
        with np.errstate(all="ignore"):
            cpu = sdr.slab_shared(rlo, rhi, o, (np.float32(1) / d).astype(np.float32))
        print("   the numpy restatement decides otherwise on %d rays" % int((cpu != shared).sum()))
        total += len(flags)
    assert total == sdr.N_RAYS


@pytest.mark.parametrize("name,base,edits", SCENES, ids=[s[0].replace(" ", "_") for s in SCENES])
def test_frames_equal_the_oracle_the_ball_classes_and_their_single_calls(gpu, oracle, tmp_path, name, base, edits):
    path = _scene_file(tmp_path, base, edits)
    on = _child(tmp_path, path, W, H, ITERS, False)
    off = _child(tmp_path, path, W, H, ITERS, True)
    if base == "textured":
        import scatter_diet_child as child
        sc = child.white_textured_scene(gpu, oracle, W, H)
    else:
        sc = gpu.Scene(path)
        sc.set_resolution(W, H)
    want = np.zeros(W * H * 3, np.float32)
    orc = oracle.Renderer(sc.camera.view(oracle.CAMERA_DTYPE), sc.geoms.view(oracle.GEOM_DTYPE), sc.materials.view(oracle.MATERIAL_DTYPE), DEPTH)
    for it in range(1, ITERS + 1):
        orc.iterate(it, want)
    c = on[3]
    print("%s: scatters %d, candidates by the ball alone %d, by the rule in force %d, by the ball beside it %d (ball classes: %d); candidate tiles %d of %d" % (
        name, c[4], c[5], c[6], c[7], off[3][6], c[1], c[0]))
    assert want.max() > 0
    assert _same(on[0], want)                                       # the batch against the oracle
    assert _same(off[0], want)                                      # ... under the switch
    assert _same(on[1], on[0]) and _same(off[1], off[0])            # single calls against their batch
    assert on[2][0] == off[2][0] == on[2][1] == off[2][1]           # light hits
    assert c[7] <= c[6] and c[7] <= c[5]                            # the candidates only grow against the ball beside the rule
    assert off[3][7] == off[3][6] == off[3][5]


def test_the_light_beyond_its_bound_leaves_every_far_scatter_a_candidate(gpu, tmp_path):
    # the guard fails wherever |o|_1 exceeds the bound (5 S - big of pt_init's wall_box, a few units for this cube; the room's origins reach 20): the slab certifies nothing there and,
    # with no ball beside it, those scatters are candidates -- more than the ball alone would leave
    name, base, edits = SCENES[3]
    c = _child(tmp_path, _scene_file(tmp_path, base, edits), W, H, ITERS, False)[3]
    print("%s: scatters %d, candidates by the ball alone %d, by the rule in force %d, by the ball beside it %d" % (name, c[4], c[5], c[6], c[7]))
    assert c[4] > 0 and c[6] > c[5] >= c[7]


def test_no_binned_hit_is_classed_away_and_the_candidates_only_grow(gpu, tmp_path):
    path = os.path.join(ROOT, "scenes", "cornell.txt")
    on = _child(tmp_path, path, W, H, 8, False)[3]
    off = _child(tmp_path, path, W, H, 8, True)[3]
    print("cornell %dx%d, 8 iterations: candidate tiles %d of %d (ball classes %d of %d); scatters %d, candidates by the ball alone %d, by the rule in force %d, "
          "by the ball beside it %d; lanes of candidate tiles that hit a binned primitive %d / %d" % (
              W, H, on[1], on[0], off[1], off[0], on[4], on[5], on[6], on[7], on[3], off[3]))
    assert on[4] == off[4] > 0 and on[5] == off[5]                  # the same paths are scattered in both arms
    assert on[3] == off[3] > 0                                      # every lane that hit a binned primitive sat in a candidate tile
    assert on[7] <= on[6] < on[5]                                   # the rule leaves at least the parent rule's candidates, and far fewer than the ball
    assert off[7] == off[6] == off[5]
