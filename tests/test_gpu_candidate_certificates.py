"""The scatter's tighter candidacy on the device (k_bounce, class bit 3; KParams::binCull / binBox; tests/candidate_ref.py and
tests/test_candidate_certificates_cpu.py restate and check the certificates on the CPU).

Sweeps, 2^22 rays each: the slab certificate against wall_box's inflated world box, under its bound on the origin -- in both of its
evaluations, ptd::wallCertainMiss (the walls') and ptd::wallCertainMissByAxis (the one the scatter runs for a binned cube): a hit that
either certifies, or a ray on which they disagree, is a violation -- on cubes of the size that gets binned -- Cornell's light, a thin slab at a ceiling, a 100 : 1 plate, rotated and small ones -- and the
half-line certificate on binned-size spheres, in the packed sweep's form and in the scatter's own (ptd::certainMissClamped: the sweep
counts a violation of either): no ray that the full test hits is certified, and certificates are issued.

Frames at 96x64, depth 8, 4 iterations in one batch, of cornell.txt, cornell_glass.txt and three scenes written here -- a rotated small
emitting cube off the ceiling, a light in front of the back wall (wall and light distances compete), a sphere touching a wall: equal to
the oracle's bit for bit, and equal with PT_AMD_NO_TIGHT_CANDIDATES=1 (the classes of the bounding balls alone).  Every render is a process
of its own: the plan reads the switch from its environment.

The tally (pt_test_candidate_tally) on Cornell at 160x90, 8 iterations: with the switch the rule in force IS the ball's at every scatter
(the parent's classes); without it the share of candidate tiles is strictly lower, fewer scatters come out as candidates, and the lanes of
candidate tiles that hit a binned primitive are the same -- no hit was classed away.  The size of the drop is printed, not pinned
(profiles/candidate_tiles.txt records it at the benchmark's size).  PtCounters::misses is NOT compared between the arms: paths of the last
bounce that cannot reach an emitter are not traced and appear in no tally (include/pt_amd.h), and the tighter rule finds more of them.

Candidate one-wall tiles do NOT take the wall's certified face: built, swept and counted, it did not lower a later launch's vector
instructions and was left out (profiles/candidate_tiles.txt, 6), so it has no sweep here.  Tally [2] counts the tiles it would have served."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = "PT_AMD_NO_TIGHT_CANDIDATES"
W, H, DEPTH, ITERS = 96, 64, 8, 4
RAYS = 1 << 22

# (name, base scene file, {object index: (TRANS, ROTAT, SCALE)} to rewrite)
SCENES = [
    ("cornell", "cornell.txt", {}),
    ("glass", "cornell_glass.txt", {}),
    ("rotated small light off the ceiling", "cornell.txt", {0: ("1 7.5 -1", "20 30 10", "2 .4 1.5")}),
    ("light in front of the back wall", "cornell.txt", {0: ("0 5 -4.6", "0 0 0", "3 3 .3")}),
    ("sphere touching the left wall", "cornell.txt", {6: ("-3.495 4 -1", "0 0 0", "3 3 3")}),
]


@pytest.fixture(scope="module")
def gpu(pt):
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return pt


def _scene_file(tmp_path, base, edits):
    """the base scene's text with the named objects' TRANS / ROTAT / SCALE rewritten"""
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
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "candidate_child.py"), scene_path, str(w), str(h), str(DEPTH), str(iters), out],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(out)
    return z["img"], z["tallies"], z["cand"]


def test_the_slab_certificate_never_rejects_a_hit_of_a_binned_size_cube(gpu, oracle):
    S = oracle.make_geom
    cubes = np.concatenate([
        S(1, 0, (0, 10, 0), (0, 0, 0), (3, .3, 3)),                 # Cornell's light
        S(1, 0, (2, 9.99, -1), (0, 0, 0), (2.5, .02, 2.5)),         # a thin slab at a ceiling
        S(1, 0, (1, 6, -2), (0, 0, 0), (4, .04, 4)),                # 100 : 1
        S(1, 0, (-2, 5, 1), (25, 40, -15), (5, .05, 3)),            # 100 : 1, rotated
        S(1, 0, (2, 3, -1), (30, 45, 10), (1.5, 1, 2)),
        S(1, 0, (0.02, -0.01, 0.03), (10, 20, 30), (.1, .1, .1)),   # small, at the world's origin: a bound on the origin below 1.3
        S(1, 0, (-3, 2, 2), (0, 60, 20), (.03, 3, .03)),
    ]).view(gpu.GEOM_DTYPE)
    culled, violations = gpu.test_wall_box_sweep(cubes, seed=20251020, rays=RAYS)
    print("slab certificate on binned-size cubes: %d of %d rays certified, %d violations" % (culled, RAYS, violations))
    assert violations == 0
    assert culled > 0


def test_the_half_line_certificate_never_rejects_a_hit_of_a_binned_size_sphere(gpu, oracle):
    S = oracle.make_geom
    spheres = np.concatenate([
        S(0, 4, (-1, 4, -1), (0, 0, 0), (3, 3, 3)),                 # Cornell's sphere
        S(0, 1, (2, 1, 3), (0, 0, 0), (.5, .5, .5)),
        S(0, 1, (-3, 6, -2), (20, 70, -40), (1, 1, 1)),
        S(0, 1, (1, 7, 1), (15, -30, 60), (1.2, 1, .9)),
        S(0, 1, (-3.495, 4, -1), (0, 0, 0), (3, 3, 3)),
    ]).view(gpu.GEOM_DTYPE)
    culled, behind, violations = gpu.test_sphere_halfline_sweep(spheres, seed=20251021, rays=RAYS)
    print("half-line certificate on binned-size spheres: %d of %d rays certified, %d with the centre behind, %d violations" % (culled, RAYS, behind, violations))
    assert violations == 0
    assert culled > 0 and behind > 0


@pytest.mark.parametrize("name,base,edits", SCENES, ids=[s[0].replace(" ", "_") for s in SCENES])
def test_frames_equal_the_oracle_with_and_without_the_tight_candidacy(gpu, oracle, tmp_path, name, base, edits):
    path = _scene_file(tmp_path, base, edits)
    on = _child(tmp_path, path, W, H, ITERS, False)
    off = _child(tmp_path, path, W, H, ITERS, True)
    sc = gpu.Scene(path)
    sc.set_resolution(W, H)
    want = np.zeros(W * H * 3, np.float32)
    orc = oracle.Renderer(sc.camera.view(oracle.CAMERA_DTYPE), sc.geoms.view(oracle.GEOM_DTYPE), sc.materials.view(oracle.MATERIAL_DTYPE), DEPTH)
    for it in range(1, ITERS + 1):
        orc.iterate(it, want)
    print("%s: candidate tiles %d of %d (ball alone: %d of %d), scatters classed candidates %d of %d (ball alone %d)" % (
        name, on[2][1], on[2][0], off[2][1], off[2][0], on[2][6], on[2][4], on[2][5]))
    assert want.max() > 0
    assert np.array_equal(on[0].reshape(-1).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(off[0].reshape(-1).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(on[0].view(np.uint32), off[0].view(np.uint32))
    assert on[1][-2] == off[1][-2]                                  # light hits


def test_fewer_candidate_tiles_and_every_binned_hit_still_in_one(gpu, tmp_path):
    path = os.path.join(ROOT, "scenes", "cornell.txt")
    on = _child(tmp_path, path, 160, 90, 8, False)[2]
    off = _child(tmp_path, path, 160, 90, 8, True)[2]
    share_on, share_off = on[1] / on[0], off[1] / off[0]
    print("candidate tiles: %d of %d (%.2f %%) against %d of %d (%.2f %%) by the balls alone; scatters classed candidates %d against %d of %d; "
          "lanes of candidate tiles that hit a binned primitive %d / %d" % (on[1], on[0], 100 * share_on, off[1], off[0], 100 * share_off, on[6], off[6], off[4], on[3], off[3]))
    assert on[0] > 0 and off[0] > 0 and off[4] > 0
    # with the switch the rule in force is the ball's, scatter for scatter: the parent's classes
    assert off[6] == off[5]
    # the same paths are scattered in both arms, and the ball says the same of them
    assert on[4] == off[4] and on[5] == off[5]
    # strictly fewer candidates, by scatters and by tiles
    assert on[6] < on[5]
    assert share_on < share_off
    # every lane that hit a binned primitive sat in a candidate tile in both arms
    assert on[3] == off[3] > 0
    # the one-wall candidate tiles whose wall has an inner face: some of the candidate tiles, in both arms (the count is recorded, not pinned)
    print("candidate tiles of one wall that has an inner face: %d (ball alone: %d)" % (on[2], off[2]))
    assert 0 < on[2] <= on[1] and 0 < off[2] <= off[1]
