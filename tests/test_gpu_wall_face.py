"""The later bounces' resolved one-wall tiles on the device (k_bounce: ptd::wallFaceCertificate, ptd::boxFacePoint; pt_init:
choose_wall_faces).

The sweep: 2^20 rays per wall of tests/wall_face_ref.py's families, generated on the device, against Cornell's five walls and the three
rooms with one wall turned by 90 degrees -- wherever the certificate accepts, the resolved test's hit point equals
boxIntersectionTest<true, false>(., false, true)'s bit for bit, with the face, `outside` and a positive return value; no mismatch, and the
certificate accepts (it is not vacuous).

End to end: at 96x64, depth 8, 4 iterations in one batch, Cornell, the closed Cornell box, the glass box (the form that is not PLAIN) and a
Cornell box whose floor is the reflective material 4 -- the frame with the resolve on equals the frame with PT_AMD_NO_WALL_RESOLVE=1, both
equal the oracle's, bit for bit, the path tallies are equal, and the test library's tally says that resolved wave-tiles were run (and
none with the switch).  Every render is a process of its own: pt_init reads the switch from its environment."""
import os
import subprocess
import sys

import numpy as np
import pytest

import wall_face_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = "PT_AMD_NO_WALL_RESOLVE"
W, H, DEPTH, ITERS = 96, 64, 8, 4
RAYS_PER_WALL = 1 << 20

# (name, scene file, material of the floor or -1: the file's)
SCENES = [("cornell", "cornell.txt", -1), ("closed", "cornell_closed.txt", -1), ("glass", "cornell_glass.txt", -1), ("mirror floor", "cornell.txt", 4)]


@pytest.fixture(scope="module")
def gpu(pt):
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return pt


def test_the_resolved_box_test_equals_the_box_test_wherever_the_certificate_accepts(gpu):
    for name, sc, walls in ref.load_scenes(gpu):
        geoms = sc.geoms.view(gpu.GEOM_DTYPE)
        face, _ = gpu.wall_faces(sc)
        room = [1, 2, 3, 4, 5]                                  # the five walls, as pt_init numbers them among themselves
        assert all(face[g] >= 0 for g in room)
        accepted, bad, refused_hits, refused = gpu.test_wall_face_sweep(geoms[room], seed=20250611 + len(name), rays=len(room) * RAYS_PER_WALL)
        print("%s: accepted %d, mismatching %d, refused although hit through the face %d, refused %d" % (name, accepted, bad, refused_hits, refused))
        assert accepted + refused == len(room) * RAYS_PER_WALL
        assert bad == 0
        assert accepted > 0 and accepted > refused_hits         # (not vacuous: what it refuses among the hits is the margin band)


def _child(tmp_path, tag, scene_file, floor_mat, off):
    out = str(tmp_path / ("%s_%d.npz" % (tag.replace(" ", "_"), int(off))))
    env = dict(os.environ)
    env.pop(SWITCH, None)
    if off:
        env[SWITCH] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wall_face_child.py"), os.path.join(ROOT, "scenes", scene_file), str(floor_mat),
                        str(W), str(H), str(DEPTH), str(ITERS), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(out)
    return z["img"], z["tallies"], z["resolve"]


@pytest.mark.parametrize("name,scene_file,floor_mat", SCENES)
def test_resolved_tiles_render_what_the_box_test_does(gpu, oracle, tmp_path, name, scene_file, floor_mat):
    on = _child(tmp_path, name, scene_file, floor_mat, False)
    off = _child(tmp_path, name, scene_file, floor_mat, True)
    print("%s: later wave-tiles %d, one-wall tiles with a face %d, resolved %d, lanes in doubt %d" % ((name,) + tuple(int(v) for v in on[2])))
    assert on[0].max() > 0 and on[1][0] > 0
    assert np.array_equal(on[0].view(np.uint32), off[0].view(np.uint32))
    assert np.array_equal(on[1], off[1])
    sc = gpu.Scene(os.path.join(ROOT, "scenes", scene_file))
    sc.set_resolution(W, H)
    if floor_mat >= 0:
        sc.geoms["materialid"][1] = floor_mat
    want = np.zeros(W * H * 3, np.float32)
    orc = oracle.Renderer(sc.camera.view(oracle.CAMERA_DTYPE), sc.geoms.view(oracle.GEOM_DTYPE), sc.materials.view(oracle.MATERIAL_DTYPE), DEPTH)
    for it in range(1, ITERS + 1):
        orc.iterate(it, want)
    assert np.array_equal(on[0].reshape(-1).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(off[0].reshape(-1).view(np.uint32), want.view(np.uint32))
    # the resolved branch ran, and not under the switch
    assert on[2][0] > 0 and on[2][2] > 0 and on[2][2] <= on[2][1] <= on[2][0]
    # (the number of wave-tiles itself is not a property of the frame: how a queue's paths fall into tiles depends on the order of the reservations)
    assert off[2][0] > 0 and off[2][1] == 0 and off[2][2] == 0
