"""The resolved waves of the camera rays' work list on the device (pt_init: camera_face_certificate; k_bounce<true, ...>: ptd::boxFaceHit)
against the same list with every wave unresolved (PT_AMD_NO_CAMERA_RESOLVE, a tests-only switch of pt_init): the frame and the tallies
of light hits, misses and live paths per bounce are identical, byte for byte -- four iterations as one batch and as four single calls,
unsharded and in three row shards; Cornell and the glass box also against the oracle's frame.  And a device sweep of boxFaceHit
against boxIntersectionTest on every resolved pixel of Cornell at 320x180: 64 seeded jitters and the corners of the certificate's
footprint, (t > 0, outside, face, P) bit for bit."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = "PT_AMD_NO_CAMERA_RESOLVE"
ITERS = 4

# (scene, W, H, depth, compared with the oracle's frame)
CASES = [
    ("cornell.txt", 97, 61, 8, True), ("cornell.txt", 160, 90, 8, True), ("cornell_glass.txt", 63, 200, 16, True),
    ("room_tilted.txt", 97, 61, 8, False),
]


@pytest.fixture(scope="module")
def gpu(pt):
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return pt


def _render(gpu, sc, monkeypatch, off, depth, batch, shard=(0, 1)):
    monkeypatch.delenv(SWITCH, raising=False)
    if off:
        monkeypatch.setenv(SWITCH, "1")
    W, H = (int(v) for v in sc.camera["resolution"][0])
    gpu.pathtraceFree()
    gpu.pathtraceInit(sc, shard_rank=shard[0], shard_count=shard[1], traceDepth=depth, max_batch=ITERS, pipeline_depth=1)
    gpu.counters_reset()
    if batch:
        gpu.pathtrace_batch(None, 0, 1, ITERS)
    else:
        for it in range(1, ITERS + 1):
            gpu.pathtrace(None, 0, it)
    img = gpu.readback(W * H).reshape(H, W, 3).copy()
    c = gpu.counters()
    tallies = np.array([int(c.live[d]) for d in range(1, depth + 1)] + [int(c.light_hits), int(c.misses)], np.int64)
    gpu.pathtraceFree()
    monkeypatch.delenv(SWITCH, raising=False)
    return img, tallies


def _same(a, b):
    assert np.array_equal(a[1], b[1])
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


@pytest.mark.parametrize("name,W,H,depth,vs_oracle", CASES)
def test_resolved_waves_render_what_unresolved_ones_do(gpu, oracle, monkeypatch, name, W, H, depth, vs_oracle):
    sc = gpu.Scene(os.path.join(ROOT, "scenes", name))
    sc.set_resolution(W, H)
    cam, geoms = sc.camera.view(gpu.CAMERA_DTYPE), sc.geoms.view(gpu.GEOM_DTYPE)
    face = gpu.camera_resolved(cam, geoms)[3]
    assert np.any(face >= 0)                                    # (not vacuous: the default build takes the branch)
    whole = _render(gpu, sc, monkeypatch, False, depth, True)
    assert whole[0].max() > 0 and whole[1][0] > 0
    _same(whole, _render(gpu, sc, monkeypatch, True, depth, True))
    _same(whole, _render(gpu, sc, monkeypatch, False, depth, False))
    _same(whole, _render(gpu, sc, monkeypatch, True, depth, False))
    for batch in (True, False):
        for off in (False, True):
            img = np.zeros_like(whole[0])
            tallies = np.zeros_like(whole[1])
            for rank in range(3):
                part = _render(gpu, sc, monkeypatch, off, depth, batch, shard=(rank, 3))
                img[rank::3] = part[0][rank::3]
                tallies += part[1]
            _same(whole, (img, tallies))
    if vs_oracle:
        ref = oracle.Renderer(sc.camera.view(oracle.CAMERA_DTYPE), sc.geoms.view(oracle.GEOM_DTYPE), sc.materials.view(oracle.MATERIAL_DTYPE), depth)
        want = np.zeros(W * H * 3, np.float32)
        for it in range(1, ITERS + 1):
            ref.iterate(it, want)
        assert np.array_equal(whole[0].reshape(-1).view(np.uint32), want.view(np.uint32))


def test_face_hit_equals_the_box_test_on_every_resolved_pixel(gpu):
    sc = gpu.Scene(os.path.join(ROOT, "scenes", "cornell.txt"))
    sc.set_resolution(320, 180)
    cam, geoms = sc.camera.view(gpu.CAMERA_DTYPE), sc.geoms.view(gpu.GEOM_DTYPE)
    pix, _, _, face = gpu.camera_resolved(cam, geoms)
    resolved = int((pix.reshape(-1, 64)[face >= 0] != 0xFFFFFFFF).sum())
    rays, bad, pixels = gpu.test_face_hit_sweep(cam, geoms, samples=64, seed=20240607)
    # (not vacuous: the sweep visits the list's resolved pixels, and at this size they are more than the 0.25 of the listed ones asked of 97x61)
    assert pixels == resolved > 0.25 * int((pix != 0xFFFFFFFF).sum())
    assert rays == pixels * 68
    assert bad == 0
