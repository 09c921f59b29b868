"""The camera-ray bounce over the packed work list (pt_init: build_camera_list, k_bounce<true, ...>) on the device, against the
row-band tiles it replaces (PT_AMD_NO_CAMERA_LIST, a tests-only switch of pt_init) and against no culling at all
(PT_AMD_NO_CAMERA_CULL): the frame and the tallies are identical, bit for bit -- at the benchmark's full frame, in row shards, after a
camera move, and where the list is not built (thin lens, a mesh scene, a frame too wide for the row lists)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("PT_AMD_NO_CAMERA_LIST", "PT_AMD_NO_CAMERA_CULL")


@pytest.fixture(scope="module")
def gpu(pt):
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return pt


def _scene(gpu, name, W, H):
    sc = gpu.Scene(os.path.join(ROOT, "scenes", name))
    sc.set_resolution(W, H)
    return sc


def _render(gpu, sc, monkeypatch, switch=None, depth=8, iters=2, shard=(0, 1), **kw):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    if switch:
        monkeypatch.setenv(switch, "1")
    W, H = (int(v) for v in sc.camera["resolution"][0])
    gpu.pathtraceFree()
    gpu.pathtraceInit(sc, shard_rank=shard[0], shard_count=shard[1], traceDepth=depth, max_batch=iters, pipeline_depth=1, **kw)
    gpu.counters_reset()
    gpu.pathtrace_batch(None, 0, 1, iters)
    img = gpu.readback(W * H).reshape(H, W, 3)
    c = gpu.counters()
    tallies = np.array([int(c.live[d]) for d in range(1, depth + 1)] + [int(c.light_hits), int(c.misses)], np.int64)
    gpu.pathtraceFree()
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    return img, tallies


def _same(a, b):
    assert np.array_equal(a[1], b[1])
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def test_cornell_full_frame_is_identical_to_the_row_bands_and_to_no_culling(gpu, monkeypatch):
    sc = _scene(gpu, "cornell.txt", 1280, 720)
    listed = _render(gpu, sc, monkeypatch)
    assert listed[0].max() > 0 and listed[1][-2] > 0
    _same(listed, _render(gpu, sc, monkeypatch, "PT_AMD_NO_CAMERA_LIST"))
    _same(listed, _render(gpu, sc, monkeypatch, "PT_AMD_NO_CAMERA_CULL"))


@pytest.mark.parametrize("count", [2, 3, 8])
def test_row_shards_add_up_to_the_unsharded_frame(gpu, monkeypatch, count):
    sc = _scene(gpu, "cornell_glass.txt", 640, 360)
    whole = _render(gpu, sc, monkeypatch, depth=6)
    img = np.zeros_like(whole[0])
    tallies = np.zeros_like(whole[1])
    for rank in range(count):
        part = _render(gpu, sc, monkeypatch, depth=6, shard=(rank, count))
        img[rank::count] = part[0][rank::count]
        tallies += part[1]
    _same(whole, (img, tallies))


def test_a_camera_move_rebuilds_the_list(gpu, monkeypatch):
    sc = _scene(gpu, "cornell.txt", 400, 300)
    first = _render(gpu, sc, monkeypatch)
    sc.camera["position"][0][0] += 1.5
    sc.camera["position"][0][1] -= 0.7
    moved = _render(gpu, sc, monkeypatch)
    assert not np.array_equal(first[0], moved[0])
    _same(moved, _render(gpu, sc, monkeypatch, "PT_AMD_NO_CAMERA_LIST"))
    _same(moved, _render(gpu, sc, monkeypatch, "PT_AMD_NO_CAMERA_CULL"))


@pytest.mark.parametrize("name,W,H,kw", [
    ("cornell.txt", 320, 180, {"lens_radius": 0.3, "focal_distance": 9.0}),      # thin lens: no culling, no list
    ("cornell_mesh.txt", 320, 180, {}),                                          # meshes: the walk's index space is the row bands'
    ("cornell.txt", 40000, 4, {}),                                               # wider than the row lists allow
])
def test_where_the_list_is_not_built_the_render_is_unchanged(gpu, monkeypatch, name, W, H, kw):
    sc = _scene(gpu, name, W, H)
    got = _render(gpu, sc, monkeypatch, depth=4, **kw)
    assert got[1][1] > 0                                       # (camera rays hit something)
    _same(got, _render(gpu, sc, monkeypatch, "PT_AMD_NO_CAMERA_LIST", depth=4, **kw))
    _same(got, _render(gpu, sc, monkeypatch, "PT_AMD_NO_CAMERA_CULL", depth=4, **kw))
