"""Who owns the library's streams, events and page-locked memory: one owner type each, beside the device buffers' (csrc/pt_owned.h: Stream,
Event, HostBuf, DevBuf), and the test library counts what those owners hold (pt_test_live_handles, pt_test_live_device_buffers).  No
teardown list names a handle, so a handle that is forgotten shows here and nowhere else.

The scenarios are tests/test_gpu_device_buffers.py's, with its scenes and sizes: renderers initialised one over the other hold the same
number of handles for the same scene, a refused pt_init changes nothing, and pathtraceFree brings the count to zero -- also after what makes
handles lazily: pt_iterate_until (its page-locked words and their two events), PT_FLAG_KERNEL_TIMING (the timing events' pool), the guide
buffers' and the filter's timed runs.  A camera move makes one handle, its own stream, the first time and none after that, whichever way
it goes, and the frame behind it is the full call's.  A group on virtual devices holds the same handles and buffers after a second
pt_group_init at another resolution, nothing after pt_group_destroy, and assembles the one-device frame."""
import os

import numpy as np
import pytest

from conftest import SCENES
from test_gpu_device_buffers import DEPTH, H, W, _frame, gpu, scenes          # noqa: F401 (the fixtures)
from test_gpu_group_devices import _VirtualGroup, _assert_frame
from test_gpu_set_camera import _pose

pytestmark = pytest.mark.gpu


def _counts(gpu):
    T = gpu.test_lib()
    return int(T.pt_test_live_handles()), int(T.pt_test_live_device_buffers())


def _frame_handles(gpu, sc, **kw):
    """_frame, and the handles the library holds behind the pt_init"""
    gpu.pathtraceInit(sc, traceDepth=DEPTH, **kw)
    held = _counts(gpu)[0]
    gpu.pathtrace(None, 0, 1, readback=False)
    return gpu.readback(W * H).view(np.uint32), held


def test_restarts_leave_no_handle_behind(gpu, scenes, monkeypatch):
    handles = gpu.test_lib().pt_test_live_handles
    with gpu.renderer_from_test_library():
        gpu.pathtraceFree()
        assert _counts(gpu) == (0, 0)
        lens = dict(lens_radius=0.1, focal_distance=9.0)
        a1, na1 = _frame_handles(gpu, scenes["a"], **lens)
        monkeypatch.setenv("PT_AMD_GROUPS", "1")
        b1, nb = _frame_handles(gpu, scenes["b"])
        monkeypatch.delenv("PT_AMD_GROUPS")
        c1, nc = _frame_handles(gpu, scenes["c"])
        gpu.gbuffer(1)
        gpu.denoise(1, levels=3)
        a2, na2 = _frame_handles(gpu, scenes["a"], **lens)
        assert a1.any() and b1.any() and c1.any()
        assert np.array_equal(a1, a2)
        assert na1 == na2 and na1 > 0 and nb > 0 and nc > 0
        gpu.pathtraceFree()
        assert _counts(gpu) == (0, 0)
        # pt_iterate_until: two page-locked copies of the statistics' words and an event each, made on first use
        gpu.pathtraceInit(scenes["c"], traceDepth=DEPTH, moments=True)
        base = handles()
        _, done = gpu.iterate_until(1, 1e-4, 6, check_every=2)
        assert done == 6 and handles() == base + 3
        gpu.iterate_until(7, 1e-4, 10, check_every=2)
        assert handles() == base + 3                    # (made once)
        gpu.pathtraceFree()
        assert _counts(gpu) == (0, 0)
        # PT_FLAG_KERNEL_TIMING: two events per bounce launch, resolved into a pool the later launches draw on
        gpu.pathtraceInit(scenes["c"], traceDepth=DEPTH, flags=gpu.PT_FLAG_KERNEL_TIMING)
        base = handles()
        gpu.pathtrace(None, 0, 1, readback=False)
        assert handles() == base + 2 * DEPTH
        assert int(gpu.counters().bounce_launches) == DEPTH and handles() == base + 2 * DEPTH        # (resolved: in the pool)
        gpu.pathtrace(None, 0, 2, readback=False)
        assert handles() == base + 2 * DEPTH            # (reused: none is created)
        gpu.pathtrace(None, 0, 3, readback=False)       # ... and freed with launches unresolved
        gpu.pathtraceFree()
        assert _counts(gpu) == (0, 0)
        # the guide buffers and the filter's levels, timed: their events go with the call
        gpu.pathtraceInit(scenes["c"], traceDepth=DEPTH)
        base = handles()
        gpu.pathtrace(None, 0, 1, readback=False)
        out, ms = gpu.test_denoise(1, 0, levels=3, timing=True)
        assert out.any() and ms[0] > 0 and handles() == base
        gpu.pathtraceFree()
        assert _counts(gpu) == (0, 0)
    assert _counts(gpu) == (0, 0)


def test_a_refused_init_leaves_the_handles_alone(gpu, scenes):
    with gpu.renderer_from_test_library():
        c1, _ = _frame(gpu, scenes["c"])
        held = _counts(gpu)
        with pytest.raises(gpu.PtError, match="pt_amd error -1"):        # PT_ERR_INVALID
            gpu.pathtraceInit(scenes["refused"], traceDepth=DEPTH)
        assert _counts(gpu) == held and held[0] > 0 and held[1] > 0     # (nothing created, nothing destroyed)
        gpu.pathtrace(None, 0, 2, readback=False)       # (the renderer that was there is still initialised)
        assert not np.array_equal(c1, gpu.readback(W * H).view(np.uint32))
        gpu.pathtraceFree()
        assert _counts(gpu) == (0, 0)


def test_a_camera_move_makes_one_stream_once(gpu, scenes):
    sc = scenes["c"]
    own = np.array(sc.camera, copy=True)
    poses = [_pose(sc), _pose(sc, (0.5, 0, 0), 10.0), _pose(sc, (-0.5, 0.3, 0), -15.0), _pose(sc, (0, 0, -1.0), 5.0), _pose(sc, (1.0, 0, 0))]
    handles = gpu.test_lib().pt_test_live_handles
    try:
        with gpu.renderer_from_test_library():
            want = []
            for cam in poses:                           # the full call's frame for every pose
                sc.camera[:] = cam
                want.append(_frame(gpu, sc)[0].copy())
            gpu.pathtraceFree()
            sc.camera[:] = poses[0]
            first, base = _frame_handles(gpu, sc)
            assert np.array_equal(first, want[0]) and base > 0
            for i, (cam, fault) in enumerate(zip(poses[1:], (False, False, True, False)), 1):
                if fault:
                    gpu.force_fault(2)                  # (a renderer with its fault word set is rebuilt: the slow path)
                gpu.pathtraceSetCamera(cam)
                assert gpu.camera_move_info()["fast"] is (not fault)
                assert handles() == base + 1, "move %d: %d handles, %d before the first move" % (i, handles(), base)
                gpu.pathtrace(None, 0, 1, readback=False)
                assert np.array_equal(gpu.readback(W * H).view(np.uint32), want[i]), "move %d: not the full call's frame" % i
            gpu.pathtraceFree()
            assert _counts(gpu) == (0, 0)
    finally:
        sc.camera[:] = own


def test_a_virtual_group_holds_the_same_after_a_second_init_and_nothing_after_destroy(gpu, scenes, monkeypatch):
    monkeypatch.setenv("PT_AMD_GROUP_THREADS", "1")
    vmap = [0, 1, 1]
    sc = scenes["c"]
    wide = gpu.Scene(os.path.join(SCENES, "cornell.txt"))
    wide.set_resolution(48, 24)
    gpu.pathtraceFree()
    gpu.pathtraceInit(sc, traceDepth=DEPTH, max_batch=3)        # the one-device frame of iterations 1 .. 3 (product library)
    gpu.pathtrace_batch(None, 0, 1, 3)
    want = gpu.readback(W * H).copy()
    gpu.pathtraceFree()
    with _VirtualGroup(gpu, vmap, "reduce") as g:
        assert g.collective == "emulated reduce (virtual devices: test library)"
        g.init(sc, traceDepth=DEPTH, max_batch=3)
        first = _counts(gpu)
        assert first[0] > 0 and first[1] > 0
        g.iterate_batch(1, 3)
        _assert_frame(g.readback(), (want,), 0, vmap, "32 x 32", shape=(H, W))
        g.init(wide, traceDepth=DEPTH, max_batch=3)     # another resolution: every frame of the group is allocated anew
        g.iterate_batch(1, 2)
        assert g.readback().any()
        assert _counts(gpu) == first
        g.init(sc, traceDepth=DEPTH, max_batch=3)
        g.iterate_batch(1, 3)
        _assert_frame(g.readback(), (want,), 0, vmap, "32 x 32 again", shape=(H, W))
        assert _counts(gpu) == first
        g.destroy()
        assert _counts(gpu) == (0, 0)
