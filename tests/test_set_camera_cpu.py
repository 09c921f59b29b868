"""The camera move -- pt_init's same-scene form, pt_init(cam, NULL, 0, NULL, 0, PT_SAME_SCENE, NULL); pathtraceSetCamera -- without a GPU: its refusals in front of any device call, and the LEDGER of the pose family (tests/camera_poses.py) that
tests/test_gpu_set_camera.py compares the device's face certificates and the moved renderers on -- through the host-only
pt_test_camera_resolved, so that the GPU test's equalities are not equalities of nothing.

The ledger as printed by this test (84 poses: cornell.txt, cornell_glass.txt and room_tilted.txt at 97x61 and 130x70, 14 poses each):
    waves' face codes over the family: -1 in 80 poses, 0 in 20, 1 in 20, 2 in 10, 3 in 30 (4 and 5 in none)
    poses that resolve >= 0.25 of their listed pixels: 30 (the sidesteps and the turns by 5 and 30 degrees: 0.30 .. 0.52)
    poses whose list has no resolved wave: 50 (an eye inside the room or behind a primitive's plane: every rectangle is the frame)
    poses without a list (nothing listed: the scene rectangle is empty): 4 (`away` on the two Cornell scenes)
"""
import collections
import ctypes as C
import os

import numpy as np

import camera_poses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 0xFFFFFFFF


def test_refusals_need_no_renderer_and_no_device(pt):
    L = pt.lib()
    # no new product function: the export set is frozen (tests/test_host.py), the move is a form of pt_init that was refused before
    assert "pt_set_camera" not in pt.ABI_SYMBOLS and not hasattr(L, "pt_set_camera") and pt.PT_SAME_SCENE == 0
    move = lambda cam: L.pt_init(cam, None, 0, None, 0, pt.PT_SAME_SCENE, None)
    sc = pt.Scene(os.path.join(ROOT, "scenes", "cornell.txt"))
    cam = np.ascontiguousarray(sc.camera)
    pt.pathtraceFree()
    # before pt_init: PT_ERR_NOT_INIT
    assert move(cam.ctypes.data_as(C.c_void_p)) == -2          # PT_ERR_NOT_INIT
    assert b"before pt_init" in L.pt_last_error()
    # a null camera: PT_ERR_INVALID, renderer or not
    assert move(None) == -1                  # PT_ERR_INVALID
    assert b"null camera" in L.pt_last_error()
    # the test library says nothing moved
    for name in ("pt_test_last_camera_move", "pt_test_camera_resolved_device"):
        assert name in pt.TEST_ABI_SYMBOLS and not hasattr(L, name)
    assert pt.camera_move_info() == {"fast": None, "tables_uploaded": 0, "bytes_uploaded": 0}


def test_the_header_declares_it_and_python_wraps_it(pt):
    hdr = open(os.path.join(ROOT, "include", "pt_amd.h")).read()
    assert "#define PT_SAME_SCENE 0\n" in hdr and "pt_init(cam, NULL, 0, NULL, 0, PT_SAME_SCENE, NULL)" in hdr
    assert "or its same-scene form (PT_SAME_SCENE)" in hdr                      # the temporal section's "made at one moment only"
    assert callable(pt.pathtraceSetCamera) and callable(pt.camera_move_info) and callable(pt.camera_resolved_device)
    try:
        pt.pathtraceFree()
        pt.pathtraceSetCamera(pt.Scene(os.path.join(ROOT, "scenes", "cornell.txt")))
    except pt.PtError as e:
        assert "before pt_init" in str(e)
    else:
        raise AssertionError("pathtraceSetCamera without a renderer must raise")


def test_ledger_of_the_pose_family(pt):
    codes = collections.Counter()
    poses = share_ok = no_resolved = no_list = 0
    for name, W, H, label, cam, geoms in camera_poses.family(pt, os.path.join(ROOT, "scenes")):
        poses += 1
        got = pt.camera_resolved(cam, geoms)
        if got is None or len(got[0]) == 0:          # (nothing listed: pt_init keeps the row bands)
            no_list += 1
            continue
        pix, wave, sig, face = got
        lanes = pix.reshape(-1, 64)
        listed = int((lanes != PAD).sum())
        resolved = int(((lanes != PAD) & (face[:, None] >= 0)).sum())
        for f in np.unique(face):
            codes[int(f)] += 1
        share_ok += resolved >= 0.25 * listed
        no_resolved += resolved == 0
    print("ledger: %d poses; face codes (poses they occur in) %r; share >= 0.25: %d; list without a resolved wave: %d; no list: %d"
          % (poses, dict(sorted(codes.items())), share_ok, no_resolved, no_list))
    assert poses == len(camera_poses.SCENES) * len(camera_poses.SIZES) * 14
    assert -1 in codes and len([f for f in codes if f >= 0]) >= 4
    assert 3 * share_ok >= poses
    assert no_resolved >= 1 and no_list >= 1
