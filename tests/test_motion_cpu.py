"""Motion blur on the host (no GPU): the TRANS_END / ROTAT_END / SCALE_END lines of the scene format, the step geoms the loader makes of
them, the header's constants and PT_MOTION_STEP, the ABI that did not change, and the refusals planning alone decides.

The loader's promise (host/scene.h): step s of a scene in motion is, byte for byte, the load of a static scene file written with the values
interpolated at t_s = (s + 0.5) / 16 (tests/motion_scenes.py restates the interpolation in numpy float32).  On a build without the
keywords TRANS_END is an unknown line, the scene has no step geoms, and the first test fails."""
import os
import re
import subprocess

import numpy as np
import pytest

import motion_scenes as ms
from conftest import ROOT, SCENES

HDR = os.path.join(ROOT, "include", "pt_amd.h")


def _sources(tmp_path):
    return {"cornell_motion": open(os.path.join(SCENES, "cornell_motion.txt")).read(), "fixture_a": ms.FIXTURE_A, "fixture_b": ms.FIXTURE_B}


@pytest.mark.parametrize("name", ["cornell_motion", "fixture_a", "fixture_b"])
def test_every_step_is_the_load_of_its_static_scene_file(pt, tmp_path, name):
    src = _sources(tmp_path)[name]
    moving = pt.Scene(ms.write(tmp_path, "moving.txt", src))
    n = len(moving.geoms)
    assert moving.step_geoms is not None and moving.step_geoms.shape == (pt.PT_MOTION_STEPS, n) and moving.step_geoms.dtype == pt.GEOM_DTYPE
    for s in range(pt.PT_MOTION_STEPS):
        static = pt.Scene(ms.write(tmp_path, "step%d.txt" % s, ms.static_text(src, s)))
        assert static.step_geoms is None
        assert static.geoms.tobytes() == moving.step_geoms[s].tobytes(), "step %d" % s
        for f in ("materials", "camera"):
            assert getattr(static, f).tobytes() == getattr(moving, f).tobytes()
    # `geoms` is the pose at shutter open: the file without the keywords, which is all a loader that skips them reads
    unmoved = pt.Scene(ms.write(tmp_path, "open.txt", ms.static_text(src, None)))
    assert unmoved.step_geoms is None and unmoved.geoms.tobytes() == moving.geoms.tobytes()
    # something does move, and what has no *_END line does not
    first, last = moving.step_geoms[0], moving.step_geoms[-1]
    moved = [g for g in range(n) if first[g].tobytes() != last[g].tobytes()]
    assert moved and len(moved) < n
    for g in set(range(n)) - set(moved):
        assert all(moving.step_geoms[s][g].tobytes() == moving.geoms[g].tobytes() for s in range(pt.PT_MOTION_STEPS))
    assert moving.meshes.keys() == unmoved.meshes.keys()


def test_the_interpolation_is_linear_in_float_per_component(pt, tmp_path):
    sc = pt.Scene(ms.write(tmp_path, "a.txt", ms.FIXTURE_A))
    F = np.float32
    for s in range(pt.PT_MOTION_STEPS):
        t = ms.shutter_time(s)
        assert float(t) == (s + 0.5) / 16
        g = sc.step_geoms[s]
        assert g["translation"][0].tolist() == ms.lerp([0.1, 6.3, -0.7], [-1.7, 6.25, 1e-3], t).tolist()
        assert g["scale"][0].tolist() == ms.lerp([3, .3, 3], [1e-1, 0.3333333, 2.9999], t).tolist()
        assert g["rotation"][0].tolist() == [0, 0, 0]                                     # (no ROTAT_END: it does not turn)
        assert g["rotation"][2].tolist() == ms.lerp([0.1, 0.2, 0.3], [359.9, -45.5, 17.123456], t).tolist()
        assert g["translation"][2].tolist() == [F(-2), F(1), F(0)]
        assert g["type"].tolist() == sc.geoms["type"].tolist() and g["materialid"].tolist() == sc.geoms["materialid"].tolist()


def test_scenes_without_the_keywords_load_as_before(pt):
    for name in ("cornell.txt", "cornell_mesh.txt", "cornell_textured.txt", "cornell_bump.txt", "spheres64.txt"):
        assert pt.Scene(os.path.join(SCENES, name)).step_geoms is None
    sc = pt.Scene(os.path.join(SCENES, "cornell_motion.txt"))
    kinds = {int(sc.geoms[g]["type"]) for g in range(len(sc.geoms)) if sc.step_geoms[0][g].tobytes() != sc.step_geoms[15][g].tobytes()}
    assert kinds == {0, 1}                                                                # the sphere translating and a cube turning


def test_header_constants_and_the_unchanged_abi(pt):
    hdr = open(HDR).read()
    assert re.search(r"PT_FLAG_MOTION = 8192\b", hdr) and pt.PT_FLAG_MOTION == 8192
    others = [v for k, v in vars(pt).items() if k.startswith("PT_FLAG_") and k != "PT_FLAG_MOTION"]
    assert others and not any(v & 8192 for v in others)
    assert re.search(r"^#define PT_MOTION_STEPS 16$", hdr, re.M) and pt.PT_MOTION_STEPS == 16 == ms.STEPS
    assert re.search(r"^#define PT_MOTION_RUN 8$", hdr, re.M) and pt.PT_MOTION_RUN == 8 == ms.RUN
    # a flag: no function, no struct
    declared = set(re.findall(r"\b(pt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    out = subprocess.run(["nm", "-D", "--defined-only", pt.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert exported == declared == set(pt.ABI_SYMBOLS) and len(exported) == 47
    assert pt.lib().pt_abi_version() == 7 and pt.PT_AMD_ABI_VERSION == 7 and "#define PT_AMD_ABI_VERSION 7\n" in hdr


def test_the_step_sequence_is_a_bit_reversed_permutation_in_runs_of_eight(pt, tmp_path):
    # the header's own macro, through the host's compiler
    (tmp_path / "seq.cpp").write_text('#include <stdio.h>\n#include "pt_amd.h"\nint main(void) { for (int i = 1; i <= 256; ++i) '
                                    'printf("%d\\n", PT_MOTION_STEP(i)); return 0; }\n')
    subprocess.run(["g++", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "seq"), str(tmp_path / "seq.cpp")], check=True)
    seq = [int(v) for v in subprocess.run([str(tmp_path / "seq")], capture_output=True, text=True, check=True).stdout.split()]
    assert seq == [pt.motion_step(i) for i in range(1, 257)]
    for i in range(1, 257):                                                               # runs of 8
        assert seq[i - 1] == seq[(i - 1) // 8 * 8]
    runs = seq[::8]
    assert runs[:16] == [int("{:04b}".format(r)[::-1], 2) for r in range(16)] == [0, 8, 4, 12, 2, 10, 6, 14, 1, 9, 5, 13, 3, 11, 7, 15]
    assert sorted(runs[:16]) == list(range(16)) and runs[16:] == runs[:16]                # a permutation per cycle of 128
    for k in (1, 2, 4, 8):                                                                # any power-of-two prefix spreads over the shutter
        assert sorted(runs[:k]) == list(range(0, 16, 16 // k))


def test_planning_refuses_the_flag_with_what_has_one_pose(pt):
    sc = pt.Scene(os.path.join(SCENES, "cornell_motion.txt"))
    sc.set_resolution(37, 23)
    M = pt.PT_FLAG_MOMENTS
    for extra in (M | pt.PT_FLAG_TEMPORAL, M | pt.PT_FLAG_TEMPORAL | pt.PT_FLAG_OBJECT_HISTORY, M | pt.PT_FLAG_DISPLAY_FILTER,
                  M | pt.PT_FLAG_DEMODULATE, M | pt.PT_FLAG_SPATIAL_VARIANCE, pt.PT_FLAG_KEEP_RENDERER):
        pt.scene_plan(sc, flags=extra)                                                    # fine without the flag
        with pytest.raises(pt.PtError, match="PT_FLAG_MOTION"):
            pt.scene_plan(sc, flags=extra | pt.PT_FLAG_MOTION)
    for fine in (0, M, pt.PT_FLAG_DIRECT_LIGHTING, pt.PT_FLAG_MIXTURE_WEIGHTED, pt.PT_FLAG_TRACE_AHEAD, pt.PT_FLAG_KERNEL_TIMING):
        pt.scene_plan(sc, flags=fine | pt.PT_FLAG_MOTION)
