"""The display filter (PT_FLAG_DISPLAY_FILTER) on the host (no GPU): the flag and the setting in the header and in Python, the frozen ABI,
the test entry point, and pt_init's refusals as the planner gives them."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENES

F = np.float32
DEFINES = {"PT_DISPLAY_LEVELS": "5", "PT_DISPLAY_GUIDE_ITER": "1", "PT_DISPLAY_SIGMA_LUM": "4.0f", "PT_DISPLAY_SIGMA_NORMAL": "0.35f",
           "PT_DISPLAY_SIGMA_POSITION": "2.0f"}


def test_flag_and_setting_in_the_header_and_in_python(pt):
    hdr = open(os.path.join(ROOT, "include", "pt_amd.h")).read()
    assert re.search(r"PT_FLAG_DISPLAY_FILTER = 128\b", hdr) and pt.PT_FLAG_DISPLAY_FILTER == 128
    for name, text in DEFINES.items():
        assert re.search(r"^#define %s %s$" % (name, re.escape(text)), hdr, re.M), name
        assert F(getattr(pt, name)) == F(text.rstrip("f")), name
    assert isinstance(pt.PT_DISPLAY_LEVELS, int) and isinstance(pt.PT_DISPLAY_GUIDE_ITER, int)
    # no other flag has the bit
    others = [v for k, v in vars(pt).items() if k.startswith("PT_FLAG_") and k != "PT_FLAG_DISPLAY_FILTER"]
    assert others and not any(v & 128 for v in others)


def test_the_setting_is_denoise_vars_default(pt):
    for fn in (pt.denoise_var, pt.denoise_var_rgba8):
        d = {k: p.default for k, p in inspect.signature(fn).parameters.items()}
        assert (d["levels"], d["guide_iter"], d["sigma_lum"], d["sigma_normal"], d["sigma_position"]) == (
            pt.PT_DISPLAY_LEVELS, pt.PT_DISPLAY_GUIDE_ITER, pt.PT_DISPLAY_SIGMA_LUM, pt.PT_DISPLAY_SIGMA_NORMAL, pt.PT_DISPLAY_SIGMA_POSITION)
    assert "display_filter" in inspect.signature(pt.pathtraceInit).parameters
    assert inspect.signature(pt.pathtraceInit).parameters["display_filter"].default is False


def test_the_abi_is_frozen_and_the_test_entry_is_the_test_librarys(pt):
    thdr = open(os.path.join(ROOT, "include", "pt_amd_test.h")).read()
    assert len(pt.ABI_SYMBOLS) == 47 and pt.lib().pt_abi_version() == 7 and pt.PT_AMD_ABI_VERSION == 7
    assert re.search(r"\bint pt_test_display\(", thdr) and "pt_test_display" in pt.TEST_ABI_SYMBOLS
    assert hasattr(pt.test_lib(), "pt_test_display") and not hasattr(pt.lib(), "pt_test_display")


def test_the_shim_refuses_the_display_filter_for_a_group(built, tmp_path):
    """PT_AMD_DISPLAY_FILTER with PT_AMD_DEVICES: pathtraceInit of the shim ends with a message before it reaches a device (pt_render is
    the reference's main() over this tree's shim)."""
    exe = os.path.join(ROOT, "project3-cuda-path-tracer_amd", "host", "pt_render")
    env = dict(os.environ, PT_AMD_DISPLAY_FILTER="1", PT_AMD_DEVICES="2")
    r = subprocess.run([exe, os.path.join(SCENES, "cornell.txt"), "--res", "16", "16", "--iterations", "2", "--out", str(tmp_path / "no")],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 1 and "PT_AMD_DEVICES" in r.stderr and "display filter" in r.stderr and "pathtraceInit" in r.stderr
    assert os.listdir(tmp_path) == []


def test_the_planner_refuses_the_flag_without_moments(pt):
    sc = pt.Scene(os.path.join(SCENES, "cornell.txt"))
    sc.set_resolution(32, 24)
    D, M = pt.PT_FLAG_DISPLAY_FILTER, pt.PT_FLAG_MOMENTS
    for bad in (dict(flags=D), dict(flags=D | pt.PT_FLAG_TRACE_AHEAD, max_batch=4), dict(flags=D | pt.PT_FLAG_DIRECT_LIGHTING)):
        with pytest.raises(pt.PtError, match="pt_amd error -1.*PT_FLAG_DISPLAY_FILTER"):
            pt.scene_plan(sc, **bad)
    # row shards refuse PT_FLAG_MOMENTS, hence the flag
    for bad in (dict(flags=D | M, shard_count=2), dict(flags=D | M | pt.PT_FLAG_ACCUM_SHARD_ROWS)):
        with pytest.raises(pt.PtError, match="pt_amd error -1"):
            pt.scene_plan(sc, **bad)
    # trace-ahead, a thin lens, direct lighting and temporal reprojection go with it, and the plan is the unflagged renderer's
    for ok in (dict(), dict(flags=pt.PT_FLAG_TRACE_AHEAD, max_batch=4), dict(lens_radius=0.1, focal_distance=5.0), dict(flags=pt.PT_FLAG_DIRECT_LIGHTING),
               dict(flags=pt.PT_FLAG_TEMPORAL)):
        base = dict(ok)
        base["flags"] = base.get("flags", 0) | M
        flagged = dict(base)
        flagged["flags"] |= D
        assert bytes(pt.scene_plan(sc, **flagged)) == bytes(pt.scene_plan(sc, **base))
    # a mesh scene whose hierarchy fits k_gbuffer's stacks is planned
    mesh = pt.Scene(os.path.join(SCENES, "mesh_small.txt"))
    mesh.set_resolution(32, 24)
    assert bytes(pt.scene_plan(mesh, flags=D | M)) == bytes(pt.scene_plan(mesh, flags=M))
