"""Which scenes carry a path's material history instead of its throughput (no GPU): the rule of csrc/pt_scene_plan.h next to `plain`,
through the test library's pt_test_scene_plan.

A code is 2 * material + (specular ? 1 : 0): b = max(1, ceil(log2(2 nmats))) bits.  traceDepth - 1 scatters lie behind a path that enters
the last bounce, so the PLAIN forms -- whose pools are history-coded (PtTestPlanSummary::histBits = b) -- are taken only where
b * (traceDepth - 1) <= 32.  A scene beyond that plans the general forms (histBits 0, no `plain` bit), as PT_AMD_NO_PLAIN does for any."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from conftest import ROOT, SCENES
from test_kernel_select_cpu import STATE, names


def _scene(pt, nmats, depth):
    """Cornell's primitives over `nmats` diffuse materials (the first emits); material ids folded into the table"""
    sc = pt.Scene(os.path.join(SCENES, "cornell.txt"))
    sc.set_resolution(32, 32)
    m = np.zeros(nmats, pt.MATERIAL_DTYPE)
    for i in range(nmats):
        m[i] = ((.5, .5, .5), 0, (0, 0, 0), 0, 0, 0, 5 if i == 0 else 0)
    g = sc.geoms.copy()
    g["materialid"] %= nmats
    return types.SimpleNamespace(geoms=g, materials=m, camera=sc.camera.copy(), traceDepth=depth, meshes={})


def _plan(pt, nmats, depth, **options):
    s = pt.scene_plan(_scene(pt, nmats, depth), **options)
    return names(s.state_bits, STATE), s.histBits


def test_code_width(pt):
    # b = max(1, ceil(log2(2 nmats))), read back from plans that take the history form (depth 2: one scatter always fits)
    for nmats, b in ((1, 1), (2, 2), (3, 3), (4, 3), (5, 4), (8, 4), (9, 5), (16, 5), (17, 6)):
        assert _plan(pt, nmats, 2) == ("plain", b), nmats


def test_eight_materials_at_depth_nine_are_in(pt):
    assert _plan(pt, 8, 9) == ("plain", 4)                      # 4 bits x 8 scatters = 32


def test_nine_materials_at_depth_nine_are_out(pt):
    assert _plan(pt, 9, 9) == ("0", 0)                          # 5 x 8 = 40


def test_eight_materials_at_depth_ten_are_out(pt):
    assert _plan(pt, 8, 10) == ("0", 0)                         # 4 x 9 = 36


def test_one_material_is_in_at_any_depth_up_to_33(pt):
    for depth in (1, 2, 8, 32, 33):
        assert _plan(pt, 1, depth) == ("plain", 1), depth
    assert _plan(pt, 1, 34) == ("0", 0)


def test_the_shipped_cornell_box_takes_the_history_form(pt):
    sc = pt.Scene(os.path.join(SCENES, "cornell.txt"))
    sc.set_resolution(32, 32)
    s = pt.scene_plan(sc)
    assert names(s.state_bits, STATE) == "plain" and s.histBits == 4 and 4 * (sc.traceDepth - 1) <= 32
    # a lens leaves the camera-ray launch without a PLAIN form; the later launches' pools are history-coded all the same
    lens = pt.scene_plan(sc, lens_radius=0.1, focal_distance=9.0)
    assert names(lens.state_bits, STATE) == "dof|plain" and lens.histBits == 4
    # direct lighting, a textured or a mesh scene: the general layout
    assert pt.scene_plan(sc, flags=pt.PT_FLAG_DIRECT_LIGHTING).histBits == 0
    for name in ("cornell_glass", "cornell_mesh", "spheres64", "cornell_textured"):
        other = pt.Scene(os.path.join(SCENES, name + ".txt"))
        other.set_resolution(32, 32)
        assert pt.scene_plan(other).histBits == 0, name


def test_pt_amd_no_plain_still_wins(pt):
    # (pt_init reads the switch from its environment: a process of its own)
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import __graft_entry__ as ge, test_path_history_cpu as t\n"
            "pt = ge.load_package()\n"
            "print(t._plan(pt, 8, 9), t._plan(pt, 1, 2))\n") % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, PT_AMD_NO_PLAIN="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "('0', 0) ('0', 0)"
