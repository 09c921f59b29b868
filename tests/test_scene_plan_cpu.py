"""The host half of pt_init (csrc/pt_scene_plan.h: plan_scene), without a GPU, through the test library's pt_test_scene_plan: the state it
plans for every scene of scenes/ is one pt_init may produce and one the library holds kernels for, and every refusal that used to come
after the renderer had been half built -- the checks of the scene's size -- is reached without a device, before anything is touched."""
import ctypes as C
import glob
import os
import types

import numpy as np
import pytest

from conftest import SCENES
from test_kernel_select_cpu import STATE, consistent, names

NAMES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(SCENES, "*.txt")))


def _scene(pt, name, w=32, h=32):
    sc = pt.Scene(os.path.join(SCENES, name + ".txt"))
    sc.set_resolution(w, h)
    return sc


def _variant(sc, **changes):
    """the scene's arrays with some replaced, as any object with these attributes is a scene to pathtraceInit and scene_plan"""
    fields = ("geoms", "materials", "camera", "traceDepth", "meshes", "mesh_normals", "mesh_materials", "textures", "geom_textures", "mesh_uvs",
              "geom_bumps", "bump_scales")
    return types.SimpleNamespace(**{**{f: getattr(sc, f, None) for f in fields}, **changes})


def test_the_scenes_are_there():
    assert {"cornell", "spheres512", "cornell_mesh", "cornell_textured", "cornell_bump"} <= set(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_every_scene_plans_a_state_the_library_holds_kernels_for(pt, name):
    T = pt.test_lib()
    assert "pt_test_scene_plan" in pt.TEST_ABI_SYMBOLS and not hasattr(pt.lib(), "pt_test_scene_plan")
    s = pt.scene_plan(_scene(pt, name))
    state = {n: bool((s.state_bits >> i) & 1) for i, n in enumerate(STATE)}
    assert not state["first"] and consistent(state), names(s.state_bits, STATE)
    for first in (0, 1):
        form = C.c_uint32(0xffffffff)
        assert T.pt_test_bounce_form(s.state_bits | first, C.byref(form)) == 0, (names(s.state_bits, STATE), T.pt_last_error())
    # what the summary carries is what the state says: the swept table of a sphere-heavy scene, its groups; the launches' LDS; the pools
    assert (s.nSphCull > 0) == state["many"] and (s.nSphGroups > 0) == state["grouped"]
    assert 0 < s.ldsBytes <= 160 * 1024 and 0 < s.ldsBytesNext <= 160 * 1024
    assert 0 <= s.nBinned <= 4 and 0 <= s.nWalls <= 6 and s.poolChunks > 0
    assert 0 <= s.firstSkipped <= 32 * 32 and s.nLocalPad >= 0 and (s.nLocalPad > 0 or s.firstSkipped == 32 * 32)


def test_the_plan_follows_the_options(pt):
    sc = _scene(pt, "cornell")
    plain = pt.scene_plan(sc)
    assert names(plain.state_bits, STATE) == "plain"
    assert names(pt.scene_plan(sc, lens_radius=0.1, focal_distance=9.0).state_bits, STATE) == "dof|plain"
    assert names(pt.scene_plan(sc, flags=pt.PT_FLAG_DIRECT_LIGHTING).state_bits, STATE) == "0"
    # rows 1, 4, .. 31 of the frame, eight iterations a batch: 11 x 32 x 8 paths are two chunks of 2048 where the frame's 1024 are one
    third = pt.scene_plan(sc, shard_rank=1, shard_count=3, max_batch=8)
    assert third.poolChunks == plain.poolChunks + 1 and third.nLocalPad + third.firstSkipped >= 11 * 32


def test_late_refusals_need_no_device(pt):
    sph, mesh = _scene(pt, "sphere"), _scene(pt, "mesh_small")
    g = next(iter(mesh.meshes))
    nmats = len(mesh.materials)
    wide = sph.camera.copy()
    wide["resolution"][0] = (32768, 16384)                     # 2^29 pixels: 29 bits of a path's index word, and max_batch 16 needs 4 more
    cases = [
        # (4096 materials: the limit of 4095 is checked behind the LDS size, which so many materials exceed first)
        (_variant(sph, materials=np.repeat(sph.materials[:1], 4096)), {}, "pt_init: scene does not fit the 160 KiB LDS (266432 B)"),
        (_variant(mesh, mesh_materials={g: np.full(len(mesh.meshes[g]), nmats, np.int32)}), {},
         "pt_init: a face of mesh geom %d names material %d of %d" % (g, nmats, nmats)),
        (_variant(sph, camera=wide), dict(max_batch=16),
         "pt_init: 32768 x 16384 pixels and max_batch 16 need 29 + 4 bits of a path's 32-bit index word: lower max_batch"),
        (sph, dict(shard_rank=3, shard_count=3), "pt_init: bad shard 3/3"),
        (sph, dict(flags=pt.PT_FLAG_MOMENTS, shard_count=2), "pt_init: PT_FLAG_MOMENTS needs the whole frame: no row shard, no PT_FLAG_ACCUM_SHARD_ROWS"),
        (_variant(mesh, meshes={}), {}, "pt_init: geom %d is a mesh without triangles (pt_set_meshes)" % g),
    ]
    for sc, options, message in cases:
        with pytest.raises(pt.PtError) as e:
            pt.scene_plan(sc, **options)
        assert str(e.value) == "pt_amd error -1: " + message                 # PT_ERR_INVALID, the text pt_init gives
    # ... and pt_init itself refuses them before it looks for a device: PT_ERR_INVALID here too, where a valid scene ends in PT_ERR_NO_GPU
    with pytest.raises(pt.PtError, match="pt_amd error -1: pt_init: scene does not fit the 160 KiB LDS"):
        pt.pathtraceInit(cases[0][0])
    assert pt.scene_plan(sph).poolChunks > 0                                 # (a refusal leaves nothing behind: the next plan is whole)
