"""The rendered cases of object history (PT_FLAG_OBJECT_HISTORY), shared by tests/test_temporal_motion_cpu.py -- which checks on the CPU
oracle's guides that every case shows enough of a moved primitive with and without history -- and tests/test_gpu_temporal_motion.py, which
renders them.  A case is a scene in its OLD poses, the geoms of the NEW view, the two eyes, and the indices of the primitives that moved."""
import os
import types

import numpy as np

import temporal_motion_ref as tm
import textured_scenes as ts
from conftest import SCENES

F = np.float32
W, H = 48, 32
DEPTH = 4
NAMES = ("sphere", "cube", "mesh", "camera", "two")


def _plain(pt, path):
    """a scene file as a namespace pathtraceInit reads, at W x H"""
    sc = pt.Scene(os.path.join(SCENES, path))
    sc.set_resolution(W, H)
    return types.SimpleNamespace(geoms=np.array(sc.geoms, copy=True), materials=np.array(sc.materials, copy=True), camera=sc.camera.copy(),
                                 traceDepth=DEPTH, meshes={}, mesh_normals={}, mesh_materials={}, image=np.zeros((H, W, 3), F))


def _look(sc, eye):
    sc.camera["position"][0] = eye
    return sc


def build(pt, orc, name):
    """dict(scene, new_geoms, eye0, eye1, moved, demod)"""
    if name == "sphere":          # Cornell, its sphere translated; the camera close enough for the sphere to fill a fifth of the frame
        sc = _look(_plain(pt, "cornell.txt"), (-0.4, 4.3, 2.4))
        new = tm.moved_geoms(orc, sc.geoms, {6: ((0.1, 4.2, -0.7), None, None)})
        return dict(scene=sc, new_geoms=new, eye0=(-0.4, 4.3, 2.4), eye1=(-0.4, 4.3, 2.4), moved=(6,), demod=False)
    if name == "cube":            # the tilted room's tall cube turned by 20 degrees about y and scaled non-uniformly
        eye = (3.5, 5.4, 5.5)       # (the file's eye moved along its view, so that the cube fills a tenth of the frame)
        sc = _look(_plain(pt, "rotated.txt"), eye)
        g = sc.geoms[2]
        r = (float(g["rotation"][0]), float(g["rotation"][1]) + 20.0, float(g["rotation"][2]))
        new = tm.moved_geoms(orc, sc.geoms, {2: (None, r, (2.5, 3.5, 1.5))})
        return dict(scene=sc, new_geoms=new, eye0=eye, eye1=eye, moved=(2,), demod=False)
    if name == "mesh":            # the textured scene's UV-mapped quad translated; the registration stays; PT_FLAG_DEMOD_HISTORY
        sc = ts.build(pt, orc, "mesh", False)
        cam = pt.Scene(os.path.join(SCENES, "cornell.txt"))
        cam.set_resolution(W, H)
        sc.camera = cam.camera.copy()
        sc.traceDepth = DEPTH
        sc.image = np.zeros((H, W, 3), F)
        q = sc.named["quad"]
        eye = (0.4, 5.5, 1.5)
        _look(sc, eye)
        new = tm.moved_geoms(orc, sc.geoms, {q: ((1.1, 5.5, -3.6), None, None)})
        return dict(scene=sc, new_geoms=new, eye0=eye, eye1=eye, moved=(q,), demod=True)
    if name == "camera":          # camera and sphere moved together
        sc = _look(_plain(pt, "cornell.txt"), (-0.4, 4.3, 2.4))
        new = tm.moved_geoms(orc, sc.geoms, {6: ((-0.8, 4.2, -1.1), (0, 30, 0), None)})
        return dict(scene=sc, new_geoms=new, eye0=(-0.4, 4.3, 2.4), eye1=(-0.2, 4.35, 2.5), moved=(6,), demod=False)
    if name == "two":             # the sphere moved, and a second sphere that had no extent in the old view (scale 0: state 2) given one
        sc = _look(_plain(pt, "cornell.txt"), (-0.4, 4.3, 2.4))
        extra = np.asarray(orc.make_geom(0, 2, (2.2, 3.0, -0.5), (0, 0, 0), (0, 0, 0))).view(sc.geoms.dtype)
        sc.geoms = np.concatenate([sc.geoms, extra])
        new = tm.moved_geoms(orc, sc.geoms, {6: ((-2.2, 4.3, -0.6), None, None), 7: (None, None, (2.5, 2.5, 2.5))})
        return dict(scene=sc, new_geoms=new, eye0=(-0.4, 4.3, 2.4), eye1=(-0.4, 4.3, 2.4), moved=(6, 7), demod=False)
    raise KeyError(name)


def oracle_guides(orc, case, new):
    """the CPU oracle's guide buffers of iteration 1 for the case's old (new=False) or new view, packed as the device holds them"""
    import denoise_ref as dr
    sc = case["scene"]
    cam = sc.camera.copy()
    cam["position"][0] = case["eye1"] if new else case["eye0"]
    geoms = case["new_geoms"] if new else sc.geoms
    ref = orc.Renderer(cam.view(orc.CAMERA_DTYPE), np.ascontiguousarray(geoms).view(orc.GEOM_DTYPE), sc.materials.view(orc.MATERIAL_DTYPE), DEPTH,
                       meshes=sc.meshes or None)
    return tm.tr.pack_guides(*dr.oracle_guides(orc, ref, 1, meshes=sc.meshes, mesh_normals=sc.mesh_normals), H, W), tm.tr.camera16(cam)
