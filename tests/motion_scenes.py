"""Scenes in motion for the motion-blur tests (TRANS_END / ROTAT_END / SCALE_END, PT_FLAG_MOTION), and the one thing both the host and the
GPU tests need of them: the STATIC scene file of a step -- the file's text with every moving component replaced by its value at the step's
shutter time and the *_END lines taken out.  The loader promises that step s of a scene in motion is, byte for byte, what it makes of that
file; the GPU law builds on it (iteration i of a motion-blurred render is iteration i of the static scene of step PT_MOTION_STEP(i)).

The interpolation is restated here in numpy float32, one IEEE operation per step as the loader does it: a + (b - a) * t with
t = (s + 0.5) / 16 (exact in float), a and b the file's decimals rounded to float as atof-and-cast rounds them.  The values are written with
repr() of the float's exact double, which reads back to the same float."""
import os
import re

import numpy as np

from conftest import SCENES

F = np.float32
STEPS = 16
RUN = 8
KEYS = ("TRANS", "ROTAT", "SCALE")


def shutter_time(step):
    return F((F(step) + F(0.5)) / F(STEPS))


def lerp(a, b, t):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return (a + (b - a) * F(t)).astype(F)


def _triple(tokens):
    return [F(float(tokens[i])) if i < len(tokens) else F(0) for i in (1, 2, 3)]


def static_text(src, step):
    """the scene text `src` as a static scene at `step` (None: the *_END lines removed and nothing else -- the pose at shutter open)"""
    out = []
    lines = src.replace("\r\n", "\n").split("\n")
    i = 0
    while i < len(lines):
        if not lines[i].startswith("OBJECT "):
            out.append(lines[i])
            i += 1
            continue
        j = i
        while j < len(lines) and lines[j] != "":
            j += 1
        block = lines[i:j]
        ends = {ln.split(" ")[0][:-4]: _triple(ln.split(" ")) for ln in block if ln.split(" ")[0] in [k + "_END" for k in KEYS]}
        block = [ln for ln in block if ln.split(" ")[0] not in [k + "_END" for k in KEYS]]
        if step is not None:
            t = shutter_time(step)
            for k, b in ends.items():
                at = [n for n, ln in enumerate(block) if ln.split(" ")[0] == k]
                a = _triple(block[at[-1]].split(" ")) if at else [F(0)] * 3
                line = k + " " + " ".join(repr(float(v)) for v in lerp(a, b, t))
                if at:
                    block[at[-1]] = line
                else:
                    block.append(line)
        out.extend(block)
        i = j
    return "\n".join(out)


class StaticScene:
    """the loaded scene `sc` with other geoms and no motion: what pathtraceInit and scene_plan read of a scene, nothing owned"""

    def __init__(self, sc, geoms):
        for f in ("materials", "camera", "iterations", "traceDepth", "imageName", "meshes", "mesh_normals", "mesh_materials", "mesh_uvs",
                  "textures", "texture_paths", "geom_textures", "geom_bumps", "bump_scales", "image"):
            setattr(self, f, getattr(sc, f))
        self.geoms = np.ascontiguousarray(geoms).copy()
        self.step_geoms = None


def link_assets(tmp_path):
    for d in ("models", "textures"):
        if not (tmp_path / d).exists():
            (tmp_path / d).symlink_to(os.path.join(SCENES, d))


def write(tmp_path, name, text):
    link_assets(tmp_path)
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def cornell(edit):
    """scenes/cornell.txt with `edit` = {object id: {"TRANS": "x y z" (replaces the line), "TRANS_END": "x y z" (added), ...}} and `extra`
    OBJECT blocks appended"""
    src = open(os.path.join(SCENES, edit.pop("base", "cornell.txt"))).read()
    extra = edit.pop("extra", "")
    for obj, lines in edit.items():
        m = re.search(r"OBJECT %d\n(?:.+\n)+" % obj, src)
        block = m.group(0)
        for k, v in lines.items():
            if re.search(r"^%s .*$" % k, block, re.M):
                block = re.sub(r"^%s .*$" % k, "%s %s" % (k, v), block, flags=re.M)
            else:
                block += "%s %s\n" % (k, v)
        src = src[:m.start()] + block + src[m.end():]
    return src.rstrip("\n") + "\n\n" + extra


# Cornell's sphere (radius 1.5) translating through the left wall at x = -5: inside the box, straddling the wall, outside
SPHERE_THROUGH_WALL = lambda: cornell({6: {"TRANS": "-2.6 4 -1", "TRANS_END": "-7.4 4.5 -0.5"}})
# the ceiling light sliding and shrinking: the emitters direct lighting samples are each pose's own
MOVING_EMITTER = lambda: cornell({0: {"TRANS_END": "2.5 10 1.5", "SCALE_END": "2 .3 1.5"}})
# Cornell with six small spheres (more than the four the queue is binned by: the MANY forms of k_bounce), a large static slab, and a slab
# that turns from axis-aligned to 20 degrees while it shrinks: large, it is the seventh of the big cubes and is swept with the spheres (the
# forms with CUBES); small, it is binned (the forms without) -- the poses of one render take different forms of k_bounce
def _turning_slab():
    s = ""
    for k in range(6):
        s += "OBJECT %d\nsphere\nmaterial %d\nTRANS %g %g %g\nROTAT 0 0 0\nSCALE 1 1 1\n\n" % (7 + k, 1 + k % 4, -3 + 1.2 * k, 1 + 0.5 * k, -2 + 0.6 * k)
    s += "OBJECT 13\ncube\nmaterial 1\nTRANS -1 5 -4\nROTAT 0 0 0\nSCALE 7 7 .3\n\n"
    s += "OBJECT 14\ncube\nmaterial 4\nTRANS 1 4 -2\nROTAT 0 0 0\nROTAT_END 0 20 0\nSCALE 6 6 .3\nSCALE_END 2 2 .3\n\n"
    return cornell({"extra": s})


TURNING_SLAB = _turning_slab
# a textured sphere and a UV-mapped mesh moving
TEXTURED = lambda: cornell({"base": "cornell_textured.txt", 6: {"TRANS_END": "0.5 4.5 0", "ROTAT_END": "0 90 20"},
                            7: {"TRANS_END": "1.5 3 1", "SCALE_END": "3 3.5 4"}})

# two small fixtures for the loader: awkward decimals, a component whose own line is missing (END alone: it starts at zero), an object
# that does not move between two that do, ids in order
_HEAD = """MATERIAL 0
RGB 1 1 1
SPECEX 0
SPECRGB 0 0 0
REFL 0
REFR 0
REFRIOR 0
EMITTANCE 5

MATERIAL 1
RGB .7 .6 .5
SPECEX 0
SPECRGB 0 0 0
REFL 0
REFR 0
REFRIOR 0
EMITTANCE 0

CAMERA
RES 37 23
FOVY 40
ITERATIONS 4
DEPTH 3
FILE fixture
EYE 0.0 2 9
VIEW 0 0 -1
UP 0 1 0

"""
FIXTURE_A = _HEAD + """OBJECT 0
cube
material 0
TRANS 0.1 6.3 -0.7
ROTAT 0 0 0
SCALE 3 .3 3
SCALE_END 1e-1 0.3333333 2.9999
TRANS_END -1.7 6.25 1e-3

OBJECT 1
sphere
material 1
TRANS 1 2 3
ROTAT 10 20 30
SCALE 1 1 1

OBJECT 2
cube
material 1
TRANS -2 1 0
ROTAT 0.1 0.2 0.3
ROTAT_END 359.9 -45.5 17.123456
SCALE 1.5 2.5 0.5

"""
FIXTURE_B = _HEAD + """OBJECT 0
sphere
material 0
SCALE 2 2 2
TRANS_END 3 -1 2.000001

OBJECT 1
mesh models/torus_small.obj
material 1
TRANS_END 1 1 1
TRANS 0 1 0
ROTAT 45 0 0
ROTAT_END 0 45 0
SCALE 2 2 2
SCALE_END 2.5 2.25 2.125

OBJECT 2
cube
material 1
TRANS 0 -1 0
ROTAT 0 0 0
SCALE 10 .01 10

"""
