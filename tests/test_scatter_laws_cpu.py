"""The float64 scatter laws (tests/scatter_laws.py) on the CPU oracle's paths, for every case tests/test_gpu_scatter_laws.py runs on the
MI355X: this validates the reference, the scenes, the ambiguity cap, the minimum counts and the bounds without a GPU.  The renderer is
deterministic and the GPU equals the oracle bit for bit, so the statistics seen here are the ones the GPU test sees.  The cases together
reach the state bits dof, many, sweptCubes, mesh, grouped and plain, with and without `first`, and the state each declares is the one
pt_init plans for it on the host (the last test).  The guide buffers of L10 are tests/denoise_ref.py's oracle_guides here.

MEASURED on the oracle (KS: sqrt(n) D, limit 1.95; z and r sqrt(n): limit 3.3; every test prints its own):
  case            jitter x / y / r     cos^2 KS by frame   azimuth KS by frame  lag pixels / bounces  mixture z  Fresnel z  on the light
  few             0.56 / 0.60 / -0.29  1.17 / 0.85 / 1.22  1.45 / 0.61 / 0.77  -1.63 / -1.07         -1.89      -0.14      358
  plain           0.56 / 0.60 / -0.29  1.16 / 0.70 / 1.04  1.34 / 0.56 / 0.88  -1.44 / -1.15         -1.67                 352
  many_mesh-lens  0.56 / 0.60 / -0.29  1.00 / 0.89 / 0.97  1.23 / 0.81 / 0.71  -1.48 / -1.57         -1.88      -0.47      324
  grouped         0.56 / 0.60 / -0.29  0.64 / 0.51 / 0.96  0.85 / 0.60 / 0.81  -2.09 / -1.53          0.81      -0.32      340
  glass           0.78 / 0.67 /  0.38  0.71 / 0.88 / 0.90  1.06 / 1.17 / 0.88  -0.19 / -0.70                    -0.42      363
  phong           1.11 / 0.52 /  0.53  1.11 / 0.99 / 0.68  1.11 / 0.61 / 0.71  -1.12 / -1.59         -1.36       0.12      361
  many-direct     0.78 / 0.67 /  0.38  0.98 / 1.02 / 0.44  1.23 / 0.67 / 0.62  -1.42 / -0.21         -1.11      -0.52      347
  mesh-direct2    0.78 / 0.67 /  0.38  0.92 / 0.75 / 0.81  0.73 / 0.57 / 0.98  -1.45 / -0.79         -1.63      -0.84      364
  vn-smooth       0.78 / 0.67 /  0.38  0.62 / 1.38 / 1.29  1.36 / 1.04 / 0.76  -1.73 / -0.89          0.44      -1.20      375
  vn-bent         0.78 / 0.67 /  0.38  0.83 / 0.72 / 1.53  1.70 / 0.87 / 0.67  -1.42 / -1.25         -0.75      -2.04      363
  faces           0.78 / 0.67 /  0.38  1.05 / 1.34 / 0.99  0.93 / 0.87 / 0.51  -1.36 / -1.73         -0.64       1.91      849
  faces-direct    0.78 / 0.67 /  0.38  0.88 / 1.15 / 1.25  1.08 / 0.91 / 0.75  -1.49 / -2.57         -0.72       2.00      855
  face-light-only 0.78 / 0.67 /  0.38  1.16 / 1.15 / 1.06  1.31 / 0.56 / 0.83  -0.29 / -1.37         -1.54                 515
  few-weighted    0.56 / 0.60 / -0.29  1.17 / 0.85 / 1.22  1.45 / 0.61 / 0.77  -1.63 / -1.07         -1.89      -0.14      358
  mesh-weighted   0.56 / 0.60 / -0.29  0.96 / 0.77 / 1.20  1.27 / 0.80 / 0.81  -1.79 / -1.56         -1.81      -0.34      345
  many_mesh-lens: lens r^2 KS 0.61, angle KS 0.78.  phong: lobe cos^(n+1) KS 1.01 over 1181 samples (limit 1.95 + 1e-3 sqrt(n) = 1.98).
  glass: 2364 total internal reflections; 610 reflections entering (Fresnel z 0.18), 483 leaving (z -0.81).
  many-direct: light target x / y / z KS 0.85 / 0.58 / 0.57.  mesh-direct2: emitter share z -0.59 over 1668 points; the cube's box
  1.30 / 0.46 / 0.64, the emissive mesh's 0.86 / 0.78 / 1.29.  Every third-frame count is between 651 and 1294 (at least 300).
  Left out as ambiguous: at most 0.5 % of the live paths at any bounce (cap: a quarter).  Directions: at most 0.23 of their tolerance;
  new origins: 7.4e-5 off at most, 1.6e-4 on the small spheres of `grouped` (tests/scatter_laws.py: what float32 leaves of a sphere's root).
  furnace, furnace-half: exact, 4099 unfinished of 24 576 paths, no miss.
  The seven cases of the mesh attributes and the weighted mixture (third-frame counts 403 .. 1061):
  vn-smooth, vn-bent: left out at most 0.6 % and 2.9 % of the live paths at a bounce (vn-bent: rays that re-enter the surface they left
  within 1e-4 and normals near square to their face); 87 and 202 glass hits under a shading normal that faces away from the ray, out of
  the Fresnel statistics; Fresnel z entering -0.18 and -1.55; directions at most 0.30 and 0.34 of their tolerance, new origins 5.6e-6 off
  along the shading normal; vn-smooth's radial statement: |Ns - the hit point's direction| <= 1.3e-6.  The float32 blend sits at most
  1.83e-5 from the float64 Ns (vn-bent, 9531 blended hits; vn-smooth 1.71e-5 over 7710): tests/scatter_laws.py, MEASURED_BLEND.
  faces, faces-direct: 5869 / 5836 hits scatter by a face's own material, 1618 / 1654 paths end on a mesh with face materials, 2448 /
  2420 go on from a dark face of an emissive object; none ends on a dark face.  faces-direct: four emitters (the light, the cube with one
  emissive face, the emissive cube with dark faces, the octahedron with one emissive face), 1026 aimed points, 38 more inside two boxes;
  share z -1.41 / -0.04 / 1.26; clear points 411 / 456 / 528 / 551; box KS at most 1.39.  face-light-only: 515 paths end on the one face
  (1622 over the three iterations), 1298 hits scatter by a face's own material.
  few-weighted, mesh-weighted: every REFL hit carries (col * 2) * either colour bit for bit (2855 and 3633 hits); the statistics of
  few-weighted are those of `few`, as they must be: the weight changes no direction.
  L10 (few, many_mesh-lens, grouped and the seven above): 4252 .. 4284 unambiguous hits and 2615 .. 2630 misses per iteration (the
  frame's corners look past the room); positions and distances at most 0.17 of their tolerance (many_mesh-lens), normals 0.12 (grouped).

MUTATIONS, each in a scratch copy of oracle/pt_oracle.cpp (never committed), and the first law that failed:
  up = u instead of sqrt(u)                   every case: L2 cos^2 KS 28.9 .. 41.8 (few, frame 0: 28.9)
  Schlick with the incident cosine inside     glass: L5 Fresnel z -8.1; mesh-direct2: -3.3
  lr = R u instead of R sqrt(u)               many_mesh-lens: L1 lens r^2 KS 29.8
  the cover weight dropped                    many-direct, mesh-direct2: L6, a point aimed at a box in full view is not recovered (cover reads 1)
  pick always 0 with two emitters             mesh-direct2: L6 emitter share z 40.8
  the mixture at u < 0.4                      the seven cases with a REFL material: L3 mirror share z -6.5 .. -15.8
  make_seed ignoring depth                    every case: L2 cos^2 KS 4.9 .. 8.5 (a bounce repeats the draws of the one before)
  sin / cos swapped in the azimuth            NO law: the two samplers are equal in law (the azimuth is uniform either way).  It is
                                              tests/test_golden.py::test_hemisphere_survey_kats that fails (components x and z change places).

MUTATIONS for the mesh attributes, the weighted mixture and the guides, in scratch copies of oracle/pt_oracle.cpp as above, run against the
seven newer cases -- the first law that failed, and where that was L10 (which runs before the bounces) the first one with L10 left out:
  1 the blend's u and v swapped                      vn-smooth, vn-bent: L10 guide normal 6027 and 5523 x its tolerance; without L10: L7, the
                                                     new origin 2.3e-4 and 2.0e-4 off the line along Ns
  2 the turn to the face's side dropped              vn-bent (the mesh whose normals lie behind their faces): L10 guide normal 19921 x its
                                                     tolerance; without L10: L5 / L7, "an opaque surface let a path through".  vn-smooth passes: its normals need no turn
  3 the object's material at the emissive end        faces, faces-direct, face-light-only: L8, a path went on from an emissive face (45, 2
                                                     and 341 paths at the first bounce that shows it)
  4 the object's material at the scatter             faces, faces-direct: L5, glass: colour and side disagree; face-light-only: L3, REFL:
                                                     neither the mirror's colour nor the diffuse one
  5 the emitters without the face-only one           faces-direct: L6, 57 of 1010 aimed points inside two emitters' boxes (the cap is a
                                                     twentieth): no point is ever aimed at the octahedron's box
  6 the weight 2 on the mirror branch only           few-weighted, mesh-weighted: L3, REFL: neither the mirror's colour nor the diffuse one
  7 the guide normal from the face, not the blend    vn-smooth, vn-bent: L10 guide normal 3534 and 4179 x its tolerance (orc_mesh_intersect_attr
                                                     without its normals: the oracle's guides are that entry point's)
  Every other of the seven cases passes under each mutation, as it should: it does not reach the mutated line.

MUTATIONS of csrc (pt_device.h, pt_trace.h; arithmetic only, no index touched), each built apart and run ONCE on the MI355X against
tests/test_gpu_scatter_laws.py -- the statistics are the oracle's under the same mutation, to the last digit:
  hemisphereDraws: up = u01 instead of its square root        8 cases fail: L2 cos^2 KS 28.9 (few) .. 41.8 (phong)
  k_bounce: Schlick's cosx = -c from inside the glass too     glass: L5 Fresnel z -8.1; mesh-direct2: -3.3
  k_bounce: the direct-lighting weight without `cover`        many-direct, mesh-direct2: L6, a point aimed at a box in full view is not recovered
  both lens samplers: lr = lensRadius * u01                   many_mesh-lens: L1 lens r^2 KS 29.8
  meshWinner, meshIntersectionTest: the blend's u, v swapped  vn-smooth, vn-bent: L10 guide normal 6027 and 5523 x its tolerance
  ... both: the turn to the face's side dropped               vn-bent: L10 guide normal 19921 x its tolerance; vn-smooth passes
  k_bounce: the weight 2 inside the mirror branch only        few-weighted, mesh-weighted: L3, REFL: neither the mirror's colour nor the diffuse one
  meshIntersectionTest (k_gbuffer's): the blend never taken   vn-smooth, vn-bent: L10 guide normal 3534 and 4179 x its tolerance
  (the oracle's mutations 3, 4 and 5 were not repeated in csrc: there they change which material record, or which emitter, is INDEXED)
"""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as dr
import scatter_laws as sl

FORM = ("FIRST", "MANY", "DOF", "MESH", "PLAIN", "CUBES", "GROUPS", "TEX", "BUMP")              # bit i of pt_test_bounce_form's form_bits


def _oracle(orc, sc):
    ref = orc.Renderer(sc.camera.view(orc.CAMERA_DTYPE), sc.geoms.view(orc.GEOM_DTYPE), sc.materials.view(orc.MATERIAL_DTYPE), sc.traceDepth, meshes=sc.meshes,
                       mesh_normals=sc.mesh_normals, mesh_materials=sc.mesh_materials)
    ref.set_extras(**sc.extras)
    if sc.variant:
        ref.set_variant(**sc.variant)
    return ref


def _paths(ref, sc):
    return {it: [tuple(a.copy() for a in ref.dump_paths(it, k)) for k in range(sc.traceDepth + 1)] for it in sc.iters}


@pytest.mark.parametrize("name", list(sl.CASES))
def test_the_oracle_keeps_every_law(pt, oracle, name):
    sc = sl.build(pt, oracle, name)
    ref = _oracle(oracle, sc)
    frame = np.zeros(sl.W * sl.H * 3, np.float32)
    ref.iterate(sc.iters[0], frame)
    guides = {it: dr.oracle_guides(oracle, ref, it, sc.meshes, sc.mesh_normals) for it in sc.guide_iters}
    st = sl.run(sc, _paths(ref, sc), frame.reshape(-1, 3), guides=guides)
    print({k: (float("%.3g" % v) if isinstance(v, float) else v) for k, v in st.items()})


@pytest.mark.parametrize("name", sl.FURNACES)
def test_the_oracle_keeps_the_furnace(pt, oracle, name):
    sc = sl.build(pt, oracle, name)
    ref = _oracle(oracle, sc)
    frame = np.zeros(sl.FW * sl.FH * 3, np.float32)
    misses = sum(ref.iterate(it, frame).misses for it in sc.iters)
    sl.furnace(sc, _paths(ref, sc), frame.reshape(-1, 3), misses)


def test_the_cases_reach_every_state_bit_with_and_without_first(pt, oracle):
    T = pt.test_lib()
    bit = {n: 1 << i for i, n in enumerate(FORM)}
    states, forms = [], set()
    for name in list(sl.CASES) + list(sl.FURNACES):
        sc = sl.build(pt, oracle, name)
        state = sc.state
        states.append(state)
        # the state a case declares is the one pt_init plans for its scene and options (on the host alone)
        flags = (pt.PT_FLAG_DIRECT_LIGHTING if sc.direct else 0) | (pt.PT_FLAG_MIXTURE_WEIGHTED if sc.weighted else 0)
        lens = {k: v for k, v in sc.extras.items() if k != "direct_lighting"}
        assert pt.scene_plan(sc, flags=flags, **lens).state_bits == sl.state_bits(state), (name, state)
        for first in (0, 1):
            got = C.c_uint32(0xffffffff)
            assert T.pt_test_bounce_form(sl.state_bits(state, first=first), C.byref(got)) == 0, T.pt_last_error()
            forms.add(got.value)
    for k in ("dof", "many", "sweptCubes", "mesh", "grouped", "plain"):
        assert any(s[k] for s in states) and not all(s[k] for s in states), k
    assert not any(s["tex"] or s["bump"] for s in states)
    for n in ("MANY", "MESH", "PLAIN", "CUBES", "GROUPS"):
        assert any(f & bit[n] and f & bit["FIRST"] for f in forms) and any(f & bit[n] and not f & bit["FIRST"] for f in forms), n
    assert any(f & bit["DOF"] for f in forms) and all(f & bit["FIRST"] for f in forms if f & bit["DOF"])      # (a launch's DOF is first && dof)
    assert any(f & ~bit["FIRST"] == 0 for f in forms)                                                         # ... and the form with none of them
