"""One scene rendered in a process of its own, for tests/test_gpu_scatter_diet.py: the plan reads PT_AMD_NO_TIGHT_CANDIDATES from the
environment this process was started with.  The renderer is the test library's (libpt_amd_test.so: the product's source plus the tally of
candidate tiles).

    python scatter_diet_child.py <scene file | "textured"> <W> <H> <depth> <iterations> <out.npz>

"textured": the `few` scene of tests/textured_scenes.py with every texel white -- the textured forms run, and the frame is the untextured
twin's (a colour times 1.0f is itself), which the oracle renders.

Writes the frame of ONE batch of <iterations>, the frame of the same iterations traced as single calls, the light hits of each, and the
tally of pt_test_candidate_tally over the batch."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def white_textured_scene(pt, orc, W, H):
    import textured_scenes as ts
    sc = ts.build(pt, orc, "few", False)
    cam = pt.Scene(os.path.join(ROOT, "scenes", "cornell.txt"))
    cam.set_resolution(W, H)
    sc.camera = cam.camera.copy()
    sc.textures = [np.ones_like(t) for t in sc.textures]
    sc.image = np.zeros((H, W, 3), np.float32)
    return sc


def main(argv):
    import __graft_entry__ as ge
    scene_file, W, H, depth, iters, out = argv[0], int(argv[1]), int(argv[2]), int(argv[3]), int(argv[4]), argv[5]
    pt = ge.load_package()
    if scene_file == "textured":
        import oracle as orc
        sc = white_textured_scene(pt, orc, W, H)
    else:
        sc = pt.Scene(scene_file)
        sc.set_resolution(W, H)
    with pt.renderer_from_test_library():
        pt.pathtraceInit(sc, traceDepth=depth, max_batch=iters, pipeline_depth=1)
        pt.counters_reset()
        pt.candidate_tally()
        pt.pathtrace_batch(None, 0, 1, iters)
        batch = pt.readback(W * H).reshape(H, W, 3).copy()
        light_batch = int(pt.counters().light_hits)
        cand = np.array(pt.candidate_tally(), np.int64)
        pt.pathtraceFree()
        pt.pathtraceInit(sc, traceDepth=depth, max_batch=iters, pipeline_depth=1)
        pt.counters_reset()
        for it in range(1, iters + 1):
            pt.pathtrace(None, 0, it, readback=False)
        single = pt.readback(W * H).reshape(H, W, 3).copy()
        light_single = int(pt.counters().light_hits)
        pt.pathtraceFree()
    np.savez(out, batch=batch, single=single, light=np.array([light_batch, light_single], np.int64), cand=cand)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
