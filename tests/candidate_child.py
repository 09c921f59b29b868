"""One render in a process of its own, for tests/test_gpu_candidate_certificates.py: the plan reads PT_AMD_NO_TIGHT_CANDIDATES from the
environment this process was started with.  The renderer is the test library's (libpt_amd_test.so: the product's source plus the tally of
candidate tiles).

    python candidate_child.py <scene file> <W> <H> <depth> <iterations> <out.npz>

Writes the frame, the path tallies (live per bounce, light hits, misses) and the tally of pt_test_candidate_tally."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv):
    import __graft_entry__ as ge
    scene_file, W, H, depth, iters, out = argv[0], int(argv[1]), int(argv[2]), int(argv[3]), int(argv[4]), argv[5]
    pt = ge.load_package()
    sc = pt.Scene(scene_file)
    sc.set_resolution(W, H)
    with pt.renderer_from_test_library():
        pt.pathtraceInit(sc, traceDepth=depth, max_batch=iters, pipeline_depth=1)
        pt.counters_reset()
        pt.candidate_tally()
        pt.pathtrace_batch(None, 0, 1, iters)
        img = pt.readback(W * H).reshape(H, W, 3).copy()
        c = pt.counters()
        tallies = np.array([int(c.live[d]) for d in range(1, depth + 1)] + [int(c.light_hits), int(c.misses)], np.int64)
        cand = np.array(pt.candidate_tally(), np.int64)
        pt.pathtraceFree()
    np.savez(out, img=img, tallies=tallies, cand=cand)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
