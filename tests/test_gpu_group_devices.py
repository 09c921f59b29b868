"""Device groups across DISTINCT devices, run on one GPU (csrc/pt_group.h; include/pt_amd_test.h: pt_test_group_create_virtual).

pt_group_create folds members that share a HIP device into one GroupDevice, and RCCL hosts one rank per GPU: on a one-GPU machine no line of
the branches taken when a group has two or more devices -- the per-device snapshot pairs, the waitRed / evRed double-buffer protocol, the
multi-rank assembly, the per-owner row copy of the host gather -- ever ran.  The test library's virtual groups give every member a virtual
device index; each distinct index is a GroupDevice of its own on the one HIP device, and the frame is assembled by an emulated reduce with
ncclReduce's semantics or by the host gather.  Everything behind the group's creation is the product's code.

The expected frames are not the group's own: after every call the frame is compared, bit for bit, with the ONE-renderer frame of the same
iterations (one pt_iterate per iteration, product library), and the last of those frames with the CPU oracle's.  The emulated reduce itself is
held to numpy's fp32 left-to-right sum (test_emulated_reduce_is_the_fp32_sum_in_rank_order), so that the group tests do not pin the product
to an emulation nobody checked.

What these tests found.  Until this file existed the root reduced IN PLACE into its own snapshot.  Run against that assembly,
test_every_call_is_the_one_renderer_frame[reduce-threads1-0.1] (virtual devices [0, 1], emulated reduce) passed iterations 1 and 2 and failed
at ITERATION 3 -- the first re-use of snapshot 0 -- with 46 wrong rows, the odd rows 5, 7, ..., 95: rows of member 1 on virtual device 1, none
of the root's ("the first is row 5 of member 1 on virtual device 1: value 234 is 8.1634..., not 4.0817...").  Every wrong row held its frame-3
value PLUS its frame-1 value ("B1 + B3"): a commit rewrites only its own member's rows of a snapshot, so the other device's rows of the root's
snapshot still held the sum the first reduce had left there.  The remaining four odd rows -- 1, 3, 97 and 99 -- are black after iteration 1
(the CPU oracle's frame 1 is zero there), so B1 + B3 is B3 and they compare equal: 46 of the 50 rows, as the analysis predicts.  The root now
receives into a result frame of its own (PtGroup::reduced) wherever a group has two or more devices; with that, every case here passes, and
nothing else turned up in the multi-device paths -- host gather and the waitRed protocol hold as written.
"""
import numpy as np
import pytest

from test_gpu_contexts import _frames_call_by_call, _oracle_frame, _scene, _single

pytestmark = pytest.mark.gpu

W, H, N_ITER = 193, 101, 11          # ragged over 2, 3 and 8 members; every member still owns a dozen rows or more
FLAGS = dict(max_batch=4, pipeline_depth=2)

MAPS = [[0, 1], [0, 1, 2], [0, 0, 1], [0, 1, 1], [0, 1, 0, 1], [0, 1, 2, 3, 0, 1, 2, 3], [0, 1, 2, 3, 4, 5, 6, 7]]
COLLECTIVE_NAME = {"reduce": "emulated reduce (virtual devices: test library)", "host": "host gather"}


def _id(vmap):
    return ".".join(str(v) for v in vmap)


@pytest.fixture(scope="module")
def gpu(pt):
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return pt


@pytest.fixture(scope="module")
def cornell(gpu):
    return _scene(gpu, res=(W, H))


@pytest.fixture(scope="module")
def want(gpu, cornell):
    """the one-renderer frame after every iteration 1 .. N_ITER (product library, one pt_iterate each): computed once, read-only"""
    frames = _frames_call_by_call(gpu, cornell, N_ITER)
    for f in frames:
        f.setflags(write=False)
    return tuple(frames)


class _VirtualGroup:
    """a virtual group inside renderer_from_test_library, destroyed before the context manager frees the test library's renderer"""

    def __init__(self, gpu, vmap, collective):
        self.gpu, self.vmap, self.collective = gpu, vmap, collective

    def __enter__(self):
        self.cm = self.gpu.renderer_from_test_library()
        self.cm.__enter__()
        try:
            self.g = self.gpu.Group(len(self.vmap), virtual=self.vmap, collective=self.collective)
        except BaseException:
            self.cm.__exit__(None, None, None)
            raise
        return self.g

    def __exit__(self, *exc):
        try:
            self.g.destroy()
        finally:
            self.cm.__exit__(*exc)
        return False


def _assert_frame(got, frames, index, vmap, what, shape=(H, W)):
    """got == frames[index] bit for bit; a failure names the first wrong row, its owner, and an earlier frame the wrong rows also hold"""
    h, w = shape
    g, e = got.view(np.uint32).reshape(h, w * 3), frames[index].view(np.uint32).reshape(h, w * 3)
    bad = np.flatnonzero((g != e).any(axis=1))
    if bad.size == 0:
        return
    n = len(vmap)
    y = int(bad[0])
    owners = sorted({vmap[int(r) % n] for r in bad})
    stale = ""
    gf, ef = got.reshape(h, w * 3)[bad], frames[index].reshape(h, w * 3)[bad]
    for j in range(index):                       # "rows of virtual device 1 hold B1 + B3"
        if np.array_equal((ef + frames[j].reshape(h, w * 3)[bad]).view(np.uint32), gf.view(np.uint32)):
            stale = "; every wrong row holds its value of frame %d PLUS its value of frame %d" % (index + 1, j + 1)
    x = int(np.flatnonzero(g[y] != e[y])[0])
    pytest.fail("%s: %d wrong rows (%s%s), all owned by virtual device(s) %s; the first is row %d of member %d on virtual device %d: value %d is %r, not %r%s"
                % (what, bad.size, ", ".join(str(int(r)) for r in bad[:6]), ", ..." if bad.size > 6 else "", owners, y, y % n, vmap[y % n], x,
                   float(got.reshape(h, w * 3)[y, x]), float(frames[index].reshape(h, w * 3)[y, x]), stale))


def test_the_expected_frames_are_the_cpu_oracles(want, cornell, oracle):
    # what every test below compares with does not rest on the library alone
    assert np.array_equal(want[N_ITER - 1].view(np.uint32), _oracle_frame(oracle, cornell, range(1, N_ITER + 1)).view(np.uint32))


# ---- a. every call, every layout ----------------------------------------------------------------------------------------------------------
CASES_A = [(m, c, "1") for m in MAPS for c in ("reduce", "host")] + [(m, c, "0") for m in (MAPS[3], MAPS[5]) for c in ("reduce", "host")]


@pytest.mark.parametrize("vmap,collective,threads", CASES_A, ids=["%s-threads%s-%s" % (c, t, _id(m)) for m, c, t in CASES_A])
def test_every_call_is_the_one_renderer_frame(gpu, cornell, want, vmap, collective, threads, monkeypatch):
    # config C3 as written on 2 .. 8 devices: one iteration on every member out of batches traced ahead, the frame's assembly, the read-back.
    # Every snapshot is written six or five times and reduced again; a member's next commit into it waits for the reduce that read it.
    monkeypatch.setenv("PT_AMD_GROUP_THREADS", threads)
    with _VirtualGroup(gpu, vmap, collective) as g:
        assert g.collective == COLLECTIVE_NAME[collective]
        g.init(cornell, flags=gpu.PT_FLAG_TRACE_AHEAD, **FLAGS)
        for it in range(1, N_ITER + 1):
            g.iterate(it)
            _assert_frame(g.readback(), want, it - 1, vmap, "iteration %d" % it)
        assert int(g.counters().iterations) == N_ITER


# ---- b. call sequences that move the double buffer differently ----------------------------------------------------------------------------
def _no_assembly(gpu, g, collective, call):
    """`call` with the next reduce armed to fail: it succeeds only if it assembles nothing"""
    if collective == "reduce":
        assert gpu.test_lib().pt_test_group_fail_next_reduce(g.handle, 1) == 0
    try:
        return call()
    finally:
        assert gpu.test_lib().pt_test_group_fail_next_reduce(g.handle, 0) == 0


@pytest.mark.parametrize("collective", ["reduce", "host"])
@pytest.mark.parametrize("vmap", [MAPS[0], MAPS[2]], ids=_id)
def test_call_sequences(gpu, cornell, want, vmap, collective, monkeypatch):
    monkeypatch.setenv("PT_AMD_GROUP_THREADS", "1")
    with _VirtualGroup(gpu, vmap, collective) as g:
        g.init(cornell, flags=gpu.PT_FLAG_TRACE_AHEAD, **FLAGS)
        # two batches into ONE snapshot without a reduce between them
        g.iterate_batch(1, 4)
        g.iterate_batch(5, 4)
        _assert_frame(g.readback(), want, 7, vmap, "two iterate_batch calls, then readback")
        # two assemblies without a read-back between them
        g.iterate(9)
        g.iterate(10)
        _assert_frame(g.readback(), want, 9, vmap, "iterate twice, then readback")
        # a second read-back with nothing committed: the same frame, and nothing is assembled again
        _assert_frame(_no_assembly(gpu, g, collective, g.readback), want, 9, vmap, "readback twice in a row")
        # reduce twice in a row with nothing committed between them: the second one is no assembly
        g.iterate_batch(11, 1)
        g.reduce()
        _no_assembly(gpu, g, collective, g.reduce)
        _assert_frame(g.readback(), want, 10, vmap, "reduce twice in a row, then readback")
        g.sync()
        # sequence breaks under PT_FLAG_TRACE_AHEAD: a batch, then one iteration (which parks iterations 5 .. 12 traced ahead) ...
        g.init(cornell, flags=gpu.PT_FLAG_TRACE_AHEAD, **FLAGS)
        g.iterate_batch(1, 4)
        g.iterate(5)
        _assert_frame(g.readback(), want, 4, vmap, "iterate_batch(1, 4), iterate(5)")
        # ... then a batch the parked ones do not continue with: they are discarded, and a discarding commit writes no snapshot
        g.iterate_batch(6, 4)
        _assert_frame(g.readback(), want, 8, vmap, "iterate_batch(6, 4) over parked batches")
        g.iterate(10)
        g.iterate(11)
        _assert_frame(g.readback(), want, 10, vmap, "iterate(10), iterate(11) after the break")
        g.sync()
        _assert_frame(g.readback(), want, 10, vmap, "readback after sync")


# ---- c. re-initialisation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("collective", ["reduce", "host"])
def test_reinit_leaves_nothing_of_the_earlier_frames(gpu, cornell, want, collective, monkeypatch):
    monkeypatch.setenv("PT_AMD_GROUP_THREADS", "1")
    vmap = [0, 1, 1]
    sm = _scene(gpu, "mesh_small.txt", (96, 64))
    wm, _ = _single(gpu, sm, [(1, 2), (3, 2)], max_batch=2)
    with _VirtualGroup(gpu, vmap, collective) as g:
        g.init(cornell, flags=gpu.PT_FLAG_TRACE_AHEAD, **FLAGS)
        for it in range(1, 4):                                      # both snapshots written and reduced, the result frame too
            g.iterate(it)
        _assert_frame(g.readback(), want, 2, vmap, "first render")
        g.init(sm, max_batch=2)                                     # another scene at another resolution, with a mesh
        g.iterate_batch(1, 2)
        g.reduce()
        g.iterate_batch(3, 2)
        _assert_frame(g.readback(), (wm,), 0, vmap, "second scene", shape=(64, 96))
        g.init(cornell, flags=gpu.PT_FLAG_TRACE_AHEAD, **FLAGS)    # the first scene again: full, snap[] and the result frame start from zero
        for it in range(1, 6):
            g.iterate(it)
            _assert_frame(g.readback(), want, it - 1, vmap, "third render, iteration %d" % it)


# ---- d. a failed reduce on a multi-rank group ---------------------------------------------------------------------------------------------
def test_a_failed_reduce_on_two_ranks(gpu, cornell, want, monkeypatch):
    # the snapshot index does not advance on a failure, and the members' pending waits for evRed survive it
    monkeypatch.setenv("PT_AMD_GROUP_THREADS", "1")
    vmap = [0, 1]
    fail_next = gpu.test_lib().pt_test_group_fail_next_reduce
    with _VirtualGroup(gpu, vmap, "reduce") as g:
        g.init(cornell, flags=gpu.PT_FLAG_TRACE_AHEAD, **FLAGS)
        g.iterate_batch(1, 4)
        assert fail_next(g.handle, 1) == 0
        with pytest.raises(gpu.PtError, match="ncclReduce failed"):
            g.readback()
        _assert_frame(g.readback(), want, 3, vmap, "the retry after one failed reduce")
        g.iterate_batch(5, 4)
        assert fail_next(g.handle, 2) == 0
        for _ in range(2):
            with pytest.raises(gpu.PtError, match="ncclReduce failed"):
                g.reduce()
        g.reduce()
        _assert_frame(g.readback(), want, 7, vmap, "the third reduce after two failed ones")
        for it in (9, 10):
            g.iterate(it)
            _assert_frame(g.readback(), want, it - 1, vmap, "iteration %d after the failures" % it)


# ---- e. counters ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vmap,collective", [(MAPS[1], "reduce"), (MAPS[2], "host")], ids=["reduce-0.1.2", "host-0.0.1"])
def test_counters_are_the_one_renderer_tallies(gpu, cornell, vmap, collective, monkeypatch):
    monkeypatch.setenv("PT_AMD_GROUP_THREADS", "1")
    whole, cnt = _single(gpu, cornell, [(1, 3), (4, 3)], max_batch=3)
    with _VirtualGroup(gpu, vmap, collective) as g:
        g.init(cornell, max_batch=3)
        g.iterate_batch(1, 3)
        g.iterate_batch(4, 3)
        _assert_frame(g.readback(), (whole,), 0, vmap, "two batches of three")
        c = g.counters()
        assert [int(c.live[d]) for d in range(1, 9)] == [int(cnt.live[d]) for d in range(1, 9)]
        assert int(c.iterations) == 6 == int(cnt.iterations)
        assert int(c.light_hits) == int(cnt.light_hits)


# ---- f. the emulation itself, held to a plain reference -----------------------------------------------------------------------------------
def _special_columns(ranks):
    """element values per rank whose fp32 sum depends on the start value, the order and the rounding of every addition"""
    r = np.arange(ranks)
    f32 = np.float32
    one_then = lambda first, rest: np.where(r == 0, f32(first), f32(rest)).astype(np.float32)
    cols = [
        np.full(ranks, -0.0, np.float32),                                        # -0 + -0 = -0: a sum that starts from +0 gives +0
        np.where(r % 2 == 0, f32(-0.0), f32(0.0)).astype(np.float32),            # -0 + +0 = +0
        (f32(1e-45) * (r + 1)).astype(np.float32),                               # denormals that stay denormal
        one_then(1.0, 2.0 ** -24),                                               # 1 + ulp/2 rounds to even every time: 1, whatever the rank count
        np.where(r < 2, f32(2.0 ** -24), f32(1.0)).astype(np.float32),           # ... the small ones first: they survive
        one_then(16777216.0, 1.0),                                               # 2^24 + 1 rounds back
        np.where(r == 0, f32(1e30), np.where(r == 1, f32(-1e30), f32(1.0))).astype(np.float32),     # cancellation before the small terms
        np.where(r == 0, f32(1.17549435e-38), np.where(r == 1, f32(-1e-45), f32(0.0))).astype(np.float32),   # a normal that becomes a denormal
        one_then(3.0e38, 1.0e38),                                                # overflow to +inf on the way
    ]
    return np.stack(cols, axis=1)                                                # (ranks, columns)


def _reduce_inputs(rng, ranks, count, rotate):
    mag = np.exp2(rng.uniform(-30, 30, (ranks, count))) * rng.uniform(1, 2, (ranks, count))
    x = (mag * rng.choice([-1.0, 1.0], (ranks, count))).astype(np.float32)
    kind = rng.random((ranks, count))
    x[kind < 0.05] = 0.0
    x[(kind >= 0.05) & (kind < 0.08)] = -0.0
    den = (kind >= 0.08) & (kind < 0.15)
    x[den] = (rng.integers(1, 1 << 23, (ranks, count)).astype(np.uint32).view(np.float32) * rng.choice([-1.0, 1.0], (ranks, count)).astype(np.float32))[den]
    spec = np.roll(_special_columns(ranks), -rotate, axis=1)
    k = min(count, spec.shape[1])
    x[:, :k] = spec[:, :k]
    return x


@pytest.mark.parametrize("ranks", [1, 2, 3, 8])
def test_emulated_reduce_is_the_fp32_sum_in_rank_order(gpu, ranks):
    rng = np.random.default_rng(20 + ranks)
    case = 0
    with np.errstate(over="ignore"):
        for count in (1, 3, 255, 256, 257, 3 * W * H):
            for in_place in (False, True):
                x = _reduce_inputs(rng, ranks, count, case)
                case += 1
                ref = x[0].copy()
                for r in range(1, ranks):
                    ref = ref + x[r]                                             # numpy's fp32 addition, left to right
                assert ref.dtype == np.float32
                recv, after = gpu.test_emulated_reduce(list(x), in_place=in_place)
                what = "%d ranks, %d floats, %s" % (ranks, count, "in place" if in_place else "out of place")
                wrong = np.flatnonzero(recv.view(np.uint32) != ref.view(np.uint32))
                assert wrong.size == 0, "%s: %d wrong sums, the first at %d: %r, not %r (inputs %r)" % (
                    what, wrong.size, wrong[0], float(recv[wrong[0]]), float(ref[wrong[0]]), x[:, wrong[0]].tolist())
                for r in range(ranks):
                    keep = ref if (r == 0 and in_place) else x[r]                # the root's in-place buffer IS the result; every other is untouched
                    assert np.array_equal(after[r].view(np.uint32), keep.view(np.uint32)), "%s: rank %d's send buffer changed" % (what, r)
