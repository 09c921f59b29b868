"""bench.py's host side without a GPU: the arguments that fix how many steps are timed, and the arrays `--dump-outputs` writes."""
import importlib
import os

import numpy as np


def _bench(monkeypatch):
    # (bench.py sets an HSA variable at import; the rest of the session keeps its own environment)
    monkeypatch.delenv("HSA_ENABLE_IPC_MODE_LEGACY", raising=False)
    import bench
    return importlib.reload(bench)


def test_steps_is_the_number_of_timed_steps(monkeypatch):
    b = _bench(monkeypatch)
    a = b.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and a.repeats == 1 and a.dump_outputs is None
    assert b.parse(["--dump-outputs", "out"]).dump_outputs == "out"


def test_dump_outputs_whole_frame(monkeypatch, tmp_path):
    b = _bench(monkeypatch)
    W, H = 5, 3
    frame = np.arange(W * H * 3, dtype=np.float32)
    b.dump_outputs(str(tmp_path / "d"), frame, W, H)
    assert sorted(os.listdir(tmp_path / "d")) == ["frame.npy"]
    got = np.load(tmp_path / "d" / "frame.npy")
    assert got.dtype == np.float32 and got.shape == (H, W, 3)
    assert np.array_equal(got.reshape(-1), frame)


def test_dump_outputs_samples_a_large_frame_the_same_way_every_time(monkeypatch, tmp_path):
    b = _bench(monkeypatch)
    monkeypatch.setattr(b, "DUMP_MAX_BYTES", 4000)
    W, H = 64, 32
    frame = np.random.default_rng(1).random(W * H * 3, dtype=np.float32)
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), frame, W, H)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["frame_sample.npy", "frame_sample_pixels.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 4000 + 2 * 128      # (+ the two .npy headers)
    for n in names:
        assert np.array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n))
    vals, pix = np.load(tmp_path / "a" / names[0]), np.load(tmp_path / "a" / names[1])
    assert vals.dtype == np.float32 and pix.dtype == np.float64 and len(vals) == len(pix) == 4000 // 20
    assert np.all(np.diff(pix) > 0) and pix[-1] < W * H
    assert np.array_equal(vals, frame.reshape(-1, 3)[pix.astype(np.int64)])


def test_full_is_off_by_default(monkeypatch):
    b = _bench(monkeypatch)
    assert b.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"]).full is False
    assert b.parse(["--full"]).full is True


def test_what_only_a_full_run_measures_needs_full():
    # (a plain run would silently leave the file unwritten or the blocks unmeasured; it refuses before touching the GPU)
    import subprocess
    import sys
    from conftest import ROOT
    for extra in (["--dump-c3-frame", "c3.npy"], ["--configs", "1"], ["--group-blocks", "1"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0"] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and "--full" in r.stderr, (extra, r.stderr[-2000:])
        assert not [l for l in r.stdout.splitlines() if l.startswith("{")]
