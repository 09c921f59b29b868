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
