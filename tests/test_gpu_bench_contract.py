"""bench.py prints ONE JSON line with the contract's keys: a plain run the headline's (metric, value, ms_per_step, ...), a `--full` run
everything else beside them (roofline, cpu_baseline, the other configurations, ...)."""
import json
import os
import subprocess
import sys
import time

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_bench_json_contract(pt, tmp_path):
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    dump, dump_c3 = str(tmp_path / "frame.npy"), str(tmp_path / "frame_c3.npy")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "3", "--warmup", "1", "--cpu-spp", "1", "--repeats", "5",
                        "--dump-frame", dump, "--dump-c3-frame", dump_c3],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["metric"] == "Mpaths/sec (paths = pixels x bounces x spp) at 1280x720, 8 bounces"
    assert d["unit"] == "Mpaths/s" and d["dtype"] == "f32" and d["data"] == "synthetic" and d["vs_baseline"] is None
    assert "workload" in d["config"] and "model" not in d["config"]
    # one step = one wavefront batch of 64 iterations of the whole frame = BASELINE config C2 (64 spp) in full
    assert d["config"]["iterations_per_step"] == 64 and d["config"]["paths_per_step_nominal"] == 1280 * 720 * 8 * 64
    assert abs(d["value"] - 1280 * 720 * 8 * 64 / (d["ms_per_step"] * 1e-3) / 1e6) / d["value"] < 0.01
    assert d["value"] > 1000.0                                   # north star: >= 1.0 Gpaths/s
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-4 and 0 < rf["frac"] < 1
    # every timed launch carries a full batch, so the committed PMC figures describe the launches that were timed:
    # measured HBM traffic within 25 % of the algorithmic bytes, and the kernel cannot beat its own VALU issue bound
    assert rf["iterations_per_launch"] == 64 and rf["launches"] == 3 * 8
    # the pipelined effective rate stands beside the per-launch fraction, labelled: same bytes over the headline pass's ms_per_step
    assert 0 < rf["frac_pipelined"] < 1
    assert abs(rf["frac_pipelined"] - rf["algorithmic_bytes_per_launch"] * 8 / (d["ms_per_step"] * 1e-3) / 8e12) < 0.02 * rf["frac_pipelined"]
    if rf["traffic"] is not None:
        assert 0.9 < rf["traffic_over_algorithmic"] < 1.25
        assert 0 < rf["valu"]["frac_of_issue_bound"]["v_fma_f32"] < 1
    # the timed block of exactly `steps` steps is repeated inside the run: the median block's wall is the line's, the spread beside it
    assert d["repeats"] == 5 and len(d["ms_per_step_blocks"]) == 5
    assert d["ms_per_step"] == sorted(d["ms_per_step_blocks"])[2]
    assert d["ms_per_step_min"] == min(d["ms_per_step_blocks"]) and d["ms_per_step_max"] == max(d["ms_per_step_blocks"])
    assert d["value_min"] <= d["value"] <= d["value_max"]
    # the line says what the box it ran on does on a fixed job (boxes of the pool differ by up to 1.8x)
    assert d["box_calibration"]["result_checked"] is True and d["box_calibration"]["algorithmic_GBps"] > 500
    # ... and what its clocks, power and temperature were WHILE the timed blocks ran (a slow line is attributable without a second run)
    tm = d["box_calibration"]["telemetry_during_timed_blocks"]
    assert "error" not in tm, tm
    assert tm["samples"] >= 1 and tm["power_cap_w"] > 0      # (5 blocks of 3 steps are ~30 ms; a hwmon read takes milliseconds)
    for k in ("sclk_mhz", "mclk_mhz", "power_w", "temp_junction_c"):
        assert tm[k]["min"] <= tm[k]["median"] <= tm[k]["max"] and tm[k]["max"] > 0, k
    assert 100 <= tm["sclk_mhz"]["max"] <= 3000 and tm["power_w"]["max"] <= 1.1 * tm["power_cap_w"]
    # BASELINE config C3 AS WRITTEN -- one pt_iterate + one reduce(sum) of zero-padded full frames per iteration -- measured at N = 1
    # as well, through a one-rank RCCL group, over the same number of steps, as the overlapped fast path
    c3 = d["value_c3_as_written"]
    assert "error" not in c3, c3
    assert c3["steps"] == 3 and c3["iterations_per_step"] == 64 and c3["value"] > 1000.0
    assert "reduce per iteration" in c3["mode"] and "RCCL" in c3["collective_backend"] and "one-rank" in c3["collective_backend"]
    assert c3["collective_bytes_per_call"] == 1280 * 720 * 12
    assert abs(c3["ms_per_iteration"] - c3["ms_per_step"] / 64) < 1e-3 and c3["ms_per_iteration"] < 0.2
    # its frame (what the LAST reduce delivered: warm-up step + 3 steps = 256 iterations) against the batched render of the same iterations
    import numpy as np
    got = np.load(dump_c3)
    sc = pt.Scene(os.path.join(ROOT, "scenes", "cornell.txt"))
    sc.set_resolution(1280, 720)
    pt.pathtraceFree()
    pt.pathtraceInit(sc, traceDepth=8, pipeline_depth=2, max_batch=64)
    for it in range(1, 257, 64):
        pt.pathtrace_batch(None, 0, it, 64)
    want = pt.readback(1280 * 720)
    pt.pathtraceFree()
    assert want.max() > 0 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] == 1 and cb["value"] > 0 and "sample" in cb
    assert cb["cpu_model"] and cb["host_cores"] >= 1 and cb["pinned_to_core"] is not None
    # BASELINE config C1 (sphere.txt 400x400, 1 spp, depth 4) on the CPU, in full
    assert cb["c1"]["value"] > 0 and cb["c1"]["runs"] == 15 and "400x400" in cb["c1"]["config"]


def test_driver_command_reports_every_one_gpu_configuration(pt):
    # round 5: `python bench.py --full` with nothing but --steps / --warmup carries, beside
    # the headline C2 line, a `configs` block: C4, C5 on one of its eight GPUs and the mesh scene, each measured by a child bench.py of its
    # own and each with a roofline priced against the bound SURVEY 8d names (C5: the vector units)
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "4", "--warmup", "2"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["steps"] == 4 and d["warmup"] == 2 and "cpu_baseline" in d and "roofline" in d
    cf = d["configs"]
    assert sorted(cf) == ["c4", "c5_one_gpu", "mesh"] and d["configs_failed"] == []      # (a failed child block is named at the top level)
    for k, v in cf.items():
        assert "error" not in v, (k, v)
        assert v["unit"] == "Mpaths/s" and v["value"] > 1000.0 and v["value_min"] <= v["value"] <= v["value_max"]
        assert v["roofline"]["launches"] > 0 and v["roofline"]["avg_launch_ms"] > 0
    assert "cornell_glass.txt 1920x1080, 16 bounces" in cf["c4"]["workload"] and cf["c4"]["roofline"]["bound"] == "hbm"
    assert "spheres64.txt 4096x4096, 8 bounces, 16 spp per step" in cf["c5_one_gpu"]["workload"]
    assert "cornell_mesh.txt 1280x720" in cf["mesh"]["workload"] and cf["mesh"]["roofline"]["bound"] == "hbm"
    rf = cf["c5_one_gpu"]["roofline"]
    assert rf["bound"] == "valu_fp32" and rf["unit"] == "TFLOP/s" and rf["peak"] == 157.3
    # (the committed counters of that very configuration: profiles/pmc_configs.json)
    assert rf["frac"] is not None and 0.3 < rf["frac"] < 1.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    assert rf["hbm"]["unit"] == "GB/s" and 0 < rf["hbm"]["frac"] < 1
    # (the mesh scene's launch is the pair k_mesh_walk + k_bounce: the walk reads the rays of the tiles that list a mesh once more and leaves an
    # 8-byte record per path, which the algorithmic figure -- the path state in and out, as for every configuration -- does not count)
    for k, hi in (("c4", 1.6), ("mesh", 1.7)):      # (mesh: 1.59-1.60 measured in rounds 5 and 6; round 5 had loosened the bound to 2.0)
        assert cf[k]["roofline"]["traffic"] is not None and 0.9 < cf[k]["roofline"]["traffic_over_algorithmic"] < hi
    # round 6: the C ABI's own multi-device host path is IN the driver's line.  Eight members on the one device
    # (a host thread each, one shared accumulator) against the headline; config C3 as written through the LIBRARY's per-iteration reduce
    # (one member, a one-rank RCCL communicator: snapshot fused into the commit, ncclReduce on the collective stream), the
    # torch.distributed reading of rounds 4-5 beside it
    g8 = d["group_8_members_one_device"]
    assert "error" not in g8, g8
    assert g8["members"] == 8 and g8["devices"] == 1 and g8["issue_threads"] == 8 and g8["collective"] == "shared accumulator"
    assert g8["iterations_per_step"] == 64 and g8["iterations_per_wavefront_batch"] == 256 and g8["value"] > 1000.0
    assert abs(g8["of_the_one_context_rate"] - g8["value"] / d["value"]) < 1e-3 and g8["of_the_one_context_rate"] > 0.8
    assert g8["host_enqueue_us_per_wavefront_batch"] < 1e3 * g8["gpu_ms_per_wavefront_batch"]     # the host is not what bounds it
    c3 = d["value_c3_as_written"]
    assert "error" not in c3, c3
    assert c3["members"] == 1 and c3["collective"].startswith("rccl reduce") and "one-rank" in c3["collective"]
    assert c3["iterations_per_step"] == 64 and c3["steps"] == 4 and 0 < c3["ms_per_iteration"] < 0.2
    assert "pt_group_iterate per iteration" in c3["mode"]
    assert "error" not in d["value_c3_as_written_torch_distributed"] and "unmeasured" in d["multi_device_note"]
    # a run that is about ONE configuration carries no block
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "2", "--warmup", "1", "--cpu-spp", "0", "--per-iteration-sample", "0",
                        "--repeats", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "configs" not in json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_plain_run_times_the_headline_alone(pt, tmp_path):
    # a plain `bench.py --gpus 1 --steps K --warmup W` does what its headline needs and nothing more: no extra pass, no child process, no CPU
    # baseline -- at most 30 s of the whole run's wall outside its warm-up and timed steps
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    steps, warmup = 3, 1
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=600)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == "Mpaths/sec (paths = pixels x bounces x spp) at 1280x720, 8 bounces"
    assert d["unit"] == "Mpaths/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == steps and d["warmup"] == warmup and d["repeats"] == 1 and d["ms_per_step"] == d["ms_per_step_blocks"][0] > 0
    assert abs(d["value"] - 1280 * 720 * 8 * 64 / (d["ms_per_step"] * 1e-3) / 1e6) / d["value"] < 0.01 and d["value"] > 1000.0
    for k in ("roofline", "cpu_baseline", "box_calibration", "value_c3_as_written", "configs", "configs_failed", "group_8_members_one_device"):
        assert k not in d, k
    # the path tallies come from the headline pass's own blocks: every pixel the camera sees starts a path
    c = d["config"]
    assert len(c["live_per_bounce_per_iteration"]) == 8 and 0 < c["live_per_bounce_per_iteration"][0] <= 1280 * 720
    assert c["live_per_bounce_per_iteration"][-1] <= c["live_per_bounce_per_iteration"][0] and c["live_Msegments_per_s"] > 0
    assert sorted(os.listdir(tmp_path / "out")) == ["frame.npy"]
    assert wall - (steps + warmup) * d["ms_per_step"] * 1e-3 < 30.0, wall


def _batched_frame(pt, iterations):
    import numpy as np
    sc = pt.Scene(os.path.join(ROOT, "scenes", "cornell.txt"))
    sc.set_resolution(1280, 720)
    pt.pathtraceFree()
    pt.pathtraceInit(sc, traceDepth=8, pipeline_depth=2, max_batch=64)
    for it in range(1, iterations + 1, 64):
        pt.pathtrace_batch(None, 0, it, 64)
    want = pt.readback(1280 * 720)
    pt.pathtraceFree()
    assert want.max() > 0
    return want


def test_group_mode_renders_the_one_device_frame(pt, tmp_path):
    # `bench.py --group M`: what the `group` blocks of the driver's line run.  The frame each mode leaves is the batched one-renderer
    # frame of the same iterations, bit for bit: 8 members on the one device in wavefront batches of 256, and config C3 as written --
    # one pt_group_iterate per iteration -- through a one-rank RCCL communicator.
    import numpy as np
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "PT_AMD_COLLECTIVE", "PT_AMD_GROUP_THREADS"):
        env.pop(k, None)
    dump = str(tmp_path / "g8.npy")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--group", "8", "--group-devices", "1", "--steps", "4", "--warmup", "1",
                        "--repeats", "2", "--dump-frame", dump], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["members"] == 8 and d["devices"] == 1 and d["collective"] == "shared accumulator" and d["iterations_committed"] == (1 + 2 * 4) * 64
    assert d["iterations_per_wavefront_batch"] == 256 and d["value"] > 1000.0 and len(d["ms_per_step_blocks"]) == 2
    assert np.array_equal(np.load(dump).view(np.uint32), _batched_frame(pt, 9 * 64).view(np.uint32))
    dump = str(tmp_path / "c3.npy")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--group", "1", "--group-c3", "1", "--steps", "2", "--warmup", "1",
                        "--repeats", "2", "--dump-frame", dump], capture_output=True, text=True, timeout=600, env=dict(env, PT_AMD_COLLECTIVE="rccl"))
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["members"] == 1 and d["collective"].startswith("rccl reduce") and d["iterations_committed"] == (1 + 2 * 2) * 64
    assert 0 < d["ms_per_iteration"] < 0.2 and d["host_enqueue_us_per_iteration"] > 0
    assert np.array_equal(np.load(dump).view(np.uint32), _batched_frame(pt, 5 * 64).view(np.uint32))


def test_steps_and_dump_outputs(pt, tmp_path):
    # `--steps K` with no `--repeats`: exactly K timed steps, `ms_per_step` their wall / K.  `--dump-outputs DIR` leaves what the
    # headline pass computed by its last step -- the frame of warm-up + timed iterations -- as DIR/frame.npy, equal on a second run.
    import numpy as np
    if pt.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    frames = []
    for k in range(2):
        out = tmp_path / ("run%d" % k)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--cpu-spp", "0",
                            "--per-iteration-sample", "0", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert d["steps"] == 3 and d["repeats"] == 1 and len(d["ms_per_step_blocks"]) == 1
        assert d["ms_per_step"] == d["ms_per_step_blocks"][0] > 0
        assert sorted(os.listdir(out)) == ["frame.npy"]
        f = np.load(out / "frame.npy")
        assert f.dtype == np.float32 and f.shape == (720, 1280, 3)
        frames.append(f)
    assert np.array_equal(frames[0].view(np.uint32), frames[1].view(np.uint32))
    assert np.array_equal(frames[0].reshape(-1).view(np.uint32), _batched_frame(pt, (1 + 3) * 64).view(np.uint32))
