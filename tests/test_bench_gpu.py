"""bench.py on the GPU: the plain line, what --full adds, the optional baseline leg and --dump-outputs (the N > 1 paths are covered in
test_dist_gpu.py)."""
import json, os, subprocess, sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_bench_reports_the_torch_operator_baseline_when_asked():
    """--torch_gpu_baseline nchw: after the timed steps the oracle's train step runs on the same GPU through PyTorch-ROCm's own operators (eager,
    bf16 autocast) and is reported beside the line -- `torch_rocm_baseline`, a baseline like `cpu_baseline`; the line itself is unchanged."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--local_batch_size", "2", "--height", "128", "--width", "192",
           "--no_cpu_baseline", "--torch_gpu_baseline", "nchw"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    base = out["torch_rocm_baseline"]
    assert out["value"] > 0 and out["vs_baseline"] is None and "cpu_baseline" not in out
    assert base["value"] is not None and base["value"] > 0, base
    assert base["unit"] == "samples/s" and base["kind"] == "port" and "nchw" in base["sample"]
    assert abs(base["this_repository_over_it"] - out["value"] / base["value"]) < 0.01 * base["this_repository_over_it"] + 0.01


def test_plain_line_carries_the_headline_only():
    """Without --full the run is set-up, warm-up, the K timed steps and the line: no roofline passes, no `also`, no CPU baseline."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--height", "128", "--width", "192"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["config"]["local_batch"] == 8 and out["dtype"] == "bf16" and out["value"] > 0 and out["higher_is_better"] is True
    assert out["steps"] == 2 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["unit"] == "samples/s"
    assert out["roofline"] is None and "also" not in out and "cpu_baseline" not in out


def test_full_line_carries_the_other_single_gpu_configurations():
    """With --full, BASELINE.json configs[1] (local batch 2, fp32, Adam), configs[2] (local batch 4, bf16) and the per-rank shape of configs[3]
    (local batch 2, bf16) ride on the line as `also`: each timed in the
    same process the same way, with its whole-step and encoder-region fraction.  Small images here; the keys are what is asserted."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--height", "128", "--width", "192", "--no_cpu_baseline",
           "--full"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["config"]["local_batch"] == 8 and out["dtype"] == "bf16" and out["value"] > 0
    assert out["roofline"]["achieved"] > 0 and "encoder_region" in out["roofline"]
    also = out["also"]
    assert [(e["config"]["local_batch"], e["dtype"], e["config"]["optimizer"]) for e in also] == [(2, "fp32", "Adam"), (4, "bf16", "LAMB"), (2, "bf16", "LAMB")]
    for e in also:
        assert e["value"] > 0 and e["unit"] == "samples/s" and e["steps"] == 2 and e["warmup"] == 1, e
        assert abs(e["ms_per_step"] * e["value"] - 1e3 * e["config"]["local_batch"]) < 1.0
        assert 0 < e["whole_step_frac"] < 1 and 0 < e["encoder_region"]["frac"] < 1
        assert e["encoder_region"]["fwd_ms"] > 0 and e["encoder_region"]["bwd_ms"] > 0
        assert e["loss_last_step"] == e["loss_last_step"]      # finite
    # --no_also leaves the line as it was
    r = subprocess.run(cmd + ["--no_also"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "also" not in json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_dump_outputs_writes_the_last_timed_step_the_same_every_run(tmp_path):
    """--dump-outputs DIR: after the K timed steps the arrays the last one left (loss, the sampled master weights and gradients, BatchNorm
    buffers) land in DIR as float32 / float64 .npy files, 64 MB at most; the same arguments give the same inputs, so two runs give the same bits."""
    import numpy as np
    runs = []
    for name in ("a", "b"):
        d = tmp_path / name
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--local_batch_size", "2", "--height", "64",
               "--width", "96", "--no_cpu_baseline", "--no_also", "--dump-outputs", str(d)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert out["steps"] == 3 and out["ms_per_step"] > 0 and abs(out["ms_per_step"] * out["value"] - 2e3) < 1.0
        files = sorted(os.listdir(d))
        assert files == sorted(out["dump_outputs"]["files"]) and "loss.npy" in files and "params_sample.npy" in files
        assert sum(os.path.getsize(d / f) for f in files) <= 64 * 2 ** 20
        arrays = {f: np.load(d / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert abs(float(arrays["loss.npy"][0]) - out["loss_last_step"]) < 1e-6
        assert arrays["params_sample.npy"].size == 1 << 22 and np.isfinite(arrays["grads_sample.npy"]).all()
        assert (arrays["bn_num_batches_tracked.npy"] == 4).all()          # one warm-up + three timed steps, nothing after them
        runs.append(arrays)
    for f in runs[0]:
        if f == "loss.npy":      # a double-precision atomic sum (1e-16 jitter), as in test_model_gpu.py::test_train_step_is_bit_reproducible
            np.testing.assert_allclose(runs[0][f], runs[1][f], rtol=1e-12, atol=0)
        else:
            np.testing.assert_array_equal(runs[0][f], runs[1][f], err_msg=f)
