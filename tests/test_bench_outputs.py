"""bench.py --dump-outputs / --full: the writer on CPU tensors, and on the GPU
one small plain run and one --full run of the config-3 bench as a process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_whole_array(tmp_path):
    import bench
    t = torch.arange(24, dtype=torch.bfloat16).reshape(2, 3, 4)
    bench.dump_outputs(str(tmp_path / "d"), {"y": t})
    a = np.load(tmp_path / "d" / "y.npy")
    assert a.dtype == np.float32 and a.shape == (2, 3, 4)
    assert np.array_equal(a, t.float().numpy())


def test_dump_outputs_samples_a_large_array_the_same_way_every_time(tmp_path, monkeypatch):
    """Beyond the byte budget each array is written as the same sorted sample
    of its flattened elements, and the arrays share the budget."""
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 4 * 200)
    x = torch.randn(37, 29, generator=torch.Generator().manual_seed(3))
    small = torch.ones(5)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"x": x, "small": small})
    a, b = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "b" / "x.npy")
    assert a.dtype == np.float32 and a.shape == (100,) and np.array_equal(a, b)
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small.numpy())
    # a sample of x in order: every value occurs in x, at increasing positions
    flat = x.reshape(-1).numpy()
    pos = -1
    for v in a:
        nxt = np.nonzero(flat[pos + 1:] == v)[0]
        assert nxt.size, "sampled value not found after the previous one"
        pos += 1 + int(nxt[0])
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 4 * 200 + 2 * 128  # the data budget + one .npy header each


def _bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "2", *argv],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_encoder_output(dev, tmp_path):
    res = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0
    assert res["unit"] == "audio-sec/sec" and res["higher_is_better"] is True and res["dtype"] == "bf16"
    # value and ms_per_step state the same time: 2 utterances x 15 s per step
    assert res["value"] == pytest.approx(2 * 15.0 / (res["ms_per_step"] * 1e-3), rel=1e-3)
    assert "roofline" not in res and "cpu_baseline" not in res
    assert os.listdir(tmp_path) == ["encoder_out.npy"]
    y = np.load(tmp_path / "encoder_out.npy")
    assert y.dtype == np.float32 and y.shape == (2, res["config"]["seq_len"], 256)
    assert np.isfinite(y).all() and np.abs(y).max() > 0
    # the same seeded weights and input through the same step in this process
    import bench
    fbank, cnn, tr = bench.build_model(256, dev)
    wav = (0.1 * torch.randn(2, int(bench.SR * bench.SECONDS), generator=torch.Generator().manual_seed(1234))).to(dev)
    ref = bench.make_step(fbank, cnn, tr, wav, torch.ones(2, device=dev))()
    assert np.array_equal(y, ref.float().cpu().numpy())


@pytest.mark.gpu
def test_full_run_adds_the_roofline(dev):
    res = _bench("--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline")
    assert res["steps"] == 3 and res["ms_per_step"] > 0
    assert res["roofline"]["unit"] == "TFLOP/s" and res["roofline"]["achieved"] > 0
    assert "cpu_baseline" not in res
