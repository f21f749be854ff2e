"""bench.py's command line: a plain run prints the headline only, --dump-outputs writes what the
last timed step left as float32 .npy files, --full is an option of its own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def test_parse_options(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2"])
    args = bench.parse()
    assert (args.steps, args.warmup, args.full, args.dump_outputs) == (3, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    args = bench.parse()
    assert args.full and args.dump_outputs == "d"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_dump_outputs_layout(tmp_path):
    """loss, parameters, gradients and running statistics, float32, in module order; names.json
    tiles each family's vector with the tensors' names."""
    import bench
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3, bias=True), torch.nn.BatchNorm2d(4)).double()
    loss = m(torch.randn(2, 3, 5, 5, dtype=torch.float64)).square().mean()
    loss.backward()
    out = str(tmp_path / "dump")
    bench.dump_outputs(out, loss, m)
    assert sorted(os.listdir(out)) == ["bn_running_stats.npy", "grads.npy", "loss.npy", "names.json",
                                       "params.npy"]
    arrays = {n: np.load(os.path.join(out, n + ".npy"))
              for n in ("loss", "params", "grads", "bn_running_stats")}
    assert all(a.dtype == np.float32 and a.ndim == 1 for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= bench.DUMP_LIMIT_BYTES
    params = list(m.named_parameters())
    want_p = np.concatenate([p.detach().numpy().ravel() for _, p in params]).astype(np.float32)
    want_g = np.concatenate([p.grad.numpy().ravel() for _, p in params]).astype(np.float32)
    assert np.array_equal(arrays["params"], want_p) and np.array_equal(arrays["grads"], want_g)
    assert np.array_equal(arrays["loss"], np.float32([loss.item()]))
    want_r = np.concatenate([m[1].running_mean.numpy(), m[1].running_var.numpy()])
    assert np.array_equal(arrays["bn_running_stats"], want_r.astype(np.float32))
    names = json.load(open(os.path.join(out, "names.json")))
    assert [r[0] for r in names["params"]] == [k for k, _ in params]
    assert names["params"][0][1] == 0 and names["params"][-1][2] == want_p.size
    assert all(a[2] == b[1] for a, b in zip(names["params"], names["params"][1:]))
    assert names["grads"] == names["params"]
    assert [r[0] for r in names["bn_running_stats"]] == ["1.running_mean", "1.running_var"]


@pytest.mark.gpu
def test_plain_run_prints_headline_and_dumps(tmp_path):
    """One small plain run: one JSON line with the headline keys and none of --full's objects,
    --steps timed steps, and the dump of the last step (finite, float32, the model's size)."""
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
                        "--warmup", "1", "--batch", "2", "--height", "96", "--width", "160",
                        "--dump-outputs", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert all(k in res for k in HEADLINE)
    assert res["steps"] == 2 and res["warmup"] == 1 and res["unit"] == "images/s"
    assert res["higher_is_better"] is True and res["dtype"] == "bf16"
    assert res["ms_per_step"] > 0
    assert abs(res["value"] - 2 / (res["ms_per_step"] * 1e-3)) <= 0.01 * res["value"]
    for k in ("roofline", "cpu_baseline", "forward_fp32", "kernel_ms_per_step_census",
              "step_ms_distribution", "train_fp16"):
        assert k not in res
    loss = np.load(os.path.join(out, "loss.npy"))
    assert loss.dtype == np.float32 and abs(float(loss[0]) - res["loss"]["final"]) < 1e-4
    for n in ("params", "grads"):
        a = np.load(os.path.join(out, n + ".npy"))
        assert a.dtype == np.float32 and a.shape == (1138051,) and np.isfinite(a).all()
    assert np.abs(np.load(os.path.join(out, "grads.npy"))).max() > 0
    assert np.isfinite(np.load(os.path.join(out, "bn_running_stats.npy"))).all()
