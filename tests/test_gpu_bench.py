"""bench.py as every change is measured with it: a plain run (`--gpus 1 --steps K --warmup W`) times the headline and nothing
else, and `--dump-outputs DIR` writes what the last timed step computed -- the same values however many untimed steps (clock
ramp, warm-up) ran before the timed ones, so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _bench(args, timeout=300):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["train", "infer"])
def test_plain_run_dumps_its_last_step_reproducibly(tmp_path, mode):
    common = ["--gpus", "1", "--case", "14", "--batch", "16", "--mode", mode, "--steps", "5"]
    a = _bench(common + ["--warmup", "2", "--clock-ramp-ms", "0", "--dump-outputs", str(tmp_path / "a")])
    b = _bench(common + ["--warmup", "7", "--clock-ramp-ms", "100", "--dump-outputs", str(tmp_path / "b")])
    for d in (a, b):
        assert d["steps"] == 5 and d["ms_per_step"] > 0 and d["value"] > 0 and d["higher_is_better"] is True
        assert d["dtype"] == "f32" and d["unit"] == "graphs/s" and d["metric"].startswith("graphs/sec")
        # nothing beyond the headline was measured
        assert d["roofline"] is None and d["kernels"] == {} and d["cpu_baseline"] is None and d["scatter_add"] is None
        assert d["median_ms_per_step"] is None and "other_configs" not in d and "eager_ms_per_step" not in d
    assert a["clock_ramp_steps"] == 0 and b["clock_ramp_steps"] > 0
    names = {"output", "loss", "params"} if mode == "train" else {"output"}
    assert {f[:-4] for f in os.listdir(tmp_path / "a")} == names
    for n in names:
        x, y = np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy")
        assert x.dtype == np.float32 and np.isfinite(x).all(), n
        assert np.array_equal(x, y), f"{n}: max diff {np.abs(x - y).max()}"
    assert np.load(tmp_path / "a" / "output.npy").shape == (16 * 14, 4)
    if mode == "train":
        assert float(np.load(tmp_path / "a" / "loss.npy")[0]) == a["final_loss"]     # the dump is the LAST timed step


def test_dump_outputs_stays_within_its_budget(tmp_path, monkeypatch):
    """Arrays that together exceed the budget are written as a fixed (seeded) sample of each; smaller ones as they are."""
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4096)
    big = torch.arange(3000, dtype=torch.float64).view(1000, 3)
    arrays = {"big": big, "small": torch.ones(7), "loss": torch.tensor(0.25)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 4096 + 3 * 128                                               # (+ the .npy headers)
    s = np.load(tmp_path / "a" / "big.npy")
    assert s.dtype == np.float32 and s.shape == (4096 // (4 * 3),) and np.all(np.diff(s) > 0)   # sorted sample of the entries
    assert np.array_equal(s, np.load(tmp_path / "b" / "big.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), np.ones(7, np.float32))
    assert np.load(tmp_path / "a" / "loss.npy").tolist() == [0.25]
