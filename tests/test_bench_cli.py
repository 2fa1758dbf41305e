"""bench.py launch contract: ``--gpus N`` must mean N ranks -- it starts them itself when no launcher did, and it
fails loudly, before touching the GPU, when the node has fewer than N devices or the launcher started a different number of ranks."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, env_extra=None, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PSSR_BENCH_FORCE_DEVICE")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout)


def test_gpus_n_without_n_devices_fails_loudly():
    import torch
    n = torch.cuda.device_count() + 1 if torch.cuda.device_count() >= 1 else 2
    r = _bench(["--gpus", str(n), "--steps", "1", "--tiles", "64"])
    assert r.returncode == 2, (r.returncode, r.stderr[-500:])
    assert f"needs {n} devices" in r.stderr
    assert '"n_gpus"' not in r.stdout            # no bench line claiming GPUs it never used


def test_gpus_disagreeing_with_launcher_fails():
    r = _bench(["--gpus", "2", "--steps", "1", "--tiles", "0", "--mode", "sheet"], env_extra={"WORLD_SIZE": "1", "RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=1" in (r.stderr + r.stdout)


import pytest


@pytest.mark.gpu
def test_rdresunet_batch4_strong_scaling_shape():
    """the per-rank shape of c3 under strong scaling on 8 GPUs (batch 32 / 8 = 4): the small-grid kernel selection of the
    RDResUNet step is exercised on one GPU before an 8-GPU node sees it -- capture, replay and a finite loss-bearing bench line."""
    import json
    r = _bench(["--model", "rdresunet", "--crappifier", "poisson", "--batch", "4", "--steps", "3", "--warmup", "3", "--tiles", "64",
                "--no-extras", "--no-cpu-baseline", "--tile-workers", "4"], timeout=400)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith('{"metric"')][0])
    assert d["value"] > 0 and d["config"]["global_batch"] == 4 and d["config"]["launch"].startswith("hipGraph")
    assert d["layerwise_bound"]["tiles_per_s"] == 6000.0


def test_steps_below_one_is_refused():
    r = _bench(["--steps", "0", "--tiles", "0", "--mode", "sheet"])
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr


def test_dump_outputs_stays_within_budget_and_is_fixed():
    """bench.dump_outputs: small arrays whole, large ones a seeded sample (the same one every time), float32 / float64, 64 MB at most."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench

    def write(path):
        g = torch.Generator().manual_seed(3)
        bench.dump_outputs(str(path), {"big": (torch.rand(40_000_000, generator=g), None), "capped": (torch.rand(3_000_000, generator=g), 1000),
                                       "small": (torch.rand(2, 3, generator=g).to(torch.bfloat16), None),
                                       "loss": (torch.tensor([0.25], dtype=torch.float64), None)})
        return {f.stem: np.load(f) for f in sorted(path.iterdir())}

    import tempfile
    from pathlib import Path
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        one, two = write(Path(a)), write(Path(b))
        total = sum(f.stat().st_size for f in Path(a).iterdir())
    assert sorted(one) == ["big", "capped", "loss", "small"] and total <= 64_000_000
    assert one["small"].shape == (2, 3) and one["small"].dtype == np.float32
    assert one["loss"].dtype == np.float64 and one["loss"].tolist() == [0.25]
    assert one["capped"].ndim == 1 and 990 <= one["capped"].size <= 1000
    assert one["big"].dtype == np.float32 and one["big"].size > 10_000_000
    for k in one:
        np.testing.assert_array_equal(one[k], two[k])


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    """A plain run (no --full) times exactly --steps steps and prints the headline line only; --dump-outputs writes the last timed step's
    prediction, input, loss and weights, and a second run with the same arguments writes the same arrays."""
    import json
    import numpy as np
    args = ["--gpus", "1", "--steps", "2", "--warmup", "3", "--tiles", "256", "--tile-workers", "4"]
    outs = []
    for i in range(2):
        r = _bench(args + ["--dump-outputs", str(tmp_path / str(i))], timeout=400)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
        assert len(lines) == 1, r.stdout[-1000:]
        d = json.loads(lines[0])
        assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0 and d["higher_is_better"] is True and d["dtype"] == "bf16"
        assert not {"roofline", "roofline_hbm", "cpu_baseline", "infer", "sheet", "f32_train", "comm"} & set(d)
        files = sorted((tmp_path / str(i)).iterdir())
        assert [f.name for f in files] == ["buffers.npy", "hr_hat.npy", "loss.npy", "lr.npy", "params.npy"]
        assert sum(f.stat().st_size for f in files) <= 64_000_000
        outs.append({f.stem: np.load(f) for f in files})
    a, b = outs
    assert a["hr_hat"].shape == (32, 1, 512, 512) and a["lr"].shape == (32, 1, 128, 128) and a["hr_hat"].dtype == np.float32
    assert a["loss"].dtype == np.float64 and np.isfinite(a["loss"]).all() and np.isfinite(a["params"]).all()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
