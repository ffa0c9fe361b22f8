"""bench.py's rank launcher and DP protocol on the CPU (no GPU needed).

The driver runs ``python bench.py --gpus N`` with no launcher: bench.py must start the N rank
processes itself (before any GPU call), report ``n_gpus == N`` and fail when a rank fails.  The
ranks run the train_image.py step (train_image.py:93-144, the one exchange step being the
gradient all-reduce of :139-144) through the gloo backend on CPU tensors at a small size."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, extra_env=None, timeout=600):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(MHADA_BENCH_BACKEND="gloo", OMP_NUM_THREADS="2")
    env.update(extra_env or {})
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, cwd=REPO, env=env,
                          capture_output=True, text=True, timeout=timeout)


def _json_lines(out):
    return [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]


# two images per rank: each rank's micro-batch is one coupled forward call
SMALL = ["--train", "--device", "cpu", "--train-res", "64", "--train-batch", "2", "--steps", "1", "--warmup", "0"]


def test_gpus_2_self_launches_two_ranks(tmp_path):
    p = _run(["--gpus", "2", "--dump-outputs", str(tmp_path)] + SMALL)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = _json_lines(p.stdout)
    assert len(lines) == 1, p.stdout  # rank 0 only
    r = lines[0]
    assert r["n_gpus"] == 2
    assert r["config"]["global_batch"] == 4 and r["config"]["backend"] == "gloo"
    ag = r["rank_agreement"]
    assert ag["identical"] and ag["world"] == 2 and ag["backend"] == "gloo", ag
    assert all(v == v for v in r["last_losses"].values())  # finite (not NaN)
    # --dump-outputs: rank 0 alone wrote the last step's losses, float64, in sorted key order
    assert sorted(os.listdir(tmp_path)) == ["losses.npy"]
    dumped = np.load(tmp_path / "losses.npy")
    assert dumped.dtype == np.float64
    assert dumped.tolist() == [r["last_losses"][k] for k in sorted(r["last_losses"])]


def test_world_size_must_match_gpus():
    p = _run(["--gpus", "2"] + SMALL, extra_env={"WORLD_SIZE": "1", "RANK": "0"})
    assert p.returncode != 0
    assert "WORLD_SIZE=1 but --gpus 2" in p.stderr


def test_failing_rank_fails_the_job():
    # a resolution the ViT rejects (not a multiple of the patch size) makes every rank raise;
    # the parent must exit non-zero instead of printing a line
    p = _run(["--gpus", "2", "--train", "--device", "cpu", "--train-res", "60", "--train-batch", "1",
              "--steps", "1", "--warmup", "0"], timeout=300)
    assert p.returncode != 0
    assert not _json_lines(p.stdout)


@pytest.mark.parametrize("argv", [["--gpus", "2", "--device", "cpu", "--steps", "1"]])
def test_cpu_device_is_training_only(argv):
    p = _run(argv, timeout=120)
    assert p.returncode != 0


def test_dump_outputs_whole_and_sampled(tmp_path):
    """bench.dump_outputs: an array within its share of the budget is written whole (float32, its
    own shape), a larger one as the same stratified sample in every call, and the files together
    stay within the budget."""
    sys.path.insert(0, REPO)
    import bench
    g = torch.Generator().manual_seed(3)
    small = torch.rand(2, 3, 5, 7, generator=g).to(torch.bfloat16)
    big = torch.rand(4, 1001, 13, generator=g)  # 52052 elements, no multiple of the stride
    f64 = torch.rand(9, generator=g, dtype=torch.float64)
    budget = 3 * 4 * 6000  # share: 6000 float32 elements per array -> stride 9, 5783 samples of big
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"small": small, "big": big, "f64": f64}, budget=budget)
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("small", "big", "f64")}
    assert a["small"].dtype == np.float32 and a["small"].shape == (2, 3, 5, 7)
    assert np.array_equal(a["small"], small.float().numpy())
    assert a["f64"].dtype == np.float64 and np.array_equal(a["f64"], f64.numpy())
    assert a["big"].dtype == np.float32 and a["big"].shape == (52052 // 9,)
    # one element of every 9 consecutive ones, in order
    flat = big.reshape(-1).numpy()
    blocks = flat[: 5783 * 9].reshape(5783, 9)
    assert (blocks == a["big"][:, None]).any(axis=1).all()
    assert not np.array_equal(a["big"], blocks[:, 0])  # seeded offsets, not a plain stride
    assert np.array_equal(a["big"], np.load(tmp_path / "b" / "big.npy"))
    assert sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in os.listdir(tmp_path / "a")) <= budget
