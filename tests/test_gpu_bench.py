"""bench.py on the GPU: the plain headline path and --dump-outputs.

The timed path is called in-process at a small size (64^2, batch 2); one test runs the command
line itself, since the plain result line and the files of --dump-outputs are what it is about."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import bench


@pytest.fixture
def bench_on_gpu(monkeypatch):
    torch.cuda.set_device(0)
    monkeypatch.setattr(bench, "_DEVICE", [torch.device("cuda", 0)])
    return bench


def test_plain_config_times_the_steps_alone_and_is_reproducible(bench_on_gpu, tmp_path):
    """Two plain runs of one config see the same seeded inputs and weights: their dumps are equal
    bit for bit, and equal to a --full run's (the event brackets change no arithmetic).  A plain
    run carries no roofline / clock figure; a --full run does."""
    dumps = []
    for tag, full in (("a", False), ("b", False), ("c", True)):
        r = bench_on_gpu.run_config(64, 2, torch.float32, 2, 1, 0, 1, full=full)
        assert ("roofline" in r) == full and ("clock_ghz" in r) == full
        assert r["ms_per_step"] > 0 and r["value"] == pytest.approx(2 * 1e3 / r["ms_per_step"])
        out = r["outputs"]
        assert sorted(out) == ["cs", "fcs"] and out["cs"].shape == (2, 3, 64, 64)
        bench_on_gpu.dump_outputs(str(tmp_path / tag), out)
        dumps.append({n: np.load(tmp_path / tag / (n + ".npy")) for n in out})
        if full:
            assert r["roofline"]["launches_timed"] == 2 * 6  # 6 attention launches per step
    for n, a in dumps[0].items():
        assert a.dtype == np.float32 and np.isfinite(a).all()
        assert a.shape == tuple(r["outputs"][n].shape)  # small: written whole
        assert np.array_equal(a, dumps[1][n]) and np.array_equal(a, dumps[2][n]), n


def test_plain_command_line_prints_the_headline_and_dumps_its_outputs(tmp_path):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    r = lines[0]
    assert r["unit"] == "frames/s" and r["higher_is_better"] is True and r["dtype"] == "f32"
    assert r["steps"] == 2 and r["warmup"] == 1 and r["n_gpus"] == 1
    assert r["value"] == pytest.approx(8 * 1e3 / r["ms_per_step"], rel=1e-3)
    # everything beside the headline waits for --full
    assert not {"configs", "cpu_baseline", "roofline", "clock_ghz"} & set(r)
    assert sorted(os.listdir(tmp_path)) == ["cs.npy", "fcs.npy"]
    cs, fcs = np.load(tmp_path / "cs.npy"), np.load(tmp_path / "fcs.npy")
    assert cs.dtype == np.float32 and cs.shape == (8, 3, 512, 512) and np.isfinite(cs).all()
    # fcs (8 x 512 x 64 x 64 fp32 = 67 MB) is over its 30 MB share: one element of every 3
    assert fcs.dtype == np.float32 and fcs.shape == (8 * 512 * 64 * 64 // 3,) and np.isfinite(fcs).all()
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 64 * 10 ** 6
