"""bench.py's own launch path: `--gpus N` without a torch.distributed launcher starts N rank processes (one per
GPU; here gloo with every rank on cuda:0, the rehearsal form) and rank 0 prints one JSON line whose n_gpus is the
process group's size."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(400)
def test_bench_gpus2_spawns_two_ranks():
    cmd = [sys.executable, "-u", "bench.py", "--gpus", "2", "--dist-backend", "gloo", "--one-device", "--steps", "5",
           "--warmup", "2", "--full", "--no-cpu-baseline", "--no-train-loop", "--no-tcsr", "--only"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=360)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2
    assert out["config"]["parallelism"] == "dp2" and out["config"]["global_batch"] == 400
    assert out["value"] > 0 and out["config"]["sampled_edges_per_step"] > 0
    assert "spawned 2 rank processes" in r.stderr


@pytest.mark.timeout(200)
def test_bench_plain_run_times_the_steps_and_dumps_outputs(tmp_path):
    """A plain run (no --full) is the headline's timed window alone: --steps timed steps (11: one 8-step graph
    group + 3 single replays), the result line without the probe / baseline legs.  --dump-outputs writes the outputs
    of its 4-step replay from the initial state as float32 / float64 .npy inside 64 MB, and two runs (started side
    by side) write the same arrays to rounding: 1e-5 absolute on scores, memory and parameters of magnitude <= 1
    (float32 eps 6e-8 through 4 steps of atomically ordered sums; measured 3e-7 after 5 steps), exact update times."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    procs = [subprocess.Popen([sys.executable, "-u", "bench.py", "--gpus", "1", "--steps", "11", "--warmup", "3",
                               "--dump-outputs", str(tmp_path / d)], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for d in ("dump", "dump2")]
    res = [p.communicate(timeout=180) for p in procs]
    for p, (_, err) in zip(procs, res):
        assert p.returncode == 0, err[-4000:]
    lines = [ln for ln in res[0][0].splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res[0][0][-2000:]
    out = json.loads(lines[0])
    assert out["metric"] == "temporal edges/sec on tgbl-wiki TGN (train step)"
    assert out["unit"] == "events/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["steps"] == 11 and out["warmup"] == 3 and out["n_gpus"] == 1
    a, b = out["config"]["timed_steps"]
    assert b - a == 11
    assert out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(200 / (out["ms_per_step"] * 1e-3), rel=1e-2)
    for leg in ("kernels_us", "cpu_baseline", "secondary_path", "train_loop", "tcsr_sampler", "val_eval_gpu",
                "gpu_tgnn_config1"):
        assert leg not in out, leg
    assert out["roofline"] is None
    got = {f[:-4]: np.load(tmp_path / "dump" / f, allow_pickle=False) for f in os.listdir(tmp_path / "dump")}
    assert set(got) == {"pos", "neg", "loss_sum", "memory", "last_update", "params"}
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    assert got["pos"].shape == (200,) and got["neg"].shape == (200,)
    assert got["pos"].std() > 0 and got["neg"].std() > 0
    assert got["memory"].shape == (9227, 100) and np.abs(got["memory"]).max() > 0
    assert got["last_update"].max() > 0
    # 4 batches of 200 events, BCE of a positive and a negative score per event (2 ln 2 at chance level)
    assert got["loss_sum"].shape == (1,) and 0 < got["loss_sum"][0] < 4 * 200 * 4 * np.log(2)
    for name, v in got.items():
        w = np.load(tmp_path / "dump2" / (name + ".npy"), allow_pickle=False)
        assert w.shape == v.shape and w.dtype == v.dtype
        tol = 0 if name == "last_update" else 1e-5 * max(1.0, float(np.abs(v).max()))
        assert np.abs(v.astype(np.float64) - w).max() <= tol, name
