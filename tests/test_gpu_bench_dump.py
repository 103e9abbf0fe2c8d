"""GPU: a plain `bench.py --dump-outputs DIR` run end to end (smoke()'s small C2-shaped configuration, one timed step):
the result line carries the timed step count and ms_per_step and none of the --full measurements, and the dumped arrays
are what that step computed — finite, float32 / float64, and the dumped advantages / returns are the CPU oracle's GAE
of the dumped rewards, values, terminals, closures and bootstraps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_dumps_the_last_steps_outputs(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle import cpu_ref
    cpu_ref.build_oracle()
    N, T = 256, 32
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", "--n-envs",
           str(N), "--horizon", str(T), "--n-epoch", "2", "--n-minibatch", "4", "--dump-outputs", str(out)]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["steps"] == 1 and res["warmup"] == 1 and res["ms_per_step"] > 0 and res["unit"] == "env-steps/s"
    assert abs(res["value"] - N * T / (res["ms_per_step"] * 1e-3)) <= 1e-3 * res["value"]
    for side in ("roofline", "c1_cartpole", "c3_atari_a2c", "c4_box376", "c5_perdqn", "cpu_baseline", "dp_update_path",
                 "gae_sweep_flushed"):
        assert res.get(side) is None, side
    d = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert sum(a.nbytes for a in d.values()) <= 64 * 2**20
    for name, a in d.items():
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), name
    assert d["mem_observations"].shape == (N, T, 17) and d["mem_actions"].shape == (N, T, 6)
    assert d["param_actor.logstd"].shape == (6,) and d["obs_mean"].shape == (17,)
    # the same pair and bound as smoke(): the f32 scan against the oracle's f32 restatement on this step's own data
    adv, ret = cpu_ref.gae_rows(d["mem_rewards"], d["mem_values"], d["mem_terminals"], d["mem_closed"].astype(np.uint8),
                                d["mem_boot"], 0.99, 0.95)
    np.testing.assert_allclose(d["mem_advantages"], adv, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(d["mem_returns"], ret, rtol=1e-5, atol=1e-5)
