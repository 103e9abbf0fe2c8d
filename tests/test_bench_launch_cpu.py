"""CPU checks of bench.py's multi-rank contract: `bench.py --gpus N` with no launcher
environment starts N ranks itself (torch.distributed.run as a child process, never an exec), relays rank 0's JSON
line, and a rank whose WORLD_SIZE disagrees with --gpus fails loudly before touching the GPU."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402


def test_mismatched_gpus_fails_loudly():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "3", "--steps", "1"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "--gpus 3" in r.stderr and "WORLD_SIZE=2" in r.stderr
    with pytest.raises(SystemExit):
        bench.check_world(4, {"WORLD_SIZE": "8"})
    assert bench.check_world(8, {"WORLD_SIZE": "8"}) == 8
    assert bench.check_world(2, {}) is None


def test_launch_command_is_torchrun_child_of_this_script():
    cmd = bench.launch_cmd(8, ["--gpus", "8", "--steps", "5"], 29500)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "8" and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[cmd.index("--master-port") + 1] == "29500"
    assert cmd[-5:] == [os.path.abspath(bench.__file__), "--gpus", "8", "--steps", "5"]


def test_self_launch_relays_rank0_json_and_status(monkeypatch, capsys):
    """The parent streams the ranks' other output to stderr and prints exactly rank 0's JSON line; the launcher's
    exit status is returned (a fake launcher stands in for the GPU ranks here)."""
    line = {"metric": "m", "value": 1.0, "n_gpus": 2}
    prog = "import json,sys; print('rank log'); print(json.dumps(%r)); sys.exit(0)" % (line,)
    monkeypatch.setattr(bench, "launch_cmd", lambda gpus, argv, port: [sys.executable, "-c", prog])

    class A:
        gpus = 2
    assert bench.self_launch(A(), []) == 0
    out, err = capsys.readouterr()
    assert json.loads(out.strip()) == line and "rank log" in err
    monkeypatch.setattr(bench, "launch_cmd", lambda gpus, argv, port: [sys.executable, "-c", "import sys; sys.exit(3)"])
    assert bench.self_launch(A(), []) == 3


def test_local_grad_sync_takes_the_dp_path_without_a_collective():
    import torch
    from xuanpolicy_amd.distributed import LocalGradSync
    from xuanpolicy_amd.flat import FlatState
    net = torch.nn.Linear(3, 2)
    fs = FlatState(net.parameters())
    h = LocalGradSync(fs)
    before = fs.flat.clone()
    h(fs.params)
    assert h.calls == 1 and h.collectives == 0 and not h.begin(fs.params[0].grad)
    assert torch.equal(fs.flat, before)


SIDE_OFF = ("no_cpu_baseline", "no_sweep", "no_per", "no_c1", "no_c3", "no_c4", "no_kernel_timing", "no_pmc",
            "no_rocprof")


def test_plain_run_measures_nothing_but_its_steps(monkeypatch):
    """Without --full every side measurement is off (the run is set-up, warm-up, the timed steps, the line); with it the
    defaults are the former ones and the --no-* options still choose among the legs."""
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert not a.full and a.steps == 3 and a.warmup == 1 and a.dump_outputs is None
    assert all(getattr(a, k) for k in SIDE_OFF) and a.dp_path == "off"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-c3"])
    a = bench.parse()
    assert a.full and a.no_c3 and not any(getattr(a, k) for k in SIDE_OFF if k != "no_c3") and a.dp_path == "on"


def test_dump_outputs_writes_float_arrays_with_a_fixed_sample(tmp_path):
    """--dump-outputs: one .npy per array in float32 / float64, an array above the per-array cap cut to the same sorted
    rows in every call, everything else whole."""
    import types

    import numpy as np
    import torch
    g = torch.Generator().manual_seed(0)
    N, T = 3000, 64
    mem = types.SimpleNamespace(
        observations=torch.randn(N, T, 17, generator=g), actions=torch.randn(N, T, 6, generator=g),
        rewards=torch.randn(N, T, generator=g), values=torch.randn(N, T, generator=g), terminals=torch.zeros(N, T),
        closed=torch.ones(N, T, dtype=torch.uint8), boot=torch.zeros(N, T), advantages=torch.randn(N, T, generator=g),
        returns=torch.randn(N, T, generator=g), auxiliary_infos={"old_logp": torch.randn(N, T, generator=g)})
    agent = types.SimpleNamespace(memory=mem, obs_mean=torch.zeros(17), obs_var=torch.ones(17),
                                  obs_count=torch.full((1,), 7.0, dtype=torch.float64), policy=torch.nn.Linear(4, 2),
                                  infos=[{"actor-loss": 0.5, "iteration": 3}])
    total = bench.dump_outputs(agent, str(tmp_path / "a"))
    bench.dump_outputs(agent, str(tmp_path / "b"))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and total <= 64 * 2**20
    assert {"mem_observations.npy", "mem_advantages.npy", "mem_aux_old_logp.npy", "param_weight.npy", "obs_count.npy",
            "info_actor-loss.npy"} <= set(names) and "info_iteration.npy" not in names
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64) and x.nbytes <= bench.DUMP_ARRAY_BYTES and np.array_equal(x, y)
    assert np.load(tmp_path / "a" / "obs_count.npy").dtype == np.float64
    assert np.array_equal(np.load(tmp_path / "a" / "mem_rewards.npy"), mem.rewards.numpy())      # under the cap: whole
    obs = np.load(tmp_path / "a" / "mem_observations.npy")                                         # above it: sampled rows
    keep = bench.DUMP_ARRAY_BYTES // (T * 17 * 4)
    rows = np.sort(np.random.default_rng(0).choice(N, keep, replace=False))
    assert obs.shape == (keep, T, 17) and np.array_equal(obs, mem.observations.numpy()[rows])


def test_agent_snapshot_puts_tensors_and_scalars_back_in_place(monkeypatch):
    """--dump-outputs restarts the last timed step from the state set-up left: tensors restored in their own storage
    (captured graphs keep their pointers), scalars and scalar lists on objects and in dicts reset."""
    import types

    import torch
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: None)
    net = torch.nn.Linear(3, 2)
    buf = torch.arange(6.0)
    agent = types.SimpleNamespace(policy=net, memory=types.SimpleNamespace(values=buf, ptr=0), iterations=0,
                                  timers={"rollout": 0.0}, lrs=[1.0, 2.0], infos=[])
    snap = bench.AgentSnapshot(agent)
    w0, ptr = net.weight.detach().clone(), net.weight.data_ptr()
    with torch.no_grad():
        net.weight.add_(1.0)
        buf.mul_(2.0)
    agent.iterations, agent.memory.ptr, agent.timers["rollout"], agent.lrs = 5, 3, 1.5, [0.5, 0.25]
    snap.restore()
    assert torch.equal(net.weight, w0) and net.weight.data_ptr() == ptr and torch.equal(buf, torch.arange(6.0))
    assert (agent.iterations, agent.memory.ptr, agent.timers["rollout"], agent.lrs) == (0, 0, 0.0, [1.0, 2.0])
