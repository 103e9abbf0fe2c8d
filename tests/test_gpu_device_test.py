"""GPU: evaluation on the device (agent.test_device; config.device_test) — the episode log and its two writers.

  * xpa_eval_post alone against a numpy statement of the reference's collection rule (ppoclip_agent.py:113-165);
  * K32E (xpa_small_eval_cartpole / _pendulum) against the training kernel K32 stepped one launch at a time: the same
    stages on the same action stream give the same episodes, statistics and env state, to the bit;
  * the stop rule and the chunking of K32E;
  * the generic tier (eager steps + xpa_eval_post) against a host-stepped loop of the same kernels, with the statistics
    restored from the log's snapshot after the steps that ran past the stop;
  * Atari life losses; the public surface (agent.test with device_test, Runner_DRL.benchmark).
All comparisons are exact: both sides run the same arithmetic."""
import os
from copy import deepcopy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _np(t):
    return t.detach().cpu().numpy().copy()


def _stats(agent):
    return [_np(agent.obs_mean), _np(agent.obs_var), _np(agent.obs_count)]


def _assert_equal_lists(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(x, y, err_msg="%s[%d]" % (what, i))


# ---- 1. xpa_eval_post alone ----------------------------------------------------------------------------------------
def _reference_entries(term, trunc, score, length, target, atari, stop=True):
    """(entries [(step, env, score, length)], steps_run, latch step) of the reference loop over per-step arrays."""
    out, steps = [], 0
    for s in range(term.shape[0]):
        for i in range(term.shape[1]):
            if (term[s, i] or trunc[s, i]) and not (atari and not trunc[s, i]):
                out.append((s, i, score[s, i], int(length[s, i])))
        steps += 1
        if stop and len(out) >= target:
            break
    return out, steps


def _check_entries(log, ref):
    assert list(zip(log["step"].tolist(), log["env"].tolist())) == [(s, i) for s, i, _, _ in ref]
    assert log["score"].tobytes() == np.asarray([sc for _, _, sc, _ in ref], np.float32).tobytes()
    assert log["length"].tolist() == [ln for _, _, _, ln in ref]


@pytest.mark.parametrize("atari", [False, True])
@pytest.mark.parametrize("N", [1, 70, 1100])   # one lane; past one wave; past one pass of the 1024-thread loop
def test_eval_post_matches_reference_rule(N, atari):
    from xuanpolicy_amd import ops
    S, D, GUARD = 6, 3, 8
    rng = np.random.default_rng(100 + N)
    term, trunc = rng.random((S, N)) < 0.3, rng.random((S, N)) < 0.3
    trunc[0, 0] = trunc[2, 0] = True
    score = rng.standard_normal((S, N)).astype(np.float32)
    length = rng.integers(1, 1000, (S, N)).astype(np.int32)
    full, _ = _reference_entries(term, trunc, score, length, 0, atari, stop=False)
    target = max(1, len([e for e in full if e[0] < 3]))       # completes at step 2 or 3 of 6
    ref, ref_steps = _reference_entries(term, trunc, score, length, target, atari)
    assert 0 < ref_steps < S and len(ref) >= target
    mean = torch.zeros((D,), device=DEV)
    var = torch.ones((D,), device=DEV)
    count = torch.full((1,), 1e-4, dtype=torch.float64, device=DEV)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    for capacity in (target + N, len(ref) - 1):
        if capacity < 1:
            continue
        log = ops.eval_log_new(target, N, D, DEV, capacity=capacity, guard=GUARD)
        cursor = ops.new_cursor(DEV)
        cursor[1] = 41
        snaps, words = [], None
        for s in range(S):
            mean += 1.0                      # the step's obs_rms.update, stood in for
            var *= 2.0
            count += float(N)
            snaps.append((_np(count), _np(mean), _np(var)))
            ops.eval_post(log, capacity, D, dev(term[s].astype(np.uint8)), dev(trunc[s].astype(np.uint8)),
                          dev(score[s]), dev(length[s]), atari, cursor, stats=(mean, var, count))
            if s == ref_steps - 1:
                words = _np(log)
        after = _np(log)
        np.testing.assert_array_equal(after, words)        # the steps after `done` changed nothing
        np.testing.assert_array_equal(after[-GUARD:], -1)  # the guard cells behind the log
        out = ops.eval_log_decode(after[:-GUARD])
        assert out["done"] and out["steps_run"] == ref_steps and out["count"] == len(ref) and out["target"] == target
        assert _np(cursor).tolist() == [0, 41 + ref_steps, 0, 0]
        for got, want in zip((out["obs_count"], out["obs_mean"], out["obs_var"]), snaps[ref_steps - 1]):
            np.testing.assert_array_equal(np.asarray(got).reshape(-1), want.reshape(-1))
        if capacity >= len(ref):
            assert not out["overflow"]
            _check_entries(out, ref)
        else:
            assert out["overflow"] and len(out["score"]) == capacity
            _check_entries(out, ref[:capacity])


# ---- 2. K32E against the training kernel ---------------------------------------------------------------------------
TRAIN_STATE = ("obs_norm", "returns", "ret_mean", "ret_var", "ret_count", "cursor", "slot_obs", "slot_t",
               "slot_overflow", "boot_obs")


def _training_state(agent):
    mem, env = agent.memory, agent.envs
    t = {k: getattr(agent, k) for k in TRAIN_STATE}
    t.update(obs=mem.observations, act=mem.actions, val=mem.values, rew=mem.rewards, term=mem.terminals,
             closed=mem.closed, boot=mem.boot, adv=mem.advantages, ret=mem.returns,
             env_state=env.state, env_obs=env.obs, env_act=env.act_in, ep_step=env.ep_step, ep_index=env.ep_index,
             ep_score=env.ep_score, ep_last_score=env.ep_last_score, ep_last_len=env.ep_last_len, env_term=env.term,
             env_trunc=env.trunc, env_rew=env.rew, env_final=env.final_obs)
    t.update({"aux_" + k: v for k, v in mem.auxiliary_infos.items()})
    t.update({"param%d" % i: p for i, p in enumerate(agent.policy.parameters())})
    out = {k: _np(v) for k, v in t.items()}
    out["_rms_pending"], out["_t"], out["ptr"] = agent._rms_pending, agent._t, (mem.ptr, mem.size)
    return out


def _k32_reference(build, steps):
    """Agent A stepped one K32 launch at a time (n_steps = 64: no update inside 63 steps): the expected log entries
    and, after every step, the obs statistics and the env's state."""
    A = build()
    assert A.plan().driver == "K32"
    env, entries, per_step = A.envs, [], []
    for s in range(steps):
        A.train(1, log=False)
        te, tr = _np(env.term), _np(env.trunc)
        sc, ln = _np(env.ep_last_score), _np(env.ep_last_len)
        for i in range(A.n_envs):
            if te[i] or tr[i]:
                entries.append((s, i, sc[i], int(ln[i]), bool(te[i]), bool(tr[i])))
        per_step.append((_stats(A), [_np(env.state), _np(env.ep_index), _np(env.ep_step), _np(env.obs)]))
    return entries, per_step


def _check_k32e(build, make_env, need_both):
    steps = 63
    entries, per_step = _k32_reference(build, steps)
    target = len(entries) // 2
    stop = next(s for s in range(steps) if sum(e[0] <= s for e in entries) >= target)
    assert 0 < stop < steps - 1    # strictly inside the window
    ref = [e for e in entries if e[0] <= stop]
    if need_both:   # the expected log holds both kinds of episode end
        assert any(e[4] for e in ref) and any(e[5] and not e[4] for e in ref)
    ref = [e[:4] for e in ref]
    B = build()
    env = make_env(B)
    before = _training_state(B)
    scores = B.test_device(env, target, rng=(B.seed, 0))
    torch.cuda.synchronize()
    assert B.plan_test(env) == "K32E"
    log = B.last_test_log
    assert log["done"] and not log["overflow"] and log["steps_run"] == stop + 1 and log["count"] == len(ref)
    _check_entries(log, ref)
    assert np.asarray(scores, np.float32).tobytes() == log["score"].tobytes()
    want_stats, want_env = per_step[stop]
    _assert_equal_lists(_stats(B), want_stats, "obs_rms")
    _assert_equal_lists([_np(env.state), _np(env.ep_index), _np(env.ep_step), _np(env.obs)], want_env, "env")
    after = _training_state(B)
    for k in before:
        if k in ("obs_mean", "obs_var", "obs_count"):
            continue
        np.testing.assert_array_equal(np.asarray(after[k]), np.asarray(before[k]), err_msg=k)


# seeds whose 63-step trajectories hold a terminal and a truncation end (deterministic: counter-hash RNG)
CARTPOLE_SEED = {(8, 64): 3, (8, 32): 3, (70, 64): 3, (256, 32): 3}


@pytest.mark.parametrize("N,hidden,obsnorm", [(8, 64, True), (8, 32, False), (70, 64, True), (256, 32, True)])
def test_k32e_cartpole_matches_training_kernel(N, hidden, obsnorm):
    from xuanpolicy_amd.runner import build_cartpole_ppo, make_envs

    def build():
        return build_cartpole_ppo(n_envs=N, n_steps=64, hidden=hidden, seed=CARTPOLE_SEED[N, hidden], device=DEV,
                                  max_episode_steps=12, use_obsnorm=obsnorm)
    _check_k32e(build, lambda B: make_envs(B.config, DEV), need_both=True)


@pytest.mark.parametrize("N", [8, 86])
def test_k32e_pendulum_matches_training_kernel(N):
    from xuanpolicy_amd.runner import build_pendulum_ppo, make_envs

    def build():
        return build_pendulum_ppo(n_envs=N, n_steps=64, hidden=64, seed=4, device=DEV, max_episode_steps=5)
    _check_k32e(build, lambda B: make_envs(B.config, DEV), need_both=False)


# ---- 3. stop rule and chunking -------------------------------------------------------------------------------------
def test_k32e_stop_rule_and_chunking():
    from xuanpolicy_amd import ops
    from xuanpolicy_amd.rollout_plan import eval_entry
    from xuanpolicy_amd.runner import build_cartpole_ppo, make_envs
    N, target = 70, 10
    res = []
    for chunk in (1, 2, 64):
        agent = build_cartpole_ppo(n_envs=N, n_steps=16, hidden=64, seed=2, device=DEV, max_episode_steps=3)
        env = make_envs(agent.config, DEV)
        scores = agent.test_device(env, target, chunk=chunk, rng=(7, 5))
        log = agent.last_test_log
        # every env truncates at its third step: 70 scores of 3.0 in env order, although 10 were asked for
        assert log["steps_run"] == 3 and log["env"].tolist() == list(range(N)) and log["step"].tolist() == [2] * N
        assert scores == [3.0] * N and log["length"].tolist() == [3] * N
        res.append([log[k] for k in ("step", "env", "score", "length")] + _stats(agent)
                   + [_np(env.state), _np(env.ep_index), _np(env.ep_step), _np(env.obs)])
    for other in res[1:]:
        _assert_equal_lists(other, res[0], "chunk")
    # launches queued behind the completing one change nothing: two launches without a look at the log, then a third
    agent = build_cartpole_ppo(n_envs=N, n_steps=16, hidden=64, seed=2, device=DEV, max_episode_steps=3)
    env = make_envs(agent.config, DEV)
    cursor = ops.new_cursor(DEV)
    cursor[1] = 5
    args, logstd = agent._build_small_eval(env, 7, cursor)
    args.steps = 2
    D, cap = agent.obs_dim, target + N
    log = ops.eval_log_new(target, N, D, DEV, guard=4)
    scratch = torch.empty((3 * N,), dtype=torch.float32, device=DEV)
    entry = eval_entry(agent._eval_facts(env))
    for _ in range(3):
        ops.small_eval(entry, args, log, cap, D, scratch)
    state = lambda: [_np(log), _np(cursor)] + _stats(agent) + [_np(env.state), _np(env.ep_index), _np(env.ep_step),
                                                                _np(env.obs)]
    first = state()
    ops.small_eval(entry, args, log, cap, D, scratch)
    _assert_equal_lists(state(), first, "after done")
    out = ops.eval_log_decode(first[0][:-4])
    assert out["done"] and out["steps_run"] == 3 and first[1].tolist() == [0, 8, 0, 0] and (first[0][-4:] == -1).all()
    _assert_equal_lists([out[k] for k in ("step", "env", "score", "length")] + first[2:], res[0], "queued")


# ---- 4. / 5. the generic tier against a host-stepped loop of the same kernels --------------------------------------
@torch.no_grad()
def _host_stepped(agent, env, target, seed, step0=0):
    """The reference rule driven from the host over the tier's own kernels: the flags are read after every step."""
    from xuanpolicy_amd import ops
    from xuanpolicy_amd.agents import _space_clip
    from xuanpolicy_amd.policies import policy_heads
    N, D = env.num_envs, agent.obs_dim
    env.reset()
    cursor = ops.new_cursor(DEV)
    cursor[1] = step0
    f32 = dict(dtype=torch.float32, device=DEV)
    A = env.act_in.shape[1]
    act = torch.empty((N, 1) if agent.discrete else (N, 1, A), **f32)
    logp, val, norm = torch.empty((N, 1), **f32), torch.empty((N, 1), **f32), torch.empty((N, D), **f32)
    ticket = torch.zeros((1,), dtype=torch.int32, device=DEV)
    clip = 1.0 if agent.discrete else _space_clip(env.action_space)
    scores, steps, lifeloss = [], 0, 0
    while len(scores) < target:
        x = env.obs
        if not agent.raw_obs:
            if agent.use_obsnorm:
                ops.rms_update(x, agent.obs_mean, agent.obs_var, agent.obs_count, ticket=ticket)
            x = ops.obs_normalize(x, agent.obs_mean, agent.obs_var, agent._obs_clip(), norm)
        head, logstd, v = policy_heads(agent.policy, x)
        ops.rollout_sample(agent.dist, head.contiguous(), logstd, v.contiguous(), cursor, seed, act, logp, val,
                           env.act_in, act_clip=clip)
        env.step_device()
        cursor[1] += 1
        te, tr, sc = _np(env.term), _np(env.trunc), _np(env.ep_last_score)
        for i in range(N):
            if te[i] or tr[i]:
                if agent.atari and not tr[i]:
                    lifeloss += 1
                    continue
                scores.append(sc[i])
        steps += 1
        assert steps < 1000
    return scores, steps, lifeloss


def _check_steps_tier(build, make_env, target, chunk=8):
    X, Y = build(), build()
    ref_scores, ref_steps, lifeloss = _host_stepped(X, make_env(X), target, 11, step0=3)
    env = make_env(Y)
    assert Y.plan_test(env) == "steps"
    scores = Y.test_device(env, target, chunk=chunk, rng=(11, 3))
    torch.cuda.synchronize()
    log = Y.last_test_log
    assert log["steps_run"] == ref_steps and log["done"] and not log["overflow"]
    assert np.asarray(scores, np.float32).tobytes() == np.asarray(ref_scores, np.float32).tobytes()
    _assert_equal_lists(_stats(Y), _stats(X), "obs_rms")
    return ref_steps, lifeloss, log


@pytest.mark.parametrize("target", [1, 350])
@pytest.mark.parametrize("discrete", [False, True])
def test_steps_tier_synthbox_matches_host_stepped_loop(discrete, target):
    from xuanpolicy_amd.envs import SynthBoxVecEnv
    from xuanpolicy_amd.runner import build_synthbox_ppo
    N, D, A = 300, 5, 3 if discrete else 2

    def build():
        return build_synthbox_ppo(n_envs=N, n_steps=8, obs_dim=D, act_dim=A, hidden=32, n_epoch=1, n_minibatch=2,
                                  seed=6, device=DEV, discrete=discrete, max_episode_steps=4, use_obsnorm=True)

    def make_env(agent):
        return SynthBoxVecEnv(N, D, A, seed=6, discrete=discrete, max_episode_steps=4, device=DEV)
    steps, _, log = _check_steps_tier(build, make_env, target)
    # every env ends by its 4th step, so one episode is there within 4 steps — short of the chunk's 8, which then ran
    # past the stop (the snapshot restore); 350 > N needs an env's second episode, within 8 steps
    assert (steps <= 4) if target == 1 else (1 < steps <= 8)
    assert log["count"] >= target


def test_steps_tier_cartpole_hidden_128():
    from xuanpolicy_amd.runner import build_cartpole_ppo, make_envs

    def build():   # 128 units: outside K32's widths
        return build_cartpole_ppo(n_envs=8, n_steps=16, hidden=128, seed=3, device=DEV, max_episode_steps=12)

    def make_env(agent):
        cfg = deepcopy(agent.config)
        cfg.parallels = 5
        return make_envs(cfg, DEV)
    steps, _, _ = _check_steps_tier(build, make_env, 7)
    assert 1 < steps <= 24


def test_steps_tier_atari_life_losses():
    from xuanpolicy_amd.envs import SynthAtariVecEnv
    from xuanpolicy_amd.runner import build_atari_a2c

    def build():
        return build_atari_a2c(n_envs=4, n_steps=8, device=DEV, n_epoch=1, n_minibatch=2, seed=5, max_episode_steps=34,
                               filters=[8, 8], kernels=[8, 4], strides=[4, 2], fc_hidden_sizes=[32])

    def make_env(agent):
        return SynthAtariVecEnv(4, agent.config.n_actions if hasattr(agent.config, "n_actions") else 6, seed=5,
                                max_episode_steps=34, device=DEV)
    steps, lifeloss, log = _check_steps_tier(build, make_env, 3)
    assert lifeloss > 0                       # term without trunc occurred, and produced no entry:
    assert log["count"] == len(log["score"]) and steps <= 34 and (log["length"] > 0).all()


# ---- 6. the public surface -----------------------------------------------------------------------------------------
class _HostCartPole:
    """A host VecEnv (no step_device): the device CartPole behind the reference's step contract alone."""

    def __init__(self, env):
        self._env = env
        self.num_envs, self.observation_space, self.action_space = env.num_envs, env.observation_space, env.action_space
        self.max_episode_steps = env.max_episode_steps
        self.closed = 0

    def reset(self):
        return self._env.reset()

    def step(self, actions):
        return self._env.step(actions)

    def close(self):
        self.closed += 1


def test_agent_test_surface(monkeypatch):
    from xuanpolicy_amd.envs import CartPoleVecEnv
    from xuanpolicy_amd.runner import build_cartpole_ppo
    made, hooked = [], []

    def env_fn():
        env = CartPoleVecEnv(3, seed=1, max_episode_steps=20, device=DEV)
        env.closed = 0
        env.close = lambda: setattr(env, "closed", env.closed + 1)
        made.append(env)
        return env
    agent = build_cartpole_ppo(n_envs=8, n_steps=16, hidden=64, seed=1, device=DEV, max_episode_steps=20,
                               device_test=True)
    agent.log_hook = lambda info, step: hooked.append((dict(info), step))
    scores = agent.test(env_fn, 4)
    assert len(scores) >= 4 and all(isinstance(s, float) and 1.0 <= s <= 20.0 for s in scores)
    assert agent.last_test_log is not None and agent.last_test_log["count"] == len(scores)
    assert made[-1].closed == 1 and len(hooked) == 1
    info, step = hooked[0]
    assert set(info) == {"Test-Episode-Rewards/Mean-Score", "Test-Episode-Rewards/Std-Score"} and step == 0
    assert info["Test-Episode-Rewards/Mean-Score"] == float(np.mean(scores))
    steps1 = agent.last_test_log["steps_run"]
    assert int(agent._eval_cursor[1]) == steps1
    again = agent.test(env_fn, 4)     # the evaluation's step counter continues across calls
    assert len(again) >= 4 and int(agent._eval_cursor[1]) == steps1 + agent.last_test_log["steps_run"]
    assert _np(agent.cursor).tolist() == [0, 0, 0, 0]      # the training stream was not advanced
    # a host VecEnv plans the host loop, with or without the key; without the key test_device is never called

    def boom(*a, **k):
        raise AssertionError("test_device called")
    monkeypatch.setattr(agent, "test_device", boom)
    host = _HostCartPole(CartPoleVecEnv(3, seed=1, max_episode_steps=20, device=DEV))
    assert agent.plan_test(host) == "host"
    assert len(agent.test(lambda: host, 3)) >= 3 and host.closed == 1
    agent.config.device_test = False
    assert len(agent.test(env_fn, 3)) >= 3 and made[-1].closed == 1
    del agent.config.device_test
    assert len(agent.test(env_fn, 3)) >= 3 and made[-1].closed == 1


def test_runner_benchmark_with_device_test(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    from xuanpolicy_amd.runner import Runner_DRL, get_arguments
    args = get_arguments("ppo", "classic_control", "CartPole-v1")
    args.device, args.device_test = "cuda:0", True
    args.parallels, args.n_steps, args.running_steps, args.eval_interval, args.test_episode = 8, 16, 256, 128, 3
    args.representation_hidden_size = args.actor_hidden_size = args.critic_hidden_size = [64]
    args.model_dir = os.path.join(os.getcwd(), "models")
    args.log_dir = os.path.join(os.getcwd(), "logs")
    runner = Runner_DRL(args)
    calls = []
    real = runner.agent.test_device
    monkeypatch.setattr(runner.agent, "test_device", lambda *a, **k: calls.append(1) or real(*a, **k))
    best = runner.benchmark()
    assert set(best) == {"mean", "std", "step"} and np.isfinite(best["mean"]) and best["mean"] >= 1.0
    assert len(calls) == 3      # before training and after each of the two evaluation intervals
