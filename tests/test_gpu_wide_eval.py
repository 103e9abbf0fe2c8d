"""GPU: the one-launch evaluation at the 128-wide classic-control nets (K32WE xpa_small_eval_wide, K32WEB
xpa_small_eval_wide_batch; config.device_test_wide) and the batched test-env reset (xpa_small_env_reset_batch;
config.device_test_batch_reset).

Every comparison is array equality: each side runs the same arithmetic (K32WE is the training kernel K32W's body with
the evaluation switch; the reset kernel forms what the env classes' reset() uploads).

  1. K32WE against the training kernel K32W stepped one launch at a time, test_gpu_device_test's scheme.
  2. The stop rule and the chunking.
  3. K32WEB: Population.test_device of 128-wide members against twins' own test_device.
  4. The batched reset against reset() on twin envs, and Population.test_device with it against without.
  5. The public surface: Population.test with both flags, and training afterwards."""
import numpy as np
import pytest
import torch

from tests.test_gpu_device_test import _assert_equal_lists, _check_entries, _np, _stats, _training_state
from tests.test_gpu_population_eval import _agent_state, _assert_logs_equal, _env_fn, _test_envs
from tests.test_gpu_wide_small import _build

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
H = 128
ENV_TENSORS = ("state", "obs", "act_in", "final_obs", "rew", "term", "trunc", "ep_step", "ep_index", "ep_score",
               "ep_last_score", "ep_last_len")


@pytest.fixture(scope="module", autouse=True)
def _setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _env_all(env):
    """Every tensor of a device env set, and its reset counter."""
    return [_np(getattr(env, k)) for k in ENV_TENSORS] + [np.asarray(env.resets)]


# ---- 1. K32WE against the training kernel --------------------------------------------------------------------------
def _k32w_reference(build, steps):
    """Agent A stepped one K32W launch at a time (n_steps = 64: no update inside 63 steps): the expected log entries
    and, after every step, the obs statistics and the env's state."""
    A = build()
    assert A.plan().driver == "K32W"
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


def _check_k32we(build, need_both):
    from xuanpolicy_amd.runner import make_envs
    steps = 63
    entries, per_step = _k32w_reference(build, steps)
    target = len(entries) // 2
    stop = next(s for s in range(steps) if sum(e[0] <= s for e in entries) >= target)
    assert 0 < stop < steps - 1    # strictly inside the window
    ref = [e for e in entries if e[0] <= stop]
    if need_both:   # the expected log holds both kinds of episode end
        assert any(e[4] for e in ref) and any(e[5] and not e[4] for e in ref)
    ref = [e[:4] for e in ref]
    B = build()
    env = make_envs(B.config, DEV)
    before = _training_state(B)
    assert B.plan_test(env) == "K32WE"
    scores = B.test_device(env, target, rng=(B.seed, 0))
    torch.cuda.synchronize()
    log = B.last_test_log
    assert log["done"] and not log["overflow"] and log["steps_run"] == stop + 1 and log["count"] == len(ref)
    _check_entries(log, ref)
    assert np.asarray(scores, np.float32).tobytes() == log["score"].tobytes()
    want_stats, want_env = per_step[stop]
    _assert_equal_lists(_stats(B), want_stats, "obs_rms")
    _assert_equal_lists([_np(env.state), _np(env.ep_index), _np(env.ep_step), _np(env.obs)], want_env, "env")
    after = _training_state(B)
    for k in before:   # byte for byte: the training state holds no obs statistics
        np.testing.assert_array_equal(np.asarray(after[k]), np.asarray(before[k]), err_msg=k)


def _n_max():
    """The largest N <= 256 whose 128-wide CartPole launch fits the LDS budget."""
    from xuanpolicy_amd import _lib
    lds = _lib.load().xpa_small_rollout_lds_floats
    return max(n for n in range(1, 257) if 0 < lds(n, 4, H, H, H, 2) <= 16384)


# CartPole seeds whose 63-step windows hold a terminal and a pure truncation end before the stop (deterministic:
# counter-hash RNG); the test asserts it
CARTPOLE_SEED = {(8, True): 3, (8, False): 3, (70, True): 3, ("max", True): 3}


@pytest.mark.parametrize("N,obsnorm", sorted(CARTPOLE_SEED, key=str))
def test_k32we_cartpole_matches_training_kernel(N, obsnorm, seed=None):
    """N = 8: one ragged 16-env tile; 70: five tiles, and the log's compaction crosses waves; the largest N the LDS
    budget admits."""
    n = _n_max() if N == "max" else N
    seed = CARTPOLE_SEED[N, obsnorm] if seed is None else seed

    def build():
        return _build("cartpole", n_envs=n, n_steps=64, hidden=H, seed=seed, max_episode_steps=12,
                      use_obsnorm=obsnorm, device_test_wide=True)
    _check_k32we(build, need_both=True)


@pytest.mark.parametrize("kind,agent,limit", [("pendulum", "PPO_Clip", 5), ("acrobot", "PPO_Clip", 12),
                                              ("mountaincar", "A2C", 12)])
def test_k32we_other_envs_match_training_kernel(kind, agent, limit):
    """The Gaussian head (d_in 3), d_in 6 and d_in 8 (A2C: the other agent's block)."""
    def build():
        return _build(kind, agent=agent, n_envs=8, n_steps=64, hidden=H, seed=4, max_episode_steps=limit,
                      device_test_wide=True)
    _check_k32we(build, need_both=False)


# ---- 2. stop rule and chunking -------------------------------------------------------------------------------------
def test_k32we_stop_rule_and_chunking():
    from xuanpolicy_amd import ops, small_path
    from xuanpolicy_amd.runner import make_envs
    N, target = 70, 10

    def build():
        return _build("cartpole", n_envs=N, n_steps=16, hidden=H, seed=2, max_episode_steps=3, device_test_wide=True)
    res = []
    for chunk in (1, 2, 128):
        agent = build()
        env = make_envs(agent.config, DEV)
        assert agent.plan_test(env) == "K32WE"
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
    agent = build()
    env = make_envs(agent.config, DEV)
    cursor = ops.new_cursor(DEV)
    cursor[1] = 5
    args, _ = agent._build_small_eval(env, 7, cursor)
    args.steps = 2
    D, cap = agent.obs_dim, target + N
    log = ops.eval_log_new(target, N, D, DEV, guard=4)
    scratch = torch.empty((3 * N,), dtype=torch.float32, device=DEV)
    for _ in range(3):
        small_path.small_eval_wide("XPA_ENV_CARTPOLE", args, log, cap, D, scratch)
    state = lambda: [_np(log), _np(cursor)] + _stats(agent) + [_np(env.state), _np(env.ep_index), _np(env.ep_step),
                                                                _np(env.obs)]
    first = state()
    small_path.small_eval_wide("XPA_ENV_CARTPOLE", args, log, cap, D, scratch)
    _assert_equal_lists(state(), first, "after done")
    out = ops.eval_log_decode(first[0][:-4])
    assert out["done"] and out["steps_run"] == 3 and first[1].tolist() == [0, 8, 0, 0]
    assert (first[0][-4:] == -1).all()   # the guard words behind the log
    _assert_equal_lists([out[k] for k in ("step", "env", "score", "length")] + first[2:], res[0], "queued")


# ---- 3. K32WEB -----------------------------------------------------------------------------------------------------
# (kind, test envs N, time limit, test_episode, member seeds).  The CartPole seeds are chosen so that the twins stop at
# different steps (deterministic: counter-hash RNG; 36, 35 and 36 on an MI355X), and the test asserts it.  Pendulum cannot: every env of every member
# truncates at the multiples of the shared time limit, so members with one target stop together.
WEB_CASES = {"cartpole": ("cartpole", 8, 12, 20, (3, 4, 5)), "pendulum": ("pendulum", 8, 5, 20, (3, 4, 5))}


def _web_members(case, **kw):
    kind, _, limit, _, seeds = WEB_CASES[case]
    return [_build(kind, n_envs=5, n_steps=48, hidden=H, seed=s, max_episode_steps=limit, **kw) for s in seeds]


@pytest.mark.parametrize("case", sorted(WEB_CASES))
def test_k32web_equals_each_members_own(case):
    from xuanpolicy_amd.population import Population
    kind, N, _, target, _ = WEB_CASES[case]
    set_a, set_b = _web_members(case, device_test_wide=True), _web_members(case, device_test_wide=True)
    pop = Population(set_a)
    envs_a, envs_b = [_test_envs(a, N) for a in set_a], [_test_envs(b, N) for b in set_b]
    plan = pop.plan_test(envs_a)
    assert plan.n_agents == 3 and plan.wide and plan.gaussian == (kind == "pendulum")
    before = [_training_state(a) for a in set_a]
    got = pop.test_device(envs_a, target, rngs=[(a.seed, 0) for a in set_a])
    want = [b.test_device(e, target, rng=(b.seed, 0)) for b, e in zip(set_b, envs_b)]
    torch.cuda.synchronize()
    steps_run = [b.last_test_log["steps_run"] for b in set_b]
    print(case, "steps_run", steps_run, "count", [b.last_test_log["count"] for b in set_b])
    for p, (a, b) in enumerate(zip(set_a, set_b)):
        tag = "member %d" % p
        assert b.plan_test(envs_b[p]) == "K32WE"
        assert got[p] == want[p] and len(got[p]) >= target, tag
        assert a.last_test_log["done"] and not a.last_test_log["overflow"]
        _assert_logs_equal(a.last_test_log, b.last_test_log, tag)
        _assert_equal_lists(_stats(a), _stats(b), tag + " obs_rms")
        _assert_equal_lists(_env_all(envs_a[p]), _env_all(envs_b[p]), tag + " env")
        after = _training_state(a)
        for k in before[p]:
            np.testing.assert_array_equal(np.asarray(after[k]), np.asarray(before[p][k]), err_msg=tag + ": " + k)
    assert not np.array_equal(_np(envs_a[0].obs), _np(envs_a[1].obs))   # different members
    if kind == "cartpole":   # the members stop at different steps: the independent stop is exercised
        assert len(set(steps_run)) > 1, steps_run
    # the evaluation's own stream: the cursor is made on first use and continues across calls, as each member's does
    got = pop.test_device(envs_a, target, chunk=7)
    want = [b.test_device(e, target, chunk=7) for b, e in zip(set_b, envs_b)]
    for p, (a, b) in enumerate(zip(set_a, set_b)):
        assert got[p] == want[p]
        np.testing.assert_array_equal(_np(a._eval_cursor), _np(b._eval_cursor))
        assert int(a._eval_cursor[1]) > 0
        _assert_logs_equal(a.last_test_log, b.last_test_log, "member %d, own stream" % p)
        _assert_equal_lists(_stats(a) + _env_all(envs_a[p]), _stats(b) + _env_all(envs_b[p]), "own stream")
    for a in set_a:
        assert _np(a.cursor).tolist() == [0, 0, 0, 0]   # the training stream was not advanced


def test_k32web_is_opt_in():
    """Members of the same shape without the flag plan the "steps" tier, as before: test_device raises."""
    from xuanpolicy_amd.population import Population
    members = _web_members("cartpole")
    pop = Population(members)
    envs = [_test_envs(a, 8) for a in members]
    assert [a.plan_test(e) for a, e in zip(members, envs)] == ["steps"] * 3
    with pytest.raises(ValueError, match="member 0: its test envs plan the 'steps' tier"):
        pop.test_device(envs, 20)
    mixed = _web_members("cartpole", device_test_wide=True)[:2] + members[2:]
    with pytest.raises(ValueError, match="member 2: its test envs plan the 'steps' tier"):
        Population(mixed).test_device([_test_envs(a, 8) for a in mixed], 20)


# ---- 4. the batched reset ------------------------------------------------------------------------------------------
KINDS = {"cartpole": ("CartPoleVecEnv", "XPA_ENV_CARTPOLE", 4, 2), "pendulum": ("PendulumVecEnv", "XPA_ENV_PENDULUM", 3, 1),
         "acrobot": ("AcrobotVecEnv", "XPA_ENV_ACROBOT", 6, 3), "mountaincar": ("MountainCarVecEnv", "XPA_ENV_MOUNTAINCAR", 8, 3)}


def _dirty_env(kind, N, seed):
    """An env set after five steps under a time limit of 3: every tensor reset() touches holds something else."""
    from xuanpolicy_amd import envs as envs_mod
    env = getattr(envs_mod, KINDS[kind][0])(N, seed=seed, max_episode_steps=3, device=DEV)
    g = torch.Generator(device="cpu").manual_seed(100 + seed)
    for _ in range(5):
        if kind == "pendulum":
            env.act_in.copy_((torch.rand((N, 1), generator=g) * 4 - 2).to(DEV))
        else:
            k = env.act_in.shape[1]
            env.act_in.copy_(torch.nn.functional.one_hot(torch.randint(k, (N,), generator=g), k).float().to(DEV))
        env.step_device()
    torch.cuda.synchronize()
    assert _np(env.ep_index).min() >= 1 and _np(env.ep_step).max() >= 1 and np.abs(_np(env.final_obs)).max() > 0
    assert np.abs(_np(env.act_in)).max() > 0 and _np(env.ep_last_len).max() == 3 and _np(env.rew).any()
    return env


def _reset_block(env, kind):
    """The fields of an evaluation block the reset reads (small_path.env_block's, without a policy)."""
    from xuanpolicy_amd import _lib
    p = torch.Tensor.data_ptr
    a = _lib.XpaSmallRolloutArgs()
    a.n_envs, a.d_in, a.k = env.num_envs, KINDS[kind][2], KINDS[kind][3]
    a.env_seed, a.max_episode_steps = env.noise_seed & 0xFFFFFFFF, env.max_episode_steps
    a.act_in, a.ld_act = p(env.act_in), env.act_in.stride(0)
    a.env_state, a.env_obs, a.ld_obs = p(env.state), p(env.obs), env.obs.stride(0)
    a.final_obs, a.env_rew, a.env_term, a.env_trunc = p(env.final_obs), p(env.rew), p(env.term), p(env.trunc)
    a.ep_step, a.ep_index, a.ep_score = p(env.ep_step), p(env.ep_index), p(env.ep_score)
    a.ep_last_score, a.ep_last_len = p(env.ep_last_score), p(env.ep_last_len)
    return a


@pytest.mark.parametrize("N", [1, 70, 256])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_env_reset_batch_equals_reset(kind, N):
    from xuanpolicy_amd import _lib, small_path
    from xuanpolicy_amd.population import _block_array
    seeds = (3, 4, 5, 6)
    envs, twins = [_dirty_env(kind, N, s) for s in seeds], [_dirty_env(kind, N, s) for s in seeds]
    _assert_equal_lists(_env_all(envs[0]), _env_all(twins[0]), "twins start equal")
    outside = _env_all(envs[3])
    arr = _block_array(_lib.XpaSmallRolloutArgs, [_reset_block(e, kind) for e in envs[:3]])
    dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    small_path.env_reset_batch(KINDS[kind][1], 3, (arr, dev), DEV)
    for e in envs[:3]:
        e.reset_host()
    for t in twins[:3]:
        t.reset()
    torch.cuda.synchronize()
    for p in range(3):
        _assert_equal_lists(_env_all(envs[p]), _env_all(twins[p]), "%s N %d set %d" % (kind, N, p))
        assert envs[p].resets == 2 and not _np(envs[p].ep_index).any() and not _np(envs[p].rew).any()
    assert not np.array_equal(_np(envs[0].state), _np(envs[1].state))      # different seeds
    if kind == "cartpole":   # reset() leaves CartPole's action input as it is, and so does the launch
        assert np.abs(_np(envs[0].act_in)).max() > 0
    else:
        assert not _np(envs[0].act_in).any()
    assert np.abs(_np(envs[0].final_obs)).max() > 0                        # final_obs is not reset()'s
    _assert_equal_lists(_env_all(envs[3]), outside, "the set outside the launch")


@pytest.mark.parametrize("hidden", [64, H])
def test_test_device_with_batch_reset_equals_without(hidden):
    from xuanpolicy_amd.population import Population
    kw = dict(n_envs=5, n_steps=48, hidden=hidden, max_episode_steps=12, device_test_wide=True)
    set_a, set_b = ([_build("cartpole", seed=s, **kw) for s in (3, 4, 5)] for _ in range(2))
    pops = Population(set_a), Population(set_b)
    envs_a, envs_b = [_test_envs(a, 8) for a in set_a], [_test_envs(b, 8) for b in set_b]
    assert pops[0].plan_test(envs_a).wide == (hidden == H)
    for call in range(2):   # the second call starts from the envs the first one left
        got = pops[0].test_device(envs_a, 20, batch_reset=True)
        want = pops[1].test_device(envs_b, 20, batch_reset=False)
        torch.cuda.synchronize()
        assert got == want and all(len(s) >= 20 for s in got)
        for p, (a, b) in enumerate(zip(set_a, set_b)):
            tag = "call %d member %d" % (call, p)
            _assert_logs_equal(a.last_test_log, b.last_test_log, tag)
            _assert_equal_lists(_stats(a) + _env_all(envs_a[p]), _stats(b) + _env_all(envs_b[p]), tag)
            np.testing.assert_array_equal(_np(a._eval_cursor), _np(b._eval_cursor))
            assert envs_a[p].resets == envs_b[p].resets == 2 + call


# ---- 5. the public surface -----------------------------------------------------------------------------------------
def _surface_set(seeds=(1, 2, 3), **flags):
    """Members of the committed CartPole-v1.yaml's shape (10 envs, [128] nets) at a small n_steps."""
    kw = dict(n_envs=10, n_steps=32, n_epoch=2, n_minibatch=2, max_episode_steps=40, hidden=H, device_test=True)
    kw.update(flags)
    agents = [_build("cartpole", seed=s, **kw) for s in seeds]
    hooks = [[] for _ in agents]
    for a, h in zip(agents, hooks):
        a.log_hook = lambda info, step, h=h: h.append((dict(info), step))
    return agents, hooks


def test_population_test_surface_and_training_afterwards():
    from xuanpolicy_amd.population import Population
    flags = dict(device_test_wide=True, device_test_batch_reset=True)
    (set_a, hooks_a), (set_b, hooks_b) = _surface_set(**flags), _surface_set(**flags)
    pop = Population(set_a)
    made_a, made_b, calls = [], [], []
    real = pop.test_device
    pop.test_device = lambda *a, **k: calls.append(k) or real(*a, **k)
    got = pop.test(_env_fn(made_a), 4)
    want = [b.test(_env_fn(made_b), 4) for b in set_b]
    assert calls == [{"batch_reset": True}] and got == want and all(len(s) >= 4 for s in got)
    assert len(made_a) == 3 and [e.closed for e in made_a] == [1, 1, 1]
    assert pop.plan_test(made_a).wide and [b.plan_test(e) for b, e in zip(set_b, made_b)] == ["K32WE"] * 3
    for p, (a, b) in enumerate(zip(set_a, set_b)):
        assert hooks_a[p] == hooks_b[p] and len(hooks_a[p]) == 1
        _assert_logs_equal(a.last_test_log, b.last_test_log, "member %d" % p)
        np.testing.assert_array_equal(_np(a._eval_cursor), _np(b._eval_cursor))
        _assert_equal_lists(_stats(a) + _env_all(made_a[p]), _stats(b) + _env_all(made_b[p]), "member %d" % p)
    # one flag alone: the wide tier without the batched reset; neither: the per-member loop on the "steps" tier
    (set_c, _), (set_d, _) = _surface_set(device_test_wide=True), _surface_set()
    for members, kwargs in ((set_c, [{"batch_reset": False}]), (set_d, [])):
        pop_c, calls_c, made_c = Population(members), [], []
        real_c = pop_c.test_device
        pop_c.test_device = lambda *a, _r=real_c, _c=calls_c, **k: _c.append(k) or _r(*a, **k)
        assert all(len(s) >= 4 for s in pop_c.test(_env_fn(made_c), 4)) and calls_c == kwargs
    # the members stayed ordinary agents: one iteration of the population equals the twins trained alone
    pop.train(32)
    for b in set_b:
        b.train(32)
    torch.cuda.synchronize()
    for p, (a, b) in enumerate(zip(set_a, set_b)):
        sa, sb = _agent_state(a), _agent_state(b)
        assert sa.keys() == sb.keys() and a.iterations == b.iterations == 1
        for k in sb:
            np.testing.assert_array_equal(np.asarray(sa[k]), np.asarray(sb[k]), err_msg="member %d: %s" % (p, k))
