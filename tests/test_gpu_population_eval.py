"""GPU: population evaluation (K32EB, xpa_small_eval_batch; Population.test_device / Population.test) — every member's
test episodes in one launch, each member computing exactly what its own K32E launch computes.

Every comparison is array equality: the batch form runs K32E's body on the same inputs, so there is no tolerance.

  1. Population.test_device against each member's own test_device on twins (scores, log, statistics, env state,
     evaluation cursor; the training state untouched).
  2. The independent stop and queued launches, by construction, through the C entry.
  3. The entry point's refusals: an error, and the logs untouched.
  4. The public surface: Population.test, the fallback to the per-member loop, training afterwards."""
import ctypes
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


def _build(kind, agent="PPO_Clip", **kw):
    from xuanpolicy_amd.runner import build_cartpole_ppo, build_classic_control, build_pendulum_ppo
    if kind == "cartpole":
        return build_cartpole_ppo(device=DEV, agent=agent, clip_grad=0.5, **kw)
    if kind == "pendulum":
        return build_pendulum_ppo(device=DEV, agent=agent, **kw)
    return build_classic_control({"acrobot": "Acrobot-v1", "mountaincar": "MountainCar-v0"}[kind], agent=agent,
                                 device=DEV, **kw)


def _test_envs(agent, n):
    """n test envs of the member's own config (its env seed and time limit)."""
    from xuanpolicy_amd.runner import make_envs
    cfg = deepcopy(agent.config)
    cfg.parallels = n
    return make_envs(cfg, DEV)


def _stats(agent):
    return [_np(agent.obs_mean), _np(agent.obs_var), _np(agent.obs_count)]


def _env_state(env):
    return [_np(env.state), _np(env.ep_index), _np(env.ep_step), _np(env.obs)]


def _assert_equal_lists(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(x, y, err_msg="%s[%d]" % (what, i))


def _assert_logs_equal(got, want, what):
    assert got.keys() == want.keys(), what
    for k in want:
        np.testing.assert_array_equal(np.asarray(got[k]), np.asarray(want[k]), err_msg="%s: %s" % (what, k))


TRAIN_STATE = ("obs_norm", "returns", "ret_mean", "ret_var", "ret_count", "cursor", "slot_obs", "slot_t",
               "slot_overflow", "boot_obs")


def _training_state(agent):
    """Everything of a member an evaluation must leave alone (the obs statistics are not in it)."""
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


# ---- 1. the batch equals each member's own launch --------------------------------------------------------------------
# (kind, agent, hidden, test envs N, obs-norm, time limit, test_episode, member seeds).  The CartPole seeds and targets
# were chosen on an MI355X so that the twins stop at different steps (deterministic: counter-hash RNG) — 35, 35 and 36
# steps at N = 8; 24, 22 and 23 at N = 70, where the 78th episode is the eighth second episode of an env that fell
# before the time limit — and the test asserts it.
CASES = {
    "cartpole-64-N8-obsnorm": ("cartpole", "PPO_Clip", 64, 8, True, 12, 20, (3, 4, 5)),
    "cartpole-32-N70": ("cartpole", "PPO_Clip", 32, 70, False, 12, 78, (2, 3, 4)),
    "pendulum-64-N8": ("pendulum", "PPO_Clip", 64, 8, True, 5, 20, (3, 4, 5)),
    "mountaincar-64-N8-a2c": ("mountaincar", "A2C", 64, 8, True, 12, 20, (3, 4, 5)),
}


def _members(case):
    kind, agent, hidden, _, obsnorm, max_ep, _, seeds = CASES[case]
    return [_build(kind, agent=agent, n_envs=5, n_steps=48, hidden=hidden, seed=s, max_episode_steps=max_ep,
                   use_obsnorm=obsnorm) for s in seeds]


@pytest.mark.parametrize("case", sorted(CASES))
def test_population_test_device_equals_each_members_own(case):
    from xuanpolicy_amd.population import Population
    kind, _, hidden, N, _, _, target, _ = CASES[case]
    set_a, set_b = _members(case), _members(case)
    pop = Population(set_a)
    envs_a, envs_b = [_test_envs(a, N) for a in set_a], [_test_envs(b, N) for b in set_b]
    plan = pop.plan_test(envs_a)
    assert plan.n_agents == 3 and plan.gaussian == (kind == "pendulum")
    before = [_training_state(a) for a in set_a]
    got = pop.test_device(envs_a, target, rngs=[(a.seed, 0) for a in set_a])
    want = [b.test_device(e, target, rng=(b.seed, 0)) for b, e in zip(set_b, envs_b)]
    torch.cuda.synchronize()
    steps_run = [b.last_test_log["steps_run"] for b in set_b]
    print(case, "steps_run", steps_run, "count", [b.last_test_log["count"] for b in set_b])
    for p, (a, b) in enumerate(zip(set_a, set_b)):
        tag = "member %d" % p
        assert b.plan_test(envs_b[p]) == "K32E"
        assert got[p] == want[p] and len(got[p]) >= target, tag
        assert a.last_test_log["done"] and not a.last_test_log["overflow"]
        _assert_logs_equal(a.last_test_log, b.last_test_log, tag)
        _assert_equal_lists(_stats(a), _stats(b), tag + " obs_rms")
        _assert_equal_lists(_env_state(envs_a[p]), _env_state(envs_b[p]), tag + " env")
        after = _training_state(a)
        for k in before[p]:
            np.testing.assert_array_equal(np.asarray(after[k]), np.asarray(before[p][k]), err_msg=tag + ": " + k)
    assert not np.array_equal(_np(envs_a[0].obs), _np(envs_a[1].obs))   # different members
    if kind == "cartpole":   # the members stop at different steps: the independent stop is exercised
        assert len(set(steps_run)) > 1, steps_run
    # the evaluation's own stream: the cursor is made on first use and continues across calls, as each member's does
    for _ in range(2):
        got = pop.test_device(envs_a, target, chunk=7)
        want = [b.test_device(e, target, chunk=7) for b, e in zip(set_b, envs_b)]
        for p, (a, b) in enumerate(zip(set_a, set_b)):
            assert got[p] == want[p]
            np.testing.assert_array_equal(_np(a._eval_cursor), _np(b._eval_cursor))
            assert int(a._eval_cursor[1]) > 0
            _assert_logs_equal(a.last_test_log, b.last_test_log, "member %d, own stream" % p)
            _assert_equal_lists(_stats(a) + _env_state(envs_a[p]), _stats(b) + _env_state(envs_b[p]), "own stream")
    for a in set_a:
        assert _np(a.cursor).tolist() == [0, 0, 0, 0]   # the training stream was not advanced


# ---- 2. independent stop and queued launches, by construction -------------------------------------------------------
def _raw_batch(code, blocks, heads, evals, n_agents=None):
    """xpa_small_eval_batch on lists of argument structs, uploaded as they stand; returns the status."""
    from xuanpolicy_amd import _lib
    from xuanpolicy_amd.population import _block_array

    def pair(struct, items):
        if not items:
            return None, None
        arr = _block_array(struct, items)
        return arr, torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)

    def addrs(p):   # (host address, device address) of an uploaded array; (NULL, NULL) without one
        return (None, None) if p[0] is None else (ctypes.addressof(p[0]), p[1].data_ptr())
    # the arrays stay referenced until the launch has run
    b, h, e = pair(_lib.XpaSmallRolloutArgs, blocks), pair(_lib.XpaSmallRolloutHead, heads), pair(_lib.XpaSmallEval, evals)
    rc = _lib.load().xpa_small_eval_batch(
        _lib.ENV_CODES[code], len(blocks) if n_agents is None else n_agents, *addrs(b), *addrs(h), *addrs(e),
        ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    torch.cuda.synchronize()
    del b, h, e
    return rc


def _stop_member(seed, cursor_step=5):
    """A CartPole member over 70 test envs that all truncate at their third step, its K32E block (2 steps per
    launch) on a cursor of its own."""
    from xuanpolicy_amd import ops
    agent = _build("cartpole", n_envs=5, n_steps=16, hidden=64, seed=seed, max_episode_steps=3)
    env = _test_envs(agent, 70)
    cursor = ops.new_cursor(DEV)
    cursor[1] = cursor_step
    args, _ = agent._build_small_eval(env, 7 + seed, cursor)
    args.steps = 2
    return agent, env, cursor, args


def test_members_stop_independently_and_queued_launches_change_nothing():
    from xuanpolicy_amd import _lib, ops
    from xuanpolicy_amd.rollout_plan import eval_entry
    N, targets, capacity, GUARD, SEEDS = 70, (10, 80, 150), 150 + 70, 4, (2, 3, 4)
    set_a, set_b = [_stop_member(s) for s in SEEDS], [_stop_member(s) for s in SEEDS]
    D = set_a[0][0].obs_dim
    total = ops.eval_log_layout(capacity, D)[1]
    logs = ops.eval_logs_new(targets, N, D, DEV, capacity=capacity, guard=GUARD)
    assert logs.shape == (3, total + GUARD) and all(logs[p].data_ptr() % 16 == 0 for p in range(3))
    scratch = torch.empty((3, 3 * N), dtype=torch.float32, device=DEV)
    evals = [_lib.XpaSmallEval(logs[p].data_ptr(), scratch[p].data_ptr(), capacity, D) for p in range(3)]
    blocks = [m[3] for m in set_a]

    def state():
        out = [_np(logs)]
        for agent, env, cursor, _ in set_a:
            out += [_np(cursor)] + _stats(agent) + _env_state(env)
        return out
    for _ in range(5):      # 10 steps issued without a look at the logs: the members need 3, 6 and 9
        assert _raw_batch("XPA_ENV_CARTPOLE", blocks, None, evals) == 0
    first = state()
    assert _raw_batch("XPA_ENV_CARTPOLE", blocks, None, evals) == 0
    _assert_equal_lists(state(), first, "a sixth launch")
    words = first[0]
    assert (words[:, total:] == -1).all()                       # the guard words behind each row
    outs = [ops.eval_log_decode(words[p, :total]) for p in range(3)]
    assert [o["steps_run"] for o in outs] == [3, 6, 9] and all(o["done"] and not o["overflow"] for o in outs)
    assert [o["count"] for o in outs] == [70, 140, 210] and [len(o["score"]) for o in outs] == [70, 140, 210]
    assert [_np(m[2]).tolist() for m in set_a] == [[0, 5 + s, 0, 0] for s in (3, 6, 9)]
    # each member's row is what the single-agent entry leaves for a twin with the same target, launched until done
    for p, (agent, env, cursor, args) in enumerate(set_b):
        log = ops.eval_log_new(targets[p], N, D, DEV, capacity=capacity, guard=GUARD)
        own = torch.empty((3 * N,), dtype=torch.float32, device=DEV)
        entry = eval_entry(agent._eval_facts(env))
        for _ in range(8):
            ops.small_eval(entry, args, log, capacity, D, own)
            if ops.eval_log_header(log)["done"]:
                break
        a_agent, a_env, a_cursor, _ = set_a[p]
        np.testing.assert_array_equal(words[p], _np(log), err_msg="member %d: log row" % p)
        _assert_equal_lists([_np(a_cursor)] + _stats(a_agent) + _env_state(a_env),
                            [_np(cursor)] + _stats(agent) + _env_state(env), "member %d" % p)
        np.testing.assert_array_equal(_np(scratch[p]), _np(own), err_msg="member %d: scratch" % p)


# ---- 3. refusals ------------------------------------------------------------------------------------------------------
def _refusal_set(kind, n):
    """n members of one kind over 8 test envs with everything a launch would need: (code, blocks, heads, evals, logs)."""
    from xuanpolicy_amd import _lib, ops
    from xuanpolicy_amd.rollout_plan import SMALL_ENVS
    N, target = 8, 5
    agents = [_build(kind, n_envs=5, n_steps=48, hidden=64, seed=s + 1, max_episode_steps=12) for s in range(n)]
    envs = [_test_envs(a, N) for a in agents]
    D = agents[0].obs_dim
    logs = ops.eval_logs_new([target] * n, N, D, DEV)
    scratch = torch.empty((n, 3 * N), dtype=torch.float32, device=DEV)
    blocks, heads, evals, cursors = [], [], [], []
    for p, (a, e) in enumerate(zip(agents, envs)):
        cursors.append(ops.new_cursor(DEV))
        args, logstd = a._build_small_eval(e, 11 + p, cursors[-1])
        args.steps = 4
        blocks.append(args)
        if logstd is not None:
            heads.append(_lib.XpaSmallRolloutHead(logstd.data_ptr(), 2.0))
        evals.append(_lib.XpaSmallEval(logs[p].data_ptr(), scratch[p].data_ptr(), target + N, D))
    row = SMALL_ENVS[kind, agents[0].dist]
    return row.code, blocks, heads, evals, logs, (agents, envs, scratch, cursors)


def _copies(items):
    out = []
    for it in items:
        c = type(it)()
        ctypes.memmove(ctypes.addressof(c), ctypes.addressof(it), ctypes.sizeof(it))
        out.append(c)
    return out


def test_refusals_launch_nothing():
    from xuanpolicy_amd import _lib
    code, blocks, _, evals, logs, keep = _refusal_set("cartpole", 3)
    clean = _np(logs)
    assert (clean[:, [0, 2, 3, 4]] == 0).all() and (clean[:, 1] == 5).all() and (clean[:, 8:] == 0).all()

    def refused(what, change, n_agents=None, heads=None, on=(code, blocks, evals, logs, clean)):
        c, b0, e0, lg, want = on
        b, e = _copies(b0), _copies(e0)
        change(b, e)
        assert _raw_batch(c, b, heads, e, n_agents=n_agents) == 1, what
        np.testing.assert_array_equal(_np(lg), want, err_msg=what)
    refused("n_agents = 0", lambda b, e: None, n_agents=0)
    refused("another n_envs", lambda b, e: setattr(b[1], "n_envs", 7))
    refused("another steps", lambda b, e: setattr(b[2], "steps", 5))

    def wide(b, e):
        for x in b:
            x.h0 = x.h1 = x.h2 = 128
    refused("h0 = 128", wide)
    refused("a NULL log", lambda b, e: setattr(e[1], "log", None))
    refused("a log at a 4-B offset", lambda b, e: setattr(e[1], "log", e[1].log + 4))
    refused("two members with the same log", lambda b, e: setattr(e[2], "log", e[0].log))
    refused("differing capacity", lambda b, e: setattr(e[1], "capacity", e[1].capacity - 1))
    refused("head arrays for cartpole", lambda b, e: None,
            heads=[_lib.XpaSmallRolloutHead(keep[0][0].obs_mean.data_ptr(), 2.0) for _ in range(3)])
    pcode, pblocks, pheads, pevals, plogs, pkeep = _refusal_set("pendulum", 2)
    assert len(pheads) == 2
    refused("head arrays missing for pendulum", lambda b, e: None, heads=None,
            on=(pcode, pblocks, pevals, plogs, _np(plogs)))
    # the same arrays, untouched, are accepted: the refusals above were refusals of the change alone
    assert _raw_batch(code, blocks, None, evals) == 0
    assert _raw_batch(pcode, pblocks, pheads, pevals) == 0
    torch.cuda.synchronize()
    assert (_np(logs)[:, 3] == 4).all() and (_np(plogs)[:, 3] == 4).all()   # four steps each


# ---- 4. the public surface ----------------------------------------------------------------------------------------------
def _surface_set(hidden, seeds=(1, 2, 3)):
    kw = dict(n_envs=5, n_steps=32, n_epoch=2, n_minibatch=2, max_episode_steps=40, hidden=hidden, device_test=True)
    agents = [_build("cartpole", seed=s, **kw) for s in seeds]
    hooks = [[] for _ in agents]
    for a, h in zip(agents, hooks):
        a.log_hook = lambda info, step, h=h: h.append((dict(info), step))
    return agents, hooks


def _env_fn(made):
    from xuanpolicy_amd.envs import CartPoleVecEnv

    def env_fn():
        env = CartPoleVecEnv(3, seed=1, max_episode_steps=20, device=DEV)
        env.closed = 0
        env.close = lambda: setattr(env, "closed", env.closed + 1)
        made.append(env)
        return env
    return env_fn


def _agent_state(a):
    fused = a.learner.fused_opt
    out = {"sd/" + k: _np(v) for k, v in a.policy.state_dict().items()}
    out.update({"train/" + k: v for k, v in _training_state(a).items()})
    out.update(exp_avg=_np(fused.exp_avg), exp_avg_sq=_np(fused.exp_avg_sq), obs_mean=_np(a.obs_mean),
               obs_var=_np(a.obs_var), obs_count=_np(a.obs_count))
    return out


def test_population_test_surface_and_training_afterwards():
    from xuanpolicy_amd.population import Population
    (set_a, hooks_a), (set_b, hooks_b) = _surface_set(64), _surface_set(64)
    pop = Population(set_a)
    made_a, made_b = [], []
    calls = []
    real = pop.test_device
    pop.test_device = lambda *a, **k: calls.append(1) or real(*a, **k)
    got = pop.test(_env_fn(made_a), 4)
    want = [b.test(_env_fn(made_b), 4) for b in set_b]
    assert len(calls) == 1 and got == want and all(len(s) >= 4 for s in got)
    assert len(made_a) == 3 and [e.closed for e in made_a] == [1, 1, 1]
    keys = {"Test-Episode-Rewards/Mean-Score", "Test-Episode-Rewards/Std-Score"}
    for p, (a, b) in enumerate(zip(set_a, set_b)):
        assert hooks_a[p] == hooks_b[p] and len(hooks_a[p]) == 1 and set(hooks_a[p][0][0]) == keys
        assert hooks_a[p][0][0]["Test-Episode-Rewards/Mean-Score"] == float(np.mean(got[p]))
        _assert_logs_equal(a.last_test_log, b.last_test_log, "member %d" % p)
        np.testing.assert_array_equal(_np(a._eval_cursor), _np(b._eval_cursor))
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


def test_ineligible_members_raise_in_test_device_and_loop_in_test():
    """128-wide members train as a population (K32W) but have no one-launch evaluation: test_device raises, test()
    is the per-member loop (each member's own "steps" tier)."""
    from xuanpolicy_amd.population import Population
    (set_a, _), (set_b, _) = _surface_set(128, seeds=(1, 2)), _surface_set(128, seeds=(1, 2))
    pop = Population(set_a)
    made_a, made_b = [], []
    with pytest.raises(ValueError, match="member 0: its test envs plan the 'steps' tier"):
        pop.test_device([_env_fn(made_a)() for _ in set_a], 4)
    del made_a[:]
    got = pop.test(_env_fn(made_a), 4)
    want = [b.test(_env_fn(made_b), 4) for b in set_b]
    assert got == want and all(len(s) >= 4 for s in got)
    assert len(made_a) == 2 and [e.closed for e in made_a] == [1, 1]
    for a, b in zip(set_a, set_b):
        _assert_logs_equal(a.last_test_log, b.last_test_log, "steps tier")
        _assert_equal_lists(_stats(a), _stats(b), "obs_rms")
