"""GPU: Acrobot-v1 and MountainCar-v0 on the device, in the one-launch small path.

  * K18A / K18M (xpa_acrobot_step, xpa_mountaincar_step) against tests/_acrobot_ref.py / _mountaincar_ref.py (numpy f64
    restatements of the header's equations).
  * K32's two instantiations (xpa_small_rollout_acrobot / _mountaincar: observation widths 6 and 8) against the
    multi-kernel step, their transitions against the checkers, their sampler against K3.
  * K30 (xpa_small_mlp_update) at the two new shapes against the multi-kernel update.
  * K32E (xpa_small_eval_acrobot / _mountaincar) against K32 stepped one launch at a time.
  * The public surface (get_runner on the committed configs) and an iteration against the CPU oracle learner."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref
from tests import _acrobot_ref as aref
from tests import _mountaincar_ref as mref
from tests._oracle_replay import _load_by_order, replay_last_step_iteration

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# kind -> (env id, checker module, checker class, observation width, f64 states planted so that terminations occur)
ENVS = {
    "acrobot": ("Acrobot-v1", aref, aref.AcrobotRef, 6, [[3.0, 0.0, 0.0, 0.0]]),
    "mountaincar": ("MountainCar-v0", mref, mref.MountainCarRef, 8, [[0.49, 0.03], [-1.19, -0.05]]),
}
KINDS = sorted(ENVS)


@pytest.fixture(scope="module", autouse=True)
def _setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cpu_ref.build_oracle()


def _np(t):
    return t.detach().cpu().numpy().copy()


def _plant(env, kind, rows):
    """Write the kind's planted states into env.state at `rows` (cycling through them); returns them as [len(rows), S]."""
    planted = np.asarray(ENVS[kind][4], np.float64)
    st = planted[np.arange(len(rows)) % len(planted)]
    env.state[torch.as_tensor(np.asarray(rows), device=DEV)] = torch.as_tensor(st, device=DEV)
    return st


def _make_env(kind, n, seed, max_ep):
    from xuanpolicy_amd.envs import AcrobotVecEnv, MountainCarVecEnv
    return {"acrobot": AcrobotVecEnv, "mountaincar": MountainCarVecEnv}[kind](n, seed=seed, max_episode_steps=max_ep,
                                                                              device=DEV)


# ---- 1. the env steps against the checkers -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_env_step_matches_reference(kind):
    """40 steps of 16 envs with time limit 7 and uniform random actions; at steps 2, 11, 20 and 33 the kind's planted
    states are written into four envs, so that terminations occur beside the truncations (Acrobot: th1 = 3, where
    -cos th1 - cos(th1 + th2) = 1.98; MountainCar: one step short of the goal, and one step short of the left wall).
    The checker is re-seeded from the device's f64 state (MountainCar: and its frame stack) before every step, so a
    last-ulp difference between libm and ocml in sin / cos cannot compound.  One-step state error: rtol 1e-12, atol
    1e-14, the Pendulum test's figures (measured on an MI355X against numpy: Acrobot's RK4 step max 5.6e-17 absolute /
    7.9e-16 relative, MountainCar 4.3e-19 / 2.3e-16; the test prints them).  Observations and rewards at rtol 1e-6, no absolute term
    (measured: the f32 observations are equal to the checker's to the bit on these trajectories); flags, ep_step, ep_index, reset states and MountainCar's frame shift exact.  The first 20 steps go through the host
    step(), the rest write the one-hot rows into act_in.  Acrobot's termination compare is asserted away from its
    boundary, on the checker alone: |-cos th1 - cos(th1 + th2) - 1| > 1e-9 at every compared step."""
    env_id, ref_mod, Ref, D, _ = ENVS[kind]
    N, steps, max_ep, seed = 16, 40, 7, 5
    env = _make_env(kind, N, seed, max_ep)
    ref = Ref(N, seed, max_ep)
    assert env.kind == kind and env.observation_space.shape == (D,) and env.action_space.n == 3
    assert env.max_episode_steps == max_ep and env.act_in.shape == (N, 3)
    if kind == "mountaincar":
        np.testing.assert_array_equal(env.observation_space.low, np.array([-1.2, -0.07] * 4, np.float32))
        np.testing.assert_array_equal(env.observation_space.high, np.array([0.6, 0.07] * 4, np.float32))
    np.testing.assert_array_equal(_np(env.state), ref.state)
    np.testing.assert_array_equal(_np(env.obs), ref.obs())
    rng = np.random.default_rng(1)
    n_term = n_trunc = 0
    max_rel = max_abs = max_obs = 0.0
    for t in range(steps):
        if t in (2, 11, 20, 33):
            _plant(env, kind, [1, 6, 10, 15])
        ref.state = _np(env.state)                       # re-seed: state, score, (MountainCar) the frame stack
        ref.ep_score = _np(env.ep_score)
        prev_obs = _np(env.obs)
        if kind == "mountaincar":
            ref.stack = prev_obs.copy()
        a = rng.integers(0, 3, N)
        if t < 20:
            obs, rew, term, trunc, infos = env.step(a)
            ep_step = np.array([i["episode_step"] for i in infos])
            ep_score = np.array([i["episode_score"] for i in infos], np.float32)
        else:
            onehot = np.zeros((N, 3), np.float32)
            onehot[np.arange(N), a] = 1.0
            env.act_in.copy_(torch.as_tensor(onehot, device=DEV))
            env.step_device()
            obs, rew = _np(env.final_obs), _np(env.rew)
            term, trunc = _np(env.term).astype(bool), _np(env.trunc).astype(bool)
            done = term | trunc
            ep_step = np.where(done, _np(env.ep_last_len), _np(env.ep_step))
            ep_score = np.where(done, _np(env.ep_last_score), _np(env.ep_score))
        f_obs, r_rew, r_term, r_trunc, r_next, r_len, r_score = ref.step(a)
        if kind == "acrobot":
            assert np.abs(aref.terminal_margin(ref.stepped)).min() > 1e-9, "step %d" % t
        nz = f_obs != 0
        if nz.any():
            max_obs = max(max_obs, float((np.abs(obs.astype(np.float64) - f_obs)[nz] / np.abs(f_obs[nz])).max()))
        np.testing.assert_allclose(obs, f_obs, rtol=1e-6, atol=0, err_msg="step %d" % t)
        np.testing.assert_allclose(rew, r_rew, rtol=1e-6, err_msg="step %d" % t)
        np.testing.assert_array_equal(term, r_term, err_msg="step %d" % t)
        np.testing.assert_array_equal(trunc, r_trunc, err_msg="step %d" % t)
        np.testing.assert_array_equal(ep_step, r_len)
        np.testing.assert_allclose(ep_score, r_score, rtol=1e-6)
        np.testing.assert_array_equal(_np(env.ep_index), ref.ep_index)
        np.testing.assert_array_equal(_np(env.ep_step), ref.ep_step)
        done = term | trunc
        nxt = _np(env.obs)
        np.testing.assert_array_equal(nxt[done], r_next[done])               # hashed reset: exact
        np.testing.assert_array_equal(nxt[~done], obs[~done])
        if kind == "mountaincar":                                            # the frame shift: exact
            np.testing.assert_array_equal(obs[:, :6], prev_obs[:, 2:])
            np.testing.assert_array_equal(nxt[done], np.tile(nxt[done][:, :2], (1, 4)))
        if t < 20:
            for i in np.nonzero(done)[0]:
                np.testing.assert_array_equal(infos[i]["reset_obs"], r_next[i])
        st = _np(env.state)
        np.testing.assert_array_equal(st[done], ref.state[done])             # reset states: exact
        err = np.abs(st[~done] - ref.state[~done])
        if err.size:
            max_abs = max(max_abs, float(err.max()))
            max_rel = max(max_rel, float((err / np.maximum(np.abs(ref.state[~done]), 1e-300)).max()))
        np.testing.assert_allclose(st, ref.state, rtol=1e-12, atol=1e-14, err_msg="step %d" % t)
        n_term += int(term.sum())
        n_trunc += int(trunc.sum())
    print("%s: one-step state error against numpy f64: max abs %.3g, max rel %.3g; observations max rel %.3g"
          % (kind, max_abs, max_rel, max_obs))
    assert n_term >= 8 and n_trunc >= 4 * N


# ---- 2. K32 against the multi-kernel step ------------------------------------------------------------------------------
def _build(kind, **kw):
    from xuanpolicy_amd.runner import build_classic_control
    return build_classic_control(ENVS[kind][0], device=DEV, **kw)


def _snapshot(agent):
    mem, env = agent.memory, agent.envs
    logp = mem.auxiliary_infos["old_logp"] if agent.algo == "ppo" else agent.logp_scratch
    return {k: _np(v) for k, v in dict(
        obs=mem.observations, act=mem.actions, rew=mem.rewards, term=mem.terminals, closed=mem.closed, boot=mem.boot,
        slot_t=agent.slot_t, slot_obs=agent.slot_obs, boot_obs=agent.boot_obs, obs_mean=agent.obs_mean,
        obs_var=agent.obs_var, obs_count=agent.obs_count, ret_mean=agent.ret_mean, ret_var=agent.ret_var,
        ret_count=agent.ret_count, returns=agent.returns, state=env.state, env_obs=env.obs, ep_index=env.ep_index,
        ep_step=env.ep_step, ep_score=env.ep_score, cursor=agent.cursor, obs_norm=agent.obs_norm, val=mem.values,
        logp=logp, trunc=env.trunc, env_term=env.term, overflow=agent.slot_overflow).items()}


EXACT = ("act", "term", "closed", "slot_t", "ep_index", "ep_step", "cursor", "trunc", "env_term", "overflow",
         "ret_count", "obs_mean", "obs_var", "obs_count")


@pytest.mark.parametrize("n_envs", [5, 48, 70])
@pytest.mark.parametrize("obsnorm", [True, False])
@pytest.mark.parametrize("hidden", [32, 64])
@pytest.mark.parametrize("agent_name", ["PPO_Clip", "A2C"])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_rollout_matches_multi_kernel_steps(kind, agent_name, hidden, obsnorm, n_envs):
    """K32's Acrobot / MountainCar instantiations against the multi-kernel step (K5, obs_normalize, the torch forward,
    K3, K18A / K18M, K8) from the same start: n_steps 32 with graph_chunk 24, so train(24) is ONE 24-step K32 launch and
    no update; time limit 7 (three truncations per env, the deferred slots fill) and the planted states in every third
    env (terminations at the first step).  n_envs 5 takes the obs-RMS sums' one-row-per-group path, 48 is past
    256 / D row groups for both widths (42 at D = 6, 32 at D = 8) and within one wave for ret_rms, 70 takes the
    block-sum ret_rms merge.  Everything but the forward is the same arithmetic: the integer and flag columns, the
    actions and the obs-RMS state are exact; float columns at the Pendulum test's 1e-4 / 1e-5."""
    res = []
    for fused in (True, False):
        agent = _build(kind, agent=agent_name, n_envs=n_envs, n_steps=32, hidden=hidden, seed=9, max_episode_steps=7,
                       fused_rollout=fused, use_obsnorm=obsnorm, graph_chunk=24)
        assert agent.defer_boot and agent.dist == "categorical" and agent.n_slots >= 4
        _plant(agent.envs, kind, list(range(0, n_envs, 3)))
        agent.train(24, log=False)
        torch.cuda.synchronize()
        plan = agent.plan()
        assert (plan.driver == "K32") == fused and plan.chunk == 24
        launches = plan.step_launches()
        assert launches == ["xpa_small_rollout_%s" % kind] if fused else "xpa_%s_step" % kind in launches
        res.append(_snapshot(agent))
    f, m = res
    assert f["cursor"][:2].tolist() == [24, 24] and f["overflow"].sum() == 0
    planted = np.asarray(ENVS[kind][4], np.float64)[np.arange(len(range(0, n_envs, 3))) % len(ENVS[kind][4])]
    n_term0 = int(ENVS[kind][1].step(planted, np.ones(len(planted)))[2].sum())   # MountainCar: the goal state only
    assert (f["slot_t"] >= 0).sum() >= 2 * n_envs and f["term"][:, 0].sum() == n_term0 > 0
    for k in f:
        if k in EXACT:
            np.testing.assert_array_equal(f[k], m[k], err_msg=k)
        elif k in ("obs", "rew", "boot", "val", "logp"):
            np.testing.assert_allclose(f[k][:, :24], m[k][:, :24], rtol=1e-4, atol=1e-5, err_msg=k)
        else:
            np.testing.assert_allclose(f[k], m[k], rtol=1e-4, atol=1e-5, err_msg=k)


# ---- 2b / 2c. K32's transitions and sampler over a full rollout --------------------------------------------------------
@pytest.fixture(scope="module", params=KINDS)
def rollout127(request):
    """127 steps of the 8-env PPO agent as ONE K32 launch (graph_chunk 127), without observation / reward
    normalisation: the buffer holds the raw observations and rewards."""
    kind = request.param
    agent = _build(kind, n_envs=8, n_steps=128, hidden=64, seed=11, max_episode_steps=40, use_obsnorm=False,
                   use_rewnorm=False, graph_chunk=127)
    assert agent.plan().driver == "K32" and agent.plan().chunk == 127
    agent.train(127, log=False)
    torch.cuda.synchronize()
    assert _np(agent.cursor)[:2].tolist() == [127, 127]
    return kind, agent, _snapshot(agent)


def _states_of(kind, obs):
    """f64 env states recovered from f32 observations [n, D]."""
    o = obs.astype(np.float64)
    if kind == "acrobot":
        return np.stack([np.arctan2(o[:, 1], o[:, 0]), np.arctan2(o[:, 3], o[:, 2]), o[:, 4], o[:, 5]], axis=1)
    return o[:, 6:8]


def test_fused_rollout_transitions_follow_the_env_equations(rollout127):
    """Every stored transition of the K32 rollout, drift-free: the state recovered from buffer column t, stepped by the
    checker with the stored action, gives column t + 1 and the stored reward at 1e-5 (MountainCar: columns 0..5 of
    column t + 1 are columns 2..7 of column t exactly); after a done the next column is the hashed reset state's
    observation exactly."""
    kind, agent, s = rollout127
    ref_mod = ENVS[kind][1]
    obs, act, rew, closed = s["obs"], s["act"], s["rew"], s["closed"].astype(bool)
    N = 8
    ep = np.zeros(N, np.int64)
    n_reset = n_plain = 0
    assert set(np.unique(act[:, :127]).tolist()) == {0.0, 1.0, 2.0}
    for t in range(126):
        nxt, r, _ = ref_mod.step(_states_of(kind, obs[:, t]), act[:, t])
        np.testing.assert_allclose(rew[:, t], r, rtol=0, atol=1e-5, err_msg="reward, column %d" % t)
        done = closed[:, t]
        ep += done
        if kind == "acrobot":
            want = aref.obs_of(nxt)
        else:
            want = mref.push(obs[:, t], nxt)
            np.testing.assert_array_equal(obs[~done, t + 1, :6], obs[~done, t, 2:])
        np.testing.assert_allclose(obs[~done, t + 1], want[~done], rtol=0, atol=1e-5, err_msg="column %d" % (t + 1))
        if done.any():
            reset = ref_mod.obs_of(ref_mod.reset_states(agent.envs.noise_seed, np.arange(N)[done], ep[done]))
            np.testing.assert_array_equal(obs[done, t + 1], reset)
        n_reset += int(done.sum())
        n_plain += int((~done).sum())
    assert n_reset >= 3 * N and n_plain > 900


def test_fused_rollout_sampler_matches_k3(rollout127):
    """The actions and log-probs K32 stored against K3 (xpa_rollout_sample) run on logits from the f64 oracle policy on
    the stored observations with the same seed / step.  The two forwards differ by f32 rounding, which can move a CDF
    boundary by ~1e-6: every sample whose uniform (the counter hash of (seed, step, env), restated here) lies further
    than 1e-5 from the oracle's CDF boundaries must be the same action — of 1016 samples about 0.04 are expected to be
    nearer —, and there the log-probs agree at replay_last_step_iteration's 1e-4 / 2e-4, as do all values."""
    from xuanpolicy_amd import ops
    from xuanpolicy_amd.envs import _hash4, _u01
    kind, agent, s = rollout127
    D = ENVS[kind][3]
    N, T = 8, 128
    pol = cpu_ref.build_actor_critic_ref(D, 3, [64], [64], [64], discrete=True, activation=agent.config.activation)
    _load_by_order(pol, agent)
    pol.double()
    with torch.no_grad():
        logits, _, v = pol.heads(torch.as_tensor(s["obs"].reshape(N * T, D).astype(np.float64)))
    cdf = np.cumsum(torch.softmax(logits, -1).reshape(N, T, 3).numpy(), -1)[:, :127, :2]
    logits = logits.reshape(N, T, 3).float().to(DEV)
    v = v.reshape(N, T).float().to(DEV)
    b_act, b_logp, b_val = (torch.zeros((N, T), dtype=torch.float32, device=DEV) for _ in range(3))
    env_in = torch.zeros((N, 3), dtype=torch.float32, device=DEV)
    cur = ops.new_cursor(DEV)
    for t in range(127):
        cur.copy_(torch.tensor([t, t, 0, 0], dtype=torch.int32))
        ops.rollout_sample("categorical", logits[:, t].contiguous(), None, v[:, t].contiguous(), cur, agent.seed, b_act,
                           b_logp, b_val, env_in)
    torch.cuda.synchronize()
    # K3's uniform: xpa_u01(xpa_hash4(seed ^ 0xAC7105ED, step, env, 0))
    u = _u01(_hash4(agent.seed ^ 0xAC7105ED, np.arange(127, dtype=np.uint32)[None, :],
                    np.arange(N, dtype=np.uint32)[:, None], np.uint32(0))).astype(np.float64)
    clear = np.abs(u[..., None] - cdf).min(-1) > 1e-5
    assert clear.mean() > 0.99
    want = (u[..., None] >= cdf).sum(-1).astype(np.float32)       # the first class whose CDF exceeds u
    np.testing.assert_array_equal(s["act"][:, :127][clear], want[clear])
    np.testing.assert_array_equal(_np(b_act)[:, :127][clear], want[clear])
    np.testing.assert_allclose(s["logp"][:, :127][clear], _np(b_logp)[:, :127][clear], rtol=1e-4, atol=2e-4)
    np.testing.assert_allclose(s["val"][:, :127], _np(b_val)[:, :127], rtol=1e-4, atol=2e-4)


# ---- 3. K30 at the new shapes ------------------------------------------------------------------------------------------
def _adv_partials(adv, idx):
    """K4's advantage moments of the minibatch: (sum, sumsq) in f64 per 64 rows (xpa_gather_num_partials)."""
    from xuanpolicy_amd import ops
    b = idx.shape[0]
    g = ops.gather_num_partials(b)
    a = torch.zeros((g * 64,), dtype=torch.float64, device=DEV)
    a[:b] = adv[idx].double()
    a = a.reshape(g, 64)
    return torch.stack([a.sum(1), (a * a).sum(1)], dim=1).contiguous()


@pytest.mark.parametrize("agent_name", ["PPO_Clip", "A2C"])
@pytest.mark.parametrize("d_in", [6, 8])
def test_small_update_matches_multi_kernel_update_at_the_new_shapes(d_in, agent_name):
    """K30 (xpa_small_mlp_update) against the multi-kernel update (K13 / hipBLASLt / K2 / K10) from the same weights
    on synthetic buffer rows at (d_in 6, k 3) and (d_in 8, k 3), hidden 64, a minibatch of 40 rows (ragged against the
    32-row workgroups), the split form on and off: the loss scalars and every parameter's raw gradient at the existing
    small-update tests' 1e-4 / 1e-5.  Learning rate 0 and no clipping, so both start every update from the same
    weights and the raw gradient stays in the flat buffer."""
    from xuanpolicy_amd.policies import policy_heads
    from xuanpolicy_amd.runner import build_synthbox_ppo
    pair = []
    for _ in range(2):
        agent = build_synthbox_ppo(n_envs=8, n_steps=16, obs_dim=d_in, act_dim=3, hidden=64, seed=13, device=DEV,
                                   agent=agent_name, discrete=True, learning_rate=0.0, ent_coef=0.01,
                                   graph_update=False)
        agent.learner._use_clip = False
        pair.append(agent)
    small, multi = pair
    assert small.dist == "categorical"
    gen = torch.Generator(device=DEV)
    gen.manual_seed(100 * d_in)
    n_rows, batch = 96, 40
    obs = torch.randn((n_rows, d_in), generator=gen, device=DEV)
    adv, ret = (torch.randn((n_rows,), generator=gen, device=DEV) for _ in range(2))
    with torch.no_grad():
        logits, _, _ = policy_heads(small.policy, obs)
        act = torch.randint(0, 3, (n_rows,), generator=gen, device=DEV)
        logp = torch.log_softmax(logits, -1).gather(1, act[:, None])[:, 0]
        old = (logp + 0.15 * torch.randn((n_rows,), generator=gen, device=DEV)).contiguous()
        act = act.float().contiguous()
    old_arg = old if small.algo == "ppo" else None
    idx = torch.randperm(n_rows, generator=gen, device=DEV)[:batch].contiguous()
    sc_m = multi.learner.update_fused(obs[idx].contiguous(), idx, act, adv, ret, old_arg,
                                      _adv_partials(adv, idx)).clone()
    g_m = [_np(p.grad) for p in multi.policy.parameters()]
    names = [n for n, _ in small.policy.named_parameters()]
    for split in (True, False):
        small.learner.small_split = split
        assert small.learner.small_update_ok(obs, batch)
        sc_s = small.learner.small_update(obs, idx, act, adv, ret, old_arg, use_advnorm=True).clone()
        torch.cuda.synchronize()
        np.testing.assert_allclose(_np(sc_s)[:6], _np(sc_m)[:6], rtol=1e-4, atol=1e-5, err_msg="split %s" % split)
        for n, p, gm in zip(names, small.policy.parameters(), g_m):
            assert np.abs(gm).max() > 0, n
            np.testing.assert_allclose(_np(p.grad), gm, rtol=1e-4, atol=1e-5, err_msg="split %s %s" % (split, n))
    assert all(torch.equal(p, q) for p, q in zip(small.policy.parameters(), multi.policy.parameters()))   # lr 0


# ---- 4. K32E against the training kernel -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_k32e_matches_single_step_k32_launches(kind):
    """test_device over 5 test envs and 3 episodes against agent A stepped one K32 launch at a time on the same action
    stream (tests/test_gpu_device_test.py's scheme): the same episodes — scores, lengths, order —, the same step count
    and the same obs-RMS and env state at the completing step, to the bit.  Time limit 7."""
    from xuanpolicy_amd.runner import make_envs
    N, target = 5, 3

    def build():
        return _build(kind, n_envs=N, n_steps=64, hidden=64, seed=4, max_episode_steps=7)
    A = build()
    assert A.plan().driver == "K32"
    env, entries = A.envs, []
    for s in range(63):
        A.train(1, log=False)
        te, tr = _np(env.term), _np(env.trunc)
        sc, ln = _np(env.ep_last_score), _np(env.ep_last_len)
        entries += [(s, i, sc[i], int(ln[i])) for i in range(N) if te[i] or tr[i]]
        if len(entries) >= target:
            break
    assert len(entries) >= target and s < 62
    want_stats = [_np(A.obs_mean), _np(A.obs_var), _np(A.obs_count)]
    want_env = [_np(env.state), _np(env.ep_index), _np(env.ep_step), _np(env.obs)]
    B = build()
    tenv = make_envs(B.config, DEV)
    assert tenv.kind == kind and tenv.num_envs == N
    scores = B.test_device(tenv, target, rng=(B.seed, 0))
    torch.cuda.synchronize()
    assert B.plan_test(tenv) == "K32E"
    log = B.last_test_log
    assert log["done"] and not log["overflow"] and log["steps_run"] == s + 1 and log["count"] == len(entries)
    assert list(zip(log["step"].tolist(), log["env"].tolist())) == [(e[0], e[1]) for e in entries]
    assert log["score"].tobytes() == np.asarray([e[2] for e in entries], np.float32).tobytes()
    assert log["length"].tolist() == [e[3] for e in entries]
    assert np.asarray(scores, np.float32).tobytes() == log["score"].tobytes()
    for got, want in zip([_np(B.obs_mean), _np(B.obs_var), _np(B.obs_count)], want_stats):
        np.testing.assert_array_equal(got, want)
    for got, want in zip([_np(tenv.state), _np(tenv.ep_index), _np(tenv.ep_step), _np(tenv.obs)], want_env):
        np.testing.assert_array_equal(got, want)


# ---- 5. the public surface ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["ppo", "a2c"])
@pytest.mark.parametrize("kind", KINDS)
def test_get_runner_builds_and_trains_on_the_small_path(kind, method):
    """get_runner on the committed configs as they stand: the plan's driver is K32 and its feed is K30's, and two
    training iterations leave finite scalars and parameters."""
    from xuanpolicy_amd.runner import get_runner
    runner = get_runner(method, "classic_control", ENVS[kind][0])
    agent = runner.agent
    assert runner.envs.kind == kind and agent.envs is runner.envs and agent.dist == "categorical"
    agent.train(2 * agent.n_steps, log=False)
    torch.cuda.synchronize()
    plan = agent.plan()
    assert plan.driver == "K32" and plan.feed == "small"
    assert plan.step_launches() == ["xpa_small_rollout_%s" % kind]
    assert torch.isfinite(agent.last_info).all()
    assert all(torch.isfinite(p).all() for p in agent.policy.parameters())


# ---- 6. an iteration against the CPU oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind,agent_name", [("acrobot", "PPO_Clip"), ("mountaincar", "A2C")])
def test_classic_iteration_matches_oracle(kind, agent_name):
    """test_pendulum_iteration_matches_oracle's replay with a Categorical head: one iteration through K32, then 127
    steps and the last step + GAE + 16 updates replayed by the f64 oracle learner at that test's tolerances; time
    limit 40, so mid-buffer truncation bootstraps occur."""
    N, T, H = 8, 128, 64
    D = ENVS[kind][3]
    agent = _build(kind, agent=agent_name, n_envs=N, n_steps=T, hidden=H, seed=3, n_epoch=4, n_minibatch=4,
                   max_episode_steps=40)
    assert agent.device_env and agent.defer_boot
    agent.train(T, log=False)
    agent.train(T - 1, log=False)
    plan = agent.plan()
    assert plan.driver == "K32" and plan.feed == "small"
    replay_last_step_iteration(agent, D, 3, [H], True, agent.algo, agent.config.ent_coef, 4, 4,
                               expect_mid_truncations=True)
