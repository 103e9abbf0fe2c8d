"""GPU: the one-launch small path at the reference's 128-wide classic-control nets.

  * K32W (xpa_small_rollout_<env> at h0 = h1 = h2 = 128) against the multi-kernel step for the four envs, its
    transitions against the env checkers and its sampler against K3 over a 127-step launch.
  * K30's one-image form (xpa_small_mlp_update / _gauss at hidden 128) against the multi-kernel update; the resident
    form at hidden 64 against values recorded from the commit before the one-image form (tests/golden/k30_h64.npz).
  * The public surface: get_runner on the committed CartPole-v1 config (hidden 128) and an iteration against the CPU
    oracle learner."""
import os

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from tests import _acrobot_ref as aref
from tests import _mountaincar_ref as mref
from tests import _pendulum_ref as pref
from tests._oracle_replay import _load_by_order, replay_last_step_iteration

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
H = 128
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k30_h64.npz")

# kind -> (env id, observation width, head width, f64 states planted so that terminations occur at the first step)
ENVS = {
    "cartpole": ("CartPole-v1", 4, 2, [[0.0, 0.0, 0.3, 0.0], [2.39, 2.0, 0.0, 0.0]]),   # past 12 degrees; past x = 2.4
    "pendulum": ("Pendulum-v1", 3, 1, None),                                             # never terminates
    "acrobot": ("Acrobot-v1", 6, 3, [[3.0, 0.0, 0.0, 0.0]]),
    "mountaincar": ("MountainCar-v0", 8, 3, [[0.49, 0.03], [-1.19, -0.05]]),
}
KINDS = sorted(ENVS)


@pytest.fixture(scope="module", autouse=True)
def _setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cpu_ref.build_oracle()


def _np(t):
    return t.detach().cpu().numpy().copy()


def _build(kind, agent="PPO_Clip", **kw):
    from xuanpolicy_amd.runner import build_cartpole_ppo, build_classic_control, build_pendulum_ppo
    if kind == "cartpole":   # the PPO config's keys for both agents (there is no A2C CartPole config: + its clip_grad)
        return build_cartpole_ppo(device=DEV, agent=agent, clip_grad=0.5, **kw)
    if kind == "pendulum":
        return build_pendulum_ppo(device=DEV, agent=agent, **kw)
    return build_classic_control(ENVS[kind][0], agent=agent, device=DEV, **kw)


def _plant(env, kind, rows):
    planted = np.asarray(ENVS[kind][3], np.float64)
    st = planted[np.arange(len(rows)) % len(planted)]
    env.state[torch.as_tensor(np.asarray(rows), device=DEV)] = torch.as_tensor(st, device=DEV)


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


def _uniforms(seed, n_envs, steps):
    """K3's uniform of (step, env): xpa_u01(xpa_hash4(seed ^ 0xAC7105ED, step, env, 0)), [n_envs, steps] f64."""
    from xuanpolicy_amd.envs import _hash4, _u01
    return _u01(_hash4(seed ^ 0xAC7105ED, np.arange(steps, dtype=np.uint32)[None, :],
                       np.arange(n_envs, dtype=np.uint32)[:, None], np.uint32(0))).astype(np.float64)


# ---- 1. K32W against the multi-kernel step --------------------------------------------------------------------------
# the Categorical sampler takes the first class whose cumulative probability exceeds the draw; the two forwards differ
# by f32 rounding (~1e-6 on a probability), so the actions can only be equal where no draw of the multi-kernel run lies
# within 1e-5 of a boundary.  Seed 9 has that property for all cases but two (measured margins 4.5e-5 .. 4.5e-3; the
# two: 8.4e-6); theirs is the smallest seed from 9 up with the property (10: 1.15e-5), computed on the multi-kernel run
# alone, and the test asserts the property for every case.
SEEDS = {("mountaincar", "PPO_Clip", True, 70): 10, ("mountaincar", "A2C", True, 70): 10}
EXACT = ("term", "closed", "slot_t", "ep_index", "ep_step", "cursor", "trunc", "env_term", "overflow", "ret_count",
         "obs_count")
EXACT_CAT = EXACT + ("act", "obs_mean", "obs_var")   # equal actions: equal observations and obs-RMS state too


def _cdf_margin(agent, snap, steps):
    """min over the first `steps` columns' draws of |u - the nearest cumulative-probability boundary|, from this
    agent's own policy (no update has run) on its own stored observations; and the classes those draws select."""
    from xuanpolicy_amd.policies import policy_heads
    N = agent.n_envs
    with torch.no_grad():
        logits, _, _ = policy_heads(agent.policy, torch.as_tensor(snap["obs"][:, :steps], device=DEV).reshape(
            N * steps, -1))
    cdf = np.cumsum(torch.softmax(logits.double(), -1).reshape(N, steps, -1).cpu().numpy(), -1)[..., :-1]
    u = _uniforms(agent.seed, N, steps)
    return float(np.abs(u[..., None] - cdf).min()), (u[..., None] >= cdf).sum(-1).astype(np.float32)


@pytest.mark.parametrize("n_envs", [5, 17, 70])
@pytest.mark.parametrize("obsnorm", [True, False])
@pytest.mark.parametrize("agent_name", ["PPO_Clip", "A2C"])
@pytest.mark.parametrize("kind", KINDS)
def test_wide_rollout_matches_multi_kernel_steps(kind, agent_name, obsnorm, n_envs):
    """K32W against the multi-kernel step (K5, obs_normalize, the torch forward, K3, the env's step kernel, K8) from the
    same start, test_gpu_classic's scheme at hidden 128: n_steps 32 with graph_chunk 24, so train(24) is ONE 24-step
    launch and no update; time limit 7 (three truncations per env, the deferred slots fill) and terminal states planted
    in every third env (Pendulum has none).  n_envs 5 is one ragged 16-env tile of the forward, 17 two tiles with the
    second ragged, 70 five tiles, the block-sum ret-RMS merge and past the 256 / D row groups of the obs-RMS sums.
    Everything but the forward is the same arithmetic: the integer and flag columns are exact, and so are the
    Categorical actions and with them the obs-RMS state — every draw of the multi-kernel run is asserted further than
    1e-5 from its CDF boundaries; Pendulum's Gaussian actions (which differ by the forwards' rounding, and the
    observations after them) and the float columns at that test's 1e-4 / 1e-5."""
    seed = SEEDS.get((kind, agent_name, obsnorm, n_envs), 9)
    cat = kind != "pendulum"
    res, margin = [], None
    for fused in (True, False):
        agent = _build(kind, agent=agent_name, n_envs=n_envs, n_steps=32, hidden=H, seed=seed, max_episode_steps=7,
                       fused_rollout=fused, use_obsnorm=obsnorm, graph_chunk=24)
        assert agent.defer_boot and agent.dist == ("categorical" if cat else "gaussian") and agent.n_slots >= 4
        if cat:
            _plant(agent.envs, kind, list(range(0, n_envs, 3)))
        agent.train(24, log=False)
        torch.cuda.synchronize()
        plan = agent.plan()
        assert plan.driver == ("K32W" if fused else "graph-chunk") and plan.chunk == 24
        launches = plan.step_launches()
        assert launches == ["xpa_small_rollout_%s" % kind] if fused else "xpa_%s_step" % kind in launches
        res.append(_snapshot(agent))
        if cat and not fused:
            margin, want = _cdf_margin(agent, res[-1], 24)
            print("%s %s obsnorm %s n_envs %d seed %d: min CDF margin of the multi-kernel run %.3g"
                  % (kind, agent_name, obsnorm, n_envs, seed, margin))
            np.testing.assert_array_equal(res[-1]["act"][:, :24], want)   # the sampler as restated here
    f, m = res
    if cat:
        assert margin > 1e-5, "a draw of the multi-kernel run within 1e-5 of a CDF boundary: pick another seed"
        assert f["term"][:, 0].sum() > 0
    assert f["cursor"][:2].tolist() == [24, 24] and f["overflow"].sum() == 0
    assert (f["slot_t"] >= 0).sum() >= 2 * n_envs
    for k in f:
        if k in (EXACT_CAT if cat else EXACT):
            np.testing.assert_array_equal(f[k], m[k], err_msg=k)
        elif k in ("obs", "act", "rew", "boot", "val", "logp"):
            np.testing.assert_allclose(f[k][:, :24], m[k][:, :24], rtol=1e-4, atol=1e-5, err_msg=k)
        else:
            np.testing.assert_allclose(f[k], m[k], rtol=1e-4, atol=1e-5, err_msg=k)


# ---- 2. K32W's transitions and sampler over a 127-step launch -------------------------------------------------------
def _cartpole_step(states, act):
    from oracle.synth_env import cartpole_dynamics
    out = [cartpole_dynamics(s.copy(), int(a)) for s, a in zip(states, act)]
    return np.stack([o[0] for o in out]), np.ones(len(out), np.float32), np.array([bool(o[1]) for o in out])


def _cartpole_resets(seed, envs, eps):
    from xuanpolicy_amd.envs import cartpole_reset_states
    return cartpole_reset_states(seed, envs, eps).astype(np.float32)


@pytest.mark.parametrize("kind", KINDS)
def test_wide_rollout_transitions_and_sampler(kind):
    """127 steps of the 8-env PPO agent at hidden 128 as ONE K32W launch (graph_chunk 127), without observation /
    reward normalisation, so that the buffer holds the raw observations and rewards.  Every stored transition follows
    the env's equations (test_gpu_classic's / test_gpu_pendulum's drift-free check: the state recovered from column t,
    stepped by the checker with the stored action, gives column t + 1 and the stored reward at 1e-5; after a done the
    next column is the hashed reset observation exactly), and the stored log-probs and values match K3
    (xpa_rollout_sample) run on the f64 oracle policy's heads of the stored rows, at those tests' 1e-4 / 2e-4
    (Categorical: on the draws further than 1e-5 from the oracle's CDF boundaries, which must be > 99 % of them)."""
    from xuanpolicy_amd import ops
    _, D, K, _ = ENVS[kind]
    N, T = 8, 128
    cat = kind != "pendulum"
    agent = _build(kind, n_envs=N, n_steps=T, hidden=H, seed=11, max_episode_steps=40, use_obsnorm=False,
                   use_rewnorm=False, graph_chunk=127)
    assert agent.plan().driver == "K32W" and agent.plan().chunk == 127
    agent.train(127, log=False)
    torch.cuda.synchronize()
    assert _np(agent.cursor)[:2].tolist() == [127, 127]
    s = _snapshot(agent)
    obs, act, rew, closed = s["obs"], s["act"], s["rew"], s["closed"].astype(bool)
    o64 = obs.astype(np.float64)
    ep = np.zeros(N, np.int64)
    n_reset = n_plain = 0
    for t in range(126):
        o = o64[:, t]
        if kind == "cartpole":
            nxt, r, _ = _cartpole_step(o, act[:, t])
            want = nxt.astype(np.float32)
        elif kind == "pendulum":
            nxt, r = pref.step(np.stack([np.arctan2(o[:, 1], o[:, 0]), o[:, 2]], axis=1), act[:, t, 0])
            want = pref.obs_of(nxt)
        elif kind == "acrobot":
            nxt, r, _ = aref.step(np.stack([np.arctan2(o[:, 1], o[:, 0]), np.arctan2(o[:, 3], o[:, 2]), o[:, 4],
                                            o[:, 5]], axis=1), act[:, t])
            want = aref.obs_of(nxt)
        else:
            nxt, r, _ = mref.step(o[:, 6:8], act[:, t])
            want = mref.push(obs[:, t], nxt)
        np.testing.assert_allclose(rew[:, t], r, rtol=0, atol=1e-5, err_msg="reward, column %d" % t)
        done = closed[:, t]
        ep += done
        np.testing.assert_allclose(obs[~done, t + 1], want[~done], rtol=0, atol=1e-5, err_msg="column %d" % (t + 1))
        if done.any():
            ids = np.arange(N)[done]
            if kind == "cartpole":
                reset = _cartpole_resets(agent.envs.noise_seed, ids, ep[done])
            else:
                ref_mod = {"pendulum": pref, "acrobot": aref, "mountaincar": mref}[kind]
                reset = ref_mod.obs_of(ref_mod.reset_states(agent.envs.noise_seed, ids, ep[done]))
            np.testing.assert_array_equal(obs[done, t + 1], reset)
        n_reset += int(done.sum())
        n_plain += int((~done).sum())
    assert n_reset >= 3 * N and n_plain > 800
    # the sampler and the value against K3 on the oracle policy's heads
    pol = cpu_ref.build_actor_critic_ref(D, K, [H], [H], [H], discrete=cat, activation=agent.config.activation)
    _load_by_order(pol, agent)
    pol.double()
    with torch.no_grad():
        head, _, v = pol.heads(torch.as_tensor(o64.reshape(N * T, D)))
    v = v.reshape(N, T).float().to(DEV)
    headf = head.reshape(N, T, K).float().to(DEV)
    b_act = torch.zeros((N, T) if cat else (N, T, 1), dtype=torch.float32, device=DEV)
    b_logp, b_val = (torch.zeros((N, T), dtype=torch.float32, device=DEV) for _ in range(2))
    env_in = torch.zeros((N, K), dtype=torch.float32, device=DEV)
    cur = ops.new_cursor(DEV)
    for t in range(127):
        cur.copy_(torch.tensor([t, t, 0, 0], dtype=torch.int32))
        if cat:
            ops.rollout_sample("categorical", headf[:, t].contiguous(), None, v[:, t].contiguous(), cur, agent.seed,
                               b_act, b_logp, b_val, env_in)
        else:
            ops.rollout_sample("gaussian", headf[:, t].contiguous(), agent.policy.actor.logstd.detach(),
                               v[:, t].contiguous(), cur, agent.seed, b_act, b_logp, b_val, env_in, act_clip=2.0)
    torch.cuda.synchronize()
    if cat:
        cdf = np.cumsum(torch.softmax(head, -1).reshape(N, T, K).numpy(), -1)[:, :127, :-1]
        u = _uniforms(agent.seed, N, 127)
        clear = np.abs(u[..., None] - cdf).min(-1) > 1e-5
        assert clear.mean() > 0.99
        want = (u[..., None] >= cdf).sum(-1).astype(np.float32)
        np.testing.assert_array_equal(act[:, :127][clear], want[clear])
        np.testing.assert_array_equal(_np(b_act)[:, :127][clear], want[clear])
    else:
        clear = np.ones((N, 127), bool)
        np.testing.assert_allclose(act[:, :127], _np(b_act)[:, :127], rtol=1e-4, atol=2e-4)
    np.testing.assert_allclose(s["logp"][:, :127][clear], _np(b_logp)[:, :127][clear], rtol=1e-4, atol=2e-4)
    np.testing.assert_allclose(s["val"][:, :127], _np(b_val)[:, :127], rtol=1e-4, atol=2e-4)


# ---- 3. K30's one-image form against the multi-kernel update --------------------------------------------------------
def _adv_partials(adv, idx):
    """K4's advantage moments of the minibatch: (sum, sumsq) in f64 per 64 rows (xpa_gather_num_partials)."""
    from xuanpolicy_amd import ops
    b = idx.shape[0]
    g = ops.gather_num_partials(b)
    a = torch.zeros((g * 64,), dtype=torch.float64, device=DEV)
    a[:b] = adv[idx].double()
    a = a.reshape(g, 64)
    return torch.stack([a.sum(1), (a * a).sum(1)], dim=1).contiguous()


def _learner_pair(d_in, hidden, agent_name, **kw):
    """Two agents with the same weights (same seed): the first learner runs K30, the second the multi-kernel update.
    d_in 3 is the Gaussian head (A = 1), the others Categorical heads of 3 actions."""
    from xuanpolicy_amd.runner import build_synthbox_ppo
    out = []
    for _ in range(2):
        out.append(build_synthbox_ppo(n_envs=8, n_steps=16, obs_dim=d_in, act_dim=1 if d_in == 3 else 3, hidden=hidden,
                                      seed=13, device=DEV, agent=agent_name, discrete=d_in != 3, ent_coef=0.01,
                                      graph_update=False, **kw))
    assert all(torch.equal(p, q) for p, q in zip(out[0].policy.parameters(), out[1].policy.parameters()))
    return out


def _rows(agent, n_rows, d_in, gen):
    """Random buffer rows; the old log-probs are the policy's own, jittered so that some ratios leave the clip range."""
    from xuanpolicy_amd.policies import policy_heads
    obs = torch.randn((n_rows, d_in), generator=gen, device=DEV)
    adv, ret = (torch.randn((n_rows,), generator=gen, device=DEV) for _ in range(2))
    with torch.no_grad():
        if agent.dist == "gaussian":
            mu, logstd, _ = policy_heads(agent.policy, obs)
            act = (mu + logstd.exp() * torch.randn((n_rows, 1), generator=gen, device=DEV)).contiguous()
            logp = torch.distributions.Normal(mu, logstd.exp()).log_prob(act).sum(-1)
        else:
            logits, _, _ = policy_heads(agent.policy, obs)
            act = torch.randint(0, 3, (n_rows,), generator=gen, device=DEV)
            logp = torch.log_softmax(logits, -1).gather(1, act[:, None])[:, 0]
            act = act.float().contiguous()
        old = (logp + 0.15 * torch.randn((n_rows,), generator=gen, device=DEV)).contiguous()
    return obs, act, adv, ret, old


@pytest.mark.parametrize("batch", [20, 40, 320])
@pytest.mark.parametrize("agent_name", ["PPO_Clip", "A2C"])
@pytest.mark.parametrize("d_in", [3, 4, 8])
def test_one_image_update_matches_multi_kernel_update(d_in, agent_name, batch):
    """K30 at hidden 128 (the one-image form: W1 and W2 through one LDS image) against the multi-kernel update (K13 /
    hipBLASLt / K2 / K10) from the same weights on synthetic buffer rows: d_in 3 with the Gaussian head (A = 1), 4 and 8
    with Categorical heads; a minibatch of 20 rows (one workgroup), 40 (ragged against the 32-row workgroups) and 320
    (the reference's minibatch: 10 workgroups).  The loss scalars and every parameter's raw gradient at the existing
    small-update tests' 1e-4 / 1e-5.  Learning rate 0 and no clipping, so the raw gradient stays in the flat buffer.
    Without the split form a 40-row minibatch does not fit, which small_update_ok reports."""
    from xuanpolicy_amd import ops
    small, multi = _learner_pair(d_in, H, agent_name, learning_rate=0.0)
    for a in (small, multi):
        a.learner._use_clip = False
    gen = torch.Generator(device=DEV)
    gen.manual_seed(100 * d_in + batch)
    n_rows = 400
    obs, act, adv, ret, old = _rows(small, n_rows, d_in, gen)
    old_arg = old if small.algo == "ppo" else None
    idx = torch.randperm(n_rows, generator=gen, device=DEV)[:batch].contiguous()
    k = 1 if d_in == 3 else 3
    rows = min(batch, 32)
    assert int(ops.lib().xpa_small_mlp_lds_floats(rows, d_in, H, H, H, k)) > 40704   # the resident layout does not fit
    assert int(ops.lib().xpa_small_mlp_one_image_lds_floats(rows, d_in, H, H, H, k)) <= 40704
    Ls = small.learner
    assert Ls.small_split and Ls.small_update_ok(obs, batch)
    Ls.small_split = False
    assert Ls.small_update_ok(obs, batch) == (batch <= 32)
    assert not Ls.small_update_ok(obs, 40)
    Ls.small_split = True
    assert not Ls.small_update_ok(obs, 513) and Ls.small_update_ok(obs, 512) and Ls.small_update_ok(obs, 1)
    sc_m = multi.learner.update_fused(obs[idx].contiguous(), idx, act, adv, ret, old_arg,
                                      _adv_partials(adv, idx)).clone()
    g_m = [_np(p.grad) for p in multi.policy.parameters()]
    names = [n for n, _ in small.policy.named_parameters()]
    assert ("logstd" in " ".join(names)) == (d_in == 3)
    sc_s = Ls.small_update(obs, idx, act, adv, ret, old_arg, use_advnorm=True).clone()
    torch.cuda.synchronize()
    np.testing.assert_allclose(_np(sc_s)[:6], _np(sc_m)[:6], rtol=1e-4, atol=1e-5)
    for n, p, gm in zip(names, small.policy.parameters(), g_m):
        assert np.abs(gm).max() > 0, n
        np.testing.assert_allclose(_np(p.grad), gm, rtol=1e-4, atol=1e-5, err_msg=n)
    assert all(torch.equal(p, q) for p, q in zip(small.policy.parameters(), multi.policy.parameters()))   # lr 0


def _two_updates(hidden):
    """Two consecutive clipped Adam updates (the config's learning rate and clip_grad_norm 0.5) of 320-row PPO
    minibatches, K30 against the multi-kernel learner; the largest parameter difference as (absolute, the least atol
    that passes at rtol 1e-4)."""
    small, multi = _learner_pair(4, hidden, "PPO_Clip")
    assert small.learner._use_clip and small.learner._max_norm == 0.5 and small.config.learning_rate > 0
    gen = torch.Generator(device=DEV)
    gen.manual_seed(77)
    n_rows = 700
    obs, act, adv, ret, old = _rows(small, n_rows, 4, gen)
    perm = torch.randperm(n_rows, generator=gen, device=DEV)
    before = [_np(p) for p in small.policy.parameters()]
    for u in range(2):
        idx = perm[320 * u:320 * (u + 1)].contiguous()
        assert small.learner.small_update_ok(obs, 320)
        multi.learner.update_fused(obs[idx].contiguous(), idx, act, adv, ret, old, _adv_partials(adv, idx))
        small.learner.small_update(obs, idx, act, adv, ret, old, use_advnorm=True)
    torch.cuda.synchronize()
    ps, pm = ([_np(p) for p in a.policy.parameters()] for a in (small, multi))
    assert max(np.abs(a - b).max() for a, b in zip(pm, before)) > 1e-4   # the weights moved
    err = max(float(np.abs(a - b).max()) for a, b in zip(ps, pm))
    need = max(float((np.abs(a - b) - 1e-4 * np.abs(b)).max()) for a, b in zip(ps, pm))
    return ps, pm, err, need


def test_one_image_update_steps_adam_as_the_multi_kernel_learner():
    """lr > 0 and clipping on, two consecutive updates: the parameters after them against the multi-kernel learner's at
    rtol 1e-4 / atol 1e-6, at hidden 128 (the one-image form, 10 workgroups + the finalize launch).  The same figures
    at hidden 64 (the resident form, as before this form existed) are measured in the same run and printed (on an
    MI355X: max |diff| 2.1e-8 at hidden 128, 1.5e-8 at hidden 64; the weights move by > 1e-4)."""
    _, _, err64, need64 = _two_updates(64)
    ps, pm, err, need = _two_updates(H)
    print("two clipped Adam updates, K30 against the multi-kernel learner: max |diff| %.3g at hidden 128 (least atol "
          "at rtol 1e-4: %.3g); hidden 64: %.3g (%.3g)" % (err, need, err64, need64))
    for a, b in zip(ps, pm):
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-6)


# ---- 4. the resident form is untouched ------------------------------------------------------------------------------
def h64_case(fix):
    """The hidden-64 PPO / Categorical update (d_in 4, 2 actions, 40 of 96 rows; learning rate 0, no clipping) from the
    inputs of fix (weights included), through K30's resident form with the split form on and off: the loss scalars and
    the flat raw gradient of each."""
    from xuanpolicy_amd.runner import build_synthbox_ppo
    agent = build_synthbox_ppo(n_envs=8, n_steps=16, obs_dim=4, act_dim=2, hidden=64, seed=13, device=DEV,
                               agent="PPO_Clip", discrete=True, learning_rate=0.0, ent_coef=0.01, graph_update=False)
    agent.learner._use_clip = False
    params = list(agent.policy.parameters())
    if "params" in fix:
        off = 0
        with torch.no_grad():
            for p in params:
                p.copy_(torch.as_tensor(fix["params"][off:off + p.numel()], device=DEV).reshape(p.shape))
                off += p.numel()
        assert off == fix["params"].size
    else:   # recording: the agent's own initial weights
        fix = dict(fix, params=np.concatenate([_np(p).ravel() for p in params]))
    obs, act, adv, ret, old = (torch.as_tensor(fix[k], device=DEV).contiguous() for k in ("obs", "act", "adv", "ret",
                                                                                          "old"))
    idx = torch.as_tensor(fix["idx"], device=DEV).contiguous()
    out = dict(fix)
    for split in (True, False):
        agent.learner.small_split = split
        assert agent.learner.small_update_ok(obs, idx.shape[0])
        sc = agent.learner.small_update(obs, idx, act, adv, ret, old, use_advnorm=True).clone()
        torch.cuda.synchronize()
        out["scalars_split%d" % split] = _np(sc)[:6]
        out["grad_split%d" % split] = np.concatenate([_np(p.grad).ravel() for p in params])
    return out


def test_resident_form_at_hidden_64_is_bit_identical_to_the_recorded_values():
    """tests/golden/k30_h64.npz holds the inputs (weights, rows, indices) and what the commit before the one-image form
    computed from them on an MI355X: the loss scalars and raw gradients of the split and the one-workgroup form.  The
    resident layout runs the code it ran then, so they are equal to the bit."""
    fix = dict(np.load(GOLDEN))
    got = h64_case({k: fix[k] for k in ("params", "obs", "act", "adv", "ret", "old", "idx")})
    for k in ("scalars_split1", "grad_split1", "scalars_split0", "grad_split0"):
        assert np.abs(fix[k]).max() > 0 and np.isfinite(fix[k]).all(), k
        assert got[k].tobytes() == fix[k].tobytes(), k


# ---- 5. the public surface, and an iteration against the CPU oracle -------------------------------------------------
def test_get_runner_takes_the_committed_cartpole_config_down_the_small_path():
    """get_runner on the committed CartPole-v1 config as it stands (the reference's values: hidden 128, 10 envs x 256
    steps, 8 minibatches of 320 rows): the rollout is K32W's launch, the updates K30's, and two iterations leave finite
    scalars and parameters."""
    from xuanpolicy_amd.runner import get_runner
    runner = get_runner("ppo", "classic_control", "CartPole-v1")
    agent = runner.agent
    cfg = agent.config
    assert cfg.representation_hidden_size == cfg.actor_hidden_size == cfg.critic_hidden_size == [H]
    assert runner.envs.kind == "cartpole" and agent.batch_size == 320
    agent.train(2 * agent.n_steps, log=False)
    torch.cuda.synchronize()
    plan = agent.plan()
    assert plan.driver == "K32W" and plan.feed == "small"
    assert plan.step_launches() == ["xpa_small_rollout_cartpole"]
    assert torch.isfinite(agent.last_info).all()
    assert all(torch.isfinite(p).all() for p in agent.policy.parameters())


@pytest.mark.parametrize("kind,agent_name", [("acrobot", "PPO_Clip"), ("pendulum", "A2C")])
def test_wide_iteration_matches_oracle(kind, agent_name):
    """test_classic_iteration_matches_oracle's replay at hidden 128: one iteration through K32W and K30's one-image
    form (256-row minibatches: 8 workgroups), then 127 steps and the last step + GAE + 16 updates replayed by the f64
    oracle learner at that test's tolerances; time limit 40, so mid-buffer truncation bootstraps occur."""
    _, D, K, _ = ENVS[kind]
    N, T = 8, 128
    agent = _build(kind, agent=agent_name, n_envs=N, n_steps=T, hidden=H, seed=3, n_epoch=4, n_minibatch=4,
                   max_episode_steps=40)
    assert agent.device_env and agent.defer_boot
    agent.train(T, log=False)
    agent.train(T - 1, log=False)
    plan = agent.plan()
    assert plan.driver == "K32W" and plan.feed == "small"
    replay_last_step_iteration(agent, D, K, [H], kind != "pendulum", agent.algo, agent.config.ent_coef, 4, 4,
                               expect_mid_truncations=True)
