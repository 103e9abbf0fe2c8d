"""Test helper: an agent's rollouts against the reference's train() loop (oracle.cpu_ref.VecAgentRef), step for step.

Shared by tests/test_gpu_hostenv.py (the agent over a host VecEnv) and tests/test_gpu_deviceenv_loop.py (the agent over
a device env):

  * _snapshot / _check_rollout / _gae_close: the reference loop's buffer at its full-buffer point, and the device
    buffer, RunningMeanStd state and return tracker of that iteration against it;
  * MirrorVecEnv + DeviceEnvRecorder: a host VecEnv for the reference loop that computes no dynamics.  The recorder
    steps the device agent one env step at a time and reads what the device env produced (final observations,
    rewards, flags, the observations the envs continue from, the stored actions); the mirror replays those, so the
    reference loop and the device agent see the same env bit for bit.  Every recorded step is also checked against
    the oracle env (oracle.synth_env) stepped from the device's pre-step state with the applied action, so a quantity
    a fused launch left stale in the env's tensors cannot pass as an env output;
  * frozen_agent / ahead_of: what _check_rollout reads of an agent, kept on the host (the negative controls re-run the
    reference loop against it without another device run), and the reference's statistics at the point a folded
    obs-RMS form leaves the device's.
"""
import copy
from types import SimpleNamespace

import numpy as np
import torch

from oracle import cpu_ref, synth_env
from tests.test_gpu_kernels import _gae_close as _gae_close_kernels


def _gae_close(got, ref, msg):
    try:
        _gae_close_kernels(got, ref)
    except AssertionError as e:
        raise AssertionError(msg + ": " + str(e)) from None


def _snapshot(mem):
    out = {k: np.array(getattr(mem, k), copy=True) for k in ("observations", "actions", "rewards", "values", "terminals",
                                                              "closed", "boot", "advantages", "returns")}
    out["old_logp"] = np.array(mem.auxiliary_infos["old_logp"], copy=True) if "old_logp" in mem.auxiliary_infos else None
    return out


def _check_rollout(agent, ref, snap, it):
    """The device buffer of one iteration against the reference loop's buffer at its full-buffer point."""
    mem = agent.memory
    msg = "iteration %d " % it
    obs = mem.observations.cpu().numpy()
    if obs.dtype == np.uint8:
        np.testing.assert_array_equal(obs, snap["observations"], err_msg=msg + "frames")
    else:
        np.testing.assert_allclose(obs, snap["observations"], rtol=1e-5, atol=1e-5, err_msg=msg + "obs")
    np.testing.assert_array_equal(mem.actions.cpu().numpy(), snap["actions"], err_msg=msg + "actions")
    np.testing.assert_array_equal(mem.terminals.cpu().numpy(), snap["terminals"], err_msg=msg + "terminals")
    np.testing.assert_array_equal(mem.closed.cpu().numpy(), snap["closed"], err_msg=msg + "closures")
    np.testing.assert_allclose(mem.rewards.cpu().numpy(), snap["rewards"], rtol=1e-5, atol=1e-6, err_msg=msg + "rew")
    np.testing.assert_allclose(mem.values.cpu().numpy(), snap["values"], rtol=1e-4, atol=1e-4, err_msg=msg + "values")
    np.testing.assert_allclose(mem.boot.cpu().numpy(), snap["boot"], rtol=1e-4, atol=1e-4, err_msg=msg + "bootstraps")
    if snap["old_logp"] is not None:
        np.testing.assert_allclose(mem.auxiliary_infos["old_logp"].cpu().numpy(), snap["old_logp"], rtol=1e-4, atol=2e-4,
                                   err_msg=msg + "old_logp")
    # (1) the device's GAE of its own columns: the oracle's finish_path arithmetic at north_star's 1e-5
    cols = [getattr(mem, k).cpu().numpy() for k in ("rewards", "values", "terminals", "closed", "boot")]
    adv_d, ret_d = mem.advantages.cpu().numpy(), mem.returns.cpu().numpy()
    adv_o, ret_o = cpu_ref.gae_rows(*cols, mem.gamma, mem.gae_lam)
    _gae_close(adv_d, adv_o, msg + "adv (device columns)")
    _gae_close(ret_d, ret_o, msg + "ret (device columns)")
    # (2) against the reference loop's own finish_path results: the columns differ by the f32-vs-f64 rounding held
    # above (values / bootstraps 1e-4, rewards 1e-5), and a discounted sum of such differences is bounded by the
    # measured column differences propagated through the scan: |d adv| <= (|d r| + (1 + gamma) |d v| + gamma |d boot|)
    # / (1 - gamma lambda) — an envelope measured on the case, not a blanket tolerance
    g, lam = float(mem.gamma), float(mem.gae_lam)
    dr = np.abs(cols[0] - snap["rewards"]).max()
    dv = np.abs(cols[1] - snap["values"]).max()
    db = np.abs(cols[4] - snap["boot"]).max()
    env_adv = (dr + (1 + g) * dv + g * db) / (1 - g * lam) + 1e-6
    np.testing.assert_allclose(adv_d, snap["advantages"], rtol=0, atol=env_adv, err_msg=msg + "adv (reference loop)")
    np.testing.assert_allclose(ret_d, snap["returns"], rtol=0, atol=env_adv + dv, err_msg=msg + "ret (reference loop)")
    assert env_adv < 2e-3, (msg, "envelope", env_adv)
    if agent.use_obsnorm:
        np.testing.assert_allclose(agent.obs_mean.cpu().numpy(), ref.obs_rms.mean, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(agent.obs_var.cpu().numpy(), ref.obs_rms.var, rtol=1e-5, atol=1e-6)
        assert abs(float(agent.obs_count) - ref.obs_rms.count) < 1e-6
    np.testing.assert_allclose(float(agent.ret_mean), float(ref.ret_rms.mean), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(float(agent.ret_var), float(ref.ret_rms.var), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(agent.returns.cpu().numpy(), ref.returns, rtol=1e-5, atol=1e-5)


# ---- the mirror VecEnv -----------------------------------------------------------------------------------------------
def _h(t):
    return t.detach().cpu().numpy().copy()


class MirrorVecEnv:
    """A host VecEnv with the contract VecAgentRef drives (buf_obs, num_envs, the spaces, max_episode_length,
    step(acts) -> (obs, rew, term, trunc, infos with reset_obs)) that replays recorded steps instead of computing any.

    steps: a list of dicts, one per env step, of numpy arrays: "act" (the applied actions), "final" (the step's
    observations: the final one of an env that ended), "rew", "term", "trunc", "next" (the observations the envs
    continue from: "final" with the reset observation in the rows of envs that ended).  buf_obs is ONE array for the
    object's life, written in place by step() as DummyVecEnv does, and it holds what a device env's buf_obs holds: its
    live `obs`, i.e. "next" — a device env has no separate copy of the final observations among its current ones, so a
    train() call starts from the rows the previous one ended on ("Device envs continue across train()
    calls as one call would") and, without obs-norm, the reference's first store of a call aliases the post-step rows.
    atari: infos carry reset_obs after a truncation only (a life loss, terminal without truncation, continues)."""

    def __init__(self, observation_space, action_space, max_episode_length, obs0, steps, atari=False):
        self.observation_space, self.action_space = observation_space, action_space
        self.max_episode_length = int(max_episode_length)
        self.buf_obs = np.array(obs0, copy=True)
        self.num_envs = self.buf_obs.shape[0]
        self.steps, self.atari, self.k = steps, bool(atari), 0

    def step(self, acts):
        s = self.steps[self.k]
        self.k += 1
        np.testing.assert_array_equal(np.asarray(acts), s["act"], err_msg="the loop must take the recorded actions")
        term, trunc = s["term"].astype(bool), s["trunc"].astype(bool)
        done = trunc if self.atari else (term | trunc)
        infos = [{"reset_obs": s["next"][i].copy()} if done[i] else {} for i in range(self.num_envs)]
        self.buf_obs[...] = s["next"]   # in place
        return s["final"].copy(), s["rew"].copy(), term.copy(), trunc.copy(), infos


# ---- oracle envs re-seeded from the device's pre-step state ----------------------------------------------------------
class _SynthBoxCheck:
    """oracle.synth_env.SynthBoxVec stepped from the device's pre-step rows (test_synthbox_step_matches_oracle's re-sync:
    tanh dynamics amplify ulps, so one step at a time), its `near` rule for the termination flag."""

    def __init__(self, env):
        self.env = env
        self.ref = synth_env.SynthBoxVec(env.num_envs, env.D, env.A, seed=env.seed, discrete=env.discrete,
                                         max_episode_steps=env.max_episode_steps)
        self.near_rows = 0

    def before(self):
        env = self.env
        return dict(state=_h(env.obs), ep=_h(env.ep_index).astype(np.uint32), t=_h(env.ep_step).astype(np.int64))

    def check(self, pre, s):
        ref = self.ref
        ref.state, ref.episode, ref.ep_step = pre["state"].copy(), pre["ep"].copy(), pre["t"].copy()
        act = s["act"].astype(np.int64) if self.env.discrete else s["act"]
        fin, r, te, tr, nxt = ref.step(act)
        np.testing.assert_allclose(s["final"], fin, rtol=1e-5, atol=2e-6, err_msg="final_obs")
        np.testing.assert_allclose(s["rew"], r, rtol=1e-5, atol=1e-6, err_msg="rew")
        near = np.abs(fin[:, 0] - synth_env.TERM_THRESH) < 1e-5
        self.near_rows += int(near.sum())
        np.testing.assert_array_equal(s["term"].astype(bool)[~near], te[~near], err_msg="term")
        np.testing.assert_array_equal(s["trunc"].astype(bool), tr, err_msg="trunc")
        done = (te | tr) & ~near
        np.testing.assert_array_equal(s["next"][done], nxt[done], err_msg="reset rows")   # hashed reset states: exact
        cont = ~(s["term"].astype(bool) | s["trunc"].astype(bool))
        np.testing.assert_array_equal(s["next"][cont], s["final"][cont], err_msg="continuing rows")


class _CartPoleCheck:
    """oracle.synth_env.CartPoleEnv per env, kept on the device's f64 env.state before every step, as
    test_cartpole_env_matches_oracle re-seeds its checker (libm and ocml sin / cos may differ in the last ulp)."""

    def __init__(self, env):
        self.env = env
        self.ref = [synth_env.CartPoleEnv(i, seed=env.seed, max_episode_steps=env.max_episode_steps)
                    for i in range(env.num_envs)]

    def before(self):
        env = self.env
        return dict(state=_h(env.state), ep=_h(env.ep_index), t=_h(env.ep_step))

    def check(self, pre, s):
        for i, r in enumerate(self.ref):
            r.state, r.ep, r.ep_step = pre["state"][i].copy(), int(pre["ep"][i]), int(pre["t"][i])
            o, rw, te, tr, _ = r.step(int(s["act"][i]))
            np.testing.assert_allclose(s["final"][i], o, rtol=1e-6, atol=1e-7, err_msg="final_obs")
            assert rw == s["rew"][i] == 1.0 and te == bool(s["term"][i]) and tr == bool(s["trunc"][i]), (i, te, tr)
            if te or tr:
                np.testing.assert_array_equal(s["next"][i], r.reset()[0], err_msg="reset rows")   # hashed reset: exact
            else:
                np.testing.assert_array_equal(s["next"][i], s["final"][i], err_msg="continuing rows")


class _SynthAtariCheck:
    """oracle.synth_env.SynthAtariEnv per env, run beside the device env from the common reset (integer dynamics: exact,
    nothing to re-seed)."""

    def __init__(self, env):
        self.env = env
        self.ref = [synth_env.SynthAtariEnv(i, seed=env.seed, n_actions=env.n_actions,
                                            max_episode_steps=env.max_episode_steps) for i in range(env.num_envs)]
        np.testing.assert_array_equal(_h(env.obs), np.stack([r.reset()[0] for r in self.ref]))

    def before(self):
        return None

    def check(self, pre, s):
        for i, r in enumerate(self.ref):
            o, rw, te, tr, info = r.step(int(s["act"][i]))
            np.testing.assert_array_equal(s["final"][i], o, err_msg="final frames")
            assert rw == s["rew"][i] and te == bool(s["term"][i]) and tr == bool(s["trunc"][i]), (i, rw, te, tr)
            np.testing.assert_array_equal(s["next"][i], info["reset_obs"] if tr else o, err_msg="next frames")


_CHECKS = {"synthbox": _SynthBoxCheck, "cartpole": _CartPoleCheck, "synthatari": _SynthAtariCheck}


class DeviceEnvRecorder:
    """Steps a device-env agent one env step at a time and records what the env produced.  step() = before() +
    agent.train(1, log=False) + after(); a caller that runs the step itself (the update replay's last step) calls
    before() / after() around it.  steps: MirrorVecEnv's records; raw: the raw observations ahead of every step
    (raw[k] is what step k's policy acted on) and after the last one."""

    def __init__(self, agent):
        self.agent, self.env = agent, agent.envs
        assert agent.device_env
        self.check = _CHECKS[self.env.kind](self.env)
        self.raw = [_h(self.env.obs)]
        self.steps = []

    def before(self):
        torch.cuda.synchronize()
        return self.agent._t, self.check.before()

    def after(self, token):
        col, pre = token
        torch.cuda.synchronize()
        env, mem = self.env, self.agent.memory
        act = _h(mem.actions[:, col])
        if self.agent.discrete:
            act = act.astype(np.int64)
        s = dict(act=act, final=_h(env.final_obs), rew=_h(env.rew), term=_h(env.term), trunc=_h(env.trunc),
                 next=_h(env.obs))
        self.check.check(pre, s)
        self.steps.append(s)
        self.raw.append(s["next"])

    def step(self):
        token = self.before()
        self.agent.train(1, log=False)
        self.after(token)

    def mirror(self, steps=None):
        """A fresh MirrorVecEnv at the recording's start (steps: a perturbed copy of self.steps)."""
        env = self.env
        return MirrorVecEnv(env.observation_space, env.action_space, env.max_episode_length, self.raw[0],
                            self.steps if steps is None else steps, atari=env.kind == "synthatari")

    def flags(self, k0, k1):
        """(term, trunc) [N, k1 - k0] of the recorded steps k0 .. k1 - 1."""
        return (np.stack([s["term"] for s in self.steps[k0:k1]], 1).astype(bool),
                np.stack([s["trunc"] for s in self.steps[k0:k1]], 1).astype(bool))


def reference_loop(agent, env, pol, algo, discrete, atari, on_full, **over):
    """VecAgentRef over env with the agent's rollout settings; it takes the actions env (a MirrorVecEnv) recorded."""
    cfg = agent.config
    kw = dict(gamma=cfg.gamma, gae_lambda=cfg.gae_lambda, use_obsnorm=agent.use_obsnorm, use_rewnorm=agent.use_rewnorm,
              obsnorm_range=cfg.obsnorm_range, rewnorm_range=cfg.rewnorm_range, atari=atari, discrete=discrete)
    kw.update(over)
    return cpu_ref.VecAgentRef(env, pol, algo, agent.n_steps, lambda _obs: env.steps[env.k]["act"], on_full=on_full, **kw)


def unalias_first_stores(snap, rec, k0, calls):
    """Without obs-norm the reference stores `obs` after envs.step, and on a train() call's first step that is
    envs.buf_obs itself (ppoclip_agent.py:59-74), which the step wrote in place: the column holds the post-step rows.
    The device-env path stores, in every column, the rows the policy acted on, whatever the calls (its rollouts do not
    depend on how train() is chunked).  For the rollout that starts at recorded step k0 and was made by reference
    train() calls of `calls` steps: assert that the reference's first-store columns are exactly the post-step rows,
    and put the rows the policy acted on in their place for the comparison with the device column."""
    c = 0
    for n in calls:
        np.testing.assert_array_equal(snap["observations"][:, c], rec.raw[k0 + c + 1],
                                      err_msg="the reference's first store of a call is the post-step buf_obs")
        snap["observations"][:, c] = rec.raw[k0 + c]
        c += n


def frozen_agent(agent):
    """What _check_rollout reads of an agent, copied to the host."""
    mem = agent.memory
    m = SimpleNamespace(gamma=mem.gamma, gae_lam=mem.gae_lam,
                        auxiliary_infos={k: v.detach().cpu().clone() for k, v in mem.auxiliary_infos.items()})
    for k in ("observations", "actions", "rewards", "values", "terminals", "closed", "boot", "advantages", "returns"):
        setattr(m, k, getattr(mem, k).detach().cpu().clone())
    out = SimpleNamespace(memory=m, use_obsnorm=agent.use_obsnorm, n_envs=agent.n_envs, n_steps=agent.n_steps)
    for k in ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "returns"):
        setattr(out, k, getattr(agent, k).detach().cpu().clone())
    return out


def ahead_of(ref, agent, next_raw, folded, check_lead=True):
    """The reference loop's statistics at the point the device's stand.  A folded obs-RMS form (rollout_plan rms
    "fold-K8" / "fold-K14F") merges the NEXT step's obs_rms.update in the step's last launch, so after a step the
    device's obs_rms already holds the rows the next step starts from (next_raw), which the reference merges at the
    top of that step (ppoclip_agent.py:62): the same update at the same place in the sequence, seen from the other
    side of the step boundary.  The lead is asserted to be exactly that — one update of n_envs rows where the plan
    folds, none otherwise — and the reference's copy is advanced by it.  check_lead = False (a negative control whose
    loop's statistics are perturbed on purpose): the copy is advanced without that assertion."""
    if not agent.use_obsnorm:
        return ref
    lead = float(agent.obs_count) - ref.obs_rms.count
    assert not check_lead or abs(lead - (agent.n_envs if folded else 0)) < 1e-6, ("obs_rms lead", lead, folded)
    if not folded:
        return ref
    rms = copy.deepcopy(ref.obs_rms)
    type(rms).update(rms, next_raw)   # the class's own update, whatever a control hung on the instance
    return SimpleNamespace(obs_rms=rms, ret_rms=ref.ret_rms, returns=ref.returns)
