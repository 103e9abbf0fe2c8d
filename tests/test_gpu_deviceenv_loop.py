"""GPU: the agent over a DEVICE env against the reference's train() loop, step for step.

Every figure the project reports comes from an agent over a device env (_OnPolicyAgent._rollout_step_device and the
K32 driver, xuanpolicy_amd/agents.py).  The other device-env tests compare device forms with each other, feed kernels
synthetic inputs, or replay an iteration from the device's own stored columns (tests/_oracle_replay.py); here
oracle.cpu_ref.VecAgentRef — the reference's loop (ppoclip_agent.py:59-111, a2c_agent.py:57-107, agent.py:104-123),
pinned to the reference by G11 — runs over a mirror of the device env (tests/_vecloop_check.MirrorVecEnv: no dynamics,
it replays what the device env produced at each step) with the actions the device drew and an f64 copy of the device
policy, and the device's whole buffer, both RunningMeanStd states and the return tracker are held to the loop's
(_check_rollout, the host-path test's assertions and tolerances unchanged).

Recording (DeviceEnvRecorder): the agent is stepped with train(1); after each step final_obs, rew, term, trunc, the
post-step obs (reset observations in the rows of envs that ended) and the stored action column are read from the env's
and the buffer's tensors.  Every form here (K14F and K14E with the env step in the head launch, K14 + the env kernel +
K8, K32) materialises all of them per step, so nothing is reconstructed; what is read is checked, step by step, against
the oracle env (SynthBoxVec / CartPoleEnv re-seeded from the device's pre-step state — CartPole from the f64 env.state
— and SynthAtariEnv run beside the device env) with the applied action: observations and rewards at the env tests'
tolerances, the flags on rows away from the termination threshold (`near`), reset rows exactly.

Where the device-env path and the reference loop differ BY DESIGN, and how the cases treat it:

  * a device env's buf_obs is its live `obs` (the rows the envs continue from), so a train() call starts where the
    previous one ended and a rollout does not depend on how train() is chunked (asserted bit for bit
    below for cases 1, 5 and 7).  The mirror's buf_obs holds the same rows, written in place; the reference's calls
    are split on steps where episodes end, so it restarts from rows the step just reset;
  * without obs-norm the reference's first store of every train() call is the post-step buf_obs (the alias of
    ppoclip_agent.py:59-74); the device-env path stores the rows the policy acted on in every column.  Cases 3, 5 and
    6 assert the reference's aliased columns are exactly the post-step rows and compare the device column with the
    pre-step rows (unalias_first_stores); every other column of those steps (values, old log-probs, rewards, ...) is
    compared as it is;
  * the folded obs-RMS form (fold-K14F) merges the next step's obs_rms.update in the step's last launch: at an
    iteration's end the device's obs_rms leads the loop's by exactly that update (ahead_of asserts the lead).
"""
import copy
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from tests._oracle_replay import _load_by_order, replay_last_step_iteration
from tests._vecloop_check import (DeviceEnvRecorder, _check_rollout, _h, _snapshot, ahead_of, frozen_agent,
                                  reference_loop, unalias_first_stores)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FOLDED = ("fold-K8", "fold-K14F")


@pytest.fixture(scope="module", autouse=True)
def _setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cpu_ref.build_oracle()
    yield
    # the cached cases hold their agents (buffers, captured graphs and their pools): let go of them, so that the
    # modules after this one run in the allocator state they would have had without it
    import gc
    _run_case.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---- the cases -------------------------------------------------------------------------------------------------------
def _synthbox(agent_name, discrete, D, A, N, obsnorm=True, max_ep=10, seed=7):
    from xuanpolicy_amd.runner import build_synthbox_ppo
    T, H = 32, 256
    agent = build_synthbox_ppo(n_envs=N, n_steps=T, obs_dim=D, act_dim=A, hidden=H, n_epoch=2, n_minibatch=4, seed=seed,
                               device=DEV, agent=agent_name, discrete=discrete, ent_coef=0.01, max_episode_steps=max_ep,
                               use_obsnorm=obsnorm, use_rewnorm=True)
    pol = cpu_ref.build_actor_critic_ref(D, A, [H], [H], [H], discrete=discrete,
                                         activation=getattr(agent.config, "activation", "LeakyReLU"))
    return agent, pol


ATARI_NET = dict(filters=[8, 8], kernels=[8, 4], strides=[4, 2], fc=[32])


def _atari(agent_name, seed=3):
    """The small CNN of test_host_vecenv_atari_a2c_matches_reference_loop over SynthAtariVecEnv; PPO_Clip: the
    coefficients of test_ppo_atari_replays_reference_agent's docstring (ppo/atari.yaml) on the config object."""
    import xuanpolicy_amd.runner as R
    N, T, K = 8, 32, 6
    cfg = R.get_arguments("a2c", "atari", "SynthAtari-v0")
    cfg.parallels, cfg.n_steps, cfg.seed, cfg.n_actions, cfg.max_episode_steps = N, T, seed, K, 40
    cfg.filters, cfg.kernels, cfg.strides = ATARI_NET["filters"], ATARI_NET["kernels"], ATARI_NET["strides"]
    cfg.fc_hidden_sizes = ATARI_NET["fc"]
    cfg.n_epoch, cfg.n_minibatch = 2, 4
    if agent_name == "PPO_Clip":
        cfg.agent = "PPO_Clip"
        cfg.learning_rate, cfg.clip_range, cfg.clip_grad_norm, cfg.use_grad_clip = 2.5e-4, 0.2, 0.5, True
        cfg.vf_coef, cfg.ent_coef, cfg.n_epoch, cfg.n_minibatch = 0.25, 0.01, 4, 4
    torch.manual_seed(seed)
    agent = R.build_agent(cfg, DEV)
    pol = cpu_ref.build_atari_ac_ref(K, ATARI_NET["filters"], ATARI_NET["kernels"], ATARI_NET["strides"], ATARI_NET["fc"])
    return agent, pol


def _cartpole(seed=3):
    from xuanpolicy_amd.runner import build_cartpole_ppo
    H = 64
    agent = build_cartpole_ppo(n_envs=8, n_steps=32, hidden=H, seed=seed, device=DEV, n_epoch=2, n_minibatch=4,
                               max_episode_steps=7)
    pol = cpu_ref.build_actor_critic_ref(4, 2, [H], [H], [H], discrete=True,
                                         activation=getattr(agent.config, "activation", "LeakyReLU"))
    return agent, pol


def _graphed(plan):
    return plan.driver in ("graph-chunk", "graph-step")


def _forms_k14f(agent, plan):
    assert _graphed(plan) and plan.head == "K14F" and plan.env == "in-head" and plan.post == "K14F", plan
    assert plan.rms == "fold-K14F" and plan.obs == "trunk" and plan.boot == "slots" and plan.mid is None, plan
    assert agent.use_obsnorm and agent.use_rewnorm and agent.defer_boot and agent.n_slots == 4


def _forms_a2c_box(agent, plan):
    assert not agent.envs.fusable_with_policy_step(agent.dist)
    assert _graphed(plan) and plan.head == "K14" and plan.env == "synthbox" and plan.post == "K8-deferred", plan
    assert plan.rms == "standalone" and plan.boot == "slots" and plan.mid == "slots-from-next", plan
    assert agent.boot_from_reset and agent.use_obsnorm and agent.defer_boot and agent.n_slots == 4


def _forms_noobsnorm(agent, plan):
    assert _graphed(plan) and plan.head == "K14F" and plan.env == "in-head" and plan.post == "K14F", plan
    assert plan.rms is None and plan.boot == "slots", plan
    assert not agent.use_obsnorm and agent.use_rewnorm and agent.n_slots == 4


def _forms_c4(agent, plan):
    assert _graphed(plan) and plan.head == "K14" and plan.env == "synthbox" and plan.obs == "K5N", plan
    assert plan.post == "K8-deferred" and plan.rms == "standalone" and plan.boot == "slots", plan
    assert agent.obs_dim == 376 and agent.n_slots == 4


def _forms_atari(agent, plan):
    assert agent.atari and agent.raw_obs and agent.raw_defer and not agent.use_obsnorm
    assert agent.memory.observations.dtype == torch.uint8
    assert _graphed(plan) and plan.obs == "raw" and plan.trunk == "cnn" and plan.head == "K3", plan
    assert plan.env == "synthatari" and plan.post == "K8" and plan.boot == "zero" and plan.close == "raw-last", plan


def _forms_k32(agent, plan):
    assert plan.driver == "K32" and plan.env == "cartpole" and plan.boot == "slots", plan
    assert agent.use_obsnorm and agent.use_rewnorm and agent.config.gamma == 0.98 and agent.n_slots == 5


# name: (builder, algo, discrete, A, atari, the reference's train() calls of iteration 1 — every boundary on a step
# where episodes end —, the plan's forms, the update replay's keywords)
C4_REPLAY = dict(loss_tol=1e-4, w_atol=1e-4, lockstep=True, free_run_updates=1)   # test_c4_shape_iteration_matches_oracle's
CASES = {
    "ppo_gauss_k14f": (lambda: _synthbox("PPO_Clip", False, 17, 6, 80), "ppo", False, 6, False, (10, 10, 12),
                       _forms_k14f, {}),
    "a2c_cat_k14_k8": (lambda: _synthbox("A2C", True, 17, 8, 80), "a2c", True, 8, False, (10, 10, 12),
                       _forms_a2c_box, {}),
    "ppo_no_obsnorm": (lambda: _synthbox("PPO_Clip", False, 17, 6, 80, obsnorm=False), "ppo", False, 6, False,
                       (10, 10, 12), _forms_noobsnorm, {}),
    "ppo_c4_width": (lambda: _synthbox("PPO_Clip", False, 376, 17, 80), "ppo", False, 17, False, (10, 10, 12),
                     _forms_c4, C4_REPLAY),
    "a2c_atari": (lambda: _atari("A2C"), "a2c", True, 6, True, (16, 16), _forms_atari, {}),
    "ppo_atari": (lambda: _atari("PPO_Clip"), "ppo", True, 6, True, (16, 16), _forms_atari, {}),
    "ppo_cartpole_k32": (_cartpole, "ppo", True, 2, False, (7, 14, 11), _forms_k32, {}),
}
CHUNKED = ("ppo_gauss_k14f", "a2c_atari", "ppo_cartpole_k32")


def _state(agent):
    """Everything two runs of one seed must agree on bit for bit: the buffer, both RMS states, the return tracker, the
    env state and the parameters."""
    mem, env = agent.memory, agent.envs
    out = {k: getattr(mem, k) for k in ("observations", "actions", "rewards", "values", "terminals", "closed", "boot",
                                        "advantages", "returns")}
    out.update({"aux_" + k: v for k, v in mem.auxiliary_infos.items()})
    out.update({k: getattr(agent, k) for k in ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count",
                                               "returns")})
    out.update({"env_" + k: getattr(env, k) for k in ("obs", "final_obs", "rew", "term", "trunc", "ep_step", "ep_index",
                                                      "ep_score", "ep_last_score", "ep_last_len")})
    for k in ("state", "lives", "paddle"):
        if hasattr(env, k):
            out["env_" + k] = getattr(env, k)
    out.update({"param_%d" % i: p for i, p in enumerate(agent.policy.parameters())})
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _run_case(name):
    """Two iterations of the case, recorded, with the reference loop beside them; cached: the negative controls re-run
    the loop against iteration 1's recording on the host."""
    build, algo, discrete, A, atari, calls, forms, replay_kw = CASES[name]
    agent, pol = build()
    N, T = agent.n_envs, agent.n_steps
    assert agent.device_env and sum(calls) == T
    plan = agent.plan()
    forms(agent, plan)
    folded = plan.rms in FOLDED
    rec = DeviceEnvRecorder(agent)
    mirror = rec.mirror()
    snaps = []
    ref = reference_loop(agent, mirror, pol, algo, discrete, atari, lambda r: snaps.append(_snapshot(r.memory)))
    _load_by_order(pol, agent)
    pol.double()
    pol0 = copy.deepcopy(pol)
    # iteration 1: the device one step per train() call, the loop in calls that end where episodes end
    for _ in range(T):
        rec.step()
    assert agent.plan() == plan and agent.iterations == 1
    for k in calls:
        ref.train(k)
    assert len(snaps) == 1 and mirror.k == T
    if not agent.use_obsnorm:
        unalias_first_stores(snaps[0], rec, 0, calls)
    _check_rollout(agent, ahead_of(ref, agent, rec.raw[T], folded), snaps[0], 0)
    # the raw observations the agent continues from are the loop's
    np.testing.assert_array_equal(_h(agent.envs.obs), ref.obs)
    np.testing.assert_array_equal(ref.obs, mirror.buf_obs)
    frozen = frozen_agent(agent)
    # iteration 2 from the device's updated weights; its last step runs inside the update replay
    _load_by_order(pol, agent)
    pol.double()
    for _ in range(T - 1):
        rec.step()
    ref.train(T - 1)
    token = rec.before()
    replay_last_step_iteration(agent, None, A, None, discrete, algo, agent.config.ent_coef, agent.n_epoch,
                               agent.n_minibatch, expect_mid_truncations=agent.defer_boot, pol=copy.deepcopy(pol),
                               **replay_kw)
    rec.after(token)
    ref.train(1)
    assert len(snaps) == 2 and mirror.k == 2 * T and agent.iterations == 2
    if not agent.use_obsnorm:
        unalias_first_stores(snaps[1], rec, T, (T - 1, 1))
    _check_rollout(agent, ahead_of(ref, agent, rec.raw[2 * T], folded), snaps[1], 1)
    np.testing.assert_array_equal(_h(agent.envs.obs), ref.obs)
    return SimpleNamespace(agent=agent, state=_state(agent), plan=plan, rec=rec, snaps=snaps, pol0=pol0, frozen=frozen,
                           folded=folded, build=build, algo=algo, discrete=discrete, atari=atari, calls=calls)


@pytest.mark.parametrize("name", list(CASES))
def test_device_env_agent_matches_reference_loop(name):
    """Per case: agent.device_env, the plan fields that make it the production form (a form not selected is a
    failure), two iterations held to the reference loop (module docstring), and the case exercised what it is there
    for: at least n_envs truncations before a rollout's last step, more than one deferred slot of one env where the
    agent defers, Atari life losses that leave the path open.

    Recorded per step for every case: final_obs, rew, term, trunc, the post-step obs (reset rows) and the action
    column; reconstructed: nothing (each recorded quantity is checked against the oracle env stepped from the device's
    pre-step state instead).  Forms: ppo_gauss_k14f K14F (head + SynthBox step + post in one launch), obs in the
    trunk, rms fold-K14F, 4 deferred slots; a2c_cat_k14_k8 K14 + xpa_synthbox_step + K8-deferred, standalone rms,
    slots-from-next (V(norm(reset_obs))); ppo_no_obsnorm K14F without obs-norm; ppo_c4_width SynthBox(376, 17) at 80
    envs: K5N (the wide K5), K14, the env kernel, K8-deferred; a2c_atari / ppo_atari SynthAtariVecEnv frames stored
    raw (uint8, compared exactly), CNN trunk, K3, K8, raw_defer ("zero" / "raw-last"); ppo_cartpole_k32 the K32
    driver at the committed CartPole config's flags, time limit 7, 5 slots."""
    r = _run_case(name)
    agent, T, N = r.agent, r.agent.n_steps, r.agent.n_envs
    for it, s in enumerate(r.snaps):
        term, trunc = r.rec.flags(it * T, (it + 1) * T)
        mid = (s["closed"][:, :T - 1] != 0) & (s["terminals"][:, :T - 1] == 0)
        if r.atari:   # a game over is terminal AND truncated (boot 0): no non-terminal close before the last step
            assert not mid.any()
        else:
            assert mid.sum() >= N and np.abs(s["boot"][:, :T - 1][mid]).min() > 0
            np.testing.assert_array_equal(mid, (trunc & ~term)[:, :T - 1])
        if agent.defer_boot:
            assert agent.n_slots > 1 and mid.sum(1).max() >= 2, "more than one deferred slot of an env must be used"
    term, trunc = r.rec.flags(0, 2 * T)
    inner = np.ones(2 * T, bool)
    inner[[T - 1, 2 * T - 1]] = False
    assert trunc[:, inner].sum() >= N, "at least n_envs truncations before a rollout's last step"
    if r.atari:
        lifeloss = sum(int(((s["terminals"] != 0) & (s["closed"] == 0)).sum()) for s in r.snaps)
        assert lifeloss > 0 and (term & ~trunc).sum() >= lifeloss, "life losses must leave the path open"


@pytest.mark.parametrize("name", CHUNKED)
def test_rollouts_do_not_depend_on_how_train_is_chunked(name):
    """A second agent of the same seed runs each iteration as one train(n_steps) call (a replayed chunk graph, K32
    with n_steps steps per launch) where the first ran one step per call: buffer, RMS states, return tracker, env
    state and parameters after both iterations are bit-identical."""
    r = _run_case(name)
    agent, _ = r.build()
    T = agent.n_steps
    assert agent.plan() == r.plan
    agent.train(T, log=False)
    agent.train(T, log=False)
    one = _state(agent)
    assert one.keys() == r.state.keys()
    diff = [k for k in one if not torch.equal(one[k], r.state[k])]
    assert not diff, diff


# ---- negative controls (host only: the reference loop re-run against iteration 1's recording) -------------------------
def _loop_against_recording(r, steps=None, **over):
    """A fresh reference loop over iteration 1's recording; returns (ref, run): run() makes the calls and holds the
    recorded device buffer to the loop's."""
    T = r.frozen.n_steps
    mirror = r.rec.mirror(steps)
    snaps = []
    ref = reference_loop(r.agent, mirror, copy.deepcopy(r.pol0), r.algo, r.discrete, r.atari,
                         lambda x: snaps.append(_snapshot(x.memory)), **over)

    def run():
        for k in r.calls:
            ref.train(k)
        assert len(snaps) == 1
        view = ahead_of(ref, r.frozen, r.rec.raw[T], r.folded, check_lead=False)
        _check_rollout(r.frozen, view, snaps[0], 0)
    return ref, run


@pytest.mark.parametrize("name", ["ppo_gauss_k14f", "a2c_cat_k14_k8"])
def test_control_the_recording_itself_passes(name):
    """The controls' baseline: the unperturbed loop over the cached recording passes the same host-side check."""
    _, run = _loop_against_recording(_run_case(name))
    run()


@pytest.mark.parametrize("name", ["ppo_gauss_k14f", "a2c_cat_k14_k8"])
def test_control_other_return_tracker_rule_fails_at_rewards(name):
    """PPO masks the return tracker with (1 - terminal) (ppoclip_agent.py:87), A2C does not (a2c_agent.py:82): the loop
    run with the other algorithm's rule feeds ret_rms other returns at every termination, and the normalised rewards
    after the first one no longer match the device's."""
    r = _run_case(name)
    T = r.frozen.n_steps
    term, _ = r.rec.flags(0, T)
    assert term[:, :T - 2].any(), "the case needs a termination inside the rollout"
    ref, run = _loop_against_recording(r)
    ref.mask_returns = not ref.mask_returns
    with pytest.raises(AssertionError, match="iteration 0 rew"):
        run()


def test_control_skipped_obs_rms_update_fails_at_observations():
    """obs_rms.update runs before every normalisation (ppoclip_agent.py:62-63): a loop that skips one stores other
    normalised observations from that step on."""
    r = _run_case("ppo_gauss_k14f")
    ref, run = _loop_against_recording(r)
    rms, calls = ref.obs_rms, {"n": 0}
    update = rms.update

    def skipping(x):
        calls["n"] += 1
        if calls["n"] != 4:
            update(x)
    rms.update = skipping
    with pytest.raises(AssertionError, match="iteration 0 obs"):
        run()


def test_control_truncation_recorded_as_termination_fails():
    """One recorded mid-rollout truncation handed to the loop as a termination: the loop stores terminal 1 and closes
    the path with 0 instead of V(norm(final obs)).  _check_rollout compares the terminal column ahead of the closures
    and the bootstraps (and, PPO masking the return tracker by it, ahead of the rewards it also moves), so that is
    where it stops; the closure's bootstrap — what the perturbation is about — is then held directly: 0 in the loop's
    buffer, the critic's value in the device's."""
    r = _run_case("ppo_gauss_k14f")
    T = r.frozen.n_steps
    term, trunc = r.rec.flags(0, T)
    rows, cols = np.nonzero((trunc & ~term)[:, :T - 1])
    i, k = int(rows[0]), int(cols[0])
    steps = [dict(s) for s in r.rec.steps[:T]]
    steps[k]["term"], steps[k]["trunc"] = steps[k]["term"].copy(), steps[k]["trunc"].copy()
    steps[k]["term"][i], steps[k]["trunc"][i] = 1, 0
    ref, run = _loop_against_recording(r, steps)
    snaps = []
    on_full = ref.on_full
    ref.on_full = lambda x: (on_full(x), snaps.append(_snapshot(x.memory)))
    with pytest.raises(AssertionError, match="iteration 0 terminals"):
        run()
    mem = r.frozen.memory
    assert snaps[0]["terminals"][i, k] == 1 and snaps[0]["closed"][i, k] == 1 and snaps[0]["boot"][i, k] == 0
    assert float(mem.terminals[i, k]) == 0 and int(mem.closed[i, k]) == 1 and abs(float(mem.boot[i, k])) > 1e-6


def test_control_a2c_final_obs_bootstrap_fails_at_bootstraps():
    """Case 2's agent with boot_from_reset = False keeps the final observation's rows in its deferred slots, as PPO
    does: against the A2C loop (V(norm(reset_obs)), a2c_agent.py:88-95) the buffer fails at the bootstraps, and at
    nothing compared before them — as test_host_vecenv_a2c_bootstrap_is_reset_obs_value shows on the host path.  (The
    one control that needs a device run of its own: one iteration.)"""
    build, algo, discrete, A, atari, calls, _, _ = CASES["a2c_cat_k14_k8"]
    agent, pol = build()
    agent.boot_from_reset = False
    T = agent.n_steps
    plan = agent.plan()
    assert agent.device_env and plan.mid is None and plan.boot == "slots", plan
    rec = DeviceEnvRecorder(agent)
    mirror = rec.mirror()
    snaps = []
    ref = reference_loop(agent, mirror, pol, algo, discrete, atari, lambda r: snaps.append(_snapshot(r.memory)))
    _load_by_order(pol, agent)
    pol.double()
    for _ in range(T):
        rec.step()
    for k in calls:
        ref.train(k)
    mid = (snaps[0]["closed"][:, :T - 1] != 0) & (snaps[0]["terminals"][:, :T - 1] == 0)
    assert mid.sum() >= agent.n_envs
    with pytest.raises(AssertionError, match="iteration 0 bootstraps"):
        _check_rollout(agent, ahead_of(ref, agent, rec.raw[T], plan.rms in FOLDED), snaps[0], 0)
