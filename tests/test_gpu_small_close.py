"""GPU: K33 (xpa_small_close / xpa_small_close_batch) — the closing of a one-launch small-path rollout in one launch.

  1. The bootstraps are K32's values, bit for bit: the rows K32 / K32W forwarded, fed back through K33's critic pass.
  2. The same bootstraps against the torch policy module's critic.
  3. The fixup's writes and the advantage scan on random rollouts against the CPU oracle and against
     xpa_rollout_bootstrap_fixup + xpa_gae_scan.
  4. The batch form against each agent's own launch.
  5. Population.train with small_close members against their solo twins; the launches of a recorded closing.
  6. A small_close agent against its default twin after one closing."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref
from tests.test_gpu_wide_small import ENVS, _build

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = -12345.0
GUARD = 64   # floats on each side of a guarded tensor (keeps the tensor 16-B aligned)


@pytest.fixture(scope="module", autouse=True)
def _setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cpu_ref.build_oracle()


def _np(t):
    return t.detach().cpu().numpy().copy()


def _d(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def _gae_tol(ref, extra=0.0):
    """tests/test_gpu_kernels.py's _gae_close tolerance (1e-5 absolute + 1e-5 relative + 2^-20 of the row's largest
    |value|: the scan's f32 rounding is relative to the row's largest partial sum), plus `extra`."""
    ref = np.asarray(ref, np.float64)
    return 1e-5 + 1e-5 * np.abs(ref) + 2.0 ** -20 * np.abs(ref).max(axis=-1, keepdims=True) + extra


def _gae_close(got, ref, extra=0.0):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    print("GAE: max |got - ref| %.3g (tolerance at that element %.3g)"
          % (err.max(), _gae_tol(ref, extra).flat[err.argmax()]))
    bad = err > _gae_tol(ref, extra)
    assert not bad.any(), ("GAE mismatch", int(bad.sum()), float(err[bad].max()))


def _guarded(n, dtype=torch.float32, fill=SENTINEL):
    """(the whole allocation, its middle n elements): what a kernel writes outside the middle shows in the guards."""
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + n]


def _guards_intact(whole, fill=SENTINEL):
    h = _np(whole)
    return (h[:GUARD] == fill).all() and (h[-GUARD:] == fill).all()


def _layers(agent):
    layers, code, slope, _ = agent.learner.small_policy_layers()
    return layers, (int(code), float(slope))


# ---- 1, 2. the bootstraps ---------------------------------------------------------------------------------------------
# (env kind, builder keywords): K32 at 64 and 32, K32W (128), and mixed K32 widths
WIDTHS = {"cartpole-64": ("cartpole", dict(hidden=64)), "pendulum-32": ("pendulum", dict(hidden=32)),
          "mountaincar-128": ("mountaincar", dict(hidden=128)),
          "acrobot-32-64-32": ("acrobot", dict(hidden=32, actor_hidden_size=[64]))}


def _one_k32_step(case, N, randomise_biases=False):
    """An agent after ONE K32 / K32W step through its own single-step launch: agent.obs_norm holds the rows the launch
    forwarded, column 0 of memory.values what it wrote for them.  Returns (agent, vboot_out of a K33 launch whose every
    row group is obs_norm, S).  case: a key of WIDTHS, or its own (env kind, builder keywords).  randomise_biases:
    every policy bias (and a Gaussian head's logstd) is overwritten in place before the rollout begins (a fresh
    policy's biases are all 0)."""
    from xuanpolicy_amd import ops
    kind, kw = WIDTHS[case] if isinstance(case, str) else case
    agent = _build(kind, n_envs=N, n_steps=8, seed=11, max_episode_steps=3, n_minibatch=1, **kw)   # 3 slots per env
    S = agent.n_slots
    assert S == 3 and agent.plan().driver == ("K32W" if kw["hidden"] == 128 else "K32")
    if randomise_biases:
        from tests._small_ref import randomise_biases as overwrite
        assert len(overwrite(agent.policy)) == (6 if kind == "pendulum" else 5)
    agent._begin_rollout()
    agent._small_rollout_launch(1)
    mem, T = agent.memory, agent.n_steps
    rows = agent.obs_norm.repeat(S + 1, 1).contiguous()
    layers, act = _layers(agent)
    slot_t = torch.full((S * N,), -1, dtype=torch.int32, device=DEV)
    z = lambda: torch.zeros((N, T), device=DEV)   # noqa: E731
    closed = torch.zeros((N, T), dtype=torch.uint8, device=DEV)
    closed[:, -1] = 1
    whole, vboot = _guarded((S + 1) * N)
    blk = ops.small_close_args(layers, act, rows, slot_t, z(), z(), z(), closed, z(), z(), z(), 0.99, 0.95, True,
                               vboot_out=vboot)
    ops.small_close(blk, DEV)
    torch.cuda.synchronize()
    assert _guards_intact(whole)
    return agent, rows, vboot.reshape(S + 1, N), S


@pytest.mark.parametrize("N", [1, 17, 256])
@pytest.mark.parametrize("case", sorted(WIDTHS))
def test_bootstraps_are_k32s_values_bit_for_bit(case, N):
    """N = 1: one row of one tile; 17: a ragged second 16-row tile; 256: the limit (16 tiles).  Every row group of K33's
    critic pass (the slot passes and the last-step pass) equals the values column K32 wrote for the same rows."""
    agent, rows, vboot, S = _one_k32_step(case, N)
    want = agent.memory.values[:, 0]
    assert torch.isfinite(want).all() and (N == 1 or float(want.std()) > 0)
    for g in range(S + 1):
        assert torch.equal(vboot[g], want), (case, N, g, float((vboot[g] - want).abs().max()))


@pytest.mark.parametrize("N", [1, 17, 256])
@pytest.mark.parametrize("case", sorted(WIDTHS))
def test_bootstraps_match_the_modules_critic(case, N):
    """The same values against the torch policy module's critic on those rows, at the project's K32-versus-multi-kernel
    values tolerance (tests/test_gpu_classic.py: rtol 1e-4, atol 2e-4)."""
    from xuanpolicy_amd.policies import policy_heads
    agent, rows, vboot, S = _one_k32_step(case, N)
    with torch.no_grad():
        want = policy_heads(agent.policy, rows)[2].reshape(S + 1, N)
    err = (vboot - want).abs().max().item()
    print("%s N %d: max |K33 - module| %.3g" % (case, N, err))
    np.testing.assert_allclose(_np(vboot), _np(want), rtol=1e-4, atol=2e-4)


# ---- 3. the fixup and the scan ----------------------------------------------------------------------------------------
def _close_case(rng, N, T, S, p_term=0.02, p_slot=0.3):
    """tests/test_gpu_kernels.py's _compact_case restated for S slots per env: random rew / val / term, rows that end on
    a terminal, per env up to S used slots at distinct times before the last step (every 7th env: one right before the
    last step), a truncation slot never a terminal.  slot: int32 [S, N] (-1: unused)."""
    rew = rng.normal(0, 1, (N, T)).astype(np.float32)
    val = rng.normal(0, 1, (N, T)).astype(np.float32)
    term = (rng.random((N, T)) < p_term).astype(np.float32)
    term[rng.random(N) < 0.1, -1] = 1.0
    slot = np.full((S, N), -1, np.int32)
    if T > 1:
        for n in range(N):
            times = rng.permutation(T - 1)[:S]                 # distinct
            for k, t in enumerate(times):
                if rng.random() < p_slot:
                    slot[k, n] = t
            if n % 7 == 0 and not (slot[:, n] == T - 2).any():
                slot[0, n] = T - 2
            used = slot[:, n][slot[:, n] >= 0]
            assert len(set(used.tolist())) == len(used)
            term[n, used] = 0.0
    return rew, val, term, slot


def _dense_record(term, slot, vboot):
    """The dense closure record K8's flags + xpa_rollout_bootstrap_fixup leave, for bootstraps vboot [(S + 1) N]."""
    N, T = term.shape
    S = slot.shape[0]
    closed = (term > 0).astype(np.uint8)
    closed[:, -1] = 1
    boot = np.zeros((N, T), np.float32)
    for k in range(S):
        rows = np.nonzero(slot[k] >= 0)[0]
        closed[rows, slot[k, rows]] = 1
        boot[rows, slot[k, rows]] = vboot[k * N + rows]
    boot[:, -1] = np.where(term[:, -1] > 0, 0.0, vboot[S * N:])
    return closed, boot


@pytest.fixture(scope="module")
def cartpole64():
    return _build("cartpole", n_envs=4, n_steps=8, hidden=64, seed=2)


@pytest.mark.parametrize("use_gae", [True, False])
@pytest.mark.parametrize("N,T,S", [(1, 1, 1), (3, 5, 1), (8, 36, 1), (10, 256, 2), (256, 128, 1), (17, 130, 2)])
def test_fixup_and_scan_match_the_oracle_and_the_two_kernels(cartpole64, N, T, S, use_gae):
    """One K33 launch on a random rollout (CartPole's [64] policy for the critic pass, random rows).  T = 1, 5, 130: the
    one-step-at-a-time scan (T % 4 != 0); 36, 128, 256: the 16-B one.  boot and slot_t exactly as the fixup leaves
    them; adv / ret against oracle/gae_ref.c on the dense record, and against xpa_rollout_bootstrap_fixup +
    xpa_gae_scan fed K33's own bootstraps at 1e-6 (test_gpu_kernels' figure for two scan orders); nothing outside
    the tensors is written."""
    from xuanpolicy_amd import ops
    rng = np.random.default_rng(1000 * N + 10 * T + S + int(use_gae))
    rew, val, term, slot = _close_case(rng, N, T, S)
    layers, act = _layers(cartpole64)
    rows = torch.as_tensor(rng.normal(0, 1, ((S + 1) * N, 4)).astype(np.float32)).to(DEV)
    closed_pre = (term > 0).astype(np.uint8)   # K8's flags: terminals, the truncation slots, the last step
    closed_pre[:, -1] = 1
    for k in range(S):
        r = np.nonzero(slot[k] >= 0)[0]
        closed_pre[r, slot[k, r]] = 1
    slot_d = _d(slot.reshape(-1))
    boot_d = torch.zeros((N, T), device=DEV)
    (wa, adv), (wr, ret), (wv, vboot) = _guarded(N * T), _guarded(N * T), _guarded((S + 1) * N)
    adv, ret = adv.view(N, T), ret.view(N, T)
    rew_d, val_d, term_d = _d(rew), _d(val), _d(term)
    blk = ops.small_close_args(layers, act, rows, slot_d, rew_d, val_d, term_d, _d(closed_pre), boot_d, adv, ret, 0.99,
                               0.95, use_gae, vboot_out=vboot)
    ops.small_close(blk, DEV)
    torch.cuda.synchronize()
    assert _guards_intact(wa) and _guards_intact(wr) and _guards_intact(wv)
    vb = _np(vboot)
    assert np.isfinite(vb).all() and (vb != SENTINEL).all()
    closed, boot = _dense_record(term, slot, vb)
    np.testing.assert_array_equal(closed, closed_pre)
    np.testing.assert_array_equal(_np(boot_d), boot)
    assert (_np(slot_d) == -1).all()
    got_adv, got_ret = _np(adv), _np(ret)
    assert (got_adv != SENTINEL).all() and (got_ret != SENTINEL).all()   # every row closes at its last step
    ref_adv, ref_ret = cpu_ref.gae_rows(rew, val, term, closed, boot, 0.99, 0.95, use_gae)
    _gae_close(got_adv, ref_adv)
    _gae_close(got_ret, ref_ret)
    # the two kernels K33 stands for, fed its bootstraps
    slot2, boot2 = _d(slot.reshape(-1)), torch.zeros((N, T), device=DEV)
    ops.bootstrap_fixup(vboot.contiguous(), slot2, term_d, boot2)
    a2, r2 = ops.gae_scan(rew_d, val_d, term_d, _d(closed_pre), boot2, 0.99, 0.95, use_gae)
    assert torch.equal(boot2, boot_d)
    np.testing.assert_allclose(got_adv, _np(a2), rtol=0, atol=1e-6)
    np.testing.assert_allclose(got_ret, _np(r2), rtol=0, atol=1e-6)


def test_scan_leaves_an_open_tail_untouched(cartpole64):
    """Steps after a row's last closure belong to no path: the oracle leaves them alone and so does K33, in the 16-B
    scan (the tail ends inside a chunk) and in the one-step one.  (A rollout's rows always close at the last step; the
    record here does not.)"""
    from xuanpolicy_amd import ops
    layers, act = _layers(cartpole64)
    for N, T in ((5, 24), (5, 23)):
        rng = np.random.default_rng(T)
        rew, val = (rng.normal(0, 1, (N, T)).astype(np.float32) for _ in range(2))
        term = np.zeros((N, T), np.float32)
        term[:, T - 1] = 1.0   # the fixup's last-step write is then 0
        closed = np.zeros((N, T), np.uint8)
        last = np.array([T - 1, T - 2, T - 6, 3, 0])   # row n's last closure
        closed[np.arange(N), last] = 1
        closed[0, 2] = closed[2, 1] = 1
        boot = np.zeros((N, T), np.float32)
        boot[closed > 0] = rng.normal(0, 1, int(closed.sum())).astype(np.float32)
        boot[:, T - 1] = 0.0
        adv, ret = (torch.full((N, T), SENTINEL, device=DEV) for _ in range(2))
        boot_d = _d(boot)
        blk = ops.small_close_args(layers, act, torch.zeros((2 * N, 4), device=DEV),
                                   torch.full((N,), -1, dtype=torch.int32, device=DEV), _d(rew), _d(val), _d(term),
                                   _d(closed), boot_d, adv, ret, 0.99, 0.95, True)
        ops.small_close(blk, DEV)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_np(boot_d), boot)
        ref_adv = np.full((N, T), SENTINEL, np.float32)
        ref_ret = ref_adv.copy()
        cpu_ref.gae_rows(rew, val, term, closed, boot, 0.99, 0.95, True, adv=ref_adv, ret=ref_ret)
        got_adv, got_ret = _np(adv), _np(ret)
        open_tail = np.arange(T)[None, :] > last[:, None]
        assert open_tail.sum() > 0 and (ref_adv[open_tail] == SENTINEL).all()
        assert (got_adv[open_tail] == SENTINEL).all() and (got_ret[open_tail] == SENTINEL).all()
        _gae_close(np.where(open_tail, 0, got_adv), np.where(open_tail, 0, ref_adv))
        _gae_close(np.where(open_tail, 0, got_ret), np.where(open_tail, 0, ref_ret))


# ---- 4. batch == single ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,hidden", [("cartpole", 64), ("mountaincar", 128)])
def test_batch_equals_each_agents_own_launch(kind, hidden):
    """P = 3 agents with different weights (seeds 3, 4, 5) and different random rollouts (10 x 64, two slots per env):
    one xpa_small_close_batch launch leaves every agent's adv, ret, boot, slot_t and vboot_out as its own
    xpa_small_close does."""
    from xuanpolicy_amd import _lib, ops
    from xuanpolicy_amd.population import _DeviceBlocks, _block_array
    N, T, S = 10, 64, 2
    agents = [_build(kind, n_envs=4, n_steps=8, hidden=hidden, seed=s) for s in (3, 4, 5)]
    D = ENVS[kind][1]
    sets = {}
    for form in ("batch", "single"):
        blocks, outs = [], []
        for p, a in enumerate(agents):
            rng = np.random.default_rng(50 + p)
            rew, val, term, slot = _close_case(rng, N, T, S)
            closed, _ = _dense_record(term, slot, np.zeros((S + 1) * N, np.float32))
            rows = _d(rng.normal(0, 1, ((S + 1) * N, D)).astype(np.float32))
            t = dict(slot_t=_d(slot.reshape(-1)), boot=torch.zeros((N, T), device=DEV),
                     adv=torch.full((N, T), SENTINEL, device=DEV), ret=torch.full((N, T), SENTINEL, device=DEV),
                     vboot=torch.full(((S + 1) * N,), SENTINEL, device=DEV))
            keep = (rows, _d(rew), _d(val), _d(term), _d(closed))
            layers, act = _layers(a)
            blocks.append(ops.small_close_args(layers, act, rows, t["slot_t"], keep[1], keep[2], keep[3], keep[4],
                                               t["boot"], t["adv"], t["ret"], 0.98, 0.9, True, vboot_out=t["vboot"]))
            outs.append((t, keep))
        if form == "batch":
            host, dev = _DeviceBlocks(DEV).get(_block_array(_lib.XpaSmallCloseArgs, blocks))
            ops.small_close_batch(len(blocks), host, dev, DEV)
        else:
            for b in blocks:
                ops.small_close(b, DEV)
        torch.cuda.synchronize()
        sets[form] = outs
    for p in range(3):
        for k in ("adv", "ret", "boot", "slot_t", "vboot"):
            got, want = sets["batch"][p][0][k], sets["single"][p][0][k]
            assert torch.equal(got, want), (p, k)
            assert (want != SENTINEL).all()
    assert not torch.equal(sets["single"][0][0]["vboot"], sets["single"][1][0]["vboot"])   # different agents


# ---- 5. end to end -----------------------------------------------------------------------------------------------------
E2E = {"cartpole-ppo-64": ("CartPole-v1", "PPO_Clip", dict(hidden=64, n_envs=5, n_steps=32, n_epoch=2, n_minibatch=2,
                                                           max_episode_steps=40), 1),
       "pendulum-a2c-64-two-slots": ("Pendulum-v1", "A2C", dict(hidden=64, n_envs=10, n_steps=256, n_epoch=1,
                                                                n_minibatch=8, max_episode_steps=200), 2)}


@pytest.mark.parametrize("case", sorted(E2E))
def test_population_train_with_small_close_equals_the_solo_twins(case, monkeypatch):
    """Members built with small_close=True: Population.train over two iterations and 7 steps of the third against the
    solo twins (the same switch) — parameters, Adam state, statistics, buffers (adv / ret among them) and infos equal.
    CartPole PPO (Categorical, one slot per env) and Pendulum A2C at 10 x 256 with a 200-step limit (Gaussian, two
    slots per env: every env truncates at step 200).  The population closes with ONE xpa_small_close_batch launch per
    iteration, each twin with its own xpa_small_close."""
    from tests.test_gpu_population import _assert_agents_equal
    from xuanpolicy_amd import _lib
    from xuanpolicy_amd.runner import build_classic_population
    env_id, agent_name, kw, S = E2E[case]
    kw = dict(kw, device=DEV, small_close=True)
    pop = build_classic_population(env_id, seeds=(1, 2, 3), agent=agent_name, **kw)
    solo = build_classic_population(env_id, seeds=(1, 2, 3), agent=agent_name, **kw).agents
    assert pop.plan().close_batch and pop.agents[0].n_slots == S and pop.agents[0].plan().gae == "K33"
    log = []
    real_call = _lib.call
    monkeypatch.setattr(_lib, "call", lambda fn, *a: (log.append(fn.__name__), real_call(fn, *a))[1])
    steps = 2 * kw["n_steps"] + 7
    pop.train(steps)
    assert log.count("xpa_small_close_batch") == 2 and "xpa_small_close" not in log
    del log[:]
    for b in solo:
        b.train(steps)
    assert log.count("xpa_small_close") == 6 and "xpa_small_close_batch" not in log
    assert not any(n.startswith("xpa_gae_scan") or n == "xpa_rollout_bootstrap_fixup" for n in log)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(pop.agents, solo)):
        assert a._t == 7 and a.iterations == 2 and a.gae_form == b.gae_form == "K33"
        assert not a.memory._dirty
        _assert_agents_equal(a, b, "member %d" % i)
    assert not np.array_equal(_np(pop.agents[0].memory._advantages), _np(pop.agents[1].memory._advantages))


def test_a_recorded_closing_launches_what_the_plan_declares(monkeypatch):
    """tests/test_gpu_rollout_plan.py's recording on a small_close agent: between the last env step and the first update
    call the library entry points are plan.close_launches() = one K33 launch and the epoch permutation."""
    from xuanpolicy_amd import _lib
    agent = _build("cartpole", n_envs=4, n_steps=12, hidden=64, seed=5, n_epoch=1, n_minibatch=2, cuda_graph=False,
                   max_episode_steps=19, small_close=True)
    plan = agent.plan()
    assert plan.driver == "K32" and plan.chunk == 1 and plan.gae == "K33"
    assert plan.close_launches() == ["xpa_small_close", "xpa_random_permutation"]
    log = []
    real_call, real_step, learner = _lib.call, agent._rollout_step_device, agent.learner
    monkeypatch.setattr(_lib, "call", lambda fn, *a: (log.append(fn.__name__), real_call(fn, *a))[1])
    monkeypatch.setattr(agent, "_rollout_step_device", lambda: (log.append("STEP"), real_step())[1])
    for entry in ("update_fused", "small_epoch", "update_epoch"):
        def logged(*a, _real=getattr(learner, entry), **k):
            log.append("UPDATE")
            return _real(*a, **k)
        monkeypatch.setattr(learner, entry, logged)
    agent.train(12, log=False)
    torch.cuda.synchronize()
    assert agent.iterations == 1 and agent.gae_form == "K33"
    last = log[len(log) - log[::-1].index("STEP"):]
    step = plan.step_launches()
    assert last[:len(step)] == step and "UPDATE" in last
    assert last[len(step):last.index("UPDATE")] == plan.close_launches()


# ---- 6. against the default closing -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,agent_name,hidden", [("mountaincar", "PPO_Clip", 64), ("pendulum", "A2C", 128)])
def test_small_close_agent_against_its_default_twin_after_one_closing(kind, agent_name, hidden):
    """Two agents built alike but for the switch run the same 32-step K32 rollout (5 envs, time limit 20: two slots per
    env) and close it: the twin with the module's critic (a library GEMM) + xpa_rollout_bootstrap_fixup + xpa_gae_scan,
    the other with K33.  Everything up to the closing is equal.  adv / ret are NOT: the bootstraps are the same
    function of the same rows in two roundings (K32's fma chains against the library's), which is what test 2 bounds
    at rtol 1e-4 / atol 2e-4; a bootstrap enters every earlier step of its path with a factor gamma^j (lambda^j) <= 1,
    so adv / ret agree at _gae_close's tolerance widened by 2e-4 + 1e-4 max |bootstrap|."""
    from tests.test_gpu_wide_small import _snapshot
    res = {}
    for sc in (False, True):
        a = _build(kind, agent=agent_name, n_envs=5, n_steps=32, hidden=hidden, seed=7, max_episode_steps=20,
                   small_close=sc)
        assert a.n_slots == 2 and a.plan().gae == ("K33" if sc else "fixup+scan")
        a._begin_rollout()
        a._small_rollout_launch(32)
        a._advance(32)
        torch.cuda.synchronize()
        before = _snapshot(a)
        a._close_rollout()
        torch.cuda.synchronize()
        assert a.gae_form == "K33" if sc else True
        res[sc] = (before, _np(a.memory._advantages), _np(a.memory._returns), _np(a.memory.boot), _np(a.slot_t))
    for k in res[False][0]:
        np.testing.assert_array_equal(res[True][0][k], res[False][0][k], err_msg=k)
    assert (res[True][0]["slot_t"] >= 0).any()   # slots were filled
    assert (res[True][4] == -1).all() and (res[False][4] == -1).all()
    boot_k, boot_m = res[True][3], res[False][3]
    np.testing.assert_allclose(boot_k, boot_m, rtol=1e-4, atol=2e-4)
    extra = 2e-4 + 1e-4 * float(np.abs(boot_m).max())
    print("%s: max |boot K33 - module| %.3g, widening %.3g" % (kind, np.abs(boot_k - boot_m).max(), extra))
    _gae_close(res[True][1], res[False][1], extra)
    _gae_close(res[True][2], res[False][2], extra)


def test_the_scans_scalars_are_the_buffers_at_each_closing():
    """K33's block is built once per plan, but gamma / lambda / use_gae are the buffer's at the launch, as the other
    closings read them: changed after the first plan(), the new values scan (against xpa_gae_scan on the record the
    closing left, at the 1e-6 of test 3)."""
    from xuanpolicy_amd import ops
    a = _build("cartpole", n_envs=5, n_steps=32, hidden=64, seed=7, max_episode_steps=20, small_close=True)
    assert a.plan().gae == "K33"
    mem = a.memory
    mem.gae_lam, mem.gamma, mem.use_gae = 0.5, 0.9, False
    a._begin_rollout()
    a._small_rollout_launch(32)
    a._advance(32)
    a._close_rollout()
    torch.cuda.synchronize()
    assert a.plan().gae == "K33" and a.gae_form == "K33"
    adv, ret = ops.gae_scan(mem.rewards, mem.values, mem.terminals, mem.closed, mem.boot, 0.9, 0.5, False)
    np.testing.assert_allclose(_np(mem._advantages), _np(adv), rtol=0, atol=1e-6)
    np.testing.assert_allclose(_np(mem._returns), _np(ret), rtol=0, atol=1e-6)
    old, _ = ops.gae_scan(mem.rewards, mem.values, mem.terminals, mem.closed, mem.boot, a.gamma, 0.95, True)
    assert not np.allclose(_np(mem._advantages), _np(old), atol=1e-3)
