"""GPU: population training — P agents per launch, each computing exactly what it computes alone.

Every comparison is torch.equal / array equality: the batch forms run the single-agent kernels' bodies on the same
inputs, so there is no tolerance to choose.

  1. xpa_small_rollout_batch against each member's own K32 / K32W launch, and the same steps in two chunks.
  2. xpa_small_mlp_update_batch against learner.small_update per member, two consecutive updates.
  3. xpa_random_permutation_batch against ops.random_permutation per row.
  4. Population.train against the members' solo twins, end to end; a member going on alone; ineligible populations."""
import numpy as np
import pytest
import torch

from tests.test_gpu_wide_small import ENVS, _build, _plant, _snapshot

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SEEDS = (3, 4, 5)


@pytest.fixture(scope="module", autouse=True)
def _setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _np(t):
    return t.detach().cpu().numpy().copy()


def _assert_snapshots_equal(got, want, tag):
    assert got.keys() == want.keys()
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (tag, k))


# ---- 1. the rollout --------------------------------------------------------------------------------------------------
def _rollout_set(kind, agent_name, hidden, **kw):
    """Three members (seeds 3, 4, 5): 5 envs (one ragged 16-env tile), a 48-step buffer, time limit 40 (an episode
    that lasts truncates inside the rollout and fills a deferred slot); terminating states planted in member 1 only,
    so the members' episodes run apart."""
    agents = [_build(kind, agent=agent_name, n_envs=5, n_steps=48, hidden=hidden, seed=s, max_episode_steps=40, **kw)
              for s in SEEDS]
    if ENVS[kind][3] is not None:
        _plant(agents[1].envs, kind, [0, 2, 3])
    for a in agents:
        assert a.plan().driver == ("K32W" if hidden == 128 else "K32") and a.plan().chunk == 48
    return agents


# every (env, width) pair with LeakyReLU, PPO and A2C at every width; ReLU / Tanh and obs-norm off on CartPole at 64
ROLLOUT_CASES = [(kind, h, ("PPO_Clip", "A2C")[(i + j) % 2], {})
                 for i, kind in enumerate(sorted(ENVS)) for j, h in enumerate((32, 64, 128))]
ROLLOUT_CASES += [("cartpole", 64, "PPO_Clip", dict(activation="ReLU")), ("cartpole", 64, "A2C", dict(activation="Tanh")),
                  ("cartpole", 64, "PPO_Clip", dict(use_obsnorm=False))]


@pytest.mark.parametrize("kind,hidden,agent_name,kw", ROLLOUT_CASES,
                         ids=["%s-%d-%s%s" % (c[0], c[1], c[2], "".join("-%s" % v for v in c[3].values()))
                              for c in ROLLOUT_CASES])
def test_rollout_batch_equals_each_members_own_launch(kind, hidden, agent_name, kw):
    """Set A: ONE 48-step xpa_small_rollout_batch launch over the three members.  Set B (built the same way): each
    member's own 48-step K32 / K32W launch.  Every tensor of _snapshot is equal, member by member."""
    from xuanpolicy_amd.population import Population
    set_a, set_b = _rollout_set(kind, agent_name, hidden, **kw), _rollout_set(kind, agent_name, hidden, **kw)
    pop = Population(set_a)
    plan = pop.plan()
    assert plan.n_agents == 3 and plan.gaussian == (kind == "pendulum")
    pop._rollout_launch(plan, 48)
    for b in set_b:
        b._small_rollout_launch(48)
    torch.cuda.synchronize()
    snaps = [_snapshot(a) for a in set_a]
    for i, (sa, b) in enumerate(zip(snaps, set_b)):
        _assert_snapshots_equal(sa, _snapshot(b), "member %d" % i)
        assert sa["cursor"][:2].tolist() == [0, 48] and sa["overflow"].sum() == 0
        if kind == "pendulum":   # never terminates: every env truncates at step 40 and fills a deferred slot
            assert (sa["slot_t"] >= 0).sum() >= 5
    if ENVS[kind][3] is not None:
        assert snaps[1]["term"][:, 0].sum() > 0 and snaps[0]["term"][:, 0].sum() == 0   # the planted member alone
    assert not np.array_equal(snaps[0]["obs"], snaps[2]["obs"])   # the members are different agents


@pytest.mark.parametrize("kind,hidden,agent_name", [("cartpole", 64, "PPO_Clip"), ("pendulum", 128, "A2C"),
                                                    ("acrobot", 32, "PPO_Clip")])
def test_rollout_batch_in_two_chunks_equals_one(kind, hidden, agent_name):
    """Batch launches of 16 + 32 steps against one of 48: everything a launch carries over lives in the members'
    tensors (cursor, env state, statistics), so the split changes nothing."""
    from xuanpolicy_amd.population import Population
    set_a, set_b = _rollout_set(kind, agent_name, hidden), _rollout_set(kind, agent_name, hidden)
    pa, pb = Population(set_a), Population(set_b)
    pa._rollout_launch(pa.plan(), 16)
    pa._rollout_launch(pa.plan(), 32)
    pb._rollout_launch(pb.plan(), 48)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(set_a, set_b)):
        _assert_snapshots_equal(_snapshot(a), _snapshot(b), "member %d" % i)


# ---- 2. the update ---------------------------------------------------------------------------------------------------
def _learner_set(d_in, k, hidden, agent_name):
    """Three agents of one shape with different weights (seeds 3, 4, 5); (3, 1) is the Gaussian head."""
    from xuanpolicy_amd.runner import build_synthbox_ppo
    return [build_synthbox_ppo(n_envs=8, n_steps=16, obs_dim=d_in, act_dim=k, hidden=hidden, seed=s, device=DEV,
                               agent=agent_name, discrete=d_in != 3, ent_coef=0.01, graph_update=False)
            for s in SEEDS]


def _rows(agent, n_rows, d_in, k, gen):
    """Random buffer rows of one member; the old log-probs are the policy's own, jittered so that some ratios leave the
    clip range."""
    from xuanpolicy_amd.policies import policy_heads
    obs = torch.randn((n_rows, d_in), generator=gen, device=DEV)
    adv, ret = (torch.randn((n_rows,), generator=gen, device=DEV) for _ in range(2))
    with torch.no_grad():
        if agent.dist == "gaussian":
            mu, logstd, _ = policy_heads(agent.policy, obs)
            act = (mu + logstd.exp() * torch.randn((n_rows, k), generator=gen, device=DEV)).contiguous()
            logp = torch.distributions.Normal(mu, logstd.exp()).log_prob(act).sum(-1)
        else:
            logits, _, _ = policy_heads(agent.policy, obs)
            act = torch.randint(0, k, (n_rows,), generator=gen, device=DEV)
            logp = torch.log_softmax(logits, -1).gather(1, act[:, None])[:, 0]
            act = act.float().contiguous()
        old = (logp + 0.15 * torch.randn((n_rows,), generator=gen, device=DEV)).contiguous()
    return obs, act, adv, ret, (old if agent.algo == "ppo" else None), True


def _learner_state(agent):
    L = agent.learner
    fused = L.fused_opt
    out = {"param/" + n: _np(p) for n, p in agent.policy.named_parameters()}
    out.update({"grad/" + n: _np(p.grad) for n, p in agent.policy.named_parameters()})
    out.update(exp_avg=_np(fused.exp_avg), exp_avg_sq=_np(fused.exp_avg_sq), cursor=_np(fused._cursor),
               total_norm=_np(fused.total_norm), flat_grad=_np(fused.fs.flat))
    return out


@pytest.mark.parametrize("hidden,batch", [(64, 20), (64, 40), (64, 114), (128, 20), (128, 40)])
@pytest.mark.parametrize("agent_name", ["PPO_Clip", "A2C"])
@pytest.mark.parametrize("d_in,k", [(4, 2), (3, 1), (8, 3)])
def test_update_batch_equals_small_update_per_member(d_in, k, agent_name, hidden, batch):
    """Two consecutive clipped Adam updates (the Adam state and the schedule cursor advance) of three members with
    different weights and different rows: one xpa_small_mlp_update_batch launch per update against learner.small_update
    per member.  Hidden 64: 20 rows (one workgroup), 40 (the split form, G = 2, ragged), 114 (G = 4, ragged last
    group); hidden 128: the one-image layout, one workgroup and split.  Equal: the loss scalars of both updates, every
    gradient view, the flat gradient, the parameters, both moments, the cursor and the total norm."""
    from xuanpolicy_amd import ops
    from xuanpolicy_amd.population import small_update_batch
    set_a, set_b = _learner_set(d_in, k, hidden, agent_name), _learner_set(d_in, k, hidden, agent_name)
    G = (batch + 31) // 32
    rows_wg = 32 if G > 1 else batch
    assert (int(ops.lib().xpa_small_mlp_lds_floats(rows_wg, d_in, hidden, hidden, hidden, k)) > 40704) == (hidden == 128)
    n_rows = 300
    rows, idxs = [], []
    for p, a in enumerate(set_a):
        gen = torch.Generator(device=DEV)
        gen.manual_seed(1000 * d_in + 10 * batch + p)
        rows.append(_rows(a, n_rows, d_in, k, gen))
        perm = torch.randperm(n_rows, generator=gen, device=DEV)
        idxs.append([perm[u * batch:(u + 1) * batch].contiguous() for u in range(2)])
    scalars = torch.zeros((2, 3, 8), dtype=torch.float32, device=DEV)
    want = []
    for u in range(2):
        small_update_batch([a.learner for a in set_a], rows, [ix[u] for ix in idxs], scalars[u])
        want.append([b.learner.small_update(*rows[p][:1], idxs[p][u], *rows[p][1:5], use_advnorm=True).clone()
                     for p, b in enumerate(set_b)])
    torch.cuda.synchronize()
    for p, (a, b) in enumerate(zip(set_a, set_b)):
        assert a.learner.small_update_ok(rows[p][0], batch) and a.learner.small_split
        for u in range(2):
            assert torch.equal(scalars[u, p, :6], want[u][p][:6]), "member %d update %d" % (p, u)
            assert torch.isfinite(scalars[u, p, :6]).all()
        sa, sb = _learner_state(a), _learner_state(b)
        for key in sb:
            np.testing.assert_array_equal(sa[key], sb[key], err_msg="member %d: %s" % (p, key))
        assert sa["cursor"][0] == 2 and np.abs(sa["exp_avg"]).max() > 0 and sa["total_norm"] > 0
        assert a.learner.iterations == b.learner.iterations == 2
        assert a.learner.fused_opt.step_count == b.learner.fused_opt.step_count == 2
    assert not np.array_equal(_np(scalars[1, 0]), _np(scalars[1, 1]))   # different members


# ---- 3. the permutations ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [80, 2560])
def test_permutation_batch_rows_equal_the_single_launches(n):
    """n = 80: one ragged block; n = 2560 (the committed CartPole config's buffer): ten blocks per agent."""
    from xuanpolicy_amd import ops
    seeds, counters = [1, 0xFFFFFFF0, 77], [0, 5, 0x80000001]
    as_i32 = lambda v: torch.from_numpy(np.asarray(v, np.uint32).view(np.int32)).to(DEV)   # noqa: E731
    out = ops.random_permutation_batch(n, as_i32(seeds), as_i32(counters))
    assert out.shape == (3, n)
    for p in range(3):
        want = ops.random_permutation(n, seeds[p], counters[p], device=DEV)
        assert torch.equal(out[p], want), p
        assert torch.equal(torch.sort(out[p]).values, torch.arange(n, device=DEV))


# ---- 4. end to end ---------------------------------------------------------------------------------------------------
def _agent_state(a):
    fused = a.learner.fused_opt
    out = {"sd/" + k: _np(v) for k, v in a.policy.state_dict().items()}
    out.update({"snap/" + k: v for k, v in _snapshot(a).items()})
    out.update(exp_avg=_np(fused.exp_avg), exp_avg_sq=_np(fused.exp_avg_sq), sched_cursor=_np(fused._cursor)[:1],
               adv=_np(a.memory._advantages), ret=_np(a.memory._returns))
    return out


def _assert_agents_equal(a, b, tag):
    sa, sb = _agent_state(a), _agent_state(b)
    assert sa.keys() == sb.keys()
    for k in sb:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg="%s: %s" % (tag, k))
    for name in ("current_step", "iterations", "_t", "_perm_counter"):
        assert getattr(a, name) == getattr(b, name), (tag, name)
    assert a.learner.iterations == b.learner.iterations and a.memory.ptr == b.memory.ptr
    assert a.learner.fused_opt.step_count == b.learner.fused_opt.step_count
    assert len(a.infos) == len(b.infos)
    for i, (ia, ib) in enumerate(zip(a.infos, b.infos)):
        assert ia == ib, (tag, i, ia, ib)


E2E = {"cartpole-ppo-64": ("CartPole-v1", "PPO_Clip", dict(hidden=64)),
       "pendulum-a2c-128": ("Pendulum-v1", "A2C", dict(hidden=128))}


def _e2e(case, seeds=(1, 2, 3)):
    from xuanpolicy_amd.runner import build_classic_population
    env_id, agent_name, kw = E2E[case]
    kw = dict(kw, n_envs=5, n_steps=32, n_epoch=2, n_minibatch=2, max_episode_steps=40, device=DEV)
    pop = build_classic_population(env_id, seeds=seeds, agent=agent_name, **kw)
    solo = build_classic_population(env_id, seeds=seeds, agent=agent_name, **kw).agents   # the twins, trained alone
    return pop, solo


@pytest.mark.parametrize("case", sorted(E2E))
def test_population_train_equals_the_members_trained_alone(case):
    """train(4 * 32 + 7): four iterations (the epoch graph's eager, capture and replay legs all run: 2 epochs each) and
    7 steps into the fifth rollout, against the three solo twins' train(135).  CartPole PPO at hidden 64 (K32, K30's
    resident layout, split over the 80-row minibatches); Pendulum A2C at hidden 128 (Gaussian head, K32W, the
    one-image layout)."""
    pop, solo = _e2e(case)
    plan = pop.plan()
    assert plan.n_agents == 3 and plan.chunk == 32 and pop.agents[0].batch_size == 80
    pop.train(4 * 32 + 7)
    for b in solo:
        b.train(4 * 32 + 7)
    torch.cuda.synchronize()
    assert any(isinstance(e[0], torch.cuda.CUDAGraph) for e in pop._epochs.values())   # the replay leg ran
    for i, (a, b) in enumerate(zip(pop.agents, solo)):
        assert a._t == 7 and a.iterations == 4 and len(a.infos) == 4 and a.current_step == 5 * 135
        _assert_agents_equal(a, b, "member %d" % i)
    assert not np.array_equal(_np(pop.agents[0].memory.observations), _np(pop.agents[1].memory.observations))


def test_a_member_goes_on_alone():
    """After Population.train(64) member 1 trains alone for 32 steps: it is where its solo twin is after train(96), and
    the population then takes all three members on from their own positions' common state."""
    pop, solo = _e2e("cartpole-ppo-64")
    pop.train(64)
    pop.agents[1].train(32)
    solo[1].train(96)
    torch.cuda.synchronize()
    _assert_agents_equal(pop.agents[1], solo[1], "member 1")
    # the others catch up alone too; the population, whole again, goes on as the twins do
    for i in (0, 2):
        pop.agents[i].train(32)
        solo[i].train(96)
    pop.train(32)
    for b in solo:
        b.train(32)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(pop.agents, solo)):
        _assert_agents_equal(a, b, "member %d after rejoining" % i)


def test_ineligible_populations_raise():
    from xuanpolicy_amd.population import Population
    from xuanpolicy_amd.runner import build_synthbox_ppo
    kw = dict(n_envs=5, n_steps=32, max_episode_steps=40)
    a64, b64 = (_build("cartpole", hidden=64, seed=s, **kw) for s in (1, 2))
    with pytest.raises(ValueError, match="member 1 differs from member 0 in dims"):
        Population([a64, _build("cartpole", hidden=128, seed=2, **kw)])
    box = build_synthbox_ppo(n_envs=5, n_steps=32, obs_dim=4, act_dim=2, hidden=64, seed=3, device=DEV, discrete=True)
    with pytest.raises(ValueError, match="member 2: rollout driver"):
        Population([a64, b64, box])
    with pytest.raises(ValueError, match="share a tensor"):
        Population([a64, a64])
    pop = Population([a64, b64])
    a64.train(3)                              # member 0 moves on alone: the members no longer stand at one step
    with pytest.raises(ValueError, match="member 1 differs from member 0 in t"):
        pop.train(8)
