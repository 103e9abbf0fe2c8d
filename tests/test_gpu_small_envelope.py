"""GPU: the one-launch small path (K30 update, K32 / K32W rollout step, K33 closing) at the shapes its admission rules
take and the rest of the suite does not run: mixed layer widths, widths 96, 160 and 256 (192 is not run), d_in up to
32, k up to 16, ReLU and Tanh, the one-image form with h1 != h2 in either order — all with NON-ZERO biases (a fresh
policy's are 0, which hides a dropped or misplaced bias) — against torch f64 (tests/_small_ref.py).

  1. K30's raw gradients and loss scalars against f64 autograd of the reference loss, every row of CASES.
  2. One negative control: the checker rejects K30's gradients against a reference side with b1 and b2 swapped.
  3. The population form (xpa_small_mlp_update_batch) against small_update per member at two mixed shapes.
  4. K30's clip-and-Adam tail (in the update kernel, and the split form's finalize kernel) against f64, two chained
     updates.
  5. K32 / K32W at mixed widths: values, log-probs and sampled actions against f64; K33's bootstraps bit for bit.

The gradient bound is tests/_small_ref.py's within_f32 with MARGIN 4 (reasoned there, not fitted): pooled over all of a
run's gradient tensors, |K30 - f64| <= 4 E32 + 2^-24 max |f64|, E32 the worst error of torch's own f32 autograd of the
same loss (on a deep copy of the policy, on the device).  Every run prints its worst |err| / E32.

Measured on an MI355X, the largest printed |err| / E32 per test (the margin used is 4 everywhere; nothing needed more):
  test_k30_gradients_match_f64                 2.25 (row 1 PPO, 32 rows); per case 1.0 .. 2.25, one-image rows <= 1.79
  test_k30_clip_and_adam_tail_matches_f64      steps 1.28, exp_avg 1.46, exp_avg_sq 1.92
  test_the_checker_rejects_k30_against_swapped_biases   5.7e6 against the swapped reference side (all 10 tensors)
  test_k32_step_and_k33_bootstraps_with_biases max |value - f64| 9.8e-8, max |log-prob - f64| 1.9e-7 (tolerance 2e-4)
No kernel bug was found and no shape's admission was narrowed.

One finding, in the tail, kept as a documented property and not changed here: the betas cross the C ABI as `float`, so
K30 (like K9, whose arithmetic it restates) runs Adam at beta2 = f32(0.999) = 0.99900001287.  It does so consistently
(1 - beta2 is exact in f32 and the schedule's bias correction is pow((double)beta2, step)), so the parameter steps
agree with f64 Adam at 0.999 itself inside the bound (step ratio 0.75 in the one run measured against it); but
exp_avg_sq scales with 1 - beta2 and so sits 1.29e-5 (relative) below torch's, 59 x E32 in that run.  tests/test_gpu_kernels.py's
test_fused_clip_adam_matches_torch holds K9's exp_avg_sq at rtol 1e-4 beside 1e-5 for exp_avg for the same reason.  The
tail test therefore gives the f64 reference and the f32 baseline the betas the kernel is given (the f32 values); against
those the bound holds with the ratios above.  Passing the betas (or 1 - beta) as doubles would remove the difference; it
changes four entry points' signatures and XpaSmallMlpArgs, which tests/test_capi_cpu.py pins.

Two places where the checks are narrower than "every run" for a reason of arithmetic, not of the kernel:
  * a 1-row minibatch has a normalised advantage of exactly 0 ((adv - mean) = 0), so with a Gaussian head the f64
    gradient of the mu path (W1, b1, Wa, ba) IS zero there; "every gradient tensor has a non-zero reference" is asserted
    for every other tensor of such a run, and those four are asserted to be exactly zero in K30's output instead;
  * one row's clip ratio is 0 or 1, so "strictly between 0 and 1" is asserted for the batches of >= 31 rows."""
import copy

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from tests import _small_ref as sr
from tests.test_gpu_small_close import _one_k32_step
from tests.test_gpu_wide_small import ENVS, _uniforms
from tests.test_small_envelope_cpu import LDS_BUDGET, TABLE, UNSPLIT, layout, wrong_reference

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cpu_ref.build_oracle()


def _np(t):
    return t.detach().cpu().numpy().copy()


# ---- 1. K30's gradients against f64 -----------------------------------------------------------------------------------
# row of the table -> ((d_in, k, h0, h1, h2), discrete, activation, the algorithms it runs with): PPO_Clip and A2C
# alternate down the table; rows 1, 7 and 10 run with both
ROWS = {1: ((4, 2, 32, 64, 32), True, "ReLU", ("PPO_Clip", "A2C")),
        2: ((5, 3, 64, 32, 96), True, "LeakyReLU", ("A2C",)),
        3: ((32, 16, 96, 64, 32), True, "Tanh", ("PPO_Clip",)),
        4: ((13, 5, 32, 256, 32), True, "LeakyReLU", ("A2C",)),
        5: ((13, 5, 32, 32, 256), True, "Tanh", ("PPO_Clip",)),
        6: ((1, 2, 256, 32, 32), True, "LeakyReLU", ("A2C",)),
        7: ((13, 5, 128, 64, 128), True, "LeakyReLU", ("PPO_Clip", "A2C")),
        8: ((32, 16, 160, 96, 32), True, "Tanh", ("A2C",)),
        9: ((5, 3, 96, 128, 160), True, "ReLU", ("PPO_Clip",)),
        10: ((3, 1, 64, 32, 96), False, "LeakyReLU", ("A2C", "PPO_Clip")),
        11: ((17, 6, 96, 128, 160), False, "Tanh", ("PPO_Clip",)),
        12: ((32, 16, 256, 64, 32), True, "LeakyReLU", ("PPO_Clip",))}
assert [r[0] for r in ROWS.values()] == list(TABLE)
CASES = [(row, name) for row, r in ROWS.items() for name in r[3]]
BATCHES = (1, 31, 32, 33, 70)


def _learner(row, agent_name, seed=13, learning_rate=0.0):
    """The agent of one row with every bias (and a Gaussian's logstd) overwritten with non-zero values."""
    from xuanpolicy_amd.runner import build_synthbox_ppo
    (d_in, k, h0, h1, h2), discrete, activation, _ = ROWS[row]
    agent = build_synthbox_ppo(n_envs=8, n_steps=16, obs_dim=d_in, act_dim=k, discrete=discrete, seed=seed, device=DEV,
                               agent=agent_name, learning_rate=learning_rate, ent_coef=0.01, graph_update=False,
                               representation_hidden_size=[h0], actor_hidden_size=[h1], critic_hidden_size=[h2],
                               activation=activation)
    names = sr.randomise_biases(agent.policy)
    assert len(names) == (5 if discrete else 6)
    for n, p in agent.policy.named_parameters():
        if n in names:
            assert float(p.detach().abs().min()) > 0, n
    assert agent.learner.small_policy_layers().dims == (d_in, h0, h1, h2, k)
    return agent


def _f64(agent, row):
    (d_in, k, h0, h1, h2), discrete, activation, _ = ROWS[row]
    pol = sr.build_f64_policy(d_in, k, h0, h1, h2, discrete, activation, src=agent)
    for (n, p), (m, q) in zip(agent.policy.named_parameters(), pol.named_parameters()):
        assert p.shape == q.shape and n.split(".")[-1] == m.split(".")[-1], (n, m)
    return pol


def _hp(agent):
    L = agent.learner
    return dict(clip_range=float(L.clip_range), vf_coef=float(L.vf_coef), ent_coef=float(L.ent_coef))


def _rows(agent, n_rows, d_in, k, gen, ret_scale=1.0):
    """Random buffer rows; the old log-probs are the policy's own, jittered by 0.15 sigma so that some ratios leave the
    clip range (tests/test_gpu_population.py's _rows)."""
    from xuanpolicy_amd.policies import policy_heads
    obs = torch.randn((n_rows, d_in), generator=gen, device=DEV)
    adv, ret = (torch.randn((n_rows,), generator=gen, device=DEV) for _ in range(2))
    ret = (ret * ret_scale).contiguous()
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
    return obs, act, adv, ret, old


def _cursor(agent):
    return int(agent.learner.fused_opt._cursor[0])


def _arm_schedule(agent):
    fused = agent.learner.fused_opt
    if not fused.sched_enabled:
        fused.enable_sched()
    fused.ensure_window(agent.learner.scheduler)
    return _cursor(agent)


def _reference_side(agent, pol64, idx, rows):
    """(f64 gradients, f64 scalars, f32 baseline gradients) of the minibatch idx."""
    mb = [x[idx] for x in rows]
    ref, sc64 = sr.small_update_ref(pol64, agent.algo, agent.dist, *mb, _hp(agent))
    base, _ = sr.f32_baseline(agent.policy, agent.algo, agent.dist, *mb, _hp(agent))
    return ref, sc64, base


def _k30(agent, idx, rows):
    """One K30 update of minibatch idx: (loss scalars [6], the gradient views, cloned)."""
    obs, act, adv, ret, old = rows
    sc = agent.learner.small_update(obs, idx, act, adv, ret, old if agent.algo == "ppo" else None,
                                    use_advnorm=True).clone()
    torch.cuda.synchronize()
    return sc[:6], [p.grad.detach().clone() for p in agent.policy.parameters()]


@pytest.mark.parametrize("row,agent_name", [c for c in CASES if c[0] != 12],
                         ids=["row%d-%s" % c for c in CASES if c[0] != 12])
def test_k30_gradients_match_f64(row, agent_name):
    """Batches of 1, 31 and 32 rows (one workgroup), 33 (the split form with a one-row second workgroup), 70 (G = 3,
    ragged), on rows 1 and 7 also 512 (G = 16, the limit), and on rows 1, 2 and 10 also 64 and 70 rows as ONE workgroup
    of two or three 32-row tiles (small_split off).  Learning rate 0 and no clipping: the raw gradient stays in the flat
    buffer and every run starts from the same weights."""
    dims, discrete, activation, _ = ROWS[row]
    d_in, k, h0, h1, h2 = dims
    kdims = (d_in, h0, h1, h2, k)
    agent = _learner(row, agent_name)
    L = agent.learner
    L._use_clip = False
    pol64 = _f64(agent, row)
    runs = [(b, True) for b in BATCHES + ((512,) if row in (1, 7) else ())]
    runs += [(b, False) for b in (64, 70)] if dims in UNSPLIT else []
    n_rows = 600 if row in (1, 7) else 160
    gen = torch.Generator(device=DEV)
    gen.manual_seed(100 * d_in + k)
    rows = _rows(agent, n_rows, d_in, k, gen)
    before = [p.detach().clone() for p in agent.policy.parameters()]
    names = [n for n, _ in agent.policy.named_parameters()]
    cur = _arm_schedule(agent)
    worst = 0.0
    for batch, split in runs:
        tag = "row %d %s batch %d split %s" % (row, agent_name, batch, split)
        L.small_split = split
        per_wg = 32 if split and 32 < batch <= 512 else batch
        lay = layout(per_wg, kdims)
        assert lay == (TABLE[dims][0] if per_wg <= 32 else "R") and L.small_update_ok(rows[0], batch), tag
        idx = torch.randperm(n_rows, generator=gen, device=DEV)[:batch].contiguous()
        ref, sc64, base = _reference_side(agent, pol64, idx, rows)
        sc, got = _k30(agent, idx, rows)
        cur += 1
        assert _cursor(agent) == cur, tag
        if agent.algo == "ppo" and batch >= 31:
            assert 0 < float(sc64[4]) < 1, tag
        np.testing.assert_allclose(_np(sc), sc64.numpy(), rtol=1e-4, atol=1e-5, err_msg=tag)
        for n, r, g in zip(names, ref, got):
            if batch == 1 and not discrete and n.startswith("actor.mu"):
                assert float(r.abs().max()) == 0 and float(g.abs().max()) == 0, (tag, n)   # (the module docstring)
            else:
                assert float(r.abs().max()) > 0, (tag, n)
        res = sr.within_f32(got, base, ref)
        print("%s (%s): worst |err| / E32 %.3g in %s (E32 %.3g, scale %.3g)"
              % (tag, lay, res.ratio, names[res.worst], res.e32, res.scale))
        assert res.ok, (tag, [names[i] for i in res.bad], res)
        worst = max(worst, res.ratio)
        assert all(torch.equal(p, q) for p, q in zip(agent.policy.parameters(), before)), tag   # lr 0
    print("row %d %s: the largest |err| / E32 of the case %.3g" % (row, agent_name, worst))
    if row == 7:   # past 512 rows the split form is off, and a one-image shape takes at most 32 rows per workgroup
        L.small_split = True
        assert L.small_update_ok(rows[0], 512) and not L.small_update_ok(rows[0], 513)


def test_the_shape_past_the_budget_is_refused():
    """Row 12: 41476 floats even as one image.  small_update_ok is False at every batch, split or not, and nothing is
    launched."""
    dims = ROWS[12][0]
    assert TABLE[dims][0] is None and TABLE[dims][2] > LDS_BUDGET
    agent = _learner(12, "PPO_Clip")
    obs = torch.zeros((600, dims[0]), device=DEV)
    for split in (True, False):
        agent.learner.small_split = split
        for batch in BATCHES + (64, 512):
            assert not agent.learner.small_update_ok(obs, batch), (split, batch)
    assert not agent.learner.fused_opt.sched_enabled or _cursor(agent) == 0


# ---- 2. the negative control ------------------------------------------------------------------------------------------
def test_the_checker_rejects_k30_against_swapped_biases():
    """Row 7 at 33 rows: K30's gradients pass against the true reference side and are rejected against the one computed
    with b1 and b2 taken from each other (tests/test_small_envelope_cpu.py's wrong_reference: f64 and its f32 baseline
    from the same wrong policy, so that E32 stays roundoff)."""
    agent = _learner(7, "PPO_Clip")
    agent.learner._use_clip = False
    d_in, k = ROWS[7][0][:2]
    pol64 = _f64(agent, 7)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(7)
    rows = _rows(agent, 160, d_in, k, gen)
    idx = torch.randperm(160, generator=gen, device=DEV)[:33].contiguous()
    ref, _, base = _reference_side(agent, pol64, idx, rows)
    _, got = _k30(agent, idx, rows)
    assert sr.within_f32(got, base, ref).ok
    mb = [x[idx].cpu() for x in rows]
    bad_ref, bad_base = wrong_reference("b1-b2-swapped", pol64, agent.algo, agent.dist, mb, _hp(agent))
    res = sr.within_f32(got, bad_base, bad_ref)
    print("swapped biases: worst |err| / E32 %.3g, rejected in tensors %s" % (res.ratio, res.bad))
    assert not res.ok and res.ratio > 1e3


# ---- 3. the population form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row,agent_name", [(7, "PPO_Clip"), (10, "A2C")])
def test_update_batch_equals_small_update_per_member_at_mixed_widths(row, agent_name):
    """tests/test_gpu_population.py's comparison at a mixed one-image shape and a mixed Gaussian one: two members with
    different seeds and rows, one xpa_small_mlp_update_batch launch against small_update per member, at 20 rows (one
    workgroup) and 33 (split) — scalars, gradient views and the flat gradient equal bit for bit."""
    from xuanpolicy_amd.population import small_update_batch
    d_in, k = ROWS[row][0][:2]
    set_a = [_learner(row, agent_name, seed=s) for s in (3, 4)]
    set_b = [_learner(row, agent_name, seed=s) for s in (3, 4)]
    for a, b in zip(set_a, set_b):   # the same (random) biases in both sets
        with torch.no_grad():
            for p, q in zip(a.policy.parameters(), b.policy.parameters()):
                q.copy_(p)
        a.learner._use_clip = b.learner._use_clip = False
    rows, gens = [], []
    for p, a in enumerate(set_a):
        gen = torch.Generator(device=DEV)
        gen.manual_seed(1000 * row + p)
        obs, act, adv, ret, old = _rows(a, 160, d_in, k, gen)
        rows.append((obs, act, adv, ret, old if a.algo == "ppo" else None, True))
        gens.append(gen)
    assert not torch.equal(rows[0][0], rows[1][0])
    for batch in (20, 33):
        idxs = [torch.randperm(160, generator=g, device=DEV)[:batch].contiguous() for g in gens]
        scalars = torch.zeros((2, 8), dtype=torch.float32, device=DEV)
        small_update_batch([a.learner for a in set_a], rows, idxs, scalars)
        want = [b.learner.small_update(rows[p][0], idxs[p], *rows[p][1:5], use_advnorm=True).clone()
                for p, b in enumerate(set_b)]
        torch.cuda.synchronize()
        for p, (a, b) in enumerate(zip(set_a, set_b)):
            tag = "row %d batch %d member %d" % (row, batch, p)
            assert a.learner.small_update_ok(rows[p][0], batch), tag
            assert torch.equal(scalars[p, :6], want[p][:6]) and torch.isfinite(scalars[p, :6]).all(), tag
            for (n, x), y in zip(a.policy.named_parameters(), b.policy.parameters()):
                assert torch.equal(x.grad, y.grad) and float(x.grad.abs().max()) > 0, (tag, n)
            assert torch.equal(a.learner.fused_opt.fs.flat, b.learner.fused_opt.fs.flat), tag
        assert not torch.equal(scalars[0], scalars[1])   # different members


# ---- 4. the clip-and-Adam tail ------------------------------------------------------------------------------------------
# (row, batch, split): the tail inside the update kernel; the finalize kernel; one image + finalize; Gaussian + finalize
TAILS = [(2, 64, False), (2, 70, True), (7, 33, True), (10, 33, True)]


def _load(pol, params):
    with torch.no_grad():
        for p, x in zip(pol.parameters(), params):
            p.copy_(x)


@pytest.mark.parametrize("clip", [True, False], ids=["clip-0.5", "no-clip"])
@pytest.mark.parametrize("row,batch,split", TAILS, ids=["row%d-%d-split%d" % t for t in TAILS])
def test_k30_clip_and_adam_tail_matches_f64(row, batch, split, clip):
    """Two consecutive updates (learning rate 1e-3 on the linear schedule, `ret` scaled by 10 so that the gradient's
    norm is past max_norm 0.5) on two minibatches.  The f64 reference chains: its second update starts from ITS state
    after the first, and so does the f32 baseline (torch's f32 autograd + clip_grad_norm_ + Adam on a deep copy).  After
    each update the parameter steps (one extra 2^-24 max |p| in the floor: the stored parameter's rounding), exp_avg
    and exp_avg_sq pass within_f32 as three sets, and total_norm is within 1e-5 of the f64 norm
    (test_fused_clip_adam_matches_torch's tolerance)."""
    agent_name = ROWS[row][3][0]
    d_in, k = ROWS[row][0][:2]
    agent = _learner(row, agent_name, learning_rate=1e-3)
    L = agent.learner
    L._max_norm, L._use_clip, L.small_split = 0.5, clip, split
    max_norm = 0.5 if clip else -1.0
    pol64 = _f64(agent, row)
    base_pol = copy.deepcopy(agent.policy).float()
    g0 = L.optimizer.param_groups[0]
    assert g0["eps"] == 1e-5 and tuple(g0["betas"]) == (0.9, 0.999)
    # the betas as the kernel receives them: they cross the C ABI as `float beta1, beta2`, and Adam at f32(0.999) is
    # what K30 (like K9) then computes, consistently — 1 - beta2 is exact in f32 and the schedule's bias correction is
    # pow((double)beta2, step).  The reference and the baseline get those betas; see the module docstring
    betas = tuple(float(np.float32(b)) for b in g0["betas"])
    base_opt = torch.optim.Adam(base_pol.parameters(), lr=g0["lr"], betas=betas, eps=1e-5)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(31 * row + batch)
    rows = _rows(agent, 160, d_in, k, gen, ret_scale=10.0)
    perm = torch.randperm(160, generator=gen, device=DEV)
    hp = _hp(agent)
    params = list(agent.policy.parameters())
    m64, v64 = ([torch.zeros_like(p) for p in pol64.parameters()] for _ in range(2))
    cur = _arm_schedule(agent)
    for u in range(2):
        tag = "row %d batch %d split %s clip %s update %d" % (row, batch, split, clip, u + 1)
        idx = perm[u * batch:(u + 1) * batch].contiguous()
        mb = [x[idx] for x in rows]
        lr = float(g0["lr"])
        assert 0 < lr <= 1e-3 and L.small_update_ok(rows[0], batch), tag
        # the f64 reference, from its own state
        p64 = [p.detach().clone() for p in pol64.parameters()]
        g64, _ = sr.small_update_ref(pol64, agent.algo, agent.dist, *mb, hp)
        if u == 0:   # measured, not asserted: exp_avg_sq at the optimizer's own (double) betas
            v_dbl = sr.clip_adam_ref(p64, g64, m64, v64, 1, lr, max_norm, (0.9, 0.999), 1e-5)[2]
        new64, m64, v64, norm64 = sr.clip_adam_ref(p64, g64, m64, v64, u + 1, lr, max_norm, betas, 1e-5)
        _load(pol64, new64)
        assert float(norm64) > 0.5, tag
        # the f32 baseline, from its own state
        b_before = [p.detach().clone() for p in base_pol.parameters()]
        gb, _ = sr.small_update_grads(base_pol, agent.algo, agent.dist, *mb, hp)
        for p, g in zip(base_pol.parameters(), gb):
            p.grad = g.clone()
        if clip:
            torch.nn.utils.clip_grad_norm_(list(base_pol.parameters()), 0.5)
        base_opt.param_groups[0]["lr"] = lr
        base_opt.step()
        # K30
        before = [p.detach().clone() for p in params]
        _k30(agent, idx, rows)
        cur += 1
        assert _cursor(agent) == cur and L.fused_opt.step_count == u + 1, tag
        sets = {
            "step": ([p.detach() - b for p, b in zip(params, before)],
                     [p.detach() - b for p, b in zip(base_pol.parameters(), b_before)],
                     [a - b for a, b in zip(new64, p64)]),
            "exp_avg": ([L.optimizer.state[p]["exp_avg"] for p in params],
                        [base_opt.state[p]["exp_avg"] for p in base_pol.parameters()], m64),
            "exp_avg_sq": ([L.optimizer.state[p]["exp_avg_sq"] for p in params],
                           [base_opt.state[p]["exp_avg_sq"] for p in base_pol.parameters()], v64)}
        pmax = max(float(p.abs().max()) for p in p64)
        for name, (got, base, ref) in sets.items():
            assert all(float(r.abs().max()) > 0 for r in ref), (tag, name)
            res = sr.within_f32(got, base, ref, extra_floor=2.0 ** -24 * pmax if name == "step" else 0.0)
            print("%s %s: worst |err| / E32 %.3g (E32 %.3g, scale %.3g)" % (tag, name, res.ratio, res.e32, res.scale))
            assert res.ok, (tag, name, res)
        np.testing.assert_allclose(float(L.fused_opt.total_norm), float(norm64), rtol=1e-5, err_msg=tag)
        if u == 0:
            # against f64 Adam at the optimizer's own betas the second moment is off by the f32 beta2's share and no
            # more: |1 - (1 - f32(0.999)) / 0.001| = 1.29e-5 of its scale, on top of the bound
            quant = abs(1.0 - (1.0 - betas[1]) / (1.0 - g0["betas"][1]))
            dev = max(float((g.detach().cpu().double() - r).abs().max()) for g, r in zip(sets["exp_avg_sq"][0], v_dbl))
            scale = max(float(r.abs().max()) for r in v_dbl)
            print("%s: max |exp_avg_sq - f64 at betas (0.9, 0.999)| / max |exp_avg_sq| %.3g (1 - f32(0.999) is 0.001 x "
                  "(1 - %.3g))" % (tag, dev / scale, quant))
            assert 1e-5 < quant < 2e-5 and dev <= quant * scale + sr.MARGIN * res.e32 + 2.0 ** -24 * scale, tag
    assert float(g0["lr"]) < 1e-3   # the schedule moved: the two updates ran at two learning rates


# ---- 5. K32 / K32W and K33 at mixed widths, non-zero biases --------------------------------------------------------------
MIXED = [(a, b, c) for a in (32, 64) for b in (32, 64) for c in (32, 64) if not a == b == c]
K32_CASES = [("cartpole", "PPO_Clip", w) for w in MIXED]
K32_CASES += [("pendulum", "A2C", (64, 32, 64)), ("pendulum", "A2C", (32, 64, 32)), ("mountaincar", "PPO_Clip", (32, 32, 64))]
K32_CASES += [("cartpole", "PPO_Clip", (h, h, h)) for h in (32, 64, 128)]   # for the bias coverage alone
assert len(MIXED) == 6


@pytest.mark.parametrize("N", [1, 17])
@pytest.mark.parametrize("kind,agent_name,widths", K32_CASES, ids=["%s-%d-%d-%d" % ((c[0],) + c[2]) for c in K32_CASES])
def test_k32_step_and_k33_bootstraps_with_biases(kind, agent_name, widths, N):
    """One K32 / K32W step of a policy whose biases (and logstd) were overwritten with non-zero values, on rows =
    agent.obs_norm: the stored values and the stored log-prob of the stored action against the f64 module at the
    project's K32 tolerance (tests/test_gpu_classic.py: rtol 1e-4, atol 2e-4); a Categorical action is the first class
    whose f64 CDF exceeds K3's uniform wherever that uniform is more than 1e-5 from a CDF edge (at least 15 of 17 envs,
    the one env at N = 1; seed 11, the helper's); K33's bootstraps of those rows equal the stored values bit for bit in
    every row group and its guards are intact (asserted in _one_k32_step)."""
    h0, h1, h2 = widths
    _, D, K, _ = ENVS[kind]
    cat = kind != "pendulum"
    kw = dict(hidden=h0, actor_hidden_size=[h1], critic_hidden_size=[h2], agent=agent_name)
    agent, rows, vboot, S = _one_k32_step((kind, kw), N, randomise_biases=True)
    assert agent.plan().driver == ("K32W" if widths == (128, 128, 128) else "K32")
    assert agent.learner.small_policy_layers().dims == (D, h0, h1, h2, K)
    for n, p in agent.policy.named_parameters():
        if n.endswith("bias") or n.endswith("logstd"):
            assert float(p.detach().abs().min()) > 0, n
    pol64 = sr.build_f64_policy(D, K, h0, h1, h2, cat, agent.config.activation, src=agent)
    with torch.no_grad():
        head64, logstd64, v64 = pol64.heads(agent.obs_norm.detach().cpu().double())
    mem = agent.memory
    val = _np(mem.values[:, 0])
    np.testing.assert_allclose(val, v64.numpy(), rtol=1e-4, atol=2e-4)
    logp = _np((mem.auxiliary_infos["old_logp"] if agent.algo == "ppo" else agent.logp_scratch)[:, 0])
    act = mem.actions[:, 0].detach().cpu()
    if cat:
        a = act.reshape(N).long()
        logp64 = torch.log_softmax(head64, -1).gather(1, a[:, None])[:, 0]
        cdf = np.cumsum(torch.softmax(head64, -1).numpy(), -1)[:, :-1]
        u = _uniforms(agent.seed, N, 1)[:, 0]
        clear = np.abs(u[:, None] - cdf).min(-1) > 1e-5
        assert clear.sum() >= (15 if N == 17 else 1)
        want = (u[:, None] >= cdf).sum(-1)
        np.testing.assert_array_equal(a.numpy()[clear], want[clear])
    else:
        logp64 = torch.distributions.Normal(head64, logstd64.detach().exp()).log_prob(act.reshape(N, K).double()).sum(-1).detach()
    print("%s %s N %d: max |value - f64| %.3g, max |logp - f64| %.3g"
          % (kind, widths, N, np.abs(val - v64.numpy()).max(), np.abs(logp - logp64.numpy()).max()))
    np.testing.assert_allclose(logp, logp64.numpy(), rtol=1e-4, atol=2e-4)
    want = mem.values[:, 0]
    assert torch.isfinite(want).all() and (N == 1 or float(want.std()) > 0)
    for g in range(S + 1):
        assert torch.equal(vboot[g], want), (kind, widths, N, g, float((vboot[g] - want).abs().max()))
