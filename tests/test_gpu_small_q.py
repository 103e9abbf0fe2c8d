"""GPU: K34 (csrc/smallq.hip) — the PER-DQN learner step of a small MLP Q-network in HIP — against a plain f64 CPU
restatement of perdqn_learner.py:23-33 plus one torch.optim.Adam step, its forward form, the learner against its eager
twin and the agent loop on the device CartPole."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GAMMA, LR = 0.99, 1e-3
EVAL = ("representation.model.0", "eval_Qhead.model.0", "eval_Qhead.model.2")
TARGET = ("target_representation.model.0", "target_Qhead.model.0", "target_Qhead.model.2")


@pytest.fixture(scope="module", autouse=True)
def _setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _policy(D, H0, H1, A, act, seed):
    """BasicQnetwork over Basic_MLP with random weights and biases, eval and target different."""
    from xuanpolicy_amd.policies import BasicQnetwork, Basic_MLP

    class Disc:
        n, shape = A, ()
    rep = Basic_MLP((D,), [H0], None, None, act, DEV)
    pol = BasicQnetwork(Disc(), rep, [H1], None, None, act, DEV)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in pol.parameters():
            scale = 0.3 if p.dim() == 1 else 1.0 / np.sqrt(p.shape[1])
            p.copy_((torch.randn(p.shape, generator=g) * scale).to(DEV))
    return pol


def _batch(n, D, A, seed):
    g = torch.Generator().manual_seed(seed)
    obs, nxt = torch.randn(n, D, generator=g), torch.randn(n, D, generator=g)
    act = torch.randint(0, A, (n,), generator=g).float()
    rew = torch.randn(n, generator=g)
    term = (torch.rand(n, generator=g) < 0.25).float()
    return obs, nxt, act, rew, term


def _forward64(sd, names, x, act):
    z0 = x @ sd[names[0] + ".weight"].T + sd[names[0] + ".bias"]
    z1 = act(z0) @ sd[names[1] + ".weight"].T + sd[names[1] + ".bias"]
    return act(z1) @ sd[names[2] + ".weight"].T + sd[names[2] + ".bias"], torch.cat([z0.reshape(-1), z1.reshape(-1)])


def _ref_step(pol, act_mod, obs, nxt, act, rew, term):
    """perdqn_learner.py:23-33 and one Adam(lr, eps=1e-5) step in f64 on the CPU.  Returns a dict of the compared
    quantities; `margin` is the smallest |hidden pre-activation| of the two forwards (the kink distance)."""
    sd = {k: v.detach().double().cpu().clone() for k, v in pol.state_dict().items()}
    params = [sd[n + s].requires_grad_() for n in EVAL for s in (".weight", ".bias")]
    a64 = act_mod()
    evalQ, z = _forward64(sd, EVAL, obs.double(), a64)
    with torch.no_grad():
        targetQ, zt = _forward64(sd, TARGET, nxt.double(), a64)
    y = rew.double() + GAMMA * (1 - term.double()) * targetQ.max(dim=-1).values
    p = evalQ.gather(1, act.long().reshape(-1, 1)).reshape(-1)
    loss = torch.nn.functional.mse_loss(p, y)
    opt = torch.optim.Adam(params, LR, eps=1e-5)
    loss.backward()
    grads = [q.grad.clone() for q in params]
    opt.step()
    return {"td": (y - p).abs().detach(), "info": [float(loss.detach()), float(p.detach().mean())], "grads": grads,
            "params": [q.detach() for q in params], "m": [opt.state[q]["exp_avg"] for q in params],
            "v": [opt.state[q]["exp_avg_sq"] for q in params], "margin": float(torch.cat([z.detach(), zt]).abs().min())}


def _eval_params(pol):
    mods = dict(pol.named_modules())
    return [t for n in EVAL for t in (mods[n].weight, mods[n].bias)]


def _target_params(pol):
    mods = dict(pol.named_modules())
    return [t for n in TARGET for t in (mods[n].weight, mods[n].bias)]


def _rel_l2(got, ref):
    got = torch.cat([g.detach().double().cpu().reshape(-1) for g in got])
    ref = torch.cat([r.reshape(-1) for r in ref])
    return float((got - ref).norm() / ref.norm())


# (D, H0, H1, A, B, activation, seed, gradient bound).  The seeds are ones for which the f64 reference has no hidden
# pre-activation within 1e-5 of the ReLU / LeakyReLU kink (asserted below).  The gradient bound is 3 x the relative L2
# distance of the eager f32 path's gradient (the learner with small_q off: hipBLASLt GEMMs + autograd) from the same
# f64 reference on the same inputs, measured on an MI355X and written beside each case.
CASES = [
    (4, 32, 32, 2, 3, torch.nn.ReLU, 1, 3 * 5.31e-8),           # one partial row tile, G = 1          eager: 5.31e-8
    (4, 64, 64, 2, 33, torch.nn.ReLU, 2, 3 * 7.43e-8),          # G = 2, one-row tail group, indexed   eager: 7.43e-8
    (6, 128, 128, 3, 64, torch.nn.ReLU, 23, 3 * 1.29e-7),       # the widest image, LDS regions reused eager: 1.29e-7
    (2, 32, 128, 3, 128, torch.nn.LeakyReLU, 4, 3 * 1.17e-7),   # mixed widths at the reference batch  eager: 1.17e-7
    (8, 128, 64, 16, 96, torch.nn.Tanh, 5, 3 * 1.89e-7),        # widest head, A = 16                  eager: 1.89e-7
]


@pytest.mark.parametrize("D,H0,H1,A,B,act,seed,grad_bound", CASES)
def test_update_kernel_matches_f64(D, H0, H1, A, B, act, seed, grad_bound):
    from xuanpolicy_amd import ops, small_path
    pol = _policy(D, H0, H1, A, act, seed)
    indexed = B == 33
    n_rows = 100 if indexed else B
    obs, nxt, actions, rew, term = _batch(n_rows, D, A, seed)
    idx = None
    if indexed:   # rows of a larger replay array, with a repeated index; row 3 is referenced once
        idx = torch.randint(8, n_rows, (B,), generator=torch.Generator().manual_seed(seed))
        idx[6], idx[2] = idx[5], 3
    rows = slice(None) if idx is None else idx
    ref = _ref_step(pol, act, obs[rows], nxt[rows], actions[rows], rew[rows], term[rows])
    assert act is torch.nn.Tanh or ref["margin"] > 1e-5, ref["margin"]
    target0 = [p.detach().clone() for p in _target_params(pol)]
    opt = torch.optim.Adam(pol.parameters(), LR, eps=1e-5)
    sq = small_path.SmallQ(pol, opt)
    dev = [t.to(DEV) for t in (obs, nxt, actions, rew, term)]
    idx_d = None if idx is None else idx.to(DEV)
    td, sc = torch.empty(B, device=DEV), torch.empty(2, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    sq.fused.ensure_window(None)
    ops.small_q_update(sq.args(*dev, idx_d, B, GAMMA, False, td, sc, err), DEV)
    sq.fused.host_step()
    np.testing.assert_allclose(td.cpu().numpy(), ref["td"].numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(sc.cpu().numpy(), ref["info"], rtol=1e-4, atol=1e-6)
    ev = _eval_params(pol)
    dist = _rel_l2([p.grad for p in ev], ref["grads"])
    print("gradient rel L2 vs f64: %.3e (bound %.3e)" % (dist, grad_bound))
    assert dist <= grad_bound
    assert all(not p.grad.any() for p in _target_params(pol))          # the target spans of the flat gradient stay 0
    for p, rp, rm, rv in zip(ev, ref["params"], ref["m"], ref["v"]):
        np.testing.assert_allclose(p.detach().cpu().numpy(), rp.numpy(), rtol=1e-3, atol=1e-5)
        np.testing.assert_allclose(opt.state[p]["exp_avg"].cpu().numpy(), rm.numpy(), rtol=1e-3, atol=1e-5)
        np.testing.assert_allclose(opt.state[p]["exp_avg_sq"].cpu().numpy(), rv.numpy(), rtol=1e-3, atol=1e-5)
    for p, p0 in zip(_target_params(pol), target0):                     # no sync_target: bit-unchanged
        assert torch.equal(p.detach(), p0)
    assert int(err) == 0
    # a second step with sync_target: the target parameters end bit-equal to the updated eval parameters
    sq.fused.ensure_window(None)
    before = [p.detach().clone() for p in ev]
    ops.small_q_update(sq.args(*dev, idx_d, B, GAMMA, True, td, sc, err), DEV)
    sq.fused.host_step()
    for p, tp, b in zip(ev, _target_params(pol), before):
        assert torch.equal(p.detach(), tp.detach()) and not torch.equal(p.detach(), b)
    if indexed:   # two out-of-range indices and one out-of-range action: clamped and counted
        idx_d[0], idx_d[1] = -1, n_rows
        dev[2][3] = float(A)
        sq.fused.ensure_window(None)
        ops.small_q_update(sq.args(*dev, idx_d, B, GAMMA, False, td, sc, err), DEV)
        sq.fused.host_step()
        assert int(err) == 3 and bool(torch.isfinite(td).all())
    assert not sq.fused.sched_overflow()


@pytest.mark.parametrize("n", [1, 10, 33])
def test_forward_form_matches_f64(n):
    from xuanpolicy_amd import ops, small_path
    pol = _policy(4, 128, 128, 2, torch.nn.ReLU, 11)
    sq = small_path.SmallQ(pol, torch.optim.Adam(pol.parameters(), LR, eps=1e-5))
    x = _batch(n, 4, 2, 12)[0]
    sd = {k: v.detach().double().cpu() for k, v in pol.state_dict().items()}
    ref, _ = _forward64(sd, EVAL, x.double(), torch.nn.ReLU())
    q = ops.small_q_values(sq.forward_block(), x.to(DEV))
    np.testing.assert_allclose(q.cpu().numpy(), ref.numpy(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("batches", [(128,) * 5, (128, 640, 640, 128)], ids=["k34", "fallback"])
def test_learner_matches_eager_twin(batches, monkeypatch):
    """fallback: batches of 640 rows are outside K34's admission and take the eager forward / backward, stepped through
    the flat state's Adam (the flat state exists from the first update on)."""
    from xuanpolicy_amd import ops
    from xuanpolicy_amd.learners import PerDQN_Learner
    D, A = 4, 2
    pol = _policy(D, 128, 128, A, torch.nn.ReLU, 21)
    learners = []
    for p, flag in ((pol, True), (copy.deepcopy(pol), False)):
        opt = torch.optim.Adam(p.parameters(), LR, eps=1e-5)
        sch = torch.optim.lr_scheduler.LinearLR(opt, start_factor=1.0, end_factor=0.5, total_iters=10)
        lrn = PerDQN_Learner(p, opt, sch, DEV, "./", GAMMA, 2)
        lrn.small_q = flag
        learners.append(lrn)
    small, eager = learners
    launches, launch = [], ops.small_q_update
    monkeypatch.setattr(ops, "small_q_update", lambda a, dev: (launches.append(a.batch), launch(a, dev)))

    def step_both(k, B):
        obs, nxt, act, rew, term = (t.to(DEV) for t in _batch(B, D, A, 100 + k))
        assert small.small_q_ok(obs, B) == (B <= 512) and not eager.small_q_ok(obs, B)
        td, info = small.update(obs, act, rew, nxt, term)
        td_e, info_e = eager.update(obs, act, rew, nxt, term)
        assert td.device.type == "cuda" and td.dtype == torch.float32
        np.testing.assert_allclose(td.cpu().numpy(), td_e.cpu().numpy(), rtol=1e-4, atol=1e-5, err_msg="update %d" % k)
        np.testing.assert_allclose([info[n] for n in ("Qloss", "learning_rate", "predictQ")],
                                   [info_e[n] for n in ("Qloss", "learning_rate", "predictQ")], rtol=1e-4, atol=1e-6)
        sd_e = eager.policy.state_dict()
        for key, v in small.policy.state_dict().items():
            np.testing.assert_allclose(v.cpu().numpy(), sd_e[key].cpu().numpy(), rtol=1e-3, atol=1e-5,
                                       err_msg="%s, update %d" % (key, k))
    for k, B in enumerate(batches):
        step_both(k, B)
    n = len(batches)
    assert small.iterations == eager.iterations == small._small_q_state().fused.step_count == n
    assert launches == [B for B in batches if B <= 512]
    # the flat optimizer's state loads into the eager one (a copy: load_state_dict keeps the tensors it is given), and
    # the eager step from the loaded moments and step count matches the small learner's next step
    sd = copy.deepcopy(small.optimizer.state_dict())
    assert all(int(st["step"]) == n for st in sd["state"].values())
    eager.optimizer.load_state_dict(sd)
    step_both(n, 128)
    assert int(small.optimizer.state_dict()["state"][0]["step"]) == n + 1


def test_agent_trains_on_device_cartpole(monkeypatch):
    from xuanpolicy_amd import ops
    from xuanpolicy_amd.runner import build_perdqn_classic
    launches, launch = [], ops.small_q_update
    monkeypatch.setattr(ops, "small_q_update", lambda a, dev: (launches.append(a.batch), launch(a, dev)))
    agent = build_perdqn_classic("CartPole-v1", small_q=True, parallels=4, n_size=256, batch_size=64, start_training=64,
                                 sync_frequency=20)
    lrn = agent.learner
    start = [p.detach().clone() for p in _eval_params(agent.policy)]
    agent.train(400)
    agent.train((-lrn.iterations) % 20 or 20)   # on to the next sync step
    torch.cuda.synchronize()
    assert lrn.iterations % 20 == 0 and lrn.iterations == len(agent.infos) > 300
    assert launches == [64] * lrn.iterations and lrn._small_q_state().fused.step_count == lrn.iterations   # K34 ran them
    assert agent.check_errors() == {"per_sample": 0, "gather": 0, "env": 0, "td_action": 0, "maxpool": 0}
    assert np.isfinite([float(i["Qloss"]) for i in agent.infos]).all()
    assert not lrn._small_q_state().fused.sched_overflow()
    for p, tp, p0 in zip(_eval_params(agent.policy), _target_params(agent.policy), start):
        assert torch.equal(p.detach(), tp.detach()) and not torch.equal(p.detach(), p0)
