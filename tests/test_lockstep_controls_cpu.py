"""CPU: negative controls for the lockstep replay (tests/_oracle_replay.py: replay_updates_lockstep).

The lockstep check lets the oracle's gradient take or drop clip-bound rows and (Leaky)ReLU kink candidates before it
holds each tensor to 1e-3 relative L2.  These tests show that it still goes red on a wrong update.  The "device" is a
stub agent whose snapshots and loss scalars come from an f64 LearnerRef stepping Adam (weights rounded to f32 before
each update, gradients cast to f32): the clean record passes, and every fault of tests/_lockstep_faults.py — sized
against the checker's own tolerances — is red at its intended assertion at updates 0, 1 and the last."""
import copy
import types

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from tests import _lockstep_faults as faults
from tests._oracle_replay import LockstepReplay, replay_updates_lockstep

N, T, H, N_EPOCH, N_MB = 64, 16, 64, 2, 4
B = N * T // N_MB
U = N_EPOCH * N_MB
GRAD_RTOL, LOSS_TOL = 1e-3, 1e-4

CASES = {
    # name: (algo, discrete, D, A, ent_coef, learning rate: large enough that rows cross a clip bound after one step)
    "ppo_gaussian": ("ppo", False, 17, 6, 0.01, 3e-3),
    "a2c_categorical": ("a2c", True, 17, 8, 0.01, 3e-3),
}


class _StubAgent:
    """What the lockstep checker touches of an agent: n_envs, n_steps, config, memory, epoch_permutation, update_log."""

    def __init__(self, algo, discrete, D, A, seed):
        self.n_envs, self.n_steps = N, T
        self.config = types.SimpleNamespace(clip_grad_norm=0.5, clip_grad=0.5, vf_coef=0.25, clip_range=0.2)
        gen = torch.Generator().manual_seed(seed)
        torch.manual_seed(seed)
        self.pol = cpu_ref.build_actor_critic_ref(D, A, [H], [H], [H], discrete=discrete)
        obs = torch.randn((N, T, D), generator=gen)
        with torch.no_grad():
            head, logstd, v = self.pol.heads(obs.reshape(N * T, D))
            d = self.pol.dist(head, logstd)
            if discrete:
                act = torch.multinomial(d.probs, 1, generator=gen)[:, 0]
                logp = d.log_prob(act)
                act = act.float().reshape(N, T)
            else:
                act = head + logstd.exp() * torch.randn(head.shape, generator=gen)
                logp = d.log_prob(act).sum(-1)
                act = act.reshape(N, T, A)
        self.memory = types.SimpleNamespace(
            observations=obs, actions=act, values=v.reshape(N, T).clone(),
            auxiliary_infos={"old_logp": logp.reshape(N, T).clone()} if algo == "ppo" else {})
        self.adv = torch.randn((N, T), generator=gen).double().numpy()
        self.ret = (v.reshape(N, T) + torch.randn((N, T), generator=gen)).double().numpy()
        self.update_log = []

    def epoch_permutation(self, n, counter):
        return torch.randperm(n, generator=torch.Generator().manual_seed(1000 + counter))


def _record(name):
    """The stub's clean record of one iteration: (agent, kwargs of replay_updates_lockstep, snaps, update_log)."""
    algo, discrete, D, A, ent, lr = CASES[name]
    agent = _StubAgent(algo, discrete, D, A, seed=7)
    kwargs = dict(pol=copy.deepcopy(agent.pol), adv=agent.adv, ret=agent.ret, discrete=discrete, A=A, algo=algo, ent=ent,
                  n_epoch=N_EPOCH, n_mb=N_MB, perm_counter=3, loss_tol=LOSS_TOL, grad_rtol=GRAD_RTOL)
    rp = LockstepReplay(agent, copy.deepcopy(agent.pol), agent.adv, agent.ret, discrete, A, algo, ent, N_EPOCH, N_MB, 3)
    dev = copy.deepcopy(agent.pol).double()   # the stand-in device: f64 math on f32-rounded weights, Adam steps
    lrn = cpu_ref.LearnerRef(dev, torch.optim.Adam(dev.parameters(), lr, eps=1e-5), None, algo, agent.config.vf_coef,
                             ent, agent.config.clip_range, 0.5, True)
    snaps, log = [], []
    for u in range(U):
        with torch.no_grad():
            for p in dev.parameters():
                p.copy_(p.float().double())
        w = [p.detach().float().clone() for p in dev.parameters()]
        o, a, r, ad, old_logp = rp.batch(u)
        info = lrn.update(o, a, r, ad, old_logp, capture_grads=True)
        snaps.append((w, [g.float() for g in lrn.last_grads]))
        loss = info["actor-loss"] - ent * info["entropy"] + agent.config.vf_coef * info["critic-loss"]
        log.append(np.array([info["actor-loss"], info["critic-loss"], info["entropy"], loss,
                             info.get("clip_ratio", 0.0), info["predict_value"]], np.float32))
    agent.update_log = log
    return agent, kwargs, snaps, log


_MADE = {}


def _make(name):
    if name not in _MADE:
        _MADE[name] = _build(name)
    return _MADE[name]


@pytest.fixture(scope="module", params=sorted(CASES))
def record(request):
    return _make(request.param)


@pytest.fixture(scope="module")
def ppo_record():
    return _make("ppo_gaussian")


def _build(name):
    agent, kwargs, snaps, log = _record(name)
    rp = LockstepReplay(agent, copy.deepcopy(kwargs["pol"]), kwargs["adv"], kwargs["ret"], kwargs["discrete"],
                        kwargs["A"], kwargs["algo"], kwargs["ent"], N_EPOCH, N_MB, 3)
    return types.SimpleNamespace(name=name, algo=kwargs["algo"], agent=agent, kwargs=kwargs, snaps=snaps,
                                 log=log, rp=rp)


def _check(rec, snaps, log, only):
    return replay_updates_lockstep(rec.agent, snaps=snaps, update_log=log, only_updates=only, **rec.kwargs)


def test_clean_record_passes_and_exercises_the_adaptation(record):
    recs = _check(record, record.snaps, record.log, None)
    assert [r["update"] for r in recs] == list(range(U))
    for r in recs:
        assert r["flips"] <= r["candidates"] <= 32
        assert r["worst_l2"] <= GRAD_RTOL
    print("LOCKSTEP-CONTROL %s clean worst relative L2 %.3e (%s), candidates %s, flips %s" % (
        record.name, max(r["worst_l2"] for r in recs), max(recs, key=lambda r: r["worst_l2"])["worst_name"],
        [r["candidates"] for r in recs], [r["flips"] for r in recs]))
    # the adaptation path is exercised: some update offers a boundary candidate, and (PPO) rows cross a clip bound
    assert any(r["candidates"] > 0 for r in recs), "no boundary candidate offered by any update"
    if record.algo == "ppo":
        assert all(float(record.log[u][4]) > 0 for u in range(1, U)), [float(x[4]) for x in record.log]


def test_only_updates_replays_the_named_updates(record):
    recs = _check(record, record.snaps, record.log, [U - 1, 2])
    assert [r["update"] for r in recs] == [2, U - 1]
    with pytest.raises(AssertionError):
        _check(record, record.snaps, record.log, [U])


def _names(record):
    out = "actor.model.2.weight" if record.kwargs["discrete"] else "actor.mu.2.weight"
    assert out in record.rp.names and "representation.model.0.weight" in record.rp.names
    return out, "representation.model.0.weight"


UPDATES = [0, 1, U - 1]


@pytest.mark.parametrize("u", UPDATES)
@pytest.mark.parametrize("which", [0, 1])
def test_scale_grad_is_red(record, u, which):
    name = _names(record)[which]
    snaps, log = faults.scale_grad(record.snaps, record.log, u, record.rp.names, name, GRAD_RTOL)
    with pytest.raises(AssertionError, match=r"lockstep grad \(relative L2\)', %d, '%s'" % (u, name.replace(".", r"\."))):
        _check(record, snaps, log, [u])


@pytest.mark.parametrize("u", UPDATES)
def test_drop_rows_is_red(record, u):
    snap = record.snaps[u]
    cand = record.rp.candidate_rows(u, snap)
    snaps, log, k = faults.drop_rows(record.snaps, record.log, u, record.rp.row_oracle(u, snap), cand, GRAD_RTOL)
    print("LOCKSTEP-CONTROL %s drop_rows update %d: k = %d of B = %d" % (record.name, u, k, B))
    assert k <= B // 64
    with pytest.raises(AssertionError, match="lockstep grad"):
        _check(record, snaps, log, [u])


@pytest.mark.parametrize("u", [0, 1, U - 2])   # (u, u + 1) exchanged: the last pair ends at the last update
def test_swap_updates_is_red(record, u):
    snaps, log = faults.swap_updates(record.snaps, record.log, u)
    for v in (u, u + 1):
        with pytest.raises(AssertionError, match="lockstep"):
            _check(record, snaps, log, [v])


@pytest.mark.parametrize("u", [0, 1, U - 2])
def test_swap_logs_is_red(record, u):
    snaps, log = faults.swap_logs(record.snaps, record.log, u)
    for v in (u, u + 1):
        with pytest.raises(AssertionError, match=r"lockstep loss|'lockstep', '(actor-loss|critic-loss|entropy)'"):
            _check(record, snaps, log, [v])


@pytest.mark.parametrize("u", UPDATES)
@pytest.mark.parametrize("key", ["actor-loss", "critic-loss", "entropy"])
def test_bias_scalar_is_red(record, u, key):
    snaps, log = faults.bias_scalar(record.snaps, record.log, u, key, LOSS_TOL)
    with pytest.raises(AssertionError, match=r"'lockstep', '%s', %d" % (key, u)):
        _check(record, snaps, log, [u])


@pytest.mark.parametrize("u", UPDATES)
def test_wrong_branch_is_red(ppo_record, u):
    record = ppo_record   # the fault is PPO's min() branch
    snaps, log, row = faults.wrong_branch(record.snaps, record.log, u, record.rp.row_oracle(u, record.snaps[u]))
    assert row not in record.rp.candidate_rows(u, record.snaps[u])
    with pytest.raises(AssertionError, match="lockstep grad"):
        _check(record, snaps, log, [u])


def test_an_undecided_candidate_is_taken_and_nothing_else(record):
    """The adaptation itself: a device that took the other side of one boundary candidate (that candidate's gradient
    added to the device gradient) still passes, with that flip counted; the same gradient added twice — no side of an
    undecided row gives that — is red whenever one candidate alone is above the tolerance."""
    clean = _check(record, record.snaps, record.log, None)
    u = next(r["update"] for r in clean if r["candidates"] > 0)
    record.rp.candidate_rows(u, record.snaps[u])
    cand = [b.clone() for b in record.rp.lrn.boundary_grads[0]]
    snaps, log = faults.copy_record(record.snaps, record.log)
    for g, b in zip(snaps[u][1], cand):
        g.add_(b.to(g.dtype))
    rec = _check(record, snaps, log, [u])[0]
    assert rec["flips"] >= 1 and rec["worst_l2"] <= GRAD_RTOL
    rel = max(float(b.norm()) / (float(g.norm()) + 1e-30) for b, g in zip(cand, record.snaps[u][1]))
    print("LOCKSTEP-CONTROL %s candidate at update %d: %.3e of its tensor's gradient" % (record.name, u, rel))
    for g, b in zip(snaps[u][1], cand):
        g.add_(b.to(g.dtype))
    if rel > 2 * GRAD_RTOL:
        with pytest.raises(AssertionError, match="lockstep grad"):
            _check(record, snaps, log, [u])
