"""Test helper: faults injected into a lockstep record (negative controls for tests/_oracle_replay.py).

A record is (snaps, update_log): snaps[u] = (weights, pre-clip gradient) of the device's update u, update_log[u] its
loss scalars in ops.OUT_KEYS order.  Every fault is a pure function on copies of the record and returns the perturbed
(snaps, update_log).  The faults are sized against the checker's own tolerances (grad_rtol, loss_tol), never against
what the device produced: a fault twice the tolerance must turn the check red, whatever the clean distance was.
The per-row gradients (drop_rows, wrong_branch) come from the oracle in f64 at snaps[u]'s weights, as the derivative of
the per-row loss terms divided by B (ppoclip_learner.py:24-65 / a2c_learner.py:19-50)."""
import copy

import numpy as np
import torch

SCALAR_INDEX = {"actor-loss": 0, "critic-loss": 1, "entropy": 2}   # ops.OUT_KEYS


def copy_record(snaps, update_log):
    """Host copies of a record (the device's record is left as it was)."""
    return ([([torch.as_tensor(w).detach().cpu().clone() for w in ws],
              [torch.as_tensor(g).detach().cpu().clone() for g in gs]) for ws, gs in snaps],
            [np.array(torch.as_tensor(x).detach().cpu().numpy(), copy=True) for x in update_log])


def scale_grad(snaps, update_log, u, names, name, grad_rtol=1e-3):
    """The device gradient of parameter `name` at update u times 1 + 2 grad_rtol."""
    snaps, update_log = copy_record(snaps, update_log)
    snaps[u][1][names.index(name)].mul_(1.0 + 2.0 * grad_rtol)
    return snaps, update_log


def swap_updates(snaps, update_log, u):
    """snaps[u] and snaps[u + 1] exchanged (the weights and gradient of another update)."""
    snaps, update_log = copy_record(snaps, update_log)
    snaps[u], snaps[u + 1] = snaps[u + 1], snaps[u]
    return snaps, update_log


def swap_logs(snaps, update_log, u):
    """update_log[u] and update_log[u + 1] exchanged (the loss scalars of another update)."""
    snaps, update_log = copy_record(snaps, update_log)
    update_log[u], update_log[u + 1] = update_log[u + 1], update_log[u]
    return snaps, update_log


def bias_scalar(snaps, update_log, u, key, loss_tol=1e-4):
    """2 loss_tol max(1, |x|) added to the loss scalar `key` (actor-loss, critic-loss or entropy) at update u."""
    snaps, update_log = copy_record(snaps, update_log)
    j = SCALAR_INDEX[key]
    x = float(update_log[u][j])
    update_log[u][j] = x + 2.0 * loss_tol * max(1.0, abs(x))
    return snaps, update_log


class RowOracle:
    """The f64 oracle of one update's per-row loss terms: policy (a copy of `pol` in f64 at `weights`), the minibatch
    `batch` = (obs, act, ret, adv, old_logp) and the loss coefficients.  terms[i] is row i's share of the loss (its
    actor, entropy and critic terms divided by B), so grad(rows) — the gradient of the sum of those rows' terms — is
    what the minibatch gradient loses when the rows are dropped."""

    def __init__(self, pol, weights, batch, algo, ent, vf_coef, clip_range):
        self.pol = copy.deepcopy(pol).double()
        self.params = list(self.pol.parameters())
        with torch.no_grad():
            for p, w in zip(self.params, weights):
                p.copy_(torch.as_tensor(w).cpu().double())
        o, a, r, ad, old_logp = batch
        if not (isinstance(o, np.ndarray) and o.dtype == np.uint8):   # raw frames: the policy scales them
            o = torch.as_tensor(np.asarray(o, np.float32)).double()
        head, logstd, v = self.pol.heads(o)
        d = self.pol.dist(head, logstd)
        a = torch.as_tensor(a)
        if self.pol.discrete:
            logp, en = d.log_prob(a), d.entropy()
        else:
            logp, en = d.log_prob(a).sum(-1), d.entropy().sum(-1)
        self.B = B = logp.shape[0]
        self.adv = adv = torch.as_tensor(np.asarray(ad, np.float64))
        ret = torch.as_tensor(np.asarray(r, np.float64))
        self.lo, self.hi = 1.0 - clip_range, 1.0 + clip_range
        if algo == "ppo":
            self.ratio = (logp - torch.as_tensor(np.asarray(old_logp, np.float64))).exp()
            actor = -torch.minimum(self.ratio.clamp(self.lo, self.hi) * adv, adv * self.ratio)
        else:
            self.ratio = None
            actor = -(adv * logp)
        self.terms = (actor - ent * en + vf_coef * (v - ret) ** 2) / B

    def _grad(self, y):
        g = torch.autograd.grad(y, self.params, retain_graph=True, allow_unused=True)
        return [torch.zeros_like(p) if x is None else x.detach() for p, x in zip(self.params, g)]

    def grad(self, rows=None):
        """The gradient of the listed rows' loss terms (None: all rows — the minibatch gradient)."""
        return self._grad(self.terms.sum() if rows is None else self.terms[list(rows)].sum())

    def unclipped_grad(self, i):
        """Row i's unclipped PPO gradient, d(-A_i ratio_i / B) / d theta."""
        return self._grad(-(self.adv[i] * self.ratio[i]) / self.B)


def drop_rows_k(oracle, candidate_rows, grad_rtol=1e-3):
    """(k, rows, dropped gradient): the first k minibatch rows that are no boundary candidates, k the smallest power of
    two for which their gradient alone exceeds 2 grad_rtol of the oracle gradient's norm on at least one tensor.  The
    oracle alone decides k; k <= B / 64, or the check cannot see dropped rows at this batch size (an assertion: a
    finding, not a skip)."""
    full = [float(g.norm()) for g in oracle.grad()]
    cand = set(int(i) for i in candidate_rows)
    free = [i for i in range(oracle.B) if i not in cand]
    k, seen = 1, []
    while k <= oracle.B // 64:
        rows = free[:k]
        g = oracle.grad(rows)
        rel = max(float(x.norm()) / (n + 1e-300) for x, n in zip(g, full) if n > 0)
        seen.append((k, rel))
        if rel > 2.0 * grad_rtol:
            return k, rows, g
        k *= 2
    raise AssertionError("the lockstep check cannot see dropped rows at B = %d: (k, largest relative gradient) %s, "
                         "needed > %g with k <= B / 64" % (oracle.B, seen, 2.0 * grad_rtol))


def drop_rows(snaps, update_log, u, oracle, candidate_rows, grad_rtol=1e-3):
    """The device gradient at update u without the contribution of k minibatch rows (drop_rows_k).  Returns
    (snaps, update_log, k)."""
    snaps, update_log = copy_record(snaps, update_log)
    k, _, g = drop_rows_k(oracle, candidate_rows, grad_rtol)
    for gd, x in zip(snaps[u][1], g):
        gd.sub_(x.to(gd.dtype))
    return snaps, update_log, k


def wrong_branch(snaps, update_log, u, oracle, window=2e-4):
    """PPO: the row nearest the clip bound that decides its min() branch (1 + clip for a positive advantage, 1 - clip for
    a negative one) but outside the undecided window takes the other branch: its unclipped gradient is removed from the
    device gradient where the row is unclipped, added where it is clipped.  Returns (snaps, update_log, row)."""
    snaps, update_log = copy_record(snaps, update_log)
    ratio, adv = oracle.ratio.detach(), oracle.adv
    bound = torch.where(adv > 0, torch.full_like(ratio, oracle.hi), torch.full_like(ratio, oracle.lo))
    dist = (ratio - bound).abs() / bound
    dist = torch.where((dist < window) | (adv == 0), torch.full_like(dist, float("inf")), dist)
    i = int(dist.argmin())
    assert np.isfinite(float(dist[i]))
    unclipped = bool(ratio[i] < oracle.hi) if float(adv[i]) > 0 else bool(ratio[i] > oracle.lo)
    sgn = -1.0 if unclipped else 1.0
    for gd, x in zip(snaps[u][1], oracle.unclipped_grad(i)):
        gd.add_((sgn * x).to(gd.dtype))
    return snaps, update_log, i
