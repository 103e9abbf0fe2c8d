"""Test helper (torch only, no device needed): the f64 reference of one small-path minibatch update, the f64 reference of
its clip-and-Adam tail, and the bound the one-launch update (K30) is held to against them.

  * small_update_ref: the reference learner's loss (ppoclip_learner.py:24-46 / a2c_learner.py:19-37) on advantages
    normalised as memory_tools.py:241-242 does — (adv - mean) / (population std + 1e-8) — with Categorical or
    DiagGaussian log-prob and entropy, differentiated by autograd.  tests/test_gpu_pendulum.py's _f64_gradients for
    both heads.  The same code in f32 (a policy that was not .double()d) is the f32 baseline.
  * clip_adam_ref: clip_grad_norm_ (coef = min(1, max_norm / (norm + 1e-6))) and torch.optim.Adam's update, in the
    dtype of its inputs.
  * within_f32: the project's GEMM convention (tests/test_gpu_sgemm3.py: error <= a multiple of the f32 baseline's
    error + a 2^-24 floor), pooled over a set of tensors so that a one-element tensor cannot make the baseline's error
    vanish:  E32 = max |base32 - ref64| and scale = max |ref64| over every element of every tensor of the set; every
    element of got must satisfy |got - ref64| <= MARGIN * E32 + 2^-24 * scale.

MARGIN is 4, not the GEMM test's 2: K30 is five chained products plus expf / logf / tanhf, the baseline has the same
chain lengths in another summation order, and two such roundoff draws over a few thousand elements differ by up to ~2x.
The defects the bound is for (a wrong stride, a wrong bias, a dropped or duplicated row, a wrong activation derivative)
move a gradient by a fraction of its own scale: 10^3 times the bound or more.  The factor is reasoned, not measured;
the tests print the worst |err| / E32 they see (tests/test_gpu_small_envelope.py's docstring records them)."""
import collections
import copy

import torch

OUT_KEYS = ("actor-loss", "critic-loss", "entropy", "loss", "clip_ratio", "predict_value")   # ops.OUT_KEYS
MARGIN = 4.0
HP = dict(clip_range=0.2, vf_coef=0.25, ent_coef=0.01)


def build_f64_policy(d_in, k, h0, h1, h2, discrete, activation, src=None):
    """oracle/cpu_ref.py's actor-critic of one layer per part, in f64 on the CPU; src: an agent (its parameters are
    loaded in state_dict order) or None (the module's own initial weights)."""
    from oracle import cpu_ref
    pol = cpu_ref.build_actor_critic_ref(d_in, k, [h0], [h1], [h2], discrete=discrete, activation=activation)
    if src is not None:
        from tests._oracle_replay import _load_by_order
        _load_by_order(pol, src)
    return pol.double()


def randomise_biases(policy, gen=None):
    """Every bias of `policy` overwritten in place with uniform(-0.5, 0.5), a Gaussian head's logstd with
    uniform(-1, 0.3): a fresh policy's biases are all 0, which hides a dropped or misplaced bias.  Returns the names."""
    names = []
    with torch.no_grad():
        for n, p in policy.named_parameters():
            if n.endswith("bias"):
                p.uniform_(-0.5, 0.5, generator=gen)
            elif n.endswith("logstd"):
                p.uniform_(-1.0, 0.3, generator=gen)
            else:
                continue
            assert float(p.abs().min()) > 0, n
            names.append(n)
    return names


def _heads(policy, obs):
    if hasattr(policy, "heads"):
        return policy.heads(obs)
    from xuanpolicy_amd.policies import policy_heads
    return policy_heads(policy, obs)


def small_loss(policy, algo, dist, obs, act, adv, ret, old_logp, hp, sample_std=False):
    """The loss and the six OUT_KEYS scalars (tensors) in the dtype and on the device of policy's parameters.
    sample_std: the (n - 1) standard deviation in the advantage normalisation (a negative control)."""
    p0 = next(policy.parameters())
    obs, adv, ret = (x.detach().to(p0.device, p0.dtype) for x in (obs, adv, ret))
    head, logstd, v = _heads(policy, obs)
    v = v.reshape(-1)
    if dist == "categorical":
        logp_all = torch.log_softmax(head, -1)
        a = act.detach().to(p0.device).long().reshape(-1, 1)
        logp = logp_all.gather(1, a)[:, 0]
        ent = -(logp_all.exp() * logp_all).sum(-1)
    else:
        d = torch.distributions.Normal(head, logstd.exp())
        logp = d.log_prob(act.detach().to(p0.device, p0.dtype).reshape(head.shape)).sum(-1)
        ent = d.entropy().sum(-1)
    n = adv.shape[0]
    mean = adv.mean()
    var = ((adv - mean) ** 2).sum() / (n - 1 if sample_std else n)
    a_n = (adv - mean) / (var.sqrt() + 1e-8)
    if algo == "ppo":
        ratio = (logp - old_logp.detach().to(p0.device, p0.dtype)).exp()
        lo, hi = 1.0 - hp["clip_range"], 1.0 + hp["clip_range"]
        a_loss = -torch.minimum(ratio.clamp(lo, hi) * a_n, ratio * a_n).mean()
        clip = ((ratio < lo) | (ratio > hi)).to(p0.dtype).mean()
    else:
        a_loss = -(a_n * logp).mean()
        clip = torch.zeros((), dtype=p0.dtype, device=p0.device)
    c_loss = ((v - ret) ** 2).mean()
    e = ent.mean()
    loss = a_loss - hp["ent_coef"] * e + hp["vf_coef"] * c_loss
    return loss, torch.stack([a_loss, c_loss, e, loss, clip, v.mean()]).detach()


def small_update_grads(policy, algo, dist, obs, act, adv, ret, old_logp, hp, **kw):
    """([every parameter's gradient, in the module's parameter order], the six scalars) in policy's dtype."""
    loss, scalars = small_loss(policy, algo, dist, obs, act, adv, ret, old_logp, hp, **kw)
    params = list(policy.parameters())
    grads = torch.autograd.grad(loss, params, allow_unused=True)
    return [torch.zeros_like(p) if g is None else g.detach() for p, g in zip(params, grads)], scalars


def small_update_ref(policy_f64, algo, dist, obs, act, adv, ret, old_logp, hp, **kw):
    """The f64 reference: policy_f64 is an f64 module on the CPU; the inputs may live anywhere."""
    assert next(policy_f64.parameters()).dtype == torch.float64
    cpu = lambda x: None if x is None else x.detach().cpu()   # noqa: E731
    return small_update_grads(policy_f64, algo, dist, cpu(obs), cpu(act), cpu(adv), cpu(ret), cpu(old_logp), hp, **kw)


def f32_baseline(policy, *args, **kw):
    """torch's own f32 autograd of the same loss on a DEEP COPY of policy (an agent's .grad tensors are views of the
    flat buffer the kernel under test writes), on policy's device."""
    pol = copy.deepcopy(policy).float()
    return small_update_grads(pol, *args, **kw)


def clip_adam_ref(params, grads, m, v, step, lr, max_norm, betas=(0.9, 0.999), eps=1e-5, coef_twice=False):
    """clip_grad_norm_ (max_norm < 0: no clipping) then Adam's update number `step` (1-based), in the inputs' dtype.
    Returns (new parameters, new exp_avg, new exp_avg_sq, the pre-clip norm).  coef_twice: the clip coefficient
    applied twice (a negative control)."""
    b1, b2 = betas
    norm = torch.sqrt(sum((g * g).sum() for g in grads))
    coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0) if max_norm >= 0 else torch.ones_like(norm)
    if coef_twice:
        coef = coef * coef
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    P, M, V = [], [], []
    for p, g, m0, v0 in zip(params, grads, m, v):
        g = g * coef
        m1 = b1 * m0 + (1.0 - b1) * g
        v1 = b2 * v0 + (1.0 - b2) * g * g
        denom = v1.sqrt() / (bc2 ** 0.5) + eps
        P.append(p - (lr / bc1) * m1 / denom)
        M.append(m1)
        V.append(v1)
    return P, M, V, norm


Bound = collections.namedtuple("Bound", "ok ratio e32 scale worst bad")


def within_f32(got, base32, ref64, margin=MARGIN, extra_floor=0.0):
    """got, base32, ref64: lists of tensors of one set.  ok: every element of got within margin * E32 + 2^-24 * scale
    (+ extra_floor) of ref64; ratio: the worst |got - ref64| / E32; worst: the index of the tensor holding it; bad: the
    indices of the tensors with an element out of bound."""
    assert len(got) == len(base32) == len(ref64) and len(got) > 0
    f = lambda t: t.detach().cpu().double()   # noqa: E731
    got, base32, ref64 = [f(t) for t in got], [f(t) for t in base32], [f(t) for t in ref64]
    for g, b, r in zip(got, base32, ref64):
        assert g.shape == b.shape == r.shape, (g.shape, b.shape, r.shape)
    e32 = max(float((b - r).abs().max()) for b, r in zip(base32, ref64))
    scale = max(float(r.abs().max()) for r in ref64)
    tol = margin * e32 + 2.0 ** -24 * scale + extra_floor
    errs = [float((g - r).abs().max()) if torch.isfinite(g).all() else float("inf") for g, r in zip(got, ref64)]
    worst = max(range(len(errs)), key=errs.__getitem__)
    bad = [i for i, e in enumerate(errs) if not e <= tol]
    return Bound(not bad, errs[worst] / max(e32, 1e-300), e32, scale, worst, bad)
