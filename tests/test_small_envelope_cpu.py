"""CPU: the checker of tests/test_gpu_small_envelope.py checked (tests/_small_ref.py).

A stand-in for the one-launch update (K30) — f32 CPU autograd of the same loss with the minibatch rows in reverse
order, which is another summation order — passes within_f32 against the f64 reference with the in-order f32 run as the
baseline; the same stand-in checked against references that are deliberately wrong is rejected, each in at least one
tensor.  The same for the clip-and-Adam tail.  And the GPU file's table of shapes takes the LDS layouts it claims."""
import copy

import pytest
import torch

from tests import _small_ref as sr

# (d_in, k, h0, h1, h2), dist, algo
SHAPES = {"cat": ((5, 3, 64, 32, 96), "categorical", "ppo"), "gauss": ((3, 1, 64, 32, 96), "gaussian", "ppo"),
          "cat-a2c": ((5, 3, 64, 32, 96), "categorical", "a2c")}
BATCH = 33


def _case(name):
    """(f64 policy with random biases, the minibatch) of one shape; the old log-probs are the policy's own plus
    0.15-sigma jitter."""
    (d_in, k, h0, h1, h2), dist, algo = SHAPES[name]
    torch.manual_seed(7 + d_in)
    pol = sr.build_f64_policy(d_in, k, h0, h1, h2, dist == "categorical", "LeakyReLU")
    # rows seed 4: the first from 3 up at which, for both shapes, some of the 33 ratios fall between the clip bounds of
    # 0.2 and 0.3 on the side their advantage makes active (at 3 the Categorical shape has none, and a clip range of
    # 0.3 is then the same loss)
    gen = torch.Generator().manual_seed(4)
    assert len(sr.randomise_biases(pol, gen)) == (5 if dist == "categorical" else 6)
    obs = torch.randn((BATCH, d_in), generator=gen)
    adv, ret = torch.randn((BATCH,), generator=gen), torch.randn((BATCH,), generator=gen)
    with torch.no_grad():
        head, logstd, _ = pol.heads(obs.double())
        if dist == "categorical":
            act = torch.randint(0, k, (BATCH,), generator=gen)
            logp = torch.log_softmax(head, -1).gather(1, act[:, None])[:, 0]
            act = act.float()
        else:
            act = (head + logstd.exp() * torch.randn((BATCH, k), generator=gen).double()).float()
            logp = torch.distributions.Normal(head, logstd.exp()).log_prob(act.double()).sum(-1)
        old = (logp + 0.15 * torch.randn((BATCH,), generator=gen).double()).float()
    return pol, algo, dist, (obs, act, adv, ret, old)


def _runs(name):
    """(stand-in gradients, baseline gradients, stand-in scalars) of one shape: both f32 CPU autograd."""
    pol, algo, dist, rows = _case(name)
    base, _ = sr.f32_baseline(pol, algo, dist, *rows, sr.HP)
    got, sc = sr.f32_baseline(pol, algo, dist, *(x.flip(0) for x in rows), sr.HP)
    return got, base, sc


def _layer(pol, name):
    """(weight-bearing Linear modules by the kernel's names) of the oracle module."""
    act = pol.actor.model if pol.discrete else pol.actor.mu
    return {"l0": pol.representation.model[0], "l1": act[0], "la": act[2], "l2": pol.critic.model[0],
            "lc": pol.critic.model[2]}[name]


def _b2_zeroed(pol, rows, hp):
    with torch.no_grad():
        _layer(pol, "l2").bias.zero_()
    return {}


def _b1_b2_swapped(pol, rows, hp):
    """b1 and b2 taken from each other: truncated or tiled to the other's length."""
    b1, b2 = _layer(pol, "l1").bias, _layer(pol, "l2").bias
    with torch.no_grad():
        old1, old2 = b1.clone(), b2.clone()
        b1.copy_(old2.repeat(-(-b1.numel() // old2.numel()))[:b1.numel()])
        b2.copy_(old1.repeat(-(-b2.numel() // old1.numel()))[:b2.numel()])
    return {}


def _slope_002(pol, rows, hp):
    n = 0
    for m in pol.modules():
        if isinstance(m, torch.nn.LeakyReLU):
            m.negative_slope, n = 0.02, n + 1
    assert n == 3
    return {}


def _last_row_left_out(pol, rows, hp):
    rows[:] = [x[:-1] for x in rows]
    return {}


def _sample_std(pol, rows, hp):
    return dict(sample_std=True)


def _clip_03(pol, rows, hp):
    hp["clip_range"] = 0.3
    return {}


WRONG = {"b2-zeroed": _b2_zeroed, "b1-b2-swapped": _b1_b2_swapped, "slope-0.02": _slope_002,
         "last-row-left-out": _last_row_left_out, "sample-std": _sample_std, "clip-range-0.3": _clip_03}


def wrong_reference(kind, pol, algo, dist, rows, hp):
    """The reference side with one deliberate mistake: (f64 gradients, its f32 baseline's gradients).  Both, because
    E32 is the distance between the two: a baseline of the TRUE loss beside a wrong f64 reference would put the defect
    itself into E32 and the bound would admit anything.  With both from the same wrong loss E32 stays f32 roundoff, and
    the question the control asks is the one the GPU test asks: does a kernel that differs from the reference side by
    this defect pass?  pol is not modified."""
    pol, rows, hp = copy.deepcopy(pol), list(rows), dict(hp)
    kw = WRONG[kind](pol, rows, hp)
    ref, _ = sr.small_update_ref(pol, algo, dist, *rows, hp, **kw)
    base, _ = sr.f32_baseline(pol, algo, dist, *rows, hp, **kw)
    return ref, base


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_the_stand_in_passes_the_bound(name):
    pol, algo, dist, rows = _case(name)
    got, base, sc = _runs(name)
    ref, sc64 = sr.small_update_ref(pol, algo, dist, *rows, sr.HP)
    assert all(float(r.abs().max()) > 0 for r in ref)
    res = sr.within_f32(got, base, ref)
    print("%s: worst |err| / E32 %.3g (E32 %.3g, scale %.3g)" % (name, res.ratio, res.e32, res.scale))
    assert res.ok, res
    if algo == "ppo":
        assert 0 < float(sc64[4]) < 1   # some ratios leave the clip range, some do not
    torch.testing.assert_close(sc.double(), sc64, rtol=1e-4, atol=1e-5)
    # the bound is not vacuous: the baseline's error is f32 roundoff of the gradient's scale
    assert 0 < res.e32 < 1e-5 * res.scale


@pytest.mark.parametrize("kind", sorted(WRONG))
@pytest.mark.parametrize("name", ["cat", "gauss"])
def test_a_wrong_reference_is_rejected(name, kind):
    pol, algo, dist, rows = _case(name)
    got, true_base, _ = _runs(name)
    before = [p.detach().clone() for p in pol.parameters()]
    ref, base = wrong_reference(kind, pol, algo, dist, rows, sr.HP)
    assert all(torch.equal(a, b) for a, b in zip(before, pol.parameters()))
    res = sr.within_f32(got, base, ref)
    print("%s / %s: rejected in tensors %s, worst |err| / E32 %.3g" % (name, kind, res.bad, res.ratio))
    assert not res.ok and len(res.bad) >= 1
    # by a wide margin, as the defects the bound is for are: not a near miss of the margin
    true_ref, _ = sr.small_update_ref(pol, algo, dist, *rows, sr.HP)
    assert res.ratio > 100 * sr.within_f32(got, true_base, true_ref).ratio


def test_a_non_finite_gradient_is_rejected():
    pol, algo, dist, rows = _case("cat")
    got, base, _ = _runs("cat")
    ref, _ = sr.small_update_ref(pol, algo, dist, *rows, sr.HP)
    got = [g.clone() for g in got]
    got[3][0] = float("nan")
    res = sr.within_f32(got, base, ref)
    assert not res.ok and res.bad == [3]


# ---- the tail ---------------------------------------------------------------------------------------------------------
TAIL_SHAPES = [(64, 5), (64,), (32, 64), (32,), (3, 32), (3,), (96, 64), (96,), (1, 96), (1,)]
TAIL_LRS = (1e-3, 9.5e-4)


def _tail_inputs():
    """f32 parameters of the (5, 3, 64, 32, 96) shape and two updates' random gradients, of norm > 0.5."""
    gen = torch.Generator().manual_seed(5)
    p32 = [torch.randn(s, generator=gen) * 0.3 for s in TAIL_SHAPES]
    grads = [[torch.randn(s, generator=gen) * 0.05 for s in TAIL_SHAPES] for _ in range(2)]
    return p32, grads


def _tail_stand_in(max_norm):
    """Two chained updates through clip_adam_ref in f32 (its own operation order): per update (steps, exp_avg,
    exp_avg_sq, norm)."""
    p, grads = _tail_inputs()
    m, v = [torch.zeros(s) for s in TAIL_SHAPES], [torch.zeros(s) for s in TAIL_SHAPES]
    out = []
    for u in range(2):
        p1, m, v, norm = sr.clip_adam_ref(p, grads[u], m, v, u + 1, TAIL_LRS[u], max_norm)
        out.append(([a - b for a, b in zip(p1, p)], m, v, norm))
        p = p1
    return out


def _tail_reference_side(max_norm, eps=1e-5, coef_twice=False):
    """(the chained f64 reference, its chained f32 baseline), per update (steps, exp_avg, exp_avg_sq[, norm]).  The
    baseline is torch's own f32 clip_grad_norm_ + Adam.  eps / coef_twice: the deliberate mistakes, made on both (see
    wrong_reference)."""
    p32, grads = _tail_inputs()
    params = [torch.nn.Parameter(p.clone()) for p in p32]
    opt = torch.optim.Adam(params, lr=TAIL_LRS[0], eps=eps)
    p = [x.double() for x in p32]
    m, v = [torch.zeros_like(x) for x in p], [torch.zeros_like(x) for x in p]
    refs, bases = [], []
    for u in range(2):
        for q, g in zip(params, grads[u]):
            q.grad = g.clone()
        before = [q.detach().clone() for q in params]
        if max_norm >= 0:
            norm = torch.nn.utils.clip_grad_norm_(params, max_norm)
            if coef_twice:
                for q in params:
                    q.grad.mul_(torch.clamp(max_norm / (norm + 1e-6), max=1.0))
        opt.param_groups[0]["lr"] = TAIL_LRS[u]
        opt.step()
        bases.append(([q.detach() - b for q, b in zip(params, before)], [opt.state[q]["exp_avg"].clone() for q in params],
                      [opt.state[q]["exp_avg_sq"].clone() for q in params]))
        p1, m, v, norm64 = sr.clip_adam_ref(p, [g.double() for g in grads[u]], m, v, u + 1, TAIL_LRS[u], max_norm,
                                            eps=eps, coef_twice=coef_twice)
        refs.append(([a - b for a, b in zip(p1, p)], m, v, norm64))
        p = p1
    return refs, bases


def _tail_ok(got, refs, bases):
    """Per update: the three sets (steps, exp_avg, exp_avg_sq) against the bound; the steps with one extra
    2^-24 max |p| in the floor for the stored parameter's rounding."""
    pmax = max(float(x.abs().max()) for x in _tail_inputs()[0])
    return [[sr.within_f32(g[i], b[i], r[i], extra_floor=2.0 ** -24 * pmax if i == 0 else 0.0) for i in range(3)]
            for g, r, b in zip(got, refs, bases)]


@pytest.mark.parametrize("max_norm", [0.5, -1.0])
def test_the_tail_stand_in_passes_and_wrong_tails_are_rejected(max_norm):
    got = _tail_stand_in(max_norm)
    refs, bases = _tail_reference_side(max_norm)
    assert float(refs[0][3]) > 0.5
    for u, res in enumerate(_tail_ok(got, refs, bases)):
        print("max_norm %g update %d: worst |err| / E32 step %.3g exp_avg %.3g exp_avg_sq %.3g"
              % (max_norm, u, res[0].ratio, res[1].ratio, res[2].ratio))
        assert all(r.ok for r in res), res
        torch.testing.assert_close(got[u][3].double(), refs[u][3], rtol=1e-5, atol=0)
    wrong = _tail_ok(got, *_tail_reference_side(max_norm, eps=1e-8))
    assert not wrong[0][0].ok and not wrong[1][0].ok   # eps enters the step ...
    assert wrong[0][1].ok and wrong[0][2].ok           # ... not the first update's moments
    twice = _tail_ok(got, *_tail_reference_side(max_norm, coef_twice=True))
    if max_norm >= 0:   # the coefficient is < 1: both moments move, and the step through eps
        assert not twice[0][1].ok and not twice[0][2].ok and not twice[1][0].ok
    else:               # no clipping: there is no coefficient
        assert all(r.ok for res in twice for r in res)


# ---- the table of shapes ----------------------------------------------------------------------------------------------
LDS_BUDGET = 40704


def lds_floats(batch, d_in, h0, h1, h2, k):
    """xpa_small_mlp_lds_floats restated (csrc/smallmlp.hip)."""
    BP = (batch + 31) & ~31
    S, DP, KP = BP + 4, (d_in + 3) & ~3, (k + 3) & ~3
    return (DP * S + (h0 + h1 + h2) * S + KP * S + 4 * S + DP * h0 + h0 * (h1 + 1) + h0 * (h2 + 1) + h1 * KP + h2 + h0
            + h1 + h2 + KP + 4 + 4 * BP + BP * KP + BP)


def one_image_lds_floats(batch, d_in, h0, h1, h2, k):
    return lds_floats(batch, d_in, h0, h1, h2, k) - h0 * (min(h1, h2) + 1)


def layout(rows, dims, fns=(lds_floats, one_image_lds_floats)):
    """"R" (resident), "O" (one image) or None (refused) for `rows` rows per workgroup: small_update_ok's rule and
    sm_args_ok's."""
    if fns[0](rows, *dims) <= LDS_BUDGET:
        return "R"
    return "O" if rows <= 32 and fns[1](rows, *dims) <= LDS_BUDGET else None


# (d_in, k, h0, h1, h2) -> (layout at <= 32 rows, resident floats at 32 rows, one-image floats at 32 rows or None)
TABLE = {(4, 2, 32, 64, 32): ("R", 9016, None), (5, 3, 64, 32, 96): ("R", 17032, None),
         (32, 16, 96, 64, 32): ("R", 23204, None), (13, 5, 32, 256, 32): ("R", 25148, None),
         (13, 5, 32, 32, 256): ("R", 23580, None), (1, 2, 256, 32, 32): ("R", 30648, None),
         (13, 5, 128, 64, 128): ("O", 40796, 32476), (32, 16, 160, 96, 32): ("O", 40708, 35428),
         (5, 3, 96, 128, 160): ("O", 44360, 31976), (3, 1, 64, 32, 96): ("R", 16632, None),
         (17, 6, 96, 128, 160): ("O", 46732, 34348), (32, 16, 256, 64, 32): (None, None, 41476)}
UNSPLIT = ((4, 2, 32, 64, 32), (5, 3, 64, 32, 96), (3, 1, 64, 32, 96))   # also run as ONE workgroup of 64 / 70 rows


def _library_fns():
    try:
        from xuanpolicy_amd import ops
        lib = ops.lib()
        return (lambda *a: int(lib.xpa_small_mlp_lds_floats(*a)),
                lambda *a: int(lib.xpa_small_mlp_one_image_lds_floats(*a)))
    except (ImportError, OSError, AttributeError):
        return None


def test_the_table_of_shapes_takes_the_layouts_it_claims():
    """d_in, k, h0, h1, h2 as (dims order of the C entry: d_in, h0, h1, h2, k).  Against the library's two functions
    when it loads without a device, and against the formula restated above either way."""
    fn_sets = [(lds_floats, one_image_lds_floats)]
    lib = _library_fns()
    if lib is not None:
        fn_sets.append(lib)
    for fns in fn_sets:
        for (d_in, k, h0, h1, h2), (lay, res, one) in TABLE.items():
            dims = (d_in, h0, h1, h2, k)
            for rows in (1, 31, 32):
                assert layout(rows, dims, fns) == lay, (dims, rows)
            if res is not None:
                assert fns[0](32, *dims) == res and (res <= LDS_BUDGET) == (lay == "R"), dims
            if one is not None:
                assert fns[1](32, *dims) == one and fns[0](32, *dims) > LDS_BUDGET, dims
                assert (one <= LDS_BUDGET) == (lay == "O"), dims
        for d_in, k, h0, h1, h2 in UNSPLIT:   # one workgroup of two or three 32-row tiles, resident
            for rows in (64, 70):
                assert layout(rows, (d_in, h0, h1, h2, k), fns) == "R"
        assert layout(513, (13, 128, 64, 128, 5), fns) is None   # past 512 rows the split form is off
        # (32, 16, 160, 96, 32) is one-image by 4 floats
        assert fns[0](32, 32, 160, 96, 32, 16) - LDS_BUDGET == 4
