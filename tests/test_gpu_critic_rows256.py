"""GPU: K40H — the mask-writing critic head on the split GEMM's 256-row block with a register epilogue
(xpa_s3_head_critic_mask, csrc/sgemm3.hip), the production form of the "K16Q-mask" critic.

Checked at B = 77 (a partial block), 256 (one block), 300 (one block + 44 rows) and 4133 (16 blocks + 37 rows):
  * against float64 autograd of the critic (the reference of test_head_gemm_kernels_vs_fp64_autograd): dz_c rebuilt
    from mask / dv, the summed partials and the loss scalars, with canaries in and around every output — a partial
    row nobody wrote would break the sums;
  * against the K16Q kernel on the same inputs: the mask bits away from a kink, and dv / the summed partials within
    2x K16Q's own error against f64 (+ 2^-24 of the scale; the factor 2 for a different summation order);
  * two launches give the same bits;
  * form 0, and a non-NULL dz under form 1, run the K16Q kernel bit for bit;
  * one learner update under form 1 against form 0."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
H, PAD, SLOPE, VF = 256, 64, 0.01, 0.25
BATCHES = [77, 256, 300, 4133]


@pytest.fixture(scope="module", autouse=True)
def _setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


_CASES = {}


def _case(B):
    """Inputs and the float64 reference for batch B, built once and left unchanged."""
    if B in _CASES:
        return _CASES[B]
    g = torch.Generator(device=DEV).manual_seed(B + 1)
    R = B + 300
    x = torch.randn(B, H, device=DEV, generator=g)
    wh = torch.randn(H, H, device=DEV, generator=g) / 16
    bh = torch.randn(H, device=DEV, generator=g) * 0.1
    w = torch.randn(1, H, device=DEV, generator=g) / 16
    b = torch.randn(1, device=DEV, generator=g) * 0.1
    idx = torch.randperm(R, device=DEV, generator=g)[:B].contiguous()
    idx[B // 2] = -1           # invalid rows contribute nothing
    idx[B - 1] = R + 5
    ret = torch.randn(R, device=DEV, generator=g)
    d = lambda t: t.detach().double().cpu()   # noqa: E731
    z64 = d(x) @ d(wh).t() + d(bh)
    near = (z64.abs() < 1e-5).any(1)   # a pre-activation within rounding of the kink takes either branch -> invalid
    assert int(near.sum()) < 0.01 * B, int(near.sum())
    idx[near.to(DEV)] = -1
    idx_c = idx.cpu()
    valid = (idx_c >= 0) & (idx_c < R)
    rows = idx_c.clamp(0, R - 1)
    zc = z64.clone().requires_grad_(True)
    wc, bc = d(w).requires_grad_(True), d(b).requires_grad_(True)
    vv = (torch.nn.functional.leaky_relu(zc, SLOPE) @ wc.t() + bc)[:, 0]
    m = valid.double()
    critic = ((vv - d(ret)[rows]) ** 2 * m).sum() / B
    (VF * critic).backward()
    ref = dict(z=z64, dz=zc.grad, dw=wc.grad, dbo=bc.grad, dbh=zc.grad.sum(0), critic=critic.item(),
               vmean=(vv.detach() * m).sum().item() / B,
               dv=(VF * 2.0 * (vv.detach() - d(ret)[rows]) / B) * m)
    from xuanpolicy_amd import ops
    c = dict(B=B, R=R, x=x, wh=wh, bh=bh, w=w, b=b, idx=idx, ret=ret, planes=ops.s3_split(wh.t()), ref=ref)
    _CASES[B] = c
    return c


class _Out:
    """Every output of a critic launch with PAD canary floats on both sides, and canaries inside wherever the launch
    must write (loss_partials: columns 1 and 4; its other columns are the actor's and start — and must stay — zero)."""

    def __init__(self, B, with_dz=False):
        from xuanpolicy_amd import ops
        L = ops.lib()
        self.B = B
        self.G = G = int(L.xpa_head_fused_num_partials(B))
        self.W = W = int(L.xpa_loss_partial_width(6))
        can = lambda n, v=555.0: torch.full((n + 2 * PAD,), v, device=DEV)   # noqa: E731
        self.p_dw, self.p_dbh, self.p_dbo = can(G * H), can(G * H), can(G)
        self.lp = can(G * W)
        inner = self.lp[PAD:PAD + G * W].view(G, W)
        inner.zero_()
        inner[:, 1] = 555.0
        inner[:, 4] = 555.0
        self.mask = torch.full((B * 8 + 2 * PAD,), -7, dtype=torch.int32, device=DEV)
        self.dv = can(B, 333.0)
        self.dz = can(B * 2 * H, 777.0) if with_dz else None

    def launch(self, fn, c, poison=True):
        from xuanpolicy_amd import ops
        L, s, p = ops.lib(), ops._stream(), ops._p
        v = lambda t: p(t[PAD:])   # noqa: E731
        if poison:
            assert L.xpa_lds_poison(s) == 0
        dz = p(self.dz[PAD + H:]) if self.dz is not None else None   # the critic's half of the [B, 512] pair
        assert fn(1, c["B"], H, p(c["x"]), H, p(c["planes"]), p(c["bh"]), 2 * H, p(c["w"]), p(c["b"]), SLOPE,
                  p(c["idx"]), c["R"], p(c["ret"]), VF, dz, v(self.p_dw), v(self.p_dbh), v(self.p_dbo), v(self.lp), self.W,
                  s, v(self.mask), v(self.dv)) == 0
        torch.cuda.synchronize()
        return self

    def tensors(self):
        return [self.p_dw, self.p_dbh, self.p_dbo, self.lp, self.mask, self.dv] + ([self.dz] if self.dz is not None else [])

    def check_pads(self):
        for t, cv in ((self.p_dw, 555.0), (self.p_dbh, 555.0), (self.p_dbo, 555.0), (self.lp, 555.0), (self.mask, -7),
                      (self.dv, 333.0)):
            assert bool((t[:PAD] == cv).all()) and bool((t[-PAD:] == cv).all()), "written out of bounds"
        inner = self.lp[PAD:-PAD].view(self.G, self.W)
        other = [j for j in range(self.W) if j not in (1, 4)]
        assert bool((inner[:, other] == 0).all()), "the actor's loss-partial columns were touched"

    def bits(self):
        m = self.mask[PAD:-PAD].view(self.B, 8).cpu().numpy().view(np.uint32)
        m = (m[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
        return torch.from_numpy(m.reshape(self.B, H).astype(bool))

    def sums(self):
        """name -> f64 CPU tensor: dv and the partials summed over their G rows."""
        G = self.G
        f = lambda t, n: t[PAD:-PAD].view(G, n).double().sum(0).cpu()   # noqa: E731
        return dict(dv=self.dv[PAD:-PAD].double().cpu(), dw=f(self.p_dw, H).view(1, H), dbh=f(self.p_dbh, H),
                    dbo=f(self.p_dbo, 1))

    def scalars(self):
        from xuanpolicy_amd import ops
        L, s = ops.lib(), ops._stream()
        sc, dls = torch.zeros(ops.N_OUT, device=DEV), torch.zeros(6, device=DEV)
        assert L.xpa_policy_loss_finalize(0, 0, self.B, 6, ops._p(self.lp[PAD:]), self.G, VF, 0.0, ops._p(sc),
                                          ops._p(dls), s) == 0
        torch.cuda.synchronize()
        return sc.double().cpu()


def _form(form):
    from xuanpolicy_amd import ops
    return ops.lib().xpa_head_critic_form(form)


def _err(got, exp):
    return (got - exp).abs().max().item(), exp.abs().max().item()


@pytest.mark.parametrize("B", BATCHES)
def test_k40h_vs_fp64_autograd(B):
    from xuanpolicy_amd import ops
    c = _case(B)
    ref = c["ref"]
    prev = _form(1)
    try:
        o = _Out(B).launch(ops.lib().xpa_s3_head_critic_mask, c)
    finally:
        _form(prev)
    o.check_pads()
    s = o.sums()
    mbits = o.bits()
    wc = c["w"][0].double().cpu()
    one = torch.ones((), dtype=torch.float64)
    dz = s["dv"][:, None] * wc[None, :] * torch.where(mbits, one, SLOPE * one)
    for what, got, exp in (("dz critic", dz, ref["dz"]), ("dW_out", s["dw"], ref["dw"]), ("db_out", s["dbo"], ref["dbo"]),
                           ("db_hidden", s["dbh"], ref["dbh"])):
        err, scale = _err(got, exp)
        print(B, what, "err", err, "scale", scale)
        assert err <= 2e-5 * (scale + 1e-12) + 1e-9, (what, err, scale)
    sc = o.scalars()
    print(B, "critic loss", sc[1].item(), ref["critic"], "value mean", sc[5].item(), ref["vmean"])
    assert abs(sc[1].item() - ref["critic"]) < 1e-5 and abs(sc[3].item() - VF * ref["critic"]) < 1e-5
    assert abs(sc[5].item() - ref["vmean"]) < 1e-5


@pytest.mark.parametrize("B", BATCHES)
def test_k40h_vs_k16q(B):
    from xuanpolicy_amd import ops
    L = ops.lib()
    c = _case(B)
    ref = c["ref"]
    prev = _form(1)
    try:
        new = _Out(B).launch(L.xpa_s3_head_critic_mask, c)
    finally:
        _form(prev)
    old = _Out(B).launch(L.xpa_head_gemm_s3q_critic_mask, c)
    clear = ref["z"].abs() > 1e-4
    assert torch.equal(new.bits()[clear], old.bits()[clear])
    assert torch.equal(new.bits()[clear], (ref["z"] > 0)[clear])
    sn, so = new.sums(), old.sums()
    for k in ("dv", "dw", "dbh", "dbo"):
        exp = ref[k]
        e_new, scale = _err(sn[k], exp)
        e_old, _ = _err(so[k], exp)
        print(B, k, "K40H err", e_new, "K16Q err", e_old, "scale", scale)
        assert e_new <= 2 * e_old + 2.0 ** -24 * scale, (k, e_new, e_old, scale)


@pytest.mark.parametrize("B", BATCHES)
def test_k40h_is_deterministic(B):
    from xuanpolicy_amd import ops
    c = _case(B)
    prev = _form(1)
    try:
        a = _Out(B).launch(ops.lib().xpa_s3_head_critic_mask, c)
        b = _Out(B).launch(ops.lib().xpa_s3_head_critic_mask, c, poison=False)
    finally:
        _form(prev)
    for i, (t, u) in enumerate(zip(a.tensors(), b.tensors())):
        assert torch.equal(t, u), i


@pytest.mark.parametrize("B", BATCHES)
def test_dispatch_to_k16q(B):
    from xuanpolicy_amd import ops
    L = ops.lib()
    c = _case(B)
    prev = _form(0)
    try:
        assert _form(-1) == 0
        ref = _Out(B).launch(L.xpa_head_gemm_s3q_critic_mask, c)
        got = _Out(B).launch(L.xpa_s3_head_critic_mask, c)
        for i, (t, u) in enumerate(zip(ref.tensors(), got.tensors())):
            assert torch.equal(t, u), ("form 0", i)
        _form(1)
        assert _form(-1) == 1
        ref = _Out(B, with_dz=True).launch(L.xpa_head_gemm_s3q_critic_mask, c)
        got = _Out(B, with_dz=True).launch(L.xpa_s3_head_critic_mask, c)
        for i, (t, u) in enumerate(zip(ref.tensors(), got.tensors())):
            assert torch.equal(t, u), ("form 1 with dz", i)
        assert not torch.equal(ref.dz, torch.full_like(ref.dz, 777.0))
    finally:
        _form(prev)


def test_learner_k40h_matches_k16q():
    """One C2-shaped update through FusedActorCritic (the bench's nets, B = 8192, the default plan) with the critic head
    on K40H and on K16Q: every parameter gradient and the loss scalars agree within the f32 GEMM's error (the figures of
    test_learner_factored_critic_matches_unfactored)."""
    from xuanpolicy_amd.runner import build_synthbox_ppo
    agent = build_synthbox_ppo(n_envs=256, n_steps=32, obs_dim=17, act_dim=6, hidden=256, n_epoch=1, n_minibatch=1,
                               seed=9, device="cuda:0")
    agent.train(32)   # a buffer to sample from (and one update, which also compiles every path)
    torch.cuda.synchronize()
    fm = agent.learner._fused_mlp()
    assert fm is not None
    res = []
    prev = _form(-1)
    try:
        for form in (1, 0):
            _form(form)
            res.append(_one_update_grads(agent))
            assert fm.last_plan.heads == "K16Q-mask"
    finally:
        _form(prev)
    (ga, sa), (gb, sb) = res
    for i, (a_, b_) in enumerate(zip(ga, gb)):
        scale = b_.abs().max().item()
        err = (a_ - b_).abs().max().item()
        print("grad", i, "err", err, "scale", scale)
        assert err <= 2e-4 * scale + 1e-12, i
    assert np.allclose(sa, sb, rtol=1e-5, atol=1e-6), (sa, sb)


def _one_update_grads(agent):
    """Gradients of one update on a fixed minibatch (the learner's fused forward / backward, no optimizer step)."""
    from xuanpolicy_amd import ops
    from xuanpolicy_amd.fused_mlp import Rows
    lrn = agent.learner
    fm = lrn._fused_mlp()
    mem = agent.memory
    N, T = mem.n_envs, mem.n_size
    g = torch.Generator(device=DEV).manual_seed(1)
    idx = torch.randperm(N * T, device=DEV, generator=g)
    flat_obs = mem.observations.view(N * T, -1)
    adv, ret = mem.advantages.view(-1), mem.returns.view(-1)
    act = mem.actions.reshape(-1)
    old = mem.auxiliary_infos["old_logp"].view(-1)
    part = torch.empty((int(ops.lib().xpa_gather_num_partials(idx.numel())), 2), dtype=torch.float64, device=DEV)
    for p_ in lrn.policy.parameters():
        p_.grad.zero_()
    ctx = fm.forward_hidden(Rows(flat_obs, idx), adv=adv, adv_partials=part)
    sc = fm.loss_backward(ctx, "ppo", "gaussian", act, adv, ret, old_logp=old, idx=idx, adv_partials=part,
                          clip_range=0.2, vf_coef=0.25, ent_coef=0.0)
    torch.cuda.synchronize()
    return [p_.grad.detach().clone() for p_ in lrn.policy.parameters()], sc.cpu().numpy()
