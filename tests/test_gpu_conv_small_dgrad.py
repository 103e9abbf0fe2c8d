"""GPU: K28R-D (xpa_conv_wsplit_t + xpa_conv_dgrad_small) against the float64 autograd input gradient of F.conv2d times
act'(y_prev), and its column sums (test_gpu_igemm.py::test_conv_dgrad_matches_f64's reference and bounds).  dz, dx and
the partials are 16-byte aligned views into one NaN-filled allocation; every byte outside dx and the partials stays."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _planes_t(L, w):
    from xuanpolicy_amd import _lib, ops
    cout, cin, k = w.shape[:3]
    pl = torch.empty(int(L.xpa_conv_wsplit_t_bytes(cin, cout, k)), dtype=torch.uint8, device=DEV)
    _lib.call(L.xpa_conv_wsplit_t, ops._p(w), cin, cout, k, ops._p(pl), ops._stream(DEV))
    return pl


def _dgrad(L, fn, dz, wp, cin, k, s, p, H, W, act, yp, slope, dx=None, part=None):   # fn: K28R-D (wp: planes) or K28
    from xuanpolicy_amd import _lib, ops
    B, OH, OW, cout = dz.shape
    if dx is None:
        dx = torch.full((B, H, W, cin), float("nan"), device=DEV)
    _lib.call(fn, ops._p(dz), B, OH, OW, cout, ops._p(wp), cin, k, s, p, H, W, act,
              ops._p(yp) if yp is not None else None, slope, ops._p(dx), ops._p(part) if part is not None else None,
              ops._stream(DEV))
    return dx


# (in_c, out_c, B, H, W, k, s, p, act_prev, slope, partials): every (out_c 16 / 32 / 64, NT 1 / 2, act' code) instance;
# in_c 5 / 32 / 40 / 64 (padded columns on both NT); k 1 s 1, k 3 s 1 p 1, k 4 s 2 p 1, k 3 s 2 p 1 (classes of 4 / 2 /
# 2 / 1 taps), k 1 s 2 (three empty classes), p 0, p > k / 2 at both strides; H != W; k 3 s 2 p 0 on 8 x 6 (input row 7
# and column 5 reached by no output); class rows below one tile, exactly 128 (2 x 8 x 8; stride 2: 2 x 16 x 16), several
# tiles with a ragged last one (900; 600 / 450 / 480 / 360); act_prev -1, 0, 1 (slope 0, 0.01), 2; with / without partials
CASES = [(5, 16, 2, 7, 5, 1, 1, 0, -1, 0.0, False), (32, 16, 2, 8, 8, 3, 1, 1, 1, 0.0, True),
         (5, 16, 3, 8, 6, 3, 2, 0, 2, 0.0, True), (40, 16, 30, 9, 7, 4, 2, 1, 1, 0.01, True),
         (64, 16, 2, 7, 6, 3, 1, 0, 2, 0.0, True), (40, 16, 2, 7, 5, 1, 2, 0, 0, 0.0, True),
         (5, 32, 5, 5, 3, 3, 1, 2, 1, 0.01, False), (32, 32, 3, 6, 3, 3, 2, 1, 0, 0.0, True),
         (32, 32, 2, 16, 16, 4, 2, 1, 2, 0.0, True), (40, 32, 2, 8, 8, 3, 1, 1, 2, 0.0, False),
         (64, 32, 30, 9, 7, 4, 2, 1, 1, 0.0, True), (64, 32, 2, 7, 5, 3, 2, 2, -1, 0.0, False),
         (5, 64, 30, 9, 7, 4, 2, 1, 0, 0.0, True), (32, 64, 2, 7, 5, 1, 1, 0, 1, 0.01, True),
         (32, 64, 3, 9, 6, 3, 2, 1, 2, 0.0, True), (40, 64, 5, 5, 3, 3, 1, 2, 1, 0.0, True),
         (64, 64, 9, 10, 10, 3, 1, 1, 2, 0.0, True), (64, 64, 2, 7, 5, 1, 2, 0, 0, 0.0, True)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_dgrad_small_matches_f64(case):
    from xuanpolicy_amd import _lib, ops
    L = ops.lib()
    cin, cout, B, H, W, k, s, p, act, slope, partials = case
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    g = torch.Generator().manual_seed(13)
    w = torch.randn(cout, cin, k, k, generator=g) / np.sqrt(cout * k * k)
    dz = torch.randn(B, OH, OW, cout, generator=g)
    z = torch.randn(B, H, W, cin, generator=g)
    y_prev = F.leaky_relu(z, slope) if act == 1 else torch.tanh(z) if act == 2 else z
    xr = torch.zeros(B, cin, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, w.double(), None, s, p).backward(dz.double().permute(0, 3, 1, 2))
    yd64 = y_prev.double()
    dact = (yd64 > 0).double() * (1 - slope) + slope if act == 1 else 1 - yd64 * yd64 if act == 2 else 1.0
    ref = xr.grad.permute(0, 2, 3, 1) * dact
    G = int(L.xpa_conv_dgrad_small_num_partials(B, H, W, s))
    # one NaN-filled allocation: [guard | dz | guard | dx | guard | partials | guard], the views 16-byte aligned
    guard, nz, nx, npart = 256, dz.numel(), (ref.numel() + 3) & ~3, (G * cin + 3) & ~3
    buf = torch.full((4 * guard + nz + nx + npart,), float("nan"), device=DEV)
    dzd = buf[guard:guard + nz].view(dz.shape)
    dzd.copy_(dz)
    x0, p0 = 2 * guard + nz, 3 * guard + nz + nx
    dxd, part = buf[x0:x0 + ref.numel()].view(B, H, W, cin), buf[p0:p0 + G * cin].view(G, cin)
    assert dzd.data_ptr() % 16 == dxd.data_ptr() % 16 == part.data_ptr() % 16 == 0
    assert L.xpa_conv_small_dgrad_ok(cin, cout, k, s)
    before = buf.view(torch.int32).clone()
    wd, ypd = w.to(DEV), y_prev.to(DEV) if act >= 0 else None
    _dgrad(L, L.xpa_conv_dgrad_small, dzd, _planes_t(L, wd), cin, k, s, p, H, W, act, ypd, slope, dxd,
           part if partials else None)
    same = buf.view(torch.int32) == before
    same[x0:x0 + ref.numel()] = True
    same[p0:p0 + (G * cin if partials and act >= 0 else 0)] = True
    assert bool(same.all()), "written outside dx and the partials"
    err = float((dxd.cpu().double() - ref).abs().max())
    assert err <= 2e-6 * max(float(ref.abs().max()), 1.0), err
    if L.xpa_conv_igemm_ok(cout, cin, k):
        prev = L.xpa_conv_igemm_form(0)          # K28 proper, the fp32-MFMA form
        d28 = _dgrad(L, L.xpa_conv_dgrad, dzd, wd, cin, k, s, p, H, W, act, ypd, slope)
        L.xpa_conv_igemm_form(prev)
        err28 = float((d28.cpu().double() - ref).abs().max())
        print("max error: K28R-D %.3e, K28 %.3e" % (err, err28))
        assert err <= 2 * err28 + 1e-9, (err, err28)
    if partials and act >= 0:
        db = torch.empty(cin, device=DEV)
        _lib.call(L.xpa_colsum_finalize, ops._p(part), G, cin, ops._p(db), ops._stream(DEV))
        np.testing.assert_allclose(db.cpu().double().numpy(), ref.sum((0, 1, 2)).numpy(), rtol=1e-5,
                                   atol=1e-5 * float(ref.abs().sum((0, 1, 2)).max()))


@pytest.mark.parametrize("k,s,p", [(3, 1, 1), (4, 2, 1)])
def test_deterministic_and_position_independent(k, s, p):
    """Two launches give the same bits; a batch of 3 images (35 pixels each) equals the 3 single-image launches."""
    from xuanpolicy_amd import ops
    L = ops.lib()
    g = torch.Generator().manual_seed(11)
    H, W = 7, 5
    dz = torch.randn(3, (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1, 32, generator=g).to(DEV)
    w = torch.randn(32, 40, k, k, generator=g).to(DEV) / 17
    yp = torch.tanh(torch.randn(3, H, W, 40, generator=g)).to(DEV)
    pl = _planes_t(L, w)
    run = lambda d, y: _dgrad(L, L.xpa_conv_dgrad_small, d, pl, 40, k, s, p, H, W, 2, y, 0.0)
    dx = run(dz, yp)
    assert torch.equal(dx, run(dz, yp)) and bool(torch.isfinite(dx).all())
    assert torch.equal(dx, torch.cat([run(dz[i:i + 1].contiguous(), yp[i:i + 1].contiguous()) for i in range(3)]))


@pytest.mark.parametrize("bad", ["out_c 48", "in_c 65", "k 13", "stride 3", "out_h + 1", "dz + 4 bytes", "NULL planes",
                                 "NULL dz", "NULL dx", "no y_prev"])
def test_rejections_write_nothing(bad):
    from xuanpolicy_amd import ops
    L = ops.lib()
    cout, cin, k = (48 if bad == "out_c 48" else 32), (65 if bad == "in_c 65" else 16), (13 if bad == "k 13" else 3)
    s = 3 if bad == "stride 3" else 1
    buf = torch.zeros(4 + 2 * 16 * 16 * 64, device=DEV)
    dz = None if bad == "NULL dz" else ops._p(buf[1:] if bad == "dz + 4 bytes" else buf)
    pl = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    dx = torch.full((2, 16, 16, 65), float("nan"), device=DEV)
    part = torch.full((64, 65), float("nan"), device=DEV)
    oh = (16 + 2 - k) // s + 1
    rc = L.xpa_conv_dgrad_small(dz, 2, oh + (bad == "out_h + 1"), oh, cout,
                                None if bad == "NULL planes" else ops._p(pl), cin, k, s, 1, 16, 16, 1,
                                None if bad == "no y_prev" else ops._p(buf), 0.0,
                                None if bad == "NULL dx" else ops._p(dx), ops._p(part), ops._stream(DEV))
    assert rc == 1 and bool(torch.isnan(dx).all()) and bool(torch.isnan(part).all())
    envelope = bad in ("out_c 48", "in_c 65", "k 13", "stride 3")
    assert bool(L.xpa_conv_small_dgrad_ok(cin, cout, k, s)) != envelope
    if envelope and bad != "stride 3":
        assert L.xpa_conv_wsplit_t_bytes(cin, cout, k) == 0
        assert L.xpa_conv_wsplit_t(ops._p(buf), cin, cout, k, ops._p(pl), ops._stream(DEV)) == 1


def _close(a, b):   # between two f32 routes: each within 2e-6 x scale of the exact result
    assert float((a.double() - b.double()).abs().max()) <= 2 * 2e-6 * max(float(b.abs().max()), 1.0)


def test_trunk_backward_and_stale_planes():
    """conv 2 (32 -> 16, 4 x 4 stride 2: not K27's shape) and conv 3 (16 -> 32, 3 x 3 stride 1) plan K28R; every
    parameter gradient agrees with the switch-off backward, again after the weights have moved (stale planes)."""
    from xuanpolicy_amd import fused_cnn
    from xuanpolicy_amd.policies import AC_CNN_Atari
    torch.manual_seed(0)
    rep = AC_CNN_Atari((36, 36, 4), [8, 4, 3], [4, 2, 1], [32, 16, 32], None, torch.nn.init.orthogonal_,
                       torch.nn.ReLU, DEV, [64])
    t = fused_cnn._Trunk(rep, fused_cnn._Part())
    fused_cnn._ensure_grads(t.params())
    g = torch.Generator().manual_seed(1)
    x = torch.randint(0, 256, (24, 36, 36, 4), dtype=torch.uint8, generator=g).to(DEV)
    ds = torch.randn(24, 64, generator=g).to(DEV)
    for step in range(2):
        grads = {}
        for key in (False, True):
            t.small_conv_bwd = key
            _, ctx = t.forward(x)
            t.backward(ctx, ds)
            grads[key] = [p.grad.clone() for p in t.params()]
            assert [c.dgrad for c in ctx.plan.convs][1:] == (["K28R", "K28R"] if key else ["miopen", "miopen"])
            assert [c.act_bwd for c in ctx.plan.convs][:2] == (["K28R-dgrad"] * 2 if key else ["K26", "K22"])
        for a, b in zip(grads[True], grads[False]):
            _close(a, b)
        vers = {i: e[0] for i, e in t._cwts.items()}
        assert sorted(vers) == [1, 2] and len(set(vers.values())) == 1
        with torch.no_grad():   # an optimizer step's effect; backward() has already bumped the weights' version
            for p in t.params():
                p.mul_(-1.25)


def test_perdqn_step_with_conv_small_rows_bwd():
    """Two PER-DQN learner steps, config key on against off from the same state: the second step's scalars (moved by
    the first's gradients) within test_a2c_agent_with_conv_small_rows's 1e-4 relative to max(1, |value|)."""
    import xuanpolicy_amd.runner as R
    g = torch.Generator().manual_seed(4)
    obs, nxt = (torch.randint(0, 256, (32, 84, 84, 4), dtype=torch.uint8, generator=g).to(DEV) for _ in range(2))
    act = torch.randint(0, 18, (32,), generator=g).float().to(DEV)
    rew, term = torch.randn(32, generator=g).to(DEV), torch.zeros(32, device=DEV)
    infos = {}
    for key in (False, True):
        ln = R.build_perdqn(n_envs=2, n_size=64, batch_size=32, seed=5, device=DEV, conv_small_rows_bwd=key).learner
        ln.update(obs, act, rew, nxt, term)
        infos[key] = ln.update(obs, act, rew, nxt, term)[1]
        trunk = ln._fused_q().eval_trunk
        assert trunk.small_conv_bwd is key and ln._fused_q().target_trunk.small_conv_bwd is False
        assert [c.dgrad for c in trunk.last_plan.convs] == ["none", "K27", "K28R" if key else "miopen"]
    for name, v in infos[False].items():
        assert abs(infos[True][name] - v) <= 1e-4 * max(1.0, abs(v)), (name, infos[True][name], v)
