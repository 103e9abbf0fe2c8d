"""GPU: K28R (xpa_conv_wsplit + xpa_conv_fwd_small, csrc/igemm_small.hip) against the float64 torch convolution at the
smallest shapes that reach every template instance and edge, with K28's bounds: the absolute bound of
test_gpu_igemm.py::test_conv_fwd_matches_f64 and, on the same inputs, at most twice K28's own error (+ 1e-9).  x and y
are 16-byte aligned views into one NaN-filled allocation, of which every byte outside y must survive the launch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _planes(L, w, cin, cout, k):
    from xuanpolicy_amd import _lib, ops
    pl = torch.empty(int(L.xpa_conv_wsplit_bytes(cin, cout, k)), dtype=torch.uint8, device=DEV)
    _lib.call(L.xpa_conv_wsplit, ops._p(w), cin, cout, k, ops._p(pl), ops._stream(DEV))
    return pl


def _small(L, x, pl, b, cout, k, s, p, act=0, slope=0.0, y=None):
    from xuanpolicy_amd import _lib, ops
    B, H, W, cin = x.shape
    if y is None:
        y = torch.full((B, (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1, cout), float("nan"), device=DEV)
    _lib.call(L.xpa_conv_fwd_small, act, ops._p(x), B, H, W, cin, ops._p(pl), ops._p(b) if b is not None else None,
              cout, k, s, p, slope, ops._p(y), ops._stream(DEV))
    return y


# (cin, cout, B, H, W, k, s, p, act, slope, bias): in_c 16 / 32 / 64 x out_c 5 / 32 / 40 / 64 (NT 1 and 2, padded
# columns on both); k 1, k 3 s 1 p 1, k 4 s 2 p 1, p 0, p > k / 2; H != W; OW = 1; rows below one tile (12, 40, 70),
# exactly one (128), several with a ragged last one (175, 360, 900) and more tiles than 8 per SIMD can hold at once
# (264 000 rows = 2063 blocks > 256 CUs x 8); every activation code, slope 0 and 0.01, no bias
CASES = [(16, 5, 2, 7, 5, 1, 1, 0, 0, 0.0, True), (16, 32, 2, 8, 8, 3, 1, 1, 1, 0.0, True),
         (16, 40, 30, 9, 7, 4, 2, 1, 1, 0.01, True), (16, 64, 2, 7, 6, 3, 1, 0, 2, 0.0, True),
         (32, 5, 5, 5, 3, 3, 1, 2, 1, 0.01, False), (32, 32, 3, 6, 3, 3, 1, 0, 0, 0.0, True),
         (32, 40, 2, 8, 8, 3, 1, 1, 2, 0.0, False), (32, 64, 30, 9, 7, 4, 2, 1, 1, 0.0, True),
         (64, 5, 30, 9, 7, 4, 2, 1, 0, 0.0, True), (64, 32, 2, 7, 5, 1, 1, 0, 1, 0.01, True),
         (64, 40, 5, 5, 3, 3, 1, 2, 1, 0.0, True), (64, 64, 9, 10, 10, 3, 1, 1, 1, 0.0, True),
         (16, 32, 660, 20, 20, 3, 1, 1, 1, 0.0, True)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_fwd_small_matches_f64(case):
    from xuanpolicy_amd import _lib, ops
    L = ops.lib()
    cin, cout, B, H, W, k, s, p, act, slope, bias = case
    g = torch.Generator().manual_seed(7)
    x = torch.rand(B, H, W, cin, generator=g) - 0.25
    w = torch.randn(cout, cin, k, k, generator=g) / np.sqrt(cin * k * k)
    b = torch.randn(cout, generator=g) * 0.1 if bias else None
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double() if bias else None, s, p).permute(0, 2, 3, 1)
    ref = F.leaky_relu(ref, slope) if act == 1 else torch.tanh(ref) if act == 2 else ref
    OH, OW = ref.shape[1], ref.shape[2]
    assert L.xpa_conv_small_ok(cin, cout, k) and L.xpa_conv_igemm_ok(cin, cout, k)
    # one NaN-filled allocation: [guard | x | guard | y | guard], the views 16-byte aligned
    guard, nx, ny = 256, x.numel(), (B * OH * OW * cout + 3) & ~3
    buf = torch.full((3 * guard + nx + ny,), float("nan"), device=DEV)
    xd = buf[guard:guard + nx].view(x.shape)
    xd.copy_(x)
    y0 = 2 * guard + nx
    yd = buf[y0:y0 + B * OH * OW * cout].view(B, OH, OW, cout)
    assert xd.data_ptr() % 16 == 0 and yd.data_ptr() % 16 == 0
    before = buf.view(torch.int32).clone()
    wd, bd = w.to(DEV), b.to(DEV) if bias else None
    _small(L, xd, _planes(L, wd, cin, cout, k), bd, cout, k, s, p, act, slope, y=yd)
    torch.cuda.synchronize()
    same = buf.view(torch.int32) == before
    assert bool(same[:y0].all()) and bool(same[y0 + yd.numel():].all()), "written outside y"
    y28 = torch.full((B, OH, OW, cout), float("nan"), device=DEV)
    prev = L.xpa_conv_igemm_form(0)          # K28 proper, the fp32-MFMA form
    _lib.call(L.xpa_conv_fwd, act, ops._p(xd), B, H, W, cin, ops._p(wd), ops._p(bd) if bias else None, cout, k, s, p,
              slope, ops._p(y28), ops._stream(DEV))
    L.xpa_conv_igemm_form(prev)
    err = float((yd.cpu().double() - ref).abs().max())
    err28 = float((y28.cpu().double() - ref).abs().max())
    print("K28R max error %.3e, K28 %.3e" % (err, err28))
    assert err <= 2e-6 * max(float(ref.abs().max()), 1.0)
    assert err <= 2 * err28 + 1e-9, (err, err28)


def test_deterministic_and_position_independent():
    """Two launches give the same bits; a batch of 3 images (35 rows each: three offsets inside one tile) equals the
    three single-image forwards stacked, bit for bit."""
    from xuanpolicy_amd import ops
    L = ops.lib()
    g = torch.Generator().manual_seed(11)
    x = torch.randn(3, 7, 5, 32, generator=g).to(DEV)
    w = torch.randn(40, 32, 3, 3, generator=g).to(DEV) / 17
    b = torch.randn(40, generator=g).to(DEV)
    pl = _planes(L, w, 32, 40, 3)
    y = _small(L, x, pl, b, 40, 3, 1, 1, 2)
    assert torch.equal(y, _small(L, x, pl, b, 40, 3, 1, 1, 2)) and bool(torch.isfinite(y).all())
    singles = torch.cat([_small(L, x[i:i + 1].contiguous(), pl, b, 40, 3, 1, 1, 2) for i in range(3)])
    assert torch.equal(y, singles)


@pytest.mark.parametrize("bad", ["in_c 12", "out_c 65", "k 13", "x + 4 bytes", "NULL planes"])
def test_rejections_write_nothing(bad):
    from xuanpolicy_amd import ops
    L = ops.lib()
    cin, cout, k = (12 if bad == "in_c 12" else 16), (65 if bad == "out_c 65" else 32), (13 if bad == "k 13" else 3)
    buf = torch.zeros(4 + 2 * 16 * 16 * 64, device=DEV)
    x = buf[1:] if bad == "x + 4 bytes" else buf
    pl = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    y = torch.full((2, 16, 16, 65), float("nan"), device=DEV)
    rc = L.xpa_conv_fwd_small(1, ops._p(x), 2, 16, 16, cin, None if bad == "NULL planes" else ops._p(pl), None, cout, k,
                              1, 1, 0.0, ops._p(y), ops._stream(DEV))
    torch.cuda.synchronize()
    assert rc == 1 and bool(torch.isnan(y).all())
    assert bool(L.xpa_conv_small_ok(cin, cout, k)) == (bad in ("x + 4 bytes", "NULL planes"))
    if not L.xpa_conv_small_ok(cin, cout, k):
        assert L.xpa_conv_wsplit_bytes(cin, cout, k) == 0
        assert L.xpa_conv_wsplit(ops._p(buf), cin, cout, k, ops._p(pl), ops._stream(DEV)) == 1


def _small_trunk(seed=0):
    from xuanpolicy_amd import fused_cnn
    from xuanpolicy_amd.policies import AC_CNN_Atari
    torch.manual_seed(seed)
    rep = AC_CNN_Atari((36, 36, 4), [8, 4, 3], [4, 2, 1], [32, 16, 32], None, torch.nn.init.orthogonal_,
                       torch.nn.ReLU, DEV, [64])
    return fused_cnn._Trunk(rep, fused_cnn._Part())


def _close(a, b):   # bound (1) between two f32 routes: each within 2e-6 x scale of the exact result
    assert float((a.double() - b.double()).abs().max()) <= 2 * 2e-6 * max(float(b.abs().max()), 1.0)


def test_trunk_forward_and_stale_planes():
    t = _small_trunk()
    x = torch.randint(0, 256, (24, 36, 36, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(DEV)
    s_off, ctx_off = t.forward(x)
    assert [c.fwd for c in t.last_plan.convs] == ["K25", "miopen", "miopen"]
    t.small_conv = True
    s_on, ctx_on = t.forward(x)
    assert [c.fwd for c in t.last_plan.convs] == ["K25", "K28R", "K28R"]
    for a, b in zip(ctx_on.hs[2:] + [s_on], ctx_off.hs[2:] + [s_off]):
        _close(a, b)
    vers = {i: e[0] for i, e in t._cws.items()}
    assert sorted(vers) == [1, 2]
    with torch.no_grad():
        t.convs[2][0].weight.mul_(-1.5)
    stale, _ = t.forward(x)                      # no refresh(): no split launch, the planes are the old weights'
    assert {i: e[0] for i, e in t._cws.items()} == vers and torch.equal(stale, s_on)
    t.refresh()
    assert all(t._cws[i][0] == vers[i] + 1 for i in vers)
    s_new, _ = t.forward(x)
    t.small_conv = False
    s_ref, _ = t.forward(x)
    _close(s_new, s_ref)
    assert float((s_new - s_on).abs().max()) > 1e-3


def test_qnetwork_target_follows_copy_target():
    from xuanpolicy_amd.fused_cnn import FusedQNetwork
    from xuanpolicy_amd.policies import BasicQnetwork, Basic_CNN

    class Disc:
        n, shape = 6, ()
    torch.manual_seed(2)
    rep = Basic_CNN((36, 36, 4), [8, 4, 3], [4, 2, 1], [32, 16, 32], None, torch.nn.init.orthogonal_, torch.nn.ReLU, DEV)
    pol = BasicQnetwork(Disc(), rep, [32], None, torch.nn.init.orthogonal_, torch.nn.ReLU, DEV)
    fq = FusedQNetwork(pol)
    fq.eval_trunk.small_conv = fq.target_trunk.small_conv = True
    x = torch.randint(0, 256, (16, 36, 36, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).to(DEV)
    q0 = fq.target(x)
    assert [c.fwd for c in fq.target_trunk.last_plan.convs] == ["K25", "K28R", "K28R"]
    with torch.no_grad():
        for p_ in pol.representation.parameters():
            p_.mul_(1.25)
    fq.eval_trunk.refresh()
    pol.copy_target()
    fq.target_trunk.refresh()                    # what PerDQN_Learner.update does after its hard update
    q1 = fq.target(x)
    assert torch.equal(q1, fq.forward(x)[0]) and not torch.equal(q1, q0)


def test_a2c_agent_with_conv_small_rows():
    """A short A2C run on SynthAtari frames with the config key on: the rollout's forwards are K28R's, and the first
    update's losses are the key-off run's within the host-env A2C replay's loss tolerance (1e-4 relative to
    max(1, |loss|), tests/_oracle_replay.py)."""
    import xuanpolicy_amd.runner as R
    infos = {}
    for key in (False, True):
        agent = R.build_atari_a2c(n_envs=16, n_steps=8, seed=5, device=DEV, conv_small_rows=key, n_minibatch=1,
                                  n_epoch=1, filters=[32, 16, 32], fc_hidden_sizes=[64])
        agent.train(8)
        torch.cuda.synchronize()
        fc = agent.learner._fused_cnn()
        assert fc is not None and fc.trunk_.small_conv is key
        infos[key] = dict(agent.infos[-1])
        if key:
            assert [c.fwd for c in fc.trunk_.last_plan.convs][1:] == ["K28R", "K28R"]
    for name, v in infos[False].items():
        if isinstance(v, float):
            assert abs(infos[True][name] - v) <= 1e-4 * max(1.0, abs(v)), (name, infos[True][name], v)
