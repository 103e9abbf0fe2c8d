"""GPU: K28R-W (xpa_conv_wgrad_small, csrc/igemm_small_wgrad.hip), the conv weight gradient of small batches on the bf16
matrix cores, through the C ABI against the float64 autograd weight gradient of F.conv2d, with K29's bound and K29's
draw of the operands (tests/test_gpu_igemm.py::test_conv_wgrad_matches_f64).  Emulated on the CPU at these shapes, a
dropped low plane of one operand lands at 0.6-1.3x the bound (a dropped middle plane far outside it); the kernel's own
error is 15-60x under it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (B, H, W, in_c, out_c, k, s, p): every (in_c, out_c) pair once, every tiles-per-wave instance, two column groups
CASES = [
    (1, 5, 7, 16, 16, 1, 2, 0),       # k 1 s 2; batch 1 (most blocks get nothing); 12 pixels per image; one tile
    (3, 4, 4, 16, 32, 1, 1, 0),       # k 1 s 1 p 0; exactly 16 pixels per image
    (2, 6, 5, 16, 64, 3, 1, 2),       # p > k / 2; 56 pixels; 4.5 column tiles (two taps per tile, the last half empty)
    (2, 9, 7, 32, 16, 4, 2, 1),       # k 4 s 2 p 1; 12 pixels
    (2, 8, 6, 32, 32, 3, 2, 0),       # the last input row and column are reached by no tap
    (300, 5, 5, 64, 64, 3, 1, 1),     # more images than blocks: a block loops over slabs and images; 36 tiles, T = 3
    (2, 9, 11, 64, 16, 5, 2, 2),      # 50 half-used tiles: two column groups
    (2, 40, 12, 64, 32, 3, 1, 1),     # an image of 7 slabs (6 rows each), the last one ragged (4); T = 2
    (2, 21, 11, 32, 64, 4, 2, 1),     # C5 conv2's block on a narrow map; 32 tiles, T = 4
]


@pytest.fixture(scope="module", autouse=True)
def _setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _operands(case):
    """x and dz as test_conv_wgrad_matches_f64 draws them (x uniform [0, 1), dz normal), and the f64 reference."""
    B, H, W, Cin, Cout, k, s, p = case
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    g = torch.Generator().manual_seed(4)
    x = torch.rand(B, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / np.sqrt(Cin * k * k)
    dz = torch.randn(B, OH, OW, Cout, generator=torch.Generator().manual_seed(5))
    wr = w.double().requires_grad_(True)
    F.conv2d(x.double().permute(0, 3, 1, 2), wr, None, s, p).backward(dz.double().permute(0, 3, 1, 2))
    return x, dz, wr.grad, OH, OW


def _arena(x, dz, G, cols):
    """dz, x and the partials as 16-byte-aligned views into one NaN-filled allocation, 20 floats between them."""
    sizes, offs, at = (dz.numel(), x.numel(), G * cols), [], 20
    for n in sizes:
        offs.append(at)
        at = (at + n + 20 + 3) & ~3
    arena = torch.full((at,), float("nan"), device=DEV)
    views = [arena[o:o + n] for o, n in zip(offs, sizes)]
    views[0].copy_(dz.reshape(-1))
    views[1].copy_(x.reshape(-1))
    return arena, views, offs[2]


def _launch(case, x, dz, OH, OW):
    from xuanpolicy_amd import _lib, ops
    L = ops.lib()
    B, H, W, Cin, Cout, k, s, p = case
    cols = Cout * Cin * k * k
    G = int(L.xpa_conv_wgrad_small_num_partials(B, H, W, Cin, Cout, k, s, p))
    assert 1 <= G <= min(B * OH, torch.cuda.get_device_properties(DEV).multi_processor_count)
    arena, (dzv, xv, part), po = _arena(x, dz, G, cols)
    before = arena.view(torch.int32).clone()
    _lib.check(L.xpa_conv_wgrad_small(ops._p(dzv), ops._p(xv), B, H, W, Cin, Cout, k, s, p, OH, OW, ops._p(part),
                                      ops._stream(DEV)), "xpa_conv_wgrad_small")
    after = arena.view(torch.int32)
    assert torch.equal(after[:po], before[:po]) and torch.equal(after[po + G * cols:], before[po + G * cols:])
    return part.clone(), G, cols


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_wgrad_small_matches_f64(case):
    from xuanpolicy_amd import _lib, ops
    L, st = ops.lib(), ops._stream(DEV)
    B, H, W, Cin, Cout, k, s, p = case
    x, dz, ref, OH, OW = _operands(case)
    part, G, cols = _launch(case, x, dz, OH, OW)
    dw = torch.empty(Cout, Cin, k, k, device=DEV)
    _lib.check(L.xpa_colsum_finalize(ops._p(part), G, cols, ops._p(dw), st), "finalize")
    assert bool(torch.isfinite(dw).all())          # no partial was left unwritten
    err = float((dw.cpu().double() - ref).abs().max())
    if L.xpa_conv_wgrad_ok(Cin, Cout, k):
        G9 = int(L.xpa_conv_wgrad_num_partials())
        p9, dw9 = torch.empty(G9, cols, device=DEV), torch.empty(Cout, Cin, k, k, device=DEV)
        dzd, xd = dz.to(DEV), x.to(DEV)
        _lib.check(L.xpa_conv_wgrad(-1, ops._p(dzd), None, 0.0, ops._p(xd), B, H, W, Cin, Cout, k, s, p, ops._p(p9), None,
                                    st), "xpa_conv_wgrad")
        _lib.check(L.xpa_colsum_finalize(ops._p(p9), G9, cols, ops._p(dw9), st), "finalize")
        err29 = float((dw9.cpu().double() - ref).abs().max())
        print("K29 max error %.3e" % err29, end="; ")
    tol = 2e-6 * float(ref.abs().max()) + 1e-6 * (B * OH * OW) ** 0.5
    print("K28R-W max error %.3e, atol %.3e, max |dW| %.3e, G %d" % (err, tol, float(ref.abs().max()), G))
    if L.xpa_conv_wgrad_ok(Cin, Cout, k):   # the split's accuracy is the f32 GEMM's (as K28R's tests hold K28R to K28)
        assert err <= 2 * err29 + 1e-9, (err, err29)
    np.testing.assert_allclose(dw.cpu().double().numpy(), ref.numpy(), rtol=1e-5, atol=tol)


def test_widest_map_and_one_wider():
    """xpa_conv_wgrad_small_fits is the launch's own rule: a 32-wide 64 -> 64 3 x 3 map runs (slabs of one output row),
    a 33-wide one is rejected before any launch."""
    from xuanpolicy_amd import _lib, ops
    L = ops.lib()
    case = (1, 3, 32, 64, 64, 3, 1, 1)
    assert L.xpa_conv_wgrad_small_fits(3, 32, 64, 64, 3, 1, 1) and not L.xpa_conv_wgrad_small_fits(3, 33, 64, 64, 3, 1, 1)
    x, dz, ref, OH, OW = _operands(case)
    part, G, cols = _launch(case, x, dz, OH, OW)
    dw = torch.empty(64, 64, 3, 3, device=DEV)
    _lib.check(L.xpa_colsum_finalize(ops._p(part), G, cols, ops._p(dw), ops._stream(DEV)), "finalize")
    tol = 2e-6 * float(ref.abs().max()) + 1e-6 * (OH * OW) ** 0.5
    np.testing.assert_allclose(dw.cpu().double().numpy(), ref.numpy(), rtol=1e-5, atol=tol)
    buf, nan = torch.zeros(3 * 33 * 64, device=DEV), torch.full((3, cols), float("nan"), device=DEV)
    assert L.xpa_conv_wgrad_small_num_partials(1, 3, 33, 64, 64, 3, 1, 1) == 0
    assert L.xpa_conv_wgrad_small(ops._p(buf), ops._p(buf), 1, 3, 33, 64, 64, 3, 1, 1, 3, 33, ops._p(nan),
                                  ops._stream(DEV)) == 1 and bool(torch.isnan(nan).all())


@pytest.mark.parametrize("case", [CASES[5], CASES[8]], ids=["s1", "s2"])
def test_deterministic(case):
    x, dz, _, OH, OW = _operands(case)
    assert torch.equal(_launch(case, x, dz, OH, OW)[0], _launch(case, x, dz, OH, OW)[0])


@pytest.mark.parametrize("bad", ["in_c 48", "out_c 65", "over the envelope", "stride 3", "out_h + 1", "x + 4 bytes",
                                 "NULL dz", "NULL x", "NULL partials"])
def test_rejections_write_nothing(bad):
    from xuanpolicy_amd import ops
    L = ops.lib()
    cin, cout = (48 if bad == "in_c 48" else 64), (65 if bad == "out_c 65" else 64)
    k, s = (4 if bad == "over the envelope" else 3), (3 if bad == "stride 3" else 1)
    buf = torch.zeros(4 + 2 * 12 * 12 * 65, device=DEV)
    part = torch.full((256, 65 * 64 * 16), float("nan"), device=DEV)
    oh = (12 + 2 - k) // s + 1
    rc = L.xpa_conv_wgrad_small(None if bad == "NULL dz" else ops._p(buf),
                                None if bad == "NULL x" else ops._p(buf[1:] if bad == "x + 4 bytes" else buf),
                                2, 12, 12, cin, cout, k, s, 1, oh + (bad == "out_h + 1"), oh,
                                None if bad == "NULL partials" else ops._p(part), ops._stream(DEV))
    assert rc == 1 and bool(torch.isnan(part).all())
    envelope = bad in ("in_c 48", "out_c 65", "over the envelope", "stride 3")
    assert bool(L.xpa_conv_small_wgrad_ok(cin, cout, k, s)) != envelope
    if envelope:
        assert L.xpa_conv_wgrad_small_num_partials(2, 12, 12, cin, cout, k, s, 1) == 0


def _close(a, b):   # test_gpu_conv_small_dgrad's: between two f32 routes, each within 2e-6 x scale of the exact result
    assert float((a.double() - b.double()).abs().max()) <= 2 * 2e-6 * max(float(b.abs().max()), 1.0)


def test_trunk_backward_wgrad_key():
    """test_trunk_backward_and_stale_planes' trunk: conv 2 (32 -> 16, 4 x 4 stride 2) and conv 3 (16 -> 32, 3 x 3) plan
    K28R-W with the switch on; every parameter gradient agrees with the switch-off backward."""
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
    grads = {}
    for key in (False, True):
        t.small_conv_wgrad = key
        _, ctx = t.forward(x)
        t.backward(ctx, ds)
        grads[key] = [p.grad.clone() for p in t.params()]
        assert [c.wgrad for c in ctx.plan.convs] == ["K26"] + (["K28R"] * 2 if key else ["miopen"] * 2)
    for a, b in zip(grads[True], grads[False]):
        _close(a, b)


def test_perdqn_step_all_three_keys():
    """Two PER-DQN learner steps with the three small-batch conv keys on against off, from the same state: the second
    step's scalars within 1e-4 relative to max(1, |value|); no library convolution is left in the eval trunk's plan."""
    import xuanpolicy_amd.runner as R
    g = torch.Generator().manual_seed(4)
    obs, nxt = (torch.randint(0, 256, (32, 84, 84, 4), dtype=torch.uint8, generator=g).to(DEV) for _ in range(2))
    act = torch.randint(0, 18, (32,), generator=g).float().to(DEV)
    rew, term = torch.randn(32, generator=g).to(DEV), torch.zeros(32, device=DEV)
    infos = {}
    for key in (False, True):
        ln = R.build_perdqn(n_envs=2, n_size=64, batch_size=32, seed=5, device=DEV, conv_small_rows=key,
                            conv_small_rows_bwd=key, conv_small_rows_wgrad=key).learner
        ln.update(obs, act, rew, nxt, term)
        infos[key] = ln.update(obs, act, rew, nxt, term)[1]
        trunk = ln._fused_q().eval_trunk
        assert trunk.small_conv_wgrad is key and ln._fused_q().target_trunk.small_conv_wgrad is False
        forms = [f for c in trunk.last_plan.convs for f in (c.wgrad, c.dgrad)]
        assert ("miopen" in forms) is not key and (not key or [c.wgrad for c in trunk.last_plan.convs][1:] == ["K28R"] * 2)
    for name, v in infos[False].items():
        assert abs(infos[True][name] - v) <= 1e-4 * max(1.0, abs(v)), (name, infos[True][name], v)


def test_a2c_agent_with_the_config_key():
    """test_a2c_agent_with_conv_small_rows' short A2C run with conv_small_rows_wgrad in the config: the key reaches the
    update's trunk through the agent, and the first update's losses are the key-off run's within 1e-4 relative to
    max(1, |loss|)."""
    import xuanpolicy_amd.runner as R
    infos = {}
    for key in (False, True):
        agent = R.build_atari_a2c(n_envs=16, n_steps=8, seed=5, device=DEV, conv_small_rows_wgrad=key, n_minibatch=1,
                                  n_epoch=1, filters=[32, 16, 32], fc_hidden_sizes=[64])
        agent.train(8)
        torch.cuda.synchronize()
        trunk = agent.learner._fused_cnn().trunk_
        assert agent.learner.conv_small_rows_wgrad is key and trunk.small_conv_wgrad is key
        assert [c.wgrad for c in trunk.plan(torch.empty((128, 0), dtype=torch.uint8, device=DEV)).convs][1:] == (
            ["K28R"] * 2 if key else ["miopen"] * 2)
        infos[key] = dict(agent.infos[-1])
    for name, v in infos[False].items():
        if isinstance(v, float):
            assert abs(infos[True][name] - v) <= 1e-4 * max(1.0, abs(v)), (name, infos[True][name], v)
