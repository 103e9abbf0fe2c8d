"""CPU checks behind the K28 / K29 envelope tests (test_gpu_igemm_envelope.py):
  * the case table (tests/_igemm_cases.py) reaches every template instance and every dispatch branch of csrc/igemm.hip,
    by the Python mirror of its dispatch arithmetic; the mirror agrees with the library's two host predicates;
  * what the planner admits to the K28 / K29 path (ConvFacts.igemm) is what both K28's forward and K29 take;
  * the comparison helper the GPU tests use passes the f32 CPU convolution and fails a moved weight tap, a zeroed input
    channel and a single element off by 1e-4 of the output's scale."""
import itertools

import pytest
import torch

from tests import _igemm_cases as T
from xuanpolicy_amd import _lib
from xuanpolicy_amd.cnn_plan import conv_facts


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


# ---- the table's coverage --------------------------------------------------------------------------------------------
def test_every_case_is_admitted_and_small():
    big = 0
    for c in T.K28_CASES:
        assert T.ig_shape(c.cin, c.cout, c.k) is not None and min(T.out_hw(c)) >= 1, c
        assert c.B * c.H * c.W * max(c.cin, c.cout) * 4 < 2 ** 31 and T.fwd_rows(c) * c.cout * 4 < 2 ** 31, c
        big += max(T.fwd_rows(c), T.dgrad_rows(c)) > 4096
    assert big == 3                       # the two persistent-loop cases and the K28B one
    for c in T.K29_CASES:
        assert T.wg_shape(c.cin, c.cout, c.k) is not None and min(T.out_hw(c)) >= 1, c
        assert T.fwd_rows(c) <= 4096, c


def test_table_reaches_every_k28_instance_and_activation():
    pairs = set(itertools.product((8, 16, 32, 64), (1, 2)))
    fwd = {T.ig_shape(c.cin, c.cout, c.k) for c in T.K28_CASES}
    dg = [c for c in T.K28_CASES if T.dgrad_admitted(c)]
    assert fwd == pairs
    assert {T.ig_shape(c.cout, c.cin, c.k) for c in dg} == pairs
    assert {c.act for c in T.K28_CASES} == {0, 1, 2}
    assert {T.dgrad_prev(c) for c in dg} == {-1, 0, 1, 2}
    assert any(T.dgrad_prev(c) == -1 and not c.prev_bias for c in dg)      # nothing but dX written
    assert any(T.dgrad_prev(c) == 0 and c.prev_bias for c in dg)           # identity with a bias gradient
    assert any(c.act == 1 and c.slope != 0 for c in T.K28_CASES) and any(c.slope != 0 and T.dgrad_prev(c) == 1 for c in dg)
    # the padded channel counts: the 4 q < CIN load mask and the n < COUT store mask, in both modes
    assert any(c.cin not in (4, 8, 16, 32, 64) for c in T.K28_CASES) and any(c.cout % 32 and c.cout > 8 for c in T.K28_CASES)
    assert any(c.cout % 4 for c in T.K28_CASES)
    assert any(c.cout not in (4, 8, 16, 32, 64) for c in dg) and any(c.cin % 32 and c.cin > 8 for c in dg)
    # K28B's own instances (input channels a multiple of 16 and unpadded) in both modes
    assert {c.cin for c in T.K28_CASES} >= {16, 32, 64} and {c.cout for c in dg} >= {16, 32, 64}
    # geometry: H != W, p = 0, p > (k - s) // 2, 1 x 1, stride 2, a stride-2 last input row without gradient
    assert any(c.H != c.W for c in T.K28_CASES) and any(c.p == 0 and c.k > 1 for c in T.K28_CASES)
    assert any(c.p > (c.k - c.s) // 2 for c in T.K28_CASES) and any(c.k == 1 and c.cin <= 8 for c in T.K28_CASES)
    assert any(c.s == 2 and (c.H + 2 * c.p - c.k) % 2 for c in dg)
    assert any(T.fwd_rows(c) == 1 and c.cout == 1 for c in T.K28_CASES)


def test_table_reaches_the_persistent_loop():
    """More than one 512-row block per workgroup in each mode (256 workgroups), and more than one of K28B's 768-row
    steps (its 3-tile waves) at a shape K28B takes."""
    dg = [c for c in T.K28_CASES if T.dgrad_admitted(c)]
    assert any(T.fwd_rows(c) > T.IG_GRID * T.IG_ROWS for c in T.K28_CASES)
    assert any(T.dgrad_rows(c) > T.IG_GRID * T.IG_ROWS for c in dg)
    assert any(T.fwd_rows(c) > T.IG_GRID * 768 and c.cin % 16 == 0 for c in T.K28_CASES)
    assert any(T.dgrad_rows(c) > T.IG_GRID * 512 and c.cout % 16 == 0 for c in dg)


def test_table_reaches_every_k29_instance_and_form():
    shapes = [T.wg_shape(c.cin, c.cout, c.k) for c in T.K29_CASES]
    assert {s[0] for s in shapes} == {1, 2, 4} and {s[1] for s in shapes} == {2, 4, 8, 9}
    assert {s[2] for s in shapes} == {1, 2, 3, 4}
    assert {c.act for c in T.K29_CASES} == {0, 1, 2} and any(c.slope != 0 for c in T.K29_CASES)   # -1: fold_act off
    forms = [T.wg_form(c) for c in T.K29_CASES]
    assert any(f[0] == "slab" and f[2] == 1 for f in forms) and any(f[0] == "slab" and f[2] > 1 for f in forms)
    natural = [c for c, f in zip(T.K29_CASES, forms) if f[0] == "stream"]
    assert any(c.cout % 4 for c in natural)                                      # by the f4 staging rule
    assert any(c.cin % 4 == 0 and c.cout % 4 == 0 for c in natural)              # no one-row slab fits
    assert any((c.k * c.k * c.cin) % 16 for c in T.K29_CASES)                    # a ragged last column tile
    assert any(c.k * c.k * c.cin == 576 for c in T.K29_CASES)                    # the envelope's edge: 36 tiles
    ow = {T.out_hw(c)[1] for c in T.K29_CASES}
    assert 1 in ow and 3 in ow and any(c.s == 3 for c in T.K29_CASES)
    assert any(c.cout % 16 and c.cout > 16 for c in T.K29_CASES)


# ---- admission -------------------------------------------------------------------------------------------------------
def _facts(lib, cin, cout, k):
    return conv_facts(cin, cout, (k, k), (1, 1), (0, 0), True, True, 1, lib.xpa_conv_igemm_ok, lib.xpa_conv_wgrad_ok)


def test_mirror_agrees_with_the_library(lib):
    for cin, cout, k in itertools.product(range(1, 69), (1, 5, 16, 17, 32, 33, 64, 65), range(1, 10)):
        assert bool(lib.xpa_conv_igemm_ok(cin, cout, k)) == (T.ig_shape(cin, cout, k) is not None), (cin, cout, k)
        assert bool(lib.xpa_conv_wgrad_ok(cin, cout, k)) == (T.wg_shape(cin, cout, k) is not None), (cin, cout, k)
    for bad in ((0, 8, 3), (8, 0, 3), (8, 8, 0), (-4, 8, 3), (8, 8, 1 << 40), (1 << 40, 8, 1)):
        assert not lib.xpa_conv_wgrad_ok(*bad) and not lib.xpa_conv_igemm_ok(*bad), bad


def test_admission_agrees_with_the_kernels(lib):
    """Every conv planned onto the K28 / K29 path is one K29 takes (k k cin <= 576) as well as K28's forward."""
    admitted = 0
    for cin, cout, k in itertools.product(range(4, 65, 4), range(1, 65), range(1, 9)):
        f = _facts(lib, cin, cout, k)
        if f.igemm:
            admitted += 1
            assert lib.xpa_conv_wgrad_ok(cin, cout, k) and lib.xpa_conv_igemm_ok(cin, cout, k), (cin, cout, k)
            assert k * k * cin <= 576
        if f.igemm_dgrad:
            assert f.igemm and lib.xpa_conv_igemm_ok(cout, cin, k), (cin, cout, k)
    assert admitted > 1000
    for cin, cout, k in ((32, 32, 5), (16, 16, 8)):       # K28's weight image fits, K29's tiles do not
        assert lib.xpa_conv_igemm_ok(cin, cout, k) and not lib.xpa_conv_wgrad_ok(cin, cout, k)
        f = _facts(lib, cin, cout, k)
        assert not f.igemm and not f.igemm_dgrad, (cin, cout, k)
    for cin, cout, k in ((32, 64, 4), (64, 64, 3), (4, 8, 8), (8, 8, 4)):   # the production and test-net convs
        assert _facts(lib, cin, cout, k).igemm, (cin, cout, k)
    # neither predicate asked: no K28 / K29
    assert not conv_facts(8, 8, (4, 4), (2, 2), (1, 1), True, True, 1).igemm
    assert not conv_facts(8, 8, (4, 4), (2, 2), (1, 1), True, True, 1, lib.xpa_conv_igemm_ok).igemm


def test_a_conv_k29_cannot_take_plans_the_library_route():
    """Conv2d(32, 32, 5) after the Nature first layer: all three directions of the block go to the library."""
    from xuanpolicy_amd import fused_cnn
    from xuanpolicy_amd.cnn_plan import plan_cnn
    from xuanpolicy_amd.policies import Basic_CNN
    rep = Basic_CNN((84, 84, 4), [8, 5], [4, 1], [32, 32], None, None, torch.nn.ReLU, "cpu")
    t = fused_cnn._Trunk(rep, fused_cnn._Part())
    assert not t.conv_facts[1].igemm
    c = plan_cnn(t.facts(16384)._replace(igemm_min_rows=0)).convs[1]
    assert (c.fwd, c.wgrad, c.dgrad) == ("miopen", "miopen", "miopen")


# ---- the comparison helper's negative control ------------------------------------------------------------------------
@pytest.mark.parametrize("c", [T.K28_CASES[0], T.K28_CASES[3]], ids=lambda c: c.id)
def test_comparison_catches_subtle_errors(c):
    x, w, b, ref = T.fwd_reference(c)

    def f32(x_, w_):
        return T.act_output(T.conv_nhwc(x_, w_, b, c), c.act, c.slope).numpy()
    T.check_fwd(f32(x, w), ref.numpy())
    moved = w.clone()                                   # one tap of one (n, c) pair moved to its neighbour
    moved[1, 2, 0, 1], moved[1, 2, 0, 0] = w[1, 2, 0, 0], w[1, 2, 0, 1]
    with pytest.raises(AssertionError):
        T.check_fwd(f32(x, moved), ref.numpy())
    dropped = x.clone()
    dropped[..., c.cin - 1] = 0                         # the last input channel lost (a load mask one quad short)
    with pytest.raises(AssertionError):
        T.check_fwd(f32(dropped, w), ref.numpy())
    one = f32(x, w)
    one[-1, -1, -1, -1] += 1e-4 * float(ref.abs().max())
    with pytest.raises(AssertionError):
        T.check_fwd(one, ref.numpy())
    nan = f32(x, w)
    nan[0, 0, 0, 0] = float("nan")                      # a pre-filled element never written
    with pytest.raises(AssertionError):
        T.check_fwd(nan, ref.numpy())


def test_wgrad_comparison_catches_a_dropped_row():
    c = T.K29_CASES[0]
    x, g, y, dw, db = T.wgrad_reference(c, True)
    dz = g * T.grad64(y.double(), c.act, c.slope).float()

    def f32(x_, dz_):
        w = torch.zeros(c.cout, c.cin, c.k, c.k, requires_grad=True)
        T.conv_nhwc(x_, w, None, c).backward(dz_)
        return w.grad.numpy()
    rows = T.fwd_rows(c)
    T.check_wgrad(f32(x, dz), dw.numpy(), rows)
    T.check_wgrad_bias(dz.sum((0, 1, 2)).numpy(), db.numpy(), rows)
    short = dz.clone()
    short[-1, -1, -1] = 0                               # the last output pixel dropped
    with pytest.raises(AssertionError):
        T.check_wgrad(f32(x, short), dw.numpy(), rows)
    with pytest.raises(AssertionError):
        T.check_wgrad(f32(x, g), dw.numpy(), rows)      # the activation backward not folded in
