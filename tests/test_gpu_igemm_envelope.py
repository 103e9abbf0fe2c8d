"""GPU: K28 / K28B / K29 (csrc/igemm.hip) against float64 torch convolutions over the envelope their dispatch admits:
the case table of tests/_igemm_cases.py (every (CINP, NT) pair in both modes, every TN / TC / wave count and both K29
forms, padded channel counts, all four activation codes, H != W, p = 0 and p > k // 2, 1 x 1, OW < 4, stride 3, and
K28's persistent loop over several row blocks per workgroup; test_igemm_envelope_cpu.py asserts that coverage).

Every operand and every output of a launch is a 16-byte aligned view into ONE allocation filled with NaN, with guard
rows between them: an output element the kernel does not write stays NaN, a read outside an operand that reaches the
arithmetic turns the result NaN, and after the launch every byte outside the outputs must be bit-unchanged (the
canaries, the operands, and — for a data gradient without bias partials — everything but dX)."""
import numpy as np
import pytest
import torch

from tests import _igemm_cases as T

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(params=[1, 3, 0], ids=["k28b", "k28b_mt3", "k28"])
def ig_form(request):
    """As test_gpu_igemm.py: K28B (bf16 matrix cores; falls back to K28 where the GEMM's input channels are not an
    unpadded multiple of 16), its 3-tile waves (forward only), and the fp32-MFMA K28."""
    from xuanpolicy_amd import ops
    L = ops.lib()
    prev = L.xpa_conv_igemm_form(-1)
    L.xpa_conv_igemm_form(request.param)
    yield request.param
    L.xpa_conv_igemm_form(prev)


class Arena:
    """Named f32 blocks in one NaN-filled device allocation: inputs copied in, outputs left NaN; every block starts
    16-byte aligned with at least two of its own rows (and 64 floats) of guard on either side."""

    def __init__(self):
        self.spec, self.n = {}, 0

    def add(self, name, shape, data=None):
        numel = int(np.prod(shape))
        guard = (2 * int(shape[-1]) + 64 + 3) & ~3
        start = self.n + guard
        self.spec[name] = (start, numel, tuple(shape), data)
        self.n = (start + numel + guard + 3) & ~3

    def build(self):
        self.buf = torch.full((self.n,), float("nan"), device=DEV)
        for name, (start, numel, shape, data) in self.spec.items():
            if data is not None:
                self.buf[start:start + numel].copy_(data.reshape(-1))
        self.before = self.buf.view(torch.int32).clone()
        assert self.buf.data_ptr() % 16 == 0
        return self

    def __getitem__(self, name):
        start, numel, shape, _ = self.spec[name]
        return self.buf[start:start + numel].view(shape)

    def assert_only_written(self, *outputs):
        """Everything outside the named blocks is bit-identical to what it was before the launch."""
        keep = torch.ones(self.n, dtype=torch.bool, device=DEV)
        for name in outputs:
            start, numel, _, _ = self.spec[name]
            keep[start:start + numel] = False
        changed = (self.buf.view(torch.int32) != self.before) & keep
        assert not bool(changed.any()), "written outside %s at float offsets %s" % (
            outputs, changed.nonzero().flatten()[:8].tolist())


def _p(t):
    from xuanpolicy_amd import ops
    return ops._p(t)


def _finalize(L, part, G, cols, shape):
    from xuanpolicy_amd import _lib, ops
    out = torch.full((cols,), float("nan"), device=DEV)
    _lib.check(L.xpa_colsum_finalize(_p(part), G, cols, _p(out), ops._stream(DEV)), "xpa_colsum_finalize")
    return out.view(shape).cpu().numpy()


@pytest.mark.parametrize("c", T.K28_CASES, ids=lambda c: c.id)
def test_conv_fwd_envelope(c, ig_form):
    from xuanpolicy_amd import _lib, ops
    L = ops.lib()
    x, w, b, ref = T.fwd_reference(c)
    OH, OW = T.out_hw(c)
    a = Arena()
    a.add("x", x.shape, x)
    a.add("w", w.shape, w)
    a.add("b", b.shape, b)
    a.add("y", (c.B, OH, OW, c.cout))
    a.build()
    assert L.xpa_conv_igemm_ok(c.cin, c.cout, c.k)
    _lib.check(L.xpa_conv_fwd(c.act, _p(a["x"]), c.B, c.H, c.W, c.cin, _p(a["w"]), _p(a["b"]), c.cout, c.k, c.s, c.p,
                              c.slope, _p(a["y"]), ops._stream(DEV)), "xpa_conv_fwd")
    torch.cuda.synchronize()
    a.assert_only_written("y")
    if c.act == 1 and c.slope:
        assert float(ref.min()) < 0          # the leaky branch is taken
    T.check_fwd(a["y"].cpu().numpy(), ref.numpy())


@pytest.mark.parametrize("c", [c for c in T.K28_CASES if T.dgrad_admitted(c)], ids=lambda c: c.id)
def test_conv_dgrad_envelope(c, ig_form):
    """dX from dZ times act_prev'(y_prev), and the previous block's bias gradient from the partials; with act_prev -1
    and no partials, nothing but dX is written."""
    from xuanpolicy_amd import _lib, ops
    L = ops.lib()
    dz, w, y_prev, dx_ref, db_ref, db_abs = T.dgrad_reference(c)
    prev = T.dgrad_prev(c)
    OH, OW = T.out_hw(c)
    G = int(L.xpa_conv_dgrad_num_partials(c.B, c.H, c.W))
    assert G == min((T.dgrad_rows(c) + T.IG_ROWS - 1) // T.IG_ROWS, T.IG_GRID)
    a = Arena()
    a.add("dz", dz.shape, dz)
    a.add("w", w.shape, w)
    if prev >= 0:
        a.add("y_prev", y_prev.shape, y_prev)
    a.add("dx", (c.B, c.H, c.W, c.cin))
    if c.prev_bias:
        a.add("part", (G, c.cin))
    a.build()
    if prev == 1 and c.slope:
        assert float(y_prev.min()) < 0
    if prev == 2:
        assert float(y_prev.abs().max()) < 1 and float(y_prev.min()) < 0
    _lib.check(L.xpa_conv_dgrad(_p(a["dz"]), c.B, OH, OW, c.cout, _p(a["w"]), c.cin, c.k, c.s, c.p, c.H, c.W, prev,
                                _p(a["y_prev"]) if prev >= 0 else None, c.slope, _p(a["dx"]),
                                _p(a["part"]) if c.prev_bias else None, ops._stream(DEV)), "xpa_conv_dgrad")
    torch.cuda.synchronize()
    a.assert_only_written(*(("dx", "part") if c.prev_bias else ("dx",)))
    T.check_fwd(a["dx"].cpu().numpy(), dx_ref.numpy())
    if c.prev_bias:
        assert bool(torch.isfinite(a["part"]).all())
        T.check_dgrad_bias(_finalize(L, a["part"], G, c.cin, (c.cin,)), db_ref.numpy(), db_abs.numpy())
        a.assert_only_written("dx", "part")     # the finalize reads the partials only


# each case in the form K29 picks for it and, where that is the slab form, in the forced streaming one too
WGRAD_RUNS = [(c, form) for c in T.K29_CASES for form in ("auto", "stream")
              if form == "auto" or T.wg_form(c)[0] == "slab"]


@pytest.mark.parametrize("c,form", WGRAD_RUNS, ids=lambda v: v if isinstance(v, str) else v.id)
@pytest.mark.parametrize("fold_act", [False, True], ids=["bare", "fold"])
def test_conv_wgrad_envelope(c, form, fold_act):
    """dW (and, with the activation folded in, the bias gradient) in K29's own choice of form and in the forced
    streaming one."""
    from xuanpolicy_amd import _lib, ops
    L = ops.lib()
    x, g, y, dw_ref, db_ref = T.wgrad_reference(c, fold_act)
    OH, OW = T.out_hw(c)
    rows, cols = T.fwd_rows(c), c.cout * c.cin * c.k * c.k
    G = int(L.xpa_conv_wgrad_num_partials())
    assert G == T.WG_GRID and L.xpa_conv_wgrad_ok(c.cin, c.cout, c.k)
    a = Arena()
    a.add("x", x.shape, x)
    a.add("g", g.shape, g)
    if fold_act:
        a.add("y", y.shape, y)
        a.add("bpart", (G, c.cout))
    a.add("part", (G, cols))
    a.build()
    if fold_act and c.act == 1 and c.slope:
        assert float(y.min()) < 0
    if fold_act and c.act == 2:
        assert float(y.abs().max()) < 1 and float(y.min()) < 0
    L.xpa_conv_wgrad_force_stream(1 if form == "stream" else 0)
    try:
        _lib.check(L.xpa_conv_wgrad(c.act if fold_act else -1, _p(a["g"]), _p(a["y"]) if fold_act else None, c.slope,
                                    _p(a["x"]), c.B, c.H, c.W, c.cin, c.cout, c.k, c.s, c.p, _p(a["part"]),
                                    _p(a["bpart"]) if fold_act else None, ops._stream(DEV)), "xpa_conv_wgrad")
    finally:
        L.xpa_conv_wgrad_force_stream(0)
    torch.cuda.synchronize()
    a.assert_only_written(*(("part", "bpart") if fold_act else ("part",)))
    assert bool(torch.isfinite(a["part"]).all())
    T.check_wgrad(_finalize(L, a["part"], G, cols, (c.cout, c.cin, c.k, c.k)), dw_ref.numpy(), rows)
    if fold_act:
        assert bool(torch.isfinite(a["bpart"]).all())
        T.check_wgrad_bias(_finalize(L, a["bpart"], G, c.cout, (c.cout,)), db_ref.numpy(), rows)


def test_k29_refuses_what_its_predicate_refuses():
    """Conv2d(32, 32, 5) and Conv2d(16, 16, 8): K28's weight image fits, K29's 36 column tiles do not — refused by the
    predicate, by the entry point before any launch, and so never planned."""
    import ctypes
    from xuanpolicy_amd import ops
    L = ops.lib()
    P = ctypes.c_void_p(256)
    for cin, cout, k in ((32, 32, 5), (16, 16, 8)):
        assert L.xpa_conv_igemm_ok(cin, cout, k) and not L.xpa_conv_wgrad_ok(cin, cout, k)
        assert L.xpa_conv_wgrad(-1, P, None, 0.0, P, 1, 16, 16, cin, cout, k, 1, 0, P, None, None) == 1
