"""The case table of the K28 / K29 envelope tests (test_igemm_envelope_cpu.py, test_gpu_igemm_envelope.py), a Python
mirror of the dispatch arithmetic of csrc/igemm.hip (ig_shape, wg_shape, the slab rule of xpa_conv_wgrad), the float64
references and the comparison helpers.  Plain data and host arithmetic: no device, no library call."""
import functools
from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F

# ---- the mirror of csrc/igemm.hip ------------------------------------------------------------------------------------
IG_LDS_FLOATS = 40960     # kIgLdsFloats: K28's weight image
IG_ROWS = 512             # kIgRows: rows per K28 block step (K28B: 8 x 32 x MT, MT = 2 | 3)
IG_GRID = 256             # kIgGrid
WS_FLOATS = 19456         # kWsFloats: K29's slab
WG_GRID = 512             # kWgGrid


def ig_shape(cin, cout, k):
    """(CINP, NT) of K28 for a GEMM with cin input and cout output channels, None where it is not taken."""
    if cin < 1 or cin > 64 or cout < 1 or cout > 64 or k < 1 or cin % 4:
        return None
    cinp = 8 if cin <= 8 else 16 if cin <= 16 else 32 if cin <= 32 else 64
    nt = 1 if cout <= 32 else 2
    return (cinp, nt) if k * k * cinp * 32 * nt <= IG_LDS_FLOATS else None


def wg_shape(cin, cout, k):
    """(TN, TC, waves) of K29, None where it is not taken."""
    if cin < 1 or cout < 1 or cout > 64 or k < 1 or k * k * cin > 576:
        return None
    tn = 1 if cout <= 16 else 2 if cout <= 32 else 4
    nct = (k * k * cin + 15) // 16
    tc = (nct + 3) // 4
    tc = 2 if tc <= 2 else 4 if tc <= 4 else 8 if tc <= 8 else 9
    waves = (nct + tc - 1) // tc
    return (tn, tc, waves) if waves <= 4 else None


def _ws_pad(need, step):
    for c in range(need, need + 64, 4):
        if (step * c) % 64 in (16, 48):
            return c
    return need


def wg_form(c, force_stream=False):
    """K29's form for case c with 16-byte aligned operands: ("slab", R, slabs per image) or ("stream",)."""
    OH, OW = out_hw(c)
    if force_stream or c.cin % 4 or c.cout % 4:
        return ("stream",)
    tn = wg_shape(c.cin, c.cout, c.k)[0]
    PW, CS, COUTS = (OW - 1) * c.s + c.k, _ws_pad(c.cin, c.s), _ws_pad(16 * tn, 1)

    def floats(r):
        return ((((r - 1) * c.s + c.k) * PW * CS + 3) & ~3) + ((r * OW + 3) & ~3) * COUTS
    r = OH
    while r >= 1 and floats(r) > WS_FLOATS:
        r -= 1
    if r < 1:
        return ("stream",)
    nsl = (OH + r - 1) // r
    return ("slab", (OH + nsl - 1) // nsl, nsl)


# ---- the cases -------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    B: int
    H: int
    W: int
    cin: int
    cout: int
    k: int
    s: int
    p: int
    act: int = 1             # the block's activation: 0 identity, 1 leaky (slope), 2 tanh
    slope: float = 0.0
    prev: int = None         # dgrad: the previous block's activation code (-1: none); None: act
    prev_bias: bool = True   # dgrad: bias partials asked for

    @property
    def id(self):
        return "%dx%dx%dx%d-%d_k%ds%dp%d_a%d" % self[:9]


def out_hw(c):
    return (c.H + 2 * c.p - c.k) // c.s + 1, (c.W + 2 * c.p - c.k) // c.s + 1


def fwd_rows(c):
    OH, OW = out_hw(c)
    return c.B * OH * OW


def dgrad_rows(c):
    return c.B * c.H * c.W


def dgrad_admitted(c):
    """What conv_facts asks of K28's data gradient."""
    return c.s <= 2 and c.cout % 4 == 0 and ig_shape(c.cout, c.cin, c.k) is not None


def dgrad_prev(c):
    return c.act if c.prev is None else c.prev


# forward and, where admitted, the data gradient
K28_CASES = [
    Case(3, 9, 13, 12, 16, 3, 1, 1, 2),                       # CINP 16 (cin 12), NT 1, H != W; dgrad CINP 16 -> 12
    Case(2, 12, 7, 16, 48, 3, 2, 0, 1, 0.01),                 # CINP 16, NT 2 (cout 48), s 2, p 0, a dead last row
    Case(2, 8, 10, 20, 32, 2, 1, 1, 0, prev=-1, prev_bias=False),   # CINP 32 (cin 20), NT 1 at 32; dgrad bare
    Case(2, 7, 9, 32, 36, 3, 1, 2, 0),                        # NT 2 (cout 36), p > k // 2; dgrad CINP 64 from 36
    Case(2, 6, 6, 44, 16, 1, 1, 0, 1, 0.01),                  # CINP 64 (cin 44), 1 x 1; dgrad CINP 16, NT 2
    Case(2, 5, 5, 8, 8, 1, 1, 0, 2),                          # one chunk per row block
    Case(1, 1, 1, 4, 1, 1, 1, 0, 1),                          # one row, one output channel
    Case(2, 9, 13, 12, 5, 3, 1, 1, 2),                        # forward only: cout % 4 != 0
    Case(2, 10, 9, 8, 8, 4, 2, 3, 1, 0.01),                   # stride-2 dgrad, p 3
    Case(2, 6, 7, 8, 40, 3, 2, 1, 0, prev=2),                 # CINP 8, NT 2; dgrad CINP 64, NT 1, tanh
    Case(2, 6, 7, 40, 8, 3, 1, 1, 1, 0.01),                   # CINP 64, NT 1; dgrad CINP 8, NT 2
    Case(2, 5, 6, 36, 24, 2, 2, 0, 2, prev=-1),               # dgrad CINP 32, NT 2, stride 2, bare with partials
    Case(8, 211, 213, 4, 8, 3, 1, 1, 1),                      # 359 544 rows: two or three row blocks per workgroup
    Case(8, 211, 213, 8, 4, 3, 1, 1, 1),                      # its mirror for the dgrad, with bias partials
    Case(30, 96, 97, 64, 64, 1, 1, 0, 1),                     # 279 360 rows at CINP 64 / NT 2; past K28B's 768 x 256
]

# weight gradient: both forms where the slab form applies, fold_act on (act) and off (-1)
K29_CASES = [
    Case(3, 9, 13, 12, 20, 3, 1, 1, 2),                       # TN 2, TC 2, 4 waves
    Case(2, 8, 10, 8, 5, 2, 1, 1, 1, 0.01),                   # cout 5: stream by rule; 1 wave
    Case(2, 7, 9, 16, 36, 3, 1, 2, 0),                        # TN 4 (cout 36), TC 4, 3 waves
    Case(2, 6, 8, 60, 16, 3, 1, 0, 1, 0.01),                  # TC 9, ragged last tile
    Case(2, 9, 7, 28, 8, 4, 2, 1, 2),                         # TC 8, last wave half empty
    Case(2, 5, 3, 8, 8, 3, 1, 1, 1),                          # OW 3
    Case(4, 6, 1, 4, 4, 3, 1, 1, 0),                          # OW 1
    Case(1, 3, 200, 64, 64, 3, 1, 1, 1, 0.01),                # no one-row slab fits: stream without the switch
    Case(2, 11, 10, 8, 12, 3, 3, 1, 2),                       # stride 3
    Case(1, 20, 24, 32, 16, 3, 1, 1, 1),                      # two slabs per image; TC 8, 3 waves
    Case(2, 6, 5, 4, 24, 2, 1, 0, 1, 0.01),                   # 16 columns: one tile, 1 wave of TC 2; TN 2
]


# ---- operands and float64 references ---------------------------------------------------------------------------------
def act64(z, code, slope):
    if code == 1:
        return torch.where(z > 0, z, z * float(np.float32(slope)))
    return torch.tanh(z) if code == 2 else z


def grad64(y, code, slope):
    """d act / d z from the activation's OUTPUT y, as the kernels form it."""
    if code == 1:
        return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, float(np.float32(slope))))
    return 1.0 - y * y if code == 2 else torch.ones_like(y)


def act_output(z, code, slope):
    """An f32 tensor that is a possible output of activation `code`: negative values under leaky, (-1, 1) under tanh."""
    return act64(z.double(), code, slope).float()


def operands(c, seed):
    """x (NHWC), w (torch layout, random normal so that a swapped tap or channel shows) and bias, f32."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(c.B, c.H, c.W, c.cin, generator=g)
    w = torch.randn(c.cout, c.cin, c.k, c.k, generator=g) / np.sqrt(c.cin * c.k * c.k)
    b = torch.randn(c.cout, generator=g) * 0.5
    return x, w, b


def conv_nhwc(x, w, b, c):
    return F.conv2d(x.permute(0, 3, 1, 2), w, b, c.s, c.p).permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def fwd_reference(c):
    """(x, w, b) f32 and the f64 act(conv(x, w) + b), NHWC."""
    x, w, b = operands(c, 11)
    ref = act64(conv_nhwc(x.double(), w.double(), b.double(), c), c.act, c.slope)
    return x, w, b, ref


@functools.lru_cache(maxsize=None)
def dgrad_reference(c):
    """(dz, w, y_prev) f32 and f64 dX * act_prev'(y_prev), its column sums and the column sums of its magnitude."""
    _, w, _ = operands(c, 12)
    OH, OW = out_hw(c)
    g = torch.Generator().manual_seed(13)
    dz = torch.randn(c.B, OH, OW, c.cout, generator=g)
    prev = dgrad_prev(c)
    y_prev = act_output(torch.randn(c.B, c.H, c.W, c.cin, generator=g), max(prev, 0), c.slope)
    xr = torch.zeros(c.B, c.cin, c.H, c.W, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, w.double(), None, c.s, c.p).backward(dz.double().permute(0, 3, 1, 2))
    dx = xr.grad.permute(0, 2, 3, 1).contiguous()
    if prev >= 0:
        dx = dx * grad64(y_prev.double(), prev, c.slope)
    return dz, w, y_prev, dx, dx.sum((0, 1, 2)), dx.abs().sum((0, 1, 2))


@functools.lru_cache(maxsize=None)
def wgrad_reference(c, fold_act):
    """(x, g, y) f32, f64 dW of dz = g * act'(y) (fold_act) or g, and dz's column sums."""
    x, w, _ = operands(c, 14)
    OH, OW = out_hw(c)
    gen = torch.Generator().manual_seed(15)
    g = torch.randn(c.B, OH, OW, c.cout, generator=gen)
    y = act_output(torch.randn(c.B, OH, OW, c.cout, generator=gen), c.act, c.slope)
    dz = g.double() * grad64(y.double(), c.act, c.slope) if fold_act else g.double()
    wr = w.double().clone().requires_grad_(True)
    F.conv2d(x.double().permute(0, 3, 1, 2), wr, None, c.s, c.p).backward(dz.permute(0, 3, 1, 2))
    return x, g, y, wr.grad, dz.sum((0, 1, 2))


# ---- the comparisons: the tolerances of test_gpu_igemm.py ------------------------------------------------------------
def check_fwd(got, ref):
    """Forward output or dX against f64: atol 2e-6 max(scale, 1), every element finite."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    np.testing.assert_allclose(got, ref, rtol=0, atol=2e-6 * max(scale, 1.0))


def check_dgrad_bias(got, ref, abs_sums):
    np.testing.assert_allclose(np.asarray(got, dtype=np.float64), np.asarray(ref), rtol=1e-5,
                               atol=1e-5 * float(np.asarray(abs_sums).max()))


def check_wgrad(got, ref, rows):
    ref = np.asarray(ref, dtype=np.float64)
    np.testing.assert_allclose(np.asarray(got, dtype=np.float64), ref, rtol=1e-5,
                               atol=2e-6 * float(np.abs(ref).max()) + 1e-6 * rows ** 0.5)


def check_wgrad_bias(got, ref, rows):
    np.testing.assert_allclose(np.asarray(got, dtype=np.float64), np.asarray(ref), rtol=1e-5, atol=1e-5 * rows ** 0.5)
