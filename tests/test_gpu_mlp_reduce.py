"""GPU: csrc/mlp.hip against f64 at every kernel form — K10 (xpa_act_bwd_colsum), K11 (xpa_head_backward) and the
column-sum finalizes (xpa_colsum_finalize, _batch, _batch_sq, _batch_map with and without the loss block).

tests/test_gpu_fused_mlp.py keeps its own, looser tests (K10's finalized sums at five shapes to 1e-3, the batched finalize
against the single one, the queue's deferred loss finalize); K11 ran only inside test_explicit_backward_matches_autograd.
This module covers the rest, through the C ABI on plain tensors with its own sq and ticket buffers:

  B1. K10: act x rows x C over both kernels (vec4 at C/4 = 1, 3, 64, 75, 256; scalar with one chunk and with a second chunk
      of 1, 4, 44 and 256 columns), dz in place / separate / null, act 0 with h null, each pointer misaligned in turn:
      every per-block partial, the partial count, dz elementwise, dh untouched, guards intact, +-0 in h.
  B2. K11: the thinned product of tests/_mlp_reduce_ref.py (every template instance x act x {full, ragged block}; ldd = K
      and K + 3 with NaN beside the slice; p_dbo null; the misaligned fallback): dz and every per-block partial; the
      argument checks.
  B3. The finalizes against f64 on inputs whose f32 running sum is outside the bound (tests/test_mlp_reduce_ref_cpu.py):
      the single entry at every unroll remainder, the batched entry on the form boundaries and tile edges (bit-equal to
      the single one), the queue at 17 and 33 segments, the output map (ld > valid, dropped columns, with sq), the norm
      partials and the two-level tickets at 1 .. 1100 tiles, two launches back to back, and the loss block.

Reference and bounds: tests/_mlp_reduce_ref.py (derived there; nothing fitted here).  Each check prints the largest
|err| / bound it saw before it asserts.

Measured on an MI355X, the largest |err| / bound per set:
  K10   partials 0.37, dz 0.99 (leaky: the one rounding the bound allows)
  K11   dz 0.36, p_dw 0.20, p_dbh 0.16, p_dbo 0.03.  Held to the plain reduction bound over |dz ref|, p_dbh was outside
        it by up to 26x in blocks of one row (rows 1 and 129), where it equals dz bit for bit and so carries the K-term
        dot's error: the bound's derivation was short there, not the kernel (see _mlp_reduce_ref.py); one-row blocks are
        now also held to that bit equality
  finalize outputs 0.99 everywhere (one rounding of the f64 sum); sq partials 0.04, totals 0.006
No kernel or queue defect was found: every bound and every bit equality held at every case.  With mlp.hip's f64
accumulators turned to f32, the leaky mask to h >= 0, sq[0] left out of the total and dropped map columns counted, 68 of
the 158 cases failed: every finalize test and every leaky case of K10 and K11.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import _mlp_reduce_ref as mr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
INVALID = 1     # hipErrorInvalidValue


@pytest.fixture(scope="module", autouse=True)
def _setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from xuanpolicy_amd import ops
    ops.lib()


def _L():
    from xuanpolicy_amd import ops
    return ops.lib()


def _call(name, *args):
    from xuanpolicy_amd import _lib
    _lib.call(getattr(_L(), name), *args)


def _p(t):
    from xuanpolicy_amd import ops
    return ops._p(t)


def _stream():
    from xuanpolicy_amd import ops
    return ops._stream(DEV)


class Buf:
    """A flat f32 device buffer of n elements inside sentinel-filled guards: `off` elements in front (off = 1: a view
    offset by one float, 4-byte aligned only) and `guard` behind."""

    def __init__(self, n, guard=64, off=0, fill=None):
        self.n, self.off = n, off
        self.full = torch.full((off + n + guard,), mr.SENTINEL, dtype=torch.float32, device=DEV)
        self.t = self.full[off:off + n]
        assert self.t.data_ptr() % 16 == (4 * off) % 16
        if fill is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(fill, np.float32).reshape(-1)))

    @property
    def ptr(self):
        return _p(self.t)

    def get(self, shape=None):
        a = self.t.cpu().numpy()
        return a if shape is None else a.reshape(shape)

    def guards_intact(self):
        f = self.full.cpu().numpy()
        return bool((f[:self.off] == mr.SENTINEL).all() and (f[self.off + self.n:] == mr.SENTINEL).all())

    def untouched(self):
        return bool((self.full == mr.SENTINEL).all())


def within(got, ref, bound, what):
    err = np.abs(np.asarray(got, np.float64) - ref)
    assert np.isfinite(err).all(), what
    pos = bound > 0
    worst = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    print("%s: max |err| / bound = %.3g" % (what, worst))
    bad = err > bound
    assert not bad.any(), "%s: %d of %d outside the bound, worst |err| / bound %.3g, first at %s" % (
        what, int(bad.sum()), bad.size, worst, np.argwhere(bad)[0].tolist())


# ---- B1. K10 --------------------------------------------------------------------------------------------------------------
def run_k10(act, rows, C, mode, unaligned=()):
    """mode: "inplace" | "separate" | "null" (act != 0), "h-null" | "h-given" (act 0, dz passed and never written).
    unaligned: which of dh, h, dz, partials sit on a view offset by one float."""
    L = _L()
    rng = np.random.default_rng([act, rows, C, len(mode), len(unaligned)])
    dh = rng.standard_normal((rows, C)).astype(np.float32)
    h = mr.hidden_values(act, (rows, C), rng)
    dz_ref, dz_b, p_ref, p_b = mr.k10_ref(act, dh, h)
    G = int(L.xpa_act_bwd_num_partials(rows))
    assert G == -(-rows // mr.K10_ROWS_PER_BLOCK) == p_ref.shape[0]
    b_dh = Buf(rows * C, 2 * C, int("dh" in unaligned), fill=dh)
    b_h = None if mode == "h-null" else Buf(rows * C, 2 * C, int("h" in unaligned), fill=h)
    b_dz = None if mode in ("inplace", "null") else Buf(rows * C, 2 * C, int("dz" in unaligned))
    b_p = Buf(G * C, 2 * C, int("partials" in unaligned))
    dz_ptr = b_dh.ptr if mode == "inplace" else None if mode == "null" else b_dz.ptr
    _call("xpa_act_bwd_colsum", act, b_dh.ptr, None if b_h is None else b_h.ptr, rows, C, mr.SLOPE, dz_ptr, b_p.ptr,
          _stream())
    torch.cuda.synchronize()
    what = "K10 act %d rows %d C %d %s %s" % (act, rows, C, mode, "/".join(unaligned))
    within(b_p.get((G, C)), p_ref, p_b, what + " partials")
    assert b_p.guards_intact() and b_dh.guards_intact(), what
    if mode == "inplace":
        within(b_dh.get((rows, C)), dz_ref, dz_b, what + " dz")
    else:
        assert np.array_equal(b_dh.get((rows, C)), dh), what + ": dh written"
    if mode == "separate":
        within(b_dz.get((rows, C)), dz_ref, dz_b, what + " dz")
        assert b_dz.guards_intact(), what
    elif b_dz is not None:
        assert b_dz.untouched(), what + ": act 0 stores no dz"
    if b_h is not None:
        assert np.array_equal(b_h.get((rows, C)), h) and b_h.guards_intact(), what
    if act == 1:    # the planted zeros took the slope branch, whatever their sign
        got = (b_dh if mode == "inplace" else b_dz).get((rows, C)) if mode != "null" else None
        z = (h == 0)
        assert z.any()
        if got is not None:
            assert np.array_equal(got[z], (dh[z].astype(np.float64) * mr.SLOPE).astype(np.float32)), what


def _k10_modes(act):
    return ("h-null", "h-given") if act == 0 else ("inplace", "separate", "null")


@pytest.mark.parametrize("C", mr.K10_COLS)
@pytest.mark.parametrize("act", mr.K10_ACTS)
def test_k10_partials_and_dz_match_f64(act, C):
    for rows in mr.K10_ROWS:
        for mode in _k10_modes(act):
            run_k10(act, rows, C, mode)


@pytest.mark.parametrize("C", mr.K10_UNALIGNED_COLS)
@pytest.mark.parametrize("act", mr.K10_ACTS)
def test_k10_alignment_fallback(act, C):
    """A vec4 width on pointers that are only 4-byte aligned runs the scalar kernel: each pointer in turn, then all."""
    ptrs = ("dh", "partials") if act == 0 else ("dh", "h", "dz", "partials")
    mode = "h-given" if act == 0 else "separate"
    for un in [(p,) for p in ptrs] + [ptrs]:
        for rows in (65, 130):
            run_k10(act, rows, C, mode, un)
    if act != 0:
        run_k10(act, 130, C, "inplace", ("dh",))
        run_k10(act, 130, C, "null", ("h",))


def test_k10_argument_checks():
    L = _L()
    dh, h, p = Buf(64 * 4, fill=np.ones((64, 4))), Buf(64 * 4, fill=np.ones((64, 4))), Buf(4)
    s = _stream()
    assert L.xpa_act_bwd_colsum(3, dh.ptr, h.ptr, 64, 4, mr.SLOPE, None, p.ptr, s) == INVALID
    assert L.xpa_act_bwd_colsum(1, dh.ptr, None, 64, 4, mr.SLOPE, None, p.ptr, s) == INVALID
    assert L.xpa_act_bwd_colsum(0, dh.ptr, None, 0, 4, mr.SLOPE, None, p.ptr, s) == INVALID
    assert L.xpa_act_bwd_colsum(0, dh.ptr, None, 64, 0, mr.SLOPE, None, p.ptr, s) == INVALID
    torch.cuda.synchronize()
    assert p.untouched()


# ---- B2. K11 --------------------------------------------------------------------------------------------------------------
def _k11_buffers(c, rng):
    rows, H, K, ldd = c["rows"], c["H"], c["K"], c["ldd"]
    d = (0.1 * rng.standard_normal((rows, K))).astype(np.float32)
    h = mr.hidden_values(c["act"], (rows, H), rng)
    w = (rng.standard_normal((K, H)) / np.sqrt(H)).astype(np.float32)
    wide = np.full((rows, ldd), np.nan, np.float32)     # NaN beside the slice: reading past K shows everywhere
    c0 = ldd - K - 1 if ldd > K else 0
    wide[:, c0:c0 + K] = d
    t_wide = torch.from_numpy(wide).to(DEV)
    G = -(-rows // mr.K11_ROWS_PER_BLOCK)
    bufs = dict(h=Buf(rows * H, 2 * H, 0 if c["aligned"] else 1, fill=h), w=Buf(K * H, fill=w), dz=Buf(rows * H, 2 * H),
                p_dw=Buf(G * K * H, K * H), p_dbh=Buf(G * H, H), p_dbo=Buf(G * K, K) if c["dbo"] else None)
    return d, h, w, t_wide, t_wide[:, c0:c0 + K], G, bufs


@pytest.mark.parametrize("c", mr.k11_cases(), ids=mr.k11_id)
def test_k11_dz_and_partials_match_f64(c):
    L = _L()
    rng = np.random.default_rng([11, c["act"], c["rows"], c["H"], c["K"], c["ldd"]])
    d, h, w, t_wide, t_d, G, b = _k11_buffers(c, rng)
    rows, H, K = c["rows"], c["H"], c["K"]
    assert int(L.xpa_head_bwd_num_partials(rows)) == G and t_d.stride(0) == c["ldd"]
    _call("xpa_head_backward", c["act"], K, _p(t_d), t_d.stride(0), b["h"].ptr, b["w"].ptr, rows, H, mr.SLOPE, b["dz"].ptr,
          b["p_dw"].ptr, b["p_dbh"].ptr, None if b["p_dbo"] is None else b["p_dbo"].ptr, _stream())
    torch.cuda.synchronize()
    ref = mr.k11_ref(c["act"], d, h, w)
    what = "K11 " + mr.k11_id(c)
    within(b["dz"].get((rows, H)), ref["dz"], ref["dz_bound"], what + " dz")
    within(b["p_dw"].get((G, K, H)), ref["p_dw"], ref["p_dw_bound"], what + " p_dw")
    within(b["p_dbh"].get((G, H)), ref["p_dbh"], ref["p_dbh_bound"], what + " p_dbh")
    if c["dbo"]:
        within(b["p_dbo"].get((G, K)), ref["p_dbo"], ref["p_dbo_bound"], what + " p_dbo")
    for name, buf in b.items():
        assert buf is None or buf.guards_intact(), what + ": guard of " + name
    assert np.array_equal(b["h"].get((rows, H)), h) and np.array_equal(b["w"].get((K, H)), w)
    if rows % mr.K11_ROWS_PER_BLOCK == 1:     # a block of one row: its sums have one term each, so they are that term
        assert np.array_equal(b["p_dbh"].get((G, H))[-1], b["dz"].get((rows, H))[-1]), what
        if c["dbo"]:
            assert np.array_equal(b["p_dbo"].get((G, K))[-1], d[-1]), what
    if c["act"] == 1:     # +-0 in h: the reference takes the slope branch there, and dz was held to it above
        assert (h == 0).any()


def test_k11_argument_checks():
    L = _L()
    rows, H = 130, 64
    rng = np.random.default_rng(5)
    d = torch.from_numpy(rng.standard_normal((rows, 40)).astype(np.float32)).to(DEV)
    h, w = Buf(rows * H, fill=rng.standard_normal((rows, H))), Buf(40 * H, fill=rng.standard_normal((40, H)))
    outs = [Buf(rows * H), Buf(2 * 40 * H), Buf(2 * H), Buf(2 * 40)]
    s = _stream()

    def rc(act, k, ldd):
        return L.xpa_head_backward(act, k, _p(d), ldd, h.ptr, w.ptr, rows, H, mr.SLOPE, outs[0].ptr, outs[1].ptr,
                                   outs[2].ptr, outs[3].ptr, s)
    assert rc(1, 33, 40) == INVALID      # K > 32
    assert rc(1, 6, 5) == INVALID        # ldd < K
    assert rc(3, 6, 40) == INVALID       # no such activation
    assert rc(1, 0, 40) == INVALID
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs)


# ---- B3. the finalizes ------------------------------------------------------------------------------------------------------
def _part(G, C, seed=0):
    x = mr.finalize_input(G, C, seed)
    return x, torch.from_numpy(x).to(DEV)


def _seg_args(parts, segs, outs):
    n = len(segs)
    keep = ((ctypes.c_void_p * n)(*[p.data_ptr() for p in parts]), (ctypes.c_int64 * n)(*[g for g, _ in segs]),
            (ctypes.c_int64 * n)(*[c for _, c in segs]), (ctypes.c_void_p * n)(*[o.t.data_ptr() for o in outs]))
    return keep, [ctypes.cast(a, ctypes.c_void_p) for a in keep]


def _tmap_arg(tmaps):
    arr = (ctypes.c_int64 * (3 * len(tmaps)))(*[v for tm in tmaps for v in (tm or (0, 0, 0))])
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def _single(t_part, G, C):
    out = Buf(C)
    _call("xpa_colsum_finalize", _p(t_part), G, C, out.ptr, _stream())
    return out


def _sq_buf(tiles, sq0):
    """tiles + 2 doubles in use, 2 guard doubles; the partial slots start at -1 (a sum of squares never is)."""
    sq = torch.full((tiles + 4,), -1.0, dtype=torch.float64, device=DEV)
    sq[0] = sq0
    return sq


def _ticket():
    from xuanpolicy_amd import _lib
    return torch.zeros((_lib.COLSUM_TICKET_INTS,), dtype=torch.int32, device=DEV)


def _check_sq(sq, segs, outs_by_col, tmaps, sq0, what):
    tiles = len(mr.tile_spans(segs))
    got = sq.cpu().numpy()
    if sq0 is not None:
        assert got[0] == sq0, what + ": sq[0] changed"
    refs, bounds = mr.sq_tile_refs(segs, outs_by_col, tmaps)
    err = np.abs(got[1:1 + tiles] - refs)
    print("%s: sq partials max |err| / bound = %.3g" % (what, float((err / np.maximum(bounds, 1e-300)).max())))
    assert (err <= bounds).all(), "%s: sq partial of tile %d" % (what, int(np.argmax(err > bounds)))
    tot, tot_b = mr.sq_total_ref(got, tiles)
    print("%s: total |err| / bound = %.3g" % (what, abs(got[1 + tiles] - tot) / tot_b))
    assert abs(got[1 + tiles] - tot) <= tot_b, what + ": total"
    assert (got[2 + tiles:] == -1.0).all(), what + ": sq guard"


def test_single_finalize_matches_f64():
    for G, C in mr.single_cases():
        x, t = _part(G, C)
        out = _single(t, G, C)
        torch.cuda.synchronize()
        ref, bound = mr.finalize_ref(x)
        within(out.get(), ref, bound, "finalize G %d C %d" % (G, C))
        assert out.guards_intact()


@pytest.mark.parametrize("i", range(len(mr.batch_launches())))
def test_batched_finalize_matches_f64_and_the_single_entry(i):
    segs = mr.batch_launches()[i]
    xs, parts = zip(*[_part(G, C) for G, C in segs])
    outs = [Buf(C) for _, C in segs]
    keep, args = _seg_args(parts, segs, outs)
    _call("xpa_colsum_finalize_batch", len(segs), *args, _stream())
    singles = [_single(t, G, C) for t, (G, C) in zip(parts, segs)]
    torch.cuda.synchronize()
    for x, (G, C), o, s in zip(xs, segs, outs, singles):
        ref, bound = mr.finalize_ref(x)
        within(o.get(), ref, bound, "batched finalize G %d C %d" % (G, C))
        assert o.guards_intact() and s.guards_intact()
        assert np.array_equal(o.get().view(np.int32), s.get().view(np.int32)), (G, C)


@pytest.mark.parametrize("n", (17, 33))
def test_colsum_queue_past_one_launch(n):
    from xuanpolicy_amd import ops
    segs = mr.batch_cases()[:n]
    q = ops.ColsumQueue()
    xs, parts, outs = [], [], []
    for G, C in segs:
        x, t = _part(G, C, seed=1)
        o = Buf(C)
        q.add(t, o.t)
        xs.append(x), parts.append(t), outs.append(o)
    total, written = q.flush(DEV)
    singles = [_single(t, G, C) for t, (G, C) in zip(parts, segs)]
    torch.cuda.synchronize()
    assert total is None and written == sum(C for _, C in segs) and not q.items
    for x, (G, C), o, s in zip(xs, segs, outs, singles):
        ref, bound = mr.finalize_ref(x)
        within(o.get(), ref, bound, "queue of %d, G %d C %d" % (n, G, C))
        assert o.guards_intact() and np.array_equal(o.get().view(np.int32), s.get().view(np.int32)), (G, C)


NO_LOSS = (0, 0, 0, 0, None, 0, 0.0, 0.0, None, None)


def _check_mapped(x, C, tm, out, what):
    """Mapped positions against f64, every other element of the sentinel-filled out intact.  -> outputs by column."""
    ref, bound = mr.finalize_ref(x)
    w, idx = mr.map_written(C, tm), mr.map_index(C, tm)
    got = out.get()
    by_col = np.where(w, got[np.where(w, idx, 0)], 0.0).astype(np.float32)
    within(by_col[w], ref[w], bound[w], what)
    rest = np.ones(out.n, bool)
    rest[idx[w]] = False
    assert len(set(idx[w].tolist())) == int(w.sum())
    assert (got[rest] == mr.SENTINEL).all() and out.guards_intact(), what + ": wrote outside the map"
    return by_col


def test_output_map_with_and_without_norm_partials():
    segs = [(G, rp * tm[0]) for G, rp, tm in mr.MAP_CASES] + [(8, 100), (300, 70)]
    tmaps = [tm for _, _, tm in mr.MAP_CASES] + [None, None]      # mapped and identity segments in one launch
    assert len(segs) <= mr.MAX_SEGS
    xs, parts = zip(*[_part(G, C, seed=2) for G, C in segs])
    tiles = len(mr.tile_spans(segs))
    tm_keep, tm_arg = _tmap_arg(tmaps)
    results = []
    for with_sq in (True, False):
        outs = [Buf(mr.map_out_size(C, tm)) for (_, C), tm in zip(segs, tmaps)]
        keep, args = _seg_args(parts, segs, outs)
        sq, ticket = (_sq_buf(tiles, 3.25), _ticket()) if with_sq else (None, None)
        _call("xpa_colsum_finalize_batch_map", len(segs), *args, tm_arg, _p(sq), _p(ticket), *NO_LOSS, _stream())
        torch.cuda.synchronize()
        by_col = [_check_mapped(x, C, tm, o, "map %s G %d C %d" % (tm, G, C))
                  for x, (G, C), tm, o in zip(xs, segs, tmaps, outs)]
        if with_sq:     # tile sums count only the written columns
            _check_sq(sq, segs, by_col, tmaps, 3.25, "map")
            assert not ticket.any()
            dropped = [i for i, ((_, C), tm) in enumerate(zip(segs, tmaps)) if not mr.map_written(C, tm).all()]
            assert len(dropped) >= 7
        results.append([o.get() for o in outs])
    for a, b in zip(*results):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_batched_finalize_argument_checks():
    L = _L()
    G, C = 8, 18
    x, t = _part(G, C)
    s = _stream()
    sq, ticket = _sq_buf(4, 0.0), _ticket()

    wide = torch.zeros(G, 8 * 256, device=DEV)

    def rc(tm, n=1, cols=C, sq_=None, ticket_=None, fn="map"):
        out = Buf(64 if cols != wide.shape[1] else 256 * 32)     # sized for the call as if it were accepted
        m = max(n, 1)
        keep = ((ctypes.c_void_p * m)(*[(wide if cols == wide.shape[1] else t).data_ptr()] * m),
                (ctypes.c_int64 * m)(*[G] * m),
                (ctypes.c_int64 * m)(*[cols] * m), (ctypes.c_void_p * m)(*[out.t.data_ptr()] * m))
        args = [ctypes.cast(a, ctypes.c_void_p) for a in keep]
        tk, ta = _tmap_arg([tm] * m)
        if fn == "map":
            r = L.xpa_colsum_finalize_batch_map(n, *args, ta, _p(sq_), _p(ticket_), *NO_LOSS, s)
        else:
            r = L.xpa_colsum_finalize_batch_sq(n, *args, _p(sq_), _p(ticket_), s)
        torch.cuda.synchronize()
        assert out.untouched() or r == 0
        return r
    assert rc((3, 4, 7)) == 0                          # the accepted neighbour of every rejection below
    assert rc((4, 4, 7)) == INVALID                    # cols % inner != 0
    assert rc((3, 7, 7)) == INVALID                    # valid > rows
    assert rc((256, 17, 17), cols=8 * 256) == INVALID  # valid > rows: a 17-wide layer needs 32 padded rows, not 8
    assert rc((3, 4, 3)) == INVALID                    # ld < valid
    assert rc(None, n=0) == INVALID
    assert rc(None, n=17) == INVALID
    assert rc(None, cols=(1 << 24) + 1) == INVALID
    assert rc(None, sq_=sq) == INVALID                 # sq without a ticket
    assert rc(None, sq_=sq, fn="sq") == INVALID
    assert rc(None, n=17, fn="sq") == INVALID
    assert float(sq[1]) == -1.0 and not ticket.any()


def _norm_launch(tiles, ticket, sq0, seed):
    segs = mr.norm_segments(tiles)
    xs, parts = zip(*[_part(G, C, seed) for G, C in segs])
    outs = [Buf(C) for _, C in segs]
    keep, args = _seg_args(parts, segs, outs)
    sq = _sq_buf(tiles, sq0)
    _call("xpa_colsum_finalize_batch_sq", len(segs), *args, _p(sq), _p(ticket), _stream())
    return segs, xs, outs, sq, (keep, parts)


def _norm_check(tiles, segs, xs, outs, sq, sq0, what):
    by_col = []
    for x, (G, C), o in zip(xs, segs, outs):
        ref, bound = mr.finalize_ref(x)
        within(o.get(), ref, bound, "%s G %d C %d" % (what, G, C))
        assert o.guards_intact()
        by_col.append(o.get())
    _check_sq(sq, segs, by_col, None, sq0, what)


@pytest.mark.parametrize("tiles", mr.TILE_COUNTS)
def test_norm_partials_and_tickets(tiles):
    ticket = _ticket()
    segs, xs, outs, sq, keep = _norm_launch(tiles, ticket, 3.25, seed=3)
    torch.cuda.synchronize()
    _norm_check(tiles, segs, xs, outs, sq, 3.25, "norm %d tiles" % tiles)
    assert ticket.numel() == 4096 and not ticket.any(), "the ticket buffer is left at zero"


@pytest.mark.parametrize("first,second", [(65, 127), (1100, 63), (2, 2)])
def test_norm_launches_back_to_back_on_one_ticket_buffer(first, second):
    """Two tile counts (other group sizes, other group counts) on one stream and one ticket buffer, no sync in between: the
    second launch starts from the counters the first one reset."""
    ticket = _ticket()
    a = _norm_launch(first, ticket, 3.25, seed=4)
    b = _norm_launch(second, ticket, 0.5, seed=5)
    torch.cuda.synchronize()
    _norm_check(first, *a[:4], 3.25, "back to back, first (%d tiles)" % first)
    _norm_check(second, *b[:4], 0.5, "back to back, second (%d tiles)" % second)
    assert not ticket.any()


@pytest.mark.parametrize("dist", (0, 1))
def test_loss_block_of_the_mapped_finalize(dist):
    """xpa_colsum_finalize_batch_map with loss_partials: scalars, d logstd and sq[0] as xpa_policy_loss_finalize_sq alone
    writes them (bitwise), the column tiles as without it, the total over sq[0 .. tiles] by the bound."""
    from xuanpolicy_amd import ops
    L, s = _L(), _stream()
    B, K = 1000, 6
    Gl, W = int(L.xpa_loss_num_partials(B)), int(L.xpa_loss_partial_width(K))
    rng = np.random.default_rng(dist)
    lp = torch.from_numpy((0.01 * rng.standard_normal((Gl, W))).astype(np.float32)).to(DEV)
    sc_ref, dls_ref = torch.zeros(ops.N_OUT, device=DEV), torch.zeros(K, device=DEV)
    sq_ref = torch.full((1,), -1.0, dtype=torch.float64, device=DEV)
    _call("xpa_policy_loss_finalize_sq", 0, dist, B, K, _p(lp), Gl, 0.25, 0.01, _p(sc_ref), _p(dls_ref), _p(sq_ref), s)
    segs = [(8, 18), (64, 600), (300, 65)]
    tmaps = [(3, 4, 7), None, None]
    xs, parts = zip(*[_part(G, C, seed=6) for G, C in segs])
    outs = [Buf(mr.map_out_size(C, tm)) for (_, C), tm in zip(segs, tmaps)]
    keep, args = _seg_args(parts, segs, outs)
    tm_keep, tm_arg = _tmap_arg(tmaps)
    tiles = len(mr.tile_spans(segs))
    sq, ticket = _sq_buf(tiles, -1.0), _ticket()
    sc, dls = torch.zeros(ops.N_OUT, device=DEV), torch.zeros(K, device=DEV)
    _call("xpa_colsum_finalize_batch_map", len(segs), *args, tm_arg, _p(sq), _p(ticket), 0, dist, B, K, _p(lp), Gl, 0.25,
          0.01, _p(sc), _p(dls), s)
    torch.cuda.synchronize()
    assert torch.equal(sc.view(torch.int32), sc_ref.view(torch.int32))
    assert torch.equal(dls.view(torch.int32), dls_ref.view(torch.int32))
    assert float(sq_ref[0]) >= 0.0 and float(sq[0]) == float(sq_ref[0])
    by_col = [_check_mapped(x, C, tm, o, "loss launch %s G %d C %d" % (tm, G, C))
              for x, (G, C), tm, o in zip(xs, segs, tmaps, outs)]
    _check_sq(sq, segs, by_col, tmaps, None, "loss launch")
    assert not ticket.any()
