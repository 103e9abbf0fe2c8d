"""f64 numpy references, error bounds and case lists for csrc/mlp.hip: K10 (xpa_act_bwd_colsum), K11
(xpa_head_backward) and the column-sum finalizes.  Shared by tests/test_mlp_reduce_ref_cpu.py (which checks this module)
and tests/test_gpu_mlp_reduce.py (which holds the kernels to it).

Every reference is formed in f64 from the f32 inputs, with `slope` taken as float32(slope): the value that crosses the
C ABI.  Every bound is derived; none is fitted to a kernel's output.  With u = 2^-24 (f32 unit roundoff) and
e = 2^-52:

  f32 reductions (K10 / K11 partials, K11's K-term dot): |got - ref| <= (n + 4) u sum|term|.  sum_{i<n} of f32 terms by
      any order of f32 additions is within (n - 1) u sum|term| (1 + O(n u)) of the exact sum (recursive summation; a tree
      or a split into row groups only lowers the depth), FMA contraction removes roundings and adds none, and each term
      (activation derivative, product) carries at most 3 roundings of its own; 4 covers those and the O(n u) factor.
      n is the number of rows of the block (K10: <= 64, K11: <= 128) or K for the dot.
  K10's dz: tanh |dh (1 - h^2)| off by <= 4 u |dh| (1 + h^2) (h^2, 1 - h^2 and the product round once each, and the
      first rounding is not damped by 1 - h^2 when |h| is near 1: hence the absolute form); leaky <= u |ref| (one
      product); identity is not stored.
  K11's dz: the dot's bound D = (K + 4) u sum_o |g_o w_o| carried through the activation: identity D; leaky
      |a'| D (1 + u) + u |ref|; tanh |1 - h^2| D + 4 u (|dot| + D) (1 + h^2).
  K11's p_dbh sums those dz: its terms are not single products but K-term dots, whose error D is not a multiple of
      u |term| when the dot cancels (a block of one row shows it: there p_dbh IS dz, bit for bit, and carries dz's bound).
      So with T = sum_rows (dz's bound): T + (n + 4) u (sum|dz ref| + T) — the reduction bound over terms that are each
      within their own bound of the reference.  p_dw and p_dbo sum single products / plain inputs: the reduction bound.
  finalize outputs (f64 accumulation in a fixed order, one rounding to f32): u |ref| + G e sum|x|.
  norm partials: sq[1 + tile] against the f64 sum of squares of the kernel's own f32 outputs of that tile (each square
      of an f32 is exact in f64): n e sum o^2, n the tile's width; the total sq[1 + tiles] against
      sq[0] + sum sq[1 .. tiles] as read back: (tiles + 1) e sum.
"""
import math

import numpy as np

U = 2.0 ** -24
E = 2.0 ** -52
SLOPE = float(np.float32(0.01))     # as it crosses the C ABI
SENTINEL = -777.25                   # exactly representable; no kernel output below is ever this value

# ---- K10 ----------------------------------------------------------------------------------------------------------------
K10_ROWS_PER_BLOCK = 64
K10_ACTS = (0, 1, 2)
K10_ROWS = (1, 63, 64, 65, 130)
K10_COLS = (1, 4, 6, 12, 256, 257, 300, 1024, 1028)
K10_UNALIGNED_COLS = (256, 300)      # run on views offset by one float: the scalar kernel at vec4 widths


def k10_form(C, aligned=True):
    """mlp.hip's launcher: ("vec4", C / 4) or ("scalar", (columns of the 1st chunk, of the last chunk))."""
    if C % 4 == 0 and C // 4 <= 256 and aligned:
        return "vec4", C // 4
    return "scalar", (min(C, 256), C - 256 * ((C - 1) // 256))


def act_grad(act, dh, h, slope=SLOPE):
    dh = np.asarray(dh, np.float64)
    if act == 0:
        return dh
    h = np.asarray(h, np.float64)
    if act == 1:
        return np.where(h > 0, dh, dh * slope)     # h = +-0 takes the slope branch
    return dh * (1.0 - h * h)


def act_grad_bound(act, dh, h, ref):
    """K10's elementwise dz bound."""
    if act == 0:
        return np.zeros_like(ref)
    if act == 1:
        return U * np.abs(ref)
    h = np.asarray(h, np.float64)
    return 4 * U * np.abs(np.asarray(dh, np.float64)) * (1.0 + h * h)


def block_sums(x, rows_per_block):
    """[rows, ...] f64 -> ([G, ...] per-block sums, [G, ...] per-block sums of magnitudes, [G] rows per block)."""
    x = np.asarray(x, np.float64)
    rows = x.shape[0]
    G = -(-rows // rows_per_block)
    s = np.stack([x[g * rows_per_block:(g + 1) * rows_per_block].sum(0) for g in range(G)])
    m = np.stack([np.abs(x[g * rows_per_block:(g + 1) * rows_per_block]).sum(0) for g in range(G)])
    n = np.array([min(rows_per_block, rows - g * rows_per_block) for g in range(G)])
    return s, m, n


def reduce_bound(n, mag):
    """(n + 4) u sum|term| with n [G] broadcast over mag [G, ...]."""
    n = np.asarray(n, np.float64).reshape((-1,) + (1,) * (mag.ndim - 1))
    return (n + 4) * U * mag


def k10_ref(act, dh, h, slope=SLOPE):
    """-> dz [rows, C], its bound, partials [G, C], their bound (all f64)."""
    dz = act_grad(act, dh, h, slope)
    s, m, n = block_sums(dz, K10_ROWS_PER_BLOCK)
    return dz, act_grad_bound(act, dh, h, dz), s, reduce_bound(n, m)


def hidden_values(act, shape, rng):
    """Activation outputs as the kernels see them: leaky -> leaky(z) with exact +0.0 and -0.0 planted, tanh -> tanh(z),
    identity -> z."""
    z = rng.standard_normal(shape)
    if act == 1:
        h = np.where(z > 0, z, z * SLOPE).astype(np.float32)
        flat = h.reshape(-1)
        flat[0::7] = 0.0
        flat[3::7] = -0.0
        return h
    if act == 2:
        return np.tanh(1.5 * z).astype(np.float32)
    return z.astype(np.float32)


# ---- K11 ----------------------------------------------------------------------------------------------------------------
K11_ROWS_PER_BLOCK = 128
K11_ROWS = (1, 127, 128, 129, 300)
K11_VEC4_HK = ((4, 1), (12, 2), (64, 3), (256, 1), (256, 2), (256, 6), (256, 8), (1024, 8))
K11_GENERIC_HK = ((7, 1), (30, 6), (256, 9), (256, 17), (256, 32), (300, 32), (1028, 2))
K11_MISALIGNED_HK = ((256, 6),)     # generic by h offset by one float


def k11_instance(H, K, aligned=True):
    """mlp.hip's dispatch: (family, KMAX)."""
    if H % 4 == 0 and H // 4 <= 256 and K <= 8 and aligned:
        return "vec4", 1 if K == 1 else 2 if K <= 2 else 8
    return "generic", 1 if K == 1 else 8 if K <= 8 else 32


K11_INSTANCES = tuple((f, km) for f, kms in (("vec4", (1, 2, 8)), ("generic", (1, 8, 32))) for km in kms)


def k11_block_kinds(rows):
    kinds = set()
    if rows >= K11_ROWS_PER_BLOCK:
        kinds.add("full")
    if rows % K11_ROWS_PER_BLOCK:
        kinds.add("ragged")
    return kinds


def k11_cases():
    """The thinned product: dicts (act, rows, H, K, ldd, aligned, dbo).  Every (H, K) x act runs two row counts, rotated
    through K11_ROWS so that each pair holds a full and a ragged block; ldd alternates K and K + 3; p_dbo is null once per
    family."""
    pairs = ((1, 128), (127, 300), (128, 129), (129, 1), (300, 127))
    shapes = [(H, K, True) for H, K in K11_VEC4_HK + K11_GENERIC_HK] + [(H, K, False) for H, K in K11_MISALIGNED_HK]
    cases = []
    for s, (H, K, aligned) in enumerate(shapes):
        for act in (0, 1, 2):
            for j, rows in enumerate(pairs[(s + act) % len(pairs)]):
                cases.append(dict(act=act, rows=rows, H=H, K=K, ldd=K + 3 * ((s + act + j) % 2), aligned=aligned, dbo=True))
    cases.append(dict(act=1, rows=129, H=256, K=6, ldd=6, aligned=True, dbo=False))
    cases.append(dict(act=2, rows=129, H=30, K=6, ldd=9, aligned=True, dbo=False))
    return cases


def k11_id(c):
    return "act%d-r%d-H%d-K%d-ldd%d%s%s" % (c["act"], c["rows"], c["H"], c["K"], c["ldd"], "" if c["aligned"] else "-unal",
                                           "" if c["dbo"] else "-nodbo")


def k11_ref(act, d_head, h, w, slope=SLOPE):
    """d_head [rows, K], h [rows, H], w [K, H] -> dict of f64 references and bounds:
    dz [rows, H]; p_dw [G, K, H]; p_dbh [G, H]; p_dbo [G, K]; each with `<name>_bound`."""
    d = np.asarray(d_head, np.float64)
    h64 = np.asarray(h, np.float64)
    w64 = np.asarray(w, np.float64)
    K = d.shape[1]
    dot = d @ w64
    D = (K + 4) * U * (np.abs(d) @ np.abs(w64))
    dz = act_grad(act, dot, h64, slope)
    if act == 0:
        dz_b = D
    elif act == 1:
        dz_b = np.where(h64 > 0, 1.0, abs(slope)) * D * (1 + U) + U * np.abs(dz)
    else:
        dz_b = np.abs(1.0 - h64 * h64) * D + 4 * U * (np.abs(dot) + D) * (1.0 + h64 * h64)
    out = {"dz": dz, "dz_bound": dz_b}
    s, m, n = block_sums(d[:, :, None] * h64[:, None, :], K11_ROWS_PER_BLOCK)
    out["p_dw"], out["p_dw_bound"] = s, reduce_bound(n, m)
    s, m, n = block_sums(dz, K11_ROWS_PER_BLOCK)
    tb = block_sums(dz_b, K11_ROWS_PER_BLOCK)[0]      # the summed terms are the kernel's dz: each already off by <= dz_b
    out["p_dbh"], out["p_dbh_bound"] = s, reduce_bound(n, m + tb) + tb
    s, m, n = block_sums(d, K11_ROWS_PER_BLOCK)
    out["p_dbo"], out["p_dbo_bound"] = s, reduce_bound(n, m)
    return out


# ---- the finalizes ------------------------------------------------------------------------------------------------------
SINGLE_G = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300, 531)
SINGLE_C = (1, 63, 64, 65, 130)
BATCH_G = (1, 7, 8, 9, 32, 33, 63, 64, 65, 67, 256, 257, 300, 513)
MAX_SEGS = 16
TICKET_GROUPS = 63
TILE_COUNTS = (1, 2, 62, 63, 64, 65, 126, 127, 190, 1100)


def tile_width(G):
    """The batched finalize's form by partial rows: 1024-column tiles up to 32 rows, 512 up to 256, else 64."""
    return 1024 if G <= 32 else 512 if G <= 256 else 64


def seg_tiles(G, C):
    return -(-C // tile_width(G))


def batch_cols(G):
    t = tile_width(G)
    cs = [1, t - 1, t, t + 1, 2 * t + 1]
    if t == 512:
        cs.insert(1, 257)      # with 513: the mid form's min(c, C - 1) clamp inside a tile's second column set
    return tuple(cs)


def single_cases():
    return [(G, C) for G in SINGLE_G for C in SINGLE_C]


def batch_cases():
    """(G, C) ordered so that consecutive launches of 16 segments mix the three forms: each form's cases are spread
    evenly over the list."""
    keyed = []
    for t in (1024, 512, 64):
        form = [(G, C) for j in range(6) for G in BATCH_G if tile_width(G) == t for C in batch_cols(G)[j:j + 1]]
        keyed += [((i + 0.5) / len(form), t, gc) for i, gc in enumerate(form)]
    return [gc for _, _, gc in sorted(keyed)]


def batch_launches():
    cs = batch_cases()
    return [cs[i:i + MAX_SEGS] for i in range(0, len(cs), MAX_SEGS)]


def finalize_input(G, C, seed=0):
    """f32 [G, C]: randn exp(2 randn), and (G >= 2) in every column one exactly cancelling pair +-b, b ~ 1e6, early and
    late in the column, so that sum|x| >> |sum x| and an f32 running sum loses the small terms in between."""
    rng = np.random.default_rng([seed, G, C])
    x = (rng.standard_normal((G, C)) * np.exp(2.0 * rng.standard_normal((G, C)))).astype(np.float32)
    if G >= 2:
        q = max(G // 4, 1)
        i = rng.integers(0, q, C)
        j = rng.integers(G - q, G, C)
        j = np.where(j == i, G - 1, j)
        b = (1e6 * (1.0 + rng.random(C))).astype(np.float32)
        cols = np.arange(C)
        x[i, cols] = b
        x[j, cols] = -b
    return x


def finalize_ref(x):
    """-> (f64 column sums, the bound u |ref| + G e sum|x|)."""
    x64 = np.asarray(x, np.float64)
    ref = x64.sum(0)
    return ref, U * np.abs(ref) + x64.shape[0] * E * np.abs(x64).sum(0)


def f32_sequential_colsum(x):
    """The baseline the bound must reject: a running float32 sum down each column."""
    acc = np.zeros(x.shape[1], np.float32)
    for row in np.asarray(x, np.float32):
        acc = (acc + row).astype(np.float32)
    return acc


def tile_spans(segs):
    """segs [(G, C), ...] -> [(segment, c0, c1), ...], one per tile in launch order."""
    spans = []
    for s, (G, C) in enumerate(segs):
        t = tile_width(G)
        spans += [(s, c0, min(c0 + t, C)) for c0 in range(0, C, t)]
    return spans


def map_written(C, tmap):
    """bool [C]: the columns an output map (inner, valid, ld) stores (None / inner 0: all)."""
    if tmap is None or tmap[0] == 0:
        return np.ones(C, bool)
    return (np.arange(C) // tmap[0]) < tmap[1]


def map_index(C, tmap):
    """int [C]: where column c lands in `out` (meaningful where map_written)."""
    c = np.arange(C)
    if tmap is None or tmap[0] == 0:
        return c
    return (c % tmap[0]) * tmap[2] + c // tmap[0]


def map_out_size(C, tmap):
    return C if tmap is None or tmap[0] == 0 else tmap[0] * tmap[2]


def sq_tile_refs(segs, outs_by_col, tmaps=None):
    """The norm partial each tile must hold: outs_by_col[s] = the kernel's f32 outputs indexed by partial column (0 where
    the map drops the column).  -> (f64 [tiles] sums of squares, their bounds n e sum o^2)."""
    refs, bounds = [], []
    for s, c0, c1 in tile_spans(segs):
        o = np.asarray(outs_by_col[s][c0:c1], np.float64)
        if tmaps is not None:
            o = np.where(map_written(segs[s][1], tmaps[s])[c0:c1], o, 0.0)
        q = float((o * o).sum())
        refs.append(q)
        bounds.append((c1 - c0) * E * q)
    return np.array(refs), np.array(bounds)


def sq_total_ref(sq, tiles):
    """sq as read back -> (the exact sum of sq[0 .. tiles], the bound (tiles + 1) e sum)."""
    t = math.fsum(float(v) for v in sq[:tiles + 1])
    return t, (tiles + 1) * E * math.fsum(abs(float(v)) for v in sq[:tiles + 1])


def ticket_groups(tiles):
    """(blocks per group, groups, blocks in the last group) of the two-level ticket for a grid of `tiles` blocks."""
    gs = -(-tiles // TICKET_GROUPS)
    ng = -(-tiles // gs)
    return gs, ng, tiles - (ng - 1) * gs


def norm_segments(tiles):
    """Segments (G, C) whose tiles add up to `tiles`: two mid-form tiles and two 64-column tiles where they fit, the
    rest from one G = 1 segment (a tile per 1024 columns, the last one ragged)."""
    if tiles == 1:
        return [(1, 1000)]
    if tiles == 2:
        return [(300, 100)]
    segs = [(40, 513), (300, 65)]
    if tiles > 4:
        segs.insert(1, (1, 1024 * (tiles - 4) - 5))
    return segs


# output-map cases: (G, rows_padded, (inner, valid, ld)); the partials are [G, rows_padded * inner]
MAP_CASES = (
    (8, 8, (256, 5, 5)), (64, 32, (256, 17, 17)), (300, 8, (256, 5, 5)), (8, 32, (256, 17, 17)),
    (8, 6, (3, 4, 7)), (64, 6, (3, 4, 7)), (300, 6, (3, 4, 7)),                 # ld > valid
    (40, 65, (1, 65, 65)), (300, 130, (1, 130, 130)),                           # (1, C, C)
    (8, 5, (4, 5, 5)), (64, 5, (4, 5, 5)), (300, 5, (4, 5, 5)),                 # valid == rows: nothing dropped
)
