"""CPU: tests/_mlp_reduce_ref.py itself — the references against torch f64 autograd, the finalize inputs' separation of
f64 from f32 accumulation, the case lists' coverage of mlp.hip's kernel forms, and seg_tiles against the library."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _mlp_reduce_ref as mr


def _act(code, z):
    if code == 1:
        return torch.nn.functional.leaky_relu(z, mr.SLOPE)
    return torch.tanh(z) if code == 2 else z


@pytest.mark.parametrize("act", (0, 1, 2))
def test_k11_reference_matches_autograd(act):
    """x -> Linear(D, H) -> act -> Linear(H, K), loss = sum(out * d_head), all in f64: autograd's gradients are k11_ref's dz
    and the block sums of its partials (300 rows: two full blocks and a ragged one)."""
    g = torch.Generator().manual_seed(act)
    rows, D, H, K = 300, 5, 12, 3
    x = torch.randn(rows, D, dtype=torch.float64, generator=g)
    l1, l2 = torch.nn.Linear(D, H).double(), torch.nn.Linear(H, K).double()
    d_head = torch.randn(rows, K, dtype=torch.float64, generator=g)
    z = l1(x)
    z.retain_grad()
    h = _act(act, z)
    (l2(h) * d_head).sum().backward()
    ref = mr.k11_ref(act, d_head.numpy(), h.detach().numpy(), l2.weight.detach().numpy())
    assert ref["p_dw"].shape == (3, K, H) and ref["p_dbh"].shape == (3, H) and ref["p_dbo"].shape == (3, K)
    for got, exp in ((ref["dz"], z.grad), (ref["p_dw"].sum(0), l2.weight.grad), (ref["p_dbh"].sum(0), l1.bias.grad),
                     (ref["p_dbo"].sum(0), l2.bias.grad)):
        np.testing.assert_allclose(got, exp.numpy(), rtol=1e-12, atol=1e-13)
    # the blocks are rows [128 g, 128 g + 128)
    np.testing.assert_allclose(ref["p_dbo"][2], d_head[256:].sum(0).numpy(), rtol=1e-12, atol=1e-13)
    for name in ("dz", "p_dw", "p_dbh", "p_dbo"):
        assert ref[name + "_bound"].shape == ref[name].shape and (ref[name + "_bound"] >= 0).all()


@pytest.mark.parametrize("act", (0, 1, 2))
def test_k10_reference_matches_autograd(act):
    g = torch.Generator().manual_seed(10 + act)
    rows, C = 130, 6
    z = torch.randn(rows, C, dtype=torch.float64, generator=g, requires_grad=True)
    dh = torch.randn(rows, C, dtype=torch.float64, generator=g)
    h = _act(act, z)
    (h * dh).sum().backward()
    dz, dz_b, part, part_b = mr.k10_ref(act, dh.numpy(), h.detach().numpy())
    np.testing.assert_allclose(dz, z.grad.numpy(), rtol=1e-12, atol=1e-13)
    assert part.shape == (3, C)
    np.testing.assert_allclose(part[1], z.grad[64:128].sum(0).numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(part[2], z.grad[128:].sum(0).numpy(), rtol=1e-12, atol=1e-13)
    assert (dz_b >= 0).all() and (part_b > 0).all()


def test_leaky_takes_the_slope_branch_at_both_zeros():
    h = mr.hidden_values(1, (64, 7), np.random.default_rng(0))
    assert (h == 0).sum() >= 2 and np.signbit(h[h == 0]).any() and not np.signbit(h[h == 0]).all()
    dh = np.ones_like(h)
    dz = mr.act_grad(1, dh, h)
    assert (dz[h == 0] == mr.SLOPE).all() and (dz[h > 0] == 1.0).all()


def test_reduce_bound_rejects_a_dropped_row_and_an_f32_slope():
    """Negative controls on the reference side: a block sum that misses one row, and a slope that is not float32(slope),
    are outside the bounds the kernels are held to."""
    rng = np.random.default_rng(1)
    dh = rng.standard_normal((130, 12)).astype(np.float32)
    h = mr.hidden_values(1, (130, 12), rng)
    dz, dz_b, part, part_b = mr.k10_ref(1, dh, h)
    short = dz[:63].sum(0)
    assert (np.abs(short - part[0]) > part_b[0]).all()
    wrong = mr.act_grad(1, dh, h, 0.01)
    neg = h <= 0
    assert (np.abs(wrong - dz)[neg & (dh != 0)] > 0).all()


def test_k10_case_list_reaches_every_form():
    vec = {mr.k10_form(C)[1] for C in mr.K10_COLS if mr.k10_form(C)[0] == "vec4"}
    assert vec == {1, 3, 64, 75, 256}       # 75 = 300 / 4: with 3, a width that does not divide the 256 threads
    scal = {mr.k10_form(C)[1] for C in mr.K10_COLS if mr.k10_form(C)[0] == "scalar"}
    scal |= {mr.k10_form(C, aligned=False)[1] for C in mr.K10_UNALIGNED_COLS}
    assert all(mr.k10_form(C, aligned=False)[0] == "scalar" for C in mr.K10_UNALIGNED_COLS)
    assert {s for s in scal if s[0] < 256} == {(1, 1), (6, 6)}                 # one chunk
    # a second chunk of 1, 44 and 4 columns, and none; 300 is a vec4 width, so its 44 run on the alignment fallback
    assert {s[1] for s in scal if s[0] == 256} == {1, 44, 4, 256}
    blocks = {-(-r // mr.K10_ROWS_PER_BLOCK) for r in mr.K10_ROWS}
    assert blocks == {1, 2, 3} and any(r % 64 for r in mr.K10_ROWS) and 64 in mr.K10_ROWS


def test_k11_case_list_covers_every_instance():
    cases = mr.k11_cases()
    ids = [mr.k11_id(c) for c in cases]
    assert len(set(ids)) == len(ids)
    seen, rows_seen, ldd_seen, nodbo, shapes = set(), set(), set(), set(), set()
    for c in cases:
        inst = mr.k11_instance(c["H"], c["K"], c["aligned"])
        for kind in mr.k11_block_kinds(c["rows"]):
            seen.add((inst, c["act"], kind))
        rows_seen.add((inst[0], c["rows"]))
        ldd_seen.add((inst[0], c["ldd"] > c["K"]))
        if not c["dbo"]:
            nodbo.add(inst[0])
        shapes.add((c["H"], c["K"], c["aligned"]))
        assert c["rows"] in mr.K11_ROWS and c["ldd"] in (c["K"], c["K"] + 3) and c["K"] <= 32
    assert seen == {(i, a, k) for i in mr.K11_INSTANCES for a in (0, 1, 2) for k in ("full", "ragged")}
    assert rows_seen == {(f, r) for f in ("vec4", "generic") for r in mr.K11_ROWS}
    assert ldd_seen == {(f, b) for f in ("vec4", "generic") for b in (False, True)}
    assert nodbo == {"vec4", "generic"}
    assert shapes == ({(H, K, True) for H, K in mr.K11_VEC4_HK + mr.K11_GENERIC_HK} |
                      {(H, K, False) for H, K in mr.K11_MISALIGNED_HK})
    # the lists land where the issue says they do
    assert all(mr.k11_instance(H, K)[0] == "vec4" for H, K in mr.K11_VEC4_HK)
    assert all(mr.k11_instance(H, K)[0] == "generic" for H, K in mr.K11_GENERIC_HK)
    assert all(mr.k11_instance(H, K, False) == ("generic", 8) for H, K in mr.K11_MISALIGNED_HK)
    # every reason for the generic kernel: K > 8, H % 4, H > 1024, alignment
    assert {(K > 8, H % 4 != 0, H > 1024) for H, K in mr.K11_GENERIC_HK} >= {(True, False, False), (False, True, False),
                                                                            (False, False, True)}


def test_finalize_inputs_separate_f64_from_f32_accumulation():
    """On exactly the inputs the GPU tests use: the f64 sum rounded once to f32 is inside the finalize bound everywhere,
    and a float32 running sum is outside it in at least one column of every case with G >= 64."""
    cases = sorted(set(mr.single_cases()) | set(mr.batch_cases()))
    assert sum(G >= 64 for G, _ in cases) >= 40
    for G, C in cases:
        x = mr.finalize_input(G, C)
        assert x.dtype == np.float32 and x.shape == (G, C)
        ref, bound = mr.finalize_ref(x)
        once = ref.astype(np.float32).astype(np.float64)
        assert (np.abs(once - ref) <= bound).all(), (G, C)
        if G >= 2:
            ratio = np.abs(x.astype(np.float64)).sum(0) / np.abs(ref)       # sum|x| >> |sum x|
            assert ratio.min() > 30 and np.median(ratio) > 1e3, (G, C)
        if G >= 64:
            seq = mr.f32_sequential_colsum(x).astype(np.float64)
            assert (np.abs(seq - ref) > bound).any(), (G, C)


def test_batch_case_list_sits_on_the_form_and_tile_edges():
    assert {mr.tile_width(G) for G in mr.BATCH_G} == {1024, 512, 64}
    assert (mr.tile_width(32), mr.tile_width(33), mr.tile_width(256), mr.tile_width(257)) == (1024, 512, 512, 64)
    cases = mr.batch_cases()
    assert len(set(cases)) == len(cases)
    for G in mr.BATCH_G:
        t = mr.tile_width(G)
        assert {C for g, C in cases if g == G} >= {1, t - 1, t, t + 1, 2 * t + 1}
    assert {C for g, C in cases if mr.tile_width(g) == 512} >= {257, 513}
    launches = mr.batch_launches()
    assert sum(len(l) for l in launches) == len(cases) and max(len(l) for l in launches) == mr.MAX_SEGS
    for l in launches:    # tile0 lookup across forms
        assert {mr.tile_width(G) for G, _ in l} == {1024, 512, 64}
    # the unroll remainders: wide 8-row rounds, mid / 64-column 16- and 4-deep rounds over 4 / 16 row groups
    assert {G % 8 for G in mr.BATCH_G if G <= 32} >= {0, 1, 7}
    assert {1, 15, 16, 17, 63, 64, 65, 255, 256, 257} <= set(mr.SINGLE_G)


def test_norm_cases_reach_every_ticket_shape():
    for tiles in mr.TILE_COUNTS:
        segs = mr.norm_segments(tiles)
        assert sum(mr.seg_tiles(G, C) for G, C in segs) == tiles and len(segs) <= mr.MAX_SEGS
        assert len(mr.tile_spans(segs)) == tiles
        assert max(C for _, C in segs) <= 1 << 24
    groups = {t: mr.ticket_groups(t) for t in mr.TILE_COUNTS}
    assert groups[63] == (1, 63, 1) and groups[64] == (2, 32, 2) and groups[65] == (2, 33, 1)
    assert any(gs > 1 and last < gs for gs, _, last in groups.values())          # a ragged last group
    assert all(ng <= mr.TICKET_GROUPS for _, ng, _ in groups.values())
    assert max(mr.TILE_COUNTS) + 1 > 1024                                          # per > 1 in the total's runs
    assert {mr.tile_width(G) for t in mr.TILE_COUNTS if t >= 4 for G, _ in mr.norm_segments(t)} == {1024, 512, 64}


def test_map_helpers():
    tm = (3, 4, 7)
    C = 18
    w, idx = mr.map_written(C, tm), mr.map_index(C, tm)
    assert w.tolist() == [True] * 12 + [False] * 6
    assert idx[:12].tolist() == [0, 7, 14, 1, 8, 15, 2, 9, 16, 3, 10, 17] and mr.map_out_size(C, tm) == 21
    assert mr.map_written(5, None).all() and mr.map_index(5, (0, 0, 0)).tolist() == [0, 1, 2, 3, 4]
    for G, rp, (inner, valid, ld) in mr.MAP_CASES:
        assert valid <= rp and ld >= valid
    assert any(ld > valid for _, _, (_, valid, ld) in mr.MAP_CASES)
    assert any(valid == rp for _, rp, (_, valid, _) in mr.MAP_CASES)
    assert {mr.tile_width(G) for G, _, _ in mr.MAP_CASES} == {1024, 512, 64}


def test_seg_tiles_matches_the_library():
    """xpa_colsum_batch_tiles is host code: it runs without a GPU."""
    from xuanpolicy_amd import ops
    L = ops.lib()

    def lib_tiles(segs):
        n = len(segs)
        g = (ctypes.c_int64 * n)(*[s[0] for s in segs])
        c = (ctypes.c_int64 * n)(*[s[1] for s in segs])
        return int(L.xpa_colsum_batch_tiles(n, ctypes.cast(g, ctypes.c_void_p), ctypes.cast(c, ctypes.c_void_p)))
    every = set(mr.single_cases()) | set(mr.batch_cases()) | {(G, rp * tm[0]) for G, rp, tm in mr.MAP_CASES}
    every |= {s for t in mr.TILE_COUNTS for s in mr.norm_segments(t)}
    for G, C in sorted(every):
        assert lib_tiles([(G, C)]) == mr.seg_tiles(G, C), (G, C)
    for segs in mr.batch_launches() + [mr.norm_segments(t) for t in mr.TILE_COUNTS]:
        assert lib_tiles(segs) == sum(mr.seg_tiles(G, C) for G, C in segs) == len(mr.tile_spans(segs))
    assert int(L.xpa_act_bwd_num_partials(130)) == 3 and int(L.xpa_head_bwd_num_partials(300)) == 3
