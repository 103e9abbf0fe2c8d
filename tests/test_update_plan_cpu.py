"""CPU checks of the minibatch update's plan (fused_mlp.UpdatePlan, FusedActorCritic.plan): host logic alone, no GPU
and no kernel launch.  The expected plans are written out from the forms the update took before the planner existed
(K-numbers: DESIGN.md §5); the policies' parameters sit in a CPU FlatState so the paired hidden layer exists."""
import itertools

import pytest
import torch

from oracle import cpu_ref
from xuanpolicy_amd import buffer as bf
from xuanpolicy_amd import ops
from xuanpolicy_amd.flat import FlatState
from xuanpolicy_amd.fused_mlp import FusedActorCritic, Rows, UpdatePlan, head_placement

B = 8192
SPLITS = ("s3p_a", "s3p_c", "dx")
SPLITS_CRIT = ("s3p_a", "s3p_c", "dx_crit")


def _fm(d, A, rep=(256,)):
    pol = cpu_ref.build_actor_critic_ref(d, A, list(rep), [256], [256])
    fm = FusedActorCritic(pol, flat=FlatState(list(pol.parameters()), placement=head_placement(pol)))
    assert fm.pair is not None and fm.gemm_heads
    return fm


def _rows(d, b=B, n=4 * B, slack=True):
    """Minibatch rows of an [n, d] buffer with (or without) the rollout buffer's slack behind its last row."""
    flat = torch.zeros(n + bf.OBS_SLACK // d + 2, d)[:n] if slack else torch.zeros(n, d)
    return Rows(flat, torch.zeros(b, dtype=torch.int64))


def _set(monkeypatch, fm, **sw):
    for k, v in sw.items():
        if k in ("S3_GEMMS", "S3_HEADS", "K16W_ENABLED"):
            monkeypatch.setattr(ops, k, v)
        elif k == "use_trunk_heads":
            fm.use_trunk_heads = v
        else:
            monkeypatch.setattr(FusedActorCritic, k, v)


C2_SIGN = dict(trunk_fwd="K13-gather-sign", hidden="heads", sign_bits="K13", early_sync=False)
C2_S3R = UpdatePlan("K13-gather-only", "heads", "K16R", SPLITS, "K41V", "K42S", "K16R", False)
C4_CRIT = dict(hidden="heads", heads="K16Q-mask", splits=SPLITS_CRIT, dw_hidden="K41P", trunk_bwd="K42C-dz",
               sign_bits="K40F", early_sync=False)
TABLE = [
    # (name, obs width, act width, switches, input kind, the whole plan)
    ("c2_default", 17, 6, {}, "rows",
     UpdatePlan(heads="K16Q-mask", splits=SPLITS_CRIT, dw_hidden="K41P", trunk_bwd="K42C", **C2_SIGN)),
    ("c2_s3q_crit_off", 17, 6, {"CRIT_FACTORED": False}, "rows",
     UpdatePlan(heads="K16Q", splits=SPLITS, dw_hidden="K41V", trunk_bwd="K42S", **C2_SIGN)),
    ("c2_s3p_crit_on", 17, 6, {"S3_HEADS": "s3p"}, "rows",
     UpdatePlan(heads="K16P", splits=SPLITS, dw_hidden="K41V", trunk_bwd="K42S", **C2_SIGN)),
    ("c2_s3p_crit_off", 17, 6, {"S3_HEADS": "s3p", "CRIT_FACTORED": False}, "rows",
     UpdatePlan(heads="K16P", splits=SPLITS, dw_hidden="K41V", trunk_bwd="K42S", **C2_SIGN)),
    ("c2_s3_crit_on", 17, 6, {"S3_HEADS": "s3"}, "rows",
     UpdatePlan(heads="K16S", splits=("dx",), dw_hidden="K41V", trunk_bwd="K42S", **C2_SIGN)),
    ("c2_s3_crit_off", 17, 6, {"S3_HEADS": "s3", "CRIT_FACTORED": False}, "rows",
     UpdatePlan(heads="K16S", splits=("dx",), dw_hidden="K41V", trunk_bwd="K42S", **C2_SIGN)),
    ("c2_f32", 17, 6, {"S3_GEMMS": False}, "rows",
     UpdatePlan("K13-gather", "heads", "K16", (), "splitk", "mm+chain", None, False)),
    ("c2_k16w", 17, 6, {"K16W_ENABLED": True}, "rows",
     UpdatePlan(heads="K16W", splits=("dx",), dw_hidden="K41V", trunk_bwd="K42S", **C2_SIGN)),
    ("c2_k16w_wide_head", 17, 18, {"K16W_ENABLED": True}, "rows",
     UpdatePlan(heads="K16S+W", splits=("dx",), dw_hidden="K41V", trunk_bwd="K42S", **C2_SIGN)),
    ("c2_trunk_heads", 17, 6, {"use_trunk_heads": True}, "rows",
     UpdatePlan("K13-gather-only", "heads", "K16X", ("dx",), "K41V", "K42", None, False)),
    ("c2_trunk_heads_f32", 17, 6, {"use_trunk_heads": True, "S3_GEMMS": False}, "rows",
     UpdatePlan("K13-gather-only", "heads", "K16X", (), "splitk", "mm+chain", None, False)),
    ("c2_s3r_sign_on", 17, 6, {"S3_HEADS": "s3p", "TRUNK_S3R": True, "SIGN_BITS": True}, "rows", C2_S3R),
    ("c2_s3r_sign_off", 17, 6, {"S3_HEADS": "s3p", "TRUNK_S3R": True, "SIGN_BITS": False}, "rows", C2_S3R),
    ("c2_s3p_sign_off", 17, 6, {"S3_HEADS": "s3p", "SIGN_BITS": False}, "rows",
     UpdatePlan("K13-gather", "heads", "K16P", SPLITS, "K41V", "K42", None, False)),
    ("c2_s3q_sign_off", 17, 6, {"SIGN_BITS": False}, "rows",   # no sign bits: no factored critic, K41V + K42
     UpdatePlan("K13-gather", "heads", "K16Q", SPLITS, "K41V", "K42", None, False)),
    ("c4_direct", 376, 17, {}, "rows", UpdatePlan(trunk_fwd="K40F-idx", **C4_CRIT)),
    ("c4_gather", 376, 17, {"WIDE_DIRECT": False}, "rows", UpdatePlan(trunk_fwd="K40F-pitched", **C4_CRIT)),
    ("c4_no_slack", 376, 17, {}, "rows_no_slack", UpdatePlan(trunk_fwd="K40F-pitched", **C4_CRIT)),
    ("c4_crit_off", 376, 17, {"CRIT_FACTORED": False}, "rows",
     UpdatePlan("K40F-idx", "heads", "K16Q", SPLITS, "K41V", "K42W", "K40F", False)),
    ("c4_off", 376, 17, {"WIDE_TRUNK": False}, "tensor",   # the agent gathers: a library trunk, K40 dX, the chain
     UpdatePlan("chain", "heads", "K16Q", SPLITS, "K41V", "K40+chain", None, False)),
    ("c2_tensor", 17, 6, {}, "tensor", UpdatePlan("K13", "heads", "K16Q", SPLITS, "K41V", "K42", None, False)),
    ("c2_two_layer_rep", 17, 6, {}, "rows2",
     UpdatePlan("K13-gather", "heads", "K16Q", SPLITS, "K41V", "K40+chain", None, False)),
]


def _input(kind, d):
    if kind == "tensor":
        return torch.zeros(B, d)
    return _rows(d, slack=kind != "rows_no_slack")


@pytest.mark.parametrize("name,d,A,sw,kind,want", TABLE, ids=[t[0] for t in TABLE])
def test_plan_table(name, d, A, sw, kind, want, monkeypatch):
    fm = _fm(d, A, rep=(256, 256) if kind == "rows2" else (256,))
    _set(monkeypatch, fm, **sw)
    assert fm.plan(_input(kind, d)) == want


def test_unpaired_policy_plans_the_chains():
    """Without the flat placement there is no paired layer: K12 on per-head hidden GEMMs, library backward."""
    fm = FusedActorCritic(cpu_ref.build_actor_critic_ref(17, 6, [256], [256], [256]))
    assert fm.plan(torch.zeros(8, 17)) == UpdatePlan("K13", "chains", "K12", (), "splitk", "chain", None, False)
    fm = FusedActorCritic(cpu_ref.build_actor_critic_ref(376, 17, [256], [256], [256]))
    with pytest.raises(ValueError):   # no paired layer: the wide trunk is off, and Rows needs K13 or K40F
        fm.plan(_rows(376))


def test_early_sync_is_planned_with_the_paired_layer():
    fm = _fm(17, 6)
    fm.early_grad_sync = lambda g: None
    p = fm.plan(_rows(17))
    assert p.early_sync and p.launches()[6:8] == ["xpa_s3_wgrad_pair", "xpa_colsum_finalize_batch"]


SWITCHES = {"S3_GEMMS": (True, False), "S3_HEADS": ("s3", "s3p", "s3q"), "K16W_ENABLED": (False, True),
            "CRIT_FACTORED": (True, False), "FUSE_TRUNK_BWD": (True, False), "TRUNK_S3R": (False, True),
            "SIGN_BITS": (True, False), "WIDE_TRUNK": (True, False), "WIDE_DIRECT": (True, False),
            "use_trunk_heads": (False, True)}


def _direct_ok(x, d, on):
    """The row-index forms' conditions, restated: contiguous [n, d] rows on a 16-B base, d % 4 == 0, K41V-IDX's
    per-slice rows (to 32) within its 1536-row index stage, zeroed slack behind the last row for the padded columns."""
    f = x.flat
    mp = (d + 127) // 128 * 128
    S = max(1, 256 // (mp // 128))
    per = (-(-x.idx.shape[0] // S) + 31) // 32 * 32
    slack = f.untyped_storage().nbytes() // 4 - f.storage_offset() - f.numel()
    return (on and f.is_contiguous() and f.shape[1] == d and d % 4 == 0 and f.data_ptr() % 16 == 0 and per <= 1536
            and slack >= max((d + 15) // 16 * 16, mp) - d)


def test_plans_are_consistent_over_every_switch_and_input(monkeypatch):
    """Replaces the source check that the factored critic and the fused trunk backward share one predicate: over the
    cross product of every switch and input kind, no plan pairs stages that cannot run together."""
    cases = [(_fm(17, 6), _rows(17), 17), (_fm(17, 6), torch.zeros(B, 17), 17), (_fm(17, 18), _rows(17), 17),
             (_fm(17, 6, rep=(256, 256)), _rows(17), 17), (_fm(376, 17), _rows(376), 376),
             (_fm(376, 17), _rows(376, slack=False), 376), (_fm(376, 17), torch.zeros(B, 376), 376),
             (_fm(1024, 6), _rows(1024, b=65536, n=65536), 1024), (_fm(1024, 6), _rows(1024, b=49152, n=65536), 1024)]
    names = list(SWITCHES)
    seen = set()
    for values in itertools.product(*SWITCHES.values()):
        sw = dict(zip(names, values))
        for early in (None, len):
            for fm, x, d in cases:
                _set(monkeypatch, fm, **sw)
                fm.early_grad_sync = early
                rows = isinstance(x, Rows)
                if rows and not fm.thin0 and not fm._wide_on():
                    with pytest.raises(ValueError):
                        fm.plan(x)
                    continue
                p = fm.plan(x)
                seen.add(p)
                ctx = (sw, p)
                masked = p.heads == "K16Q-mask"
                assert masked == (p.dw_hidden == "K41P") == ("dx_crit" in p.splits), ctx
                assert masked == (p.trunk_bwd in ("K42C", "K42C-dz")), ctx
                if p.trunk_bwd in ("K42C", "K42S", "K42C-dz", "K42W"):   # act' from h's sign bits
                    assert p.sign_bits is not None, ctx
                assert (p.sign_bits == "K13") == (p.trunk_fwd == "K13-gather-sign"), ctx
                assert (p.sign_bits == "K40F") == p.trunk_fwd.startswith("K40F") == (p.trunk_bwd in ("K42W", "K42C-dz")), ctx
                assert (p.trunk_fwd == "K13-gather-only") == (p.heads in ("K16X", "K16R")), ctx
                assert p.sign_bits != "K16R" or p.heads == "K16R", ctx
                assert ("s3p_a" in p.splits) == (p.heads in ("K16P", "K16Q", "K16Q-mask", "K16R")), ctx
                assert p.early_sync == (early is not None), ctx
                if not sw["S3_GEMMS"]:
                    assert not p.splits and p.dw_hidden == "splitk" and p.heads in ("K16", "K16W", "K16+W", "K16X"), ctx
                if rows and not fm.thin0:
                    assert (p.trunk_fwd == "K40F-idx") == _direct_ok(x, d, sw["WIDE_DIRECT"]), ctx
                else:
                    assert not p.trunk_fwd.startswith("K40F"), ctx
                assert p.heads in ops.HEAD_FORMS and p.launches()[-1].startswith("xpa_colsum_finalize_batch"), ctx
    # every form of the table's fields is reached somewhere in the product
    assert {p.trunk_bwd for p in seen} >= {"K42C", "K42S", "K42", "K42C-dz", "K42W", "K40+chain", "mm+chain"}
    assert {p.heads for p in seen} == set(ops.HEAD_FORMS) - {"K12"}


def test_a_switch_flipped_after_planning_changes_the_plan(monkeypatch):
    """The cache key holds every switch: a flip after a plan was cached takes effect, and flipping back returns the
    cached plan."""
    fm, x = _fm(17, 6), _rows(17)
    base = fm.plan(x)
    assert fm.plan(_rows(17)) is base   # same geometry: the cached plan
    flips = [({"S3_GEMMS": False}, "heads", "K16"), ({"S3_HEADS": "s3p"}, "heads", "K16P"),
             ({"K16W_ENABLED": True}, "heads", "K16W"), ({"CRIT_FACTORED": False}, "dw_hidden", "K41V"),
             ({"FUSE_TRUNK_BWD": False}, "trunk_bwd", "K40+chain"), ({"TRUNK_S3R": True}, "heads", "K16R"),
             ({"SIGN_BITS": False}, "sign_bits", None), ({"use_trunk_heads": True}, "heads", "K16X")]
    for sw, field, want in flips:
        with monkeypatch.context() as m:
            _set(m, fm, **sw)
            p = fm.plan(x)
            assert p != base and getattr(p, field) == want, (sw, p)
        fm.use_trunk_heads = False
        assert fm.plan(x) is base
    fm.early_grad_sync = len
    assert fm.plan(x).early_sync and not base.early_sync
    fm.early_grad_sync = None
    n = len(fm._plans)
    assert fm.plan(_rows(17, b=B // 2)) == base and len(fm._plans) == n + 1   # another B: its own entry
    c4, x4 = _fm(376, 17), _rows(376)
    assert c4.plan(x4).trunk_fwd == "K40F-idx"
    for sw in ({"WIDE_DIRECT": False}, {"WIDE_VIDX_MAX": 32}):
        with monkeypatch.context() as m:
            _set(m, c4, **sw)
            assert c4.plan(x4).trunk_fwd == "K40F-pitched", sw
    with monkeypatch.context() as m:
        _set(m, c4, WIDE_TRUNK=False)
        with pytest.raises(ValueError):
            c4.plan(x4)
    assert c4.plan(x4).trunk_fwd == "K40F-idx"
