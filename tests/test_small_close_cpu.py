"""CPU: K33's host side — the header binds xpa_small_close / xpa_small_close_batch and XpaSmallCloseArgs at the same
ABI version, plan_rollout emits the "K33" closing only behind the small_close switch and only for a one-launch
small-path rollout, plan_population wants the closing's form and scalars shared, and the two entry points reject bad
blocks before any HIP call (so a machine without a GPU can show it)."""
import ctypes

import pytest

from tests.test_rollout_plan_cpu import CARTPOLE, CARTPOLE_PLAN, CASES, KINDS
from xuanpolicy_amd import _lib
from xuanpolicy_amd import rollout_plan as rp
from xuanpolicy_amd.population import MemberFacts, plan_population
from xuanpolicy_amd.rollout_plan import RolloutFacts, plan_rollout

P = 0x1000   # a fake, 16-B aligned, non-null pointer: the calls below return before anything dereferences it


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def test_header_binds_the_closing_entry_points(lib):
    from ctypes import c_int, c_int64, c_void_p as p
    assert _lib.ABI_VERSION == 4 and lib.xpa_abi_version() == 4
    assert _lib.SIGNATURES["xpa_small_close"] == (c_int, [p, p])
    assert _lib.SIGNATURES["xpa_small_close_batch"] == (c_int, [c_int64, p, p, p])
    assert hasattr(lib, "xpa_small_close") and hasattr(lib, "xpa_small_close_batch")
    names = [n for n, _ in _lib.XpaSmallCloseArgs._fields_]
    assert names[:13] == ["n_envs", "horizon", "d_in", "h0", "h1", "h2", "k", "act_code", "n_slots", "use_gae", "slope",
                          "gamma", "gae_lambda"]
    assert names[13:23] == ["W0", "b0", "W1", "b1", "W2", "b2", "Wa", "ba", "Wc", "bc"]
    assert names[23:] == ["rows", "ld_rows", "slot_t", "rew", "val", "term", "closed", "boot", "adv", "ret", "vboot_out"]
    # 13 four-byte scalars (padded to 8), then 21 pointers / int64
    assert ctypes.sizeof(_lib.XpaSmallCloseArgs) == 56 + 21 * 8


# ---- plan_rollout ---------------------------------------------------------------------------------------------------
# the four classic facts at widths 64 and 128: (env, dist, d_in, k)
CLASSIC = [("cartpole", "categorical", 4, 2), ("pendulum", "gaussian", 3, 1), ("acrobot", "categorical", 6, 3),
           ("mountaincar", "categorical", 8, 3)]


def _classic(env, dist, d_in, k, hidden, n_slots):
    return CARTPOLE._replace(env=env, dist=dist, obs_dim=d_in, small=(d_in, hidden, hidden, hidden, k, 2500),
                             n_slots=n_slots)


@pytest.mark.parametrize("n_slots", [1, 2])
@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("env,dist,d_in,k", CLASSIC)
def test_small_close_plans_k33_for_the_classic_facts(env, dist, d_in, k, hidden, n_slots):
    f = _classic(env, dist, d_in, k, hidden, n_slots)
    off, on = plan_rollout(f), plan_rollout(f._replace(small_close=True))
    assert off.driver == on.driver == ("K32W" if hidden == 128 else "K32")
    assert off.gae == ("compact" if n_slots == 1 else "fixup+scan")
    assert on == off._replace(gae="K33")   # nothing else moves
    assert on.close_launches() == ["xpa_small_close", "xpa_random_permutation"]
    assert off.close_launches() == ({1: ["xpa_gae_scan_compact"], 2: ["xpa_rollout_bootstrap_fixup", "xpa_gae_scan"]}
                                    [n_slots] + ["xpa_random_permutation"])


@pytest.mark.parametrize("change", [dict(pending=True), dict(atari=True), dict(fused_rollout=False),
                                    dict(small=None), dict(defer_boot=False, n_slots=0), dict(env="synthbox"),
                                    dict(small=(4, 256, 256, 256, 2, 2500))],
                         ids=["pending", "atari", "fused_rollout_off", "no_small_shape", "defer_boot_off",
                              "another_env", "width_256"])
def test_small_close_leaves_every_other_plan_alone(change):
    """With host closures pending, Atari's life-loss handling, a driver outside K32_DRIVERS or per-step bootstraps the
    plan is today's, switch or no switch."""
    f = CARTPOLE._replace(**change)
    assert plan_rollout(f._replace(small_close=True)) == plan_rollout(f)
    assert plan_rollout(f).gae != "K33"


def test_the_switch_is_off_by_default_and_the_parents_plans_stand():
    """RolloutFacts built without the field (as every earlier caller builds it) plans what the parent planned: the
    named cases of test_rollout_plan_cpu, written out from the predicates the planner replaced, field for field; and
    over that file's env kinds the switch changes the gae field of K32-driven plans only."""
    assert RolloutFacts._fields[-1] == "small_close" and RolloutFacts._field_defaults["small_close"] is False
    assert CARTPOLE.small_close is False and plan_rollout(CARTPOLE) == CARTPOLE_PLAN
    for name, (facts, want) in CASES.items():
        assert facts.small_close is False
        got = plan_rollout(facts)
        assert got._asdict() == want._asdict(), name
        assert got.gae in rp._GAE
    assert "K33" not in rp._GAE and rp._GAE_CLOSE["K33"] == ("xpa_small_close",)
    assert {k: v for k, v in rp._GAE_CLOSE.items() if k != "K33"} == rp._GAE
    for kind in KINDS:
        for pending in (False, True):
            f = kind._replace(pending=pending)
            off, on = plan_rollout(f), plan_rollout(f._replace(small_close=True))
            if on.gae == "K33":
                assert off.driver in rp.K32_DRIVERS and not pending and on == off._replace(gae="K33")
            else:
                assert on == off


# ---- plan_population ------------------------------------------------------------------------------------------------
def _member(i, **kw):
    f = dict(driver="K32", feed="small", entry="xpa_small_rollout_cartpole", chunk=128, dims=(4, 64, 64, 64, 2),
             activation=(1, 0.01), algo="ppo", n_envs=8, n_steps=128, n_epoch=8, batch_size=128, device="cuda:0", world=1,
             t=0, scalars=(("gamma", 0.98), ("gae_lam", 0.95), ("use_gae", True)),
             tensors=tuple(0x100000 * (i + 1) + 256 * j for j in range(6)), gae="K33")
    f.update(kw)
    return MemberFacts(**f)


def test_plan_population_batches_the_closing_when_every_member_plans_k33():
    assert MemberFacts._field_defaults == {"gae": None}
    plan = plan_population([_member(i) for i in range(3)])
    assert plan.close_batch is True and plan.n_agents == 3
    assert plan_population([_member(i, gae="compact") for i in range(3)]).close_batch is False
    assert plan_population([_member(i, gae=None) for i in range(2)]).close_batch is False
    with pytest.raises(ValueError, match=r"member 1 differs from member 0 in gae: 'compact' != 'K33'"):
        plan_population([_member(0), _member(1, gae="compact")])
    with pytest.raises(ValueError, match=r"member 2 differs from member 0 in gae_lam: 0.9 != 0.95"):
        plan_population([_member(0), _member(1), _member(2, scalars=(("gamma", 0.98), ("gae_lam", 0.9),
                                                                      ("use_gae", True)))])
    with pytest.raises(ValueError, match=r"member 1 differs from member 0 in use_gae"):
        plan_population([_member(0), _member(1, scalars=(("gamma", 0.98), ("gae_lam", 0.95), ("use_gae", False)))])


# ---- the entry points' host checks ------------------------------------------------------------------------------------
def _block(h=(64, 64, 64), **kw):
    a = _lib.XpaSmallCloseArgs()
    a.n_envs, a.horizon, a.d_in, a.k, a.act_code, a.n_slots, a.use_gae = 8, 128, 4, 2, 1, 1, 1
    a.h0, a.h1, a.h2 = h
    a.slope, a.gamma, a.gae_lambda = 0.01, 0.98, 0.95
    a.ld_rows = 4
    for name, ctype in a._fields_:
        if ctype is ctypes.c_void_p and name != "vboot_out":
            setattr(a, name, P)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _array(blocks):
    arr = (_lib.XpaSmallCloseArgs * len(blocks))(*blocks)
    return arr, ctypes.addressof(arr)


BAD = {"null_rows": dict(rows=None), "null_adv": dict(adv=None), "null_slot_t": dict(slot_t=None),
       "null_Wc": dict(Wc=None), "n_envs_257": dict(n_envs=257), "n_envs_0": dict(n_envs=0), "d_in_9": dict(d_in=9),
       "d_in_0": dict(d_in=0), "n_slots_0": dict(n_slots=0), "n_slots_past_horizon": dict(n_slots=129),
       "act_code_3": dict(act_code=3), "k_4": dict(k=4), "ld_rows_short": dict(ld_rows=3), "horizon_0": dict(horizon=0)}


@pytest.mark.parametrize("name", sorted(BAD))
def test_close_entries_reject_a_bad_block_before_any_hip_call(lib, name):
    """hipErrorInvalidValue (1) straight from the host checks, single and batch form (the bad block second: block 0 is
    valid).  Nothing was launched: the pointers are fake."""
    bad = _block(**BAD[name])
    assert lib.xpa_small_close(ctypes.byref(bad), None) == 1
    keep, blocks = _array([_block(), bad])
    assert lib.xpa_small_close_batch(2, blocks, P, None) == 1
    keep, blocks = _array([bad])
    assert lib.xpa_small_close_batch(1, blocks, P, None) == 1


def test_close_entries_reject_widths_agents_and_unequal_blocks_before_any_hip_call(lib):
    assert lib.xpa_small_close(None, None) == 1
    # 128 beside another width (K32W is all 128), and a width that is no K32 width
    for h in ((128, 64, 64), (64, 128, 64), (128, 128, 32), (48, 64, 64), (256, 256, 256)):
        assert lib.xpa_small_close(ctypes.byref(_block(h)), None) == 1, h
        keep, blocks = _array([_block(h)])
        assert lib.xpa_small_close_batch(1, blocks, P, None) == 1, h
    keep, blocks = _array([_block(), _block()])
    for n in (0, -1, 65536):
        assert lib.xpa_small_close_batch(n, blocks, P, None) == 1, n
    assert lib.xpa_small_close_batch(2, None, P, None) == 1
    assert lib.xpa_small_close_batch(2, blocks, None, None) == 1
    # every block equals block 0 in every non-pointer field: one value per launch
    for field, v in (("gamma", 0.99), ("gae_lambda", 0.9), ("slope", 0.02), ("use_gae", 0), ("n_slots", 2),
                     ("horizon", 64), ("n_envs", 5), ("ld_rows", 8), ("act_code", 2), ("h1", 32)):
        other = _block(**{field: v})   # valid alone (and so never passed alone: it would be launched)
        keep, blocks = _array([_block(), other])
        assert lib.xpa_small_close_batch(2, blocks, P, None) == 1, field
