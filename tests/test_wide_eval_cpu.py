"""CPU: the 128-wide one-launch evaluation (K32WE / K32WEB) and the batched test-env reset, host side — plan_test's
opt-in tier, plan_population_test over it, the three entry points in the header, the bindings and the library, and
their refusals before any HIP call (fake pointers: a launch would fault, a return value of 1 means none was made)."""
import ctypes

import pytest

from xuanpolicy_amd import _lib
from xuanpolicy_amd.population import EvalMemberFacts, PopulationTestPlan, plan_population_test
from xuanpolicy_amd.rollout_plan import EvalFacts, plan_test

P = 0x1000   # a fake, 16-B aligned, non-null pointer: the calls below return before anything dereferences it
ENTRIES = ("xpa_small_eval_wide", "xpa_small_eval_wide_batch", "xpa_small_env_reset_batch")


# ---- plan_test -----------------------------------------------------------------------------------------------------
def _eval_facts(widths=(128, 128, 128), wide_eval=True, n_envs=10, lds=12000, raw_obs=False, cuda=True):
    return EvalFacts(cuda=cuda, env="cartpole", dist="categorical", small=(4,) + tuple(widths) + (2, lds),
                     n_envs=n_envs, obs_dim=4, raw_obs=raw_obs, world=1, sync_obs_rms=False, wide_eval=wide_eval)


@pytest.mark.parametrize("facts, tier", [
    (_eval_facts(), "K32WE"),
    (_eval_facts(wide_eval=False), "steps"),
    (_eval_facts(widths=(128, 64, 64)), "steps"),
    (_eval_facts(widths=(64, 64, 64)), "K32E"),
    (_eval_facts(n_envs=257), "steps"),
    (_eval_facts(lds=0), "steps"),
    (_eval_facts(lds=16385), "steps"),
    (_eval_facts(lds=16384), "K32WE"),
    (_eval_facts(raw_obs=True), "steps"),
    (_eval_facts(cuda=False), "host"),
])
def test_plan_test_table(facts, tier):
    assert plan_test(facts) == tier


def test_flag_off_plans_as_before():
    """wide_eval is the trailing field and defaults to off: facts built without it plan what they planned."""
    assert EvalFacts._fields[-1] == "wide_eval" and EvalFacts._field_defaults == {"wide_eval": False}
    for widths in ((32, 64, 32), (64, 64, 64), (128, 128, 128), (128, 64, 128), (256, 256, 256)):
        on, off = _eval_facts(widths=widths), _eval_facts(widths=widths, wide_eval=False)
        old = EvalFacts(*off[:-1])
        assert old == off and plan_test(old) == plan_test(off)
        if widths != (128, 128, 128):
            assert plan_test(on) == plan_test(off)


# ---- plan_population_test ------------------------------------------------------------------------------------------
def _member(i, **kw):
    return EvalMemberFacts(eval=_eval_facts(**kw), activation=(1, 0.01), use_obsnorm=True, obs_clip=5.0,
                           max_episode_steps=500, tensors=tuple(0x100000 * (i + 1) + 256 * j for j in range(15)))


def test_population_plan_over_the_wide_tier():
    assert PopulationTestPlan._fields[-1] == "wide" and PopulationTestPlan._field_defaults == {"wide": False}
    plan = plan_population_test([_member(i) for i in range(3)])
    assert plan == PopulationTestPlan(3, "XPA_ENV_CARTPOLE", False, True) and plan.wide
    assert not plan_population_test([_member(i, widths=(64, 64, 64)) for i in range(3)]).wide
    with pytest.raises(ValueError, match=r"member 2: its test envs plan the 'K32E' tier, member 0's the 'K32WE' tier"):
        plan_population_test([_member(0), _member(1), _member(2, widths=(64, 64, 64))])
    with pytest.raises(ValueError, match=r"member 1: its test envs plan the 'K32WE' tier, member 0's the 'K32E' tier"):
        plan_population_test([_member(0, widths=(64, 64, 64)), _member(1)])
    with pytest.raises(ValueError, match=r"member 1: its test envs plan the 'steps' tier, not the one-launch "
                                         r"evaluation \"K32E\""):
        plan_population_test([_member(0), _member(1, wide_eval=False)])


# ---- the header, the bindings and the library ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def test_entry_points_are_declared_bound_and_exported(lib):
    from ctypes import c_int, c_int64, c_void_p as p
    assert _lib.ABI_VERSION == 4 and lib.xpa_abi_version() == 4    # additions only
    want = {"xpa_small_eval_wide": [c_int, p, p, p, c_int64, c_int64, p, p],
            "xpa_small_eval_wide_batch": [c_int, c_int64, p, p, p, p, p, p, p],
            "xpa_small_env_reset_batch": [c_int, c_int64, p, p, p]}
    assert set(want) == set(ENTRIES)
    for name, args in want.items():
        assert _lib.SIGNATURES[name] == (c_int, args), name
        fn = getattr(lib, name)      # exported
        assert fn.restype is c_int and list(fn.argtypes) == args, name
    assert _lib.SIGNATURES["xpa_small_eval_wide_batch"] == _lib.SIGNATURES["xpa_small_eval_batch"]


# ---- the host checks -----------------------------------------------------------------------------------------------
_ENV = {0: (4, 2), 1: (3, 1), 2: (6, 3), 3: (8, 3)}   # XPA_ENV_* code -> (d_in, k)


def _block(env=0, h=(128, 128, 128), n_envs=8, **kw):
    a = _lib.XpaSmallRolloutArgs()
    d_in, k = _ENV[env]
    a.n_envs, a.horizon, a.steps, a.d_in, a.k = n_envs, 1, 16, d_in, k
    a.h0, a.h1, a.h2 = h
    a.act_code, a.use_obsnorm, a.max_episode_steps = 1, 1, 500
    a.slope, a.obs_clip = 0.01, 5.0
    a.ld_obs, a.ld_act = d_in, k
    for name in ("W0", "b0", "W1", "b1", "W2", "b2", "Wa", "ba", "Wc", "bc", "obs_mean", "obs_var", "obs_count",
                 "act_in", "env_obs", "final_obs", "env_rew", "env_term", "env_trunc", "ep_step", "ep_index",
                 "ep_score", "ep_last_score", "ep_last_len", "cursor"):
        setattr(a, name, P)     # what the evaluation form and the reset read; the training-only pointers stay NULL
    a.env_state = P
    for name, v in kw.items():
        setattr(a, name, v)
    return a


def _array(items):
    arr = (type(items[0]) * len(items))(*items)
    return arr, ctypes.addressof(arr)


def _evals(n, **kw):
    items = [_lib.XpaSmallEval(P + 0x1000 * (i + 1), P + 0x100000 * (i + 1), 18, 4) for i in range(n)]
    for name, v in kw.items():
        setattr(items[1], name, v)
    return _array(items)


def _blocks(n, env=0, **kw):
    """n blocks with an env set each (distinct env_state); kw changes block 1."""
    items = [_block(env, env_state=P + 0x10000 * (i + 1)) for i in range(n)]
    for name, v in kw.items():
        setattr(items[1], name, v)
    return _array(items)


def test_eval_wide_rejects_before_any_hip_call(lib):
    fn = lib.xpa_small_eval_wide
    head = _lib.XpaSmallRolloutHead(P, 2.0)
    ok = dict(log=P, capacity=18, snap_dim=4, scratch=P)

    def call(env, block, head=None, **kw):
        a = dict(ok, **kw)
        return fn(env, ctypes.byref(block) if block is not None else None,
                  ctypes.byref(head) if head is not None else None, a["log"], a["capacity"], a["snap_dim"],
                  a["scratch"], None)
    assert call(0, _block(h=(64, 64, 64))) == 1              # K32E's widths are refused here, as 128 is there
    assert call(0, _block(h=(32, 32, 32))) == 1
    assert call(0, _block(h=(128, 64, 128))) == 1
    assert call(0, _block(h=(128, 128, 64))) == 1
    assert call(7, _block()) == 1                             # no such env
    assert call(-1, _block()) == 1
    assert call(1, _block(env=1)) == 1                        # Pendulum without a head
    assert call(1, _block(env=1), _lib.XpaSmallRolloutHead(None, 2.0)) == 1    # ... without a logstd
    assert call(1, _block(env=1), _lib.XpaSmallRolloutHead(P, 0.0)) == 1       # ... with act_clip 0
    assert call(0, _block(), head) == 1                       # CartPole with one
    assert call(2, _block(env=2), head) == 1
    assert call(0, _block(), log=P + 4) == 1                  # an unaligned log
    assert call(0, _block(), log=None) == 1
    assert call(0, _block(), capacity=0) == 1
    assert call(0, _block(), capacity=1 << 31) == 1
    assert call(0, _block(), snap_dim=-1) == 1
    assert call(0, _block(), scratch=None) == 1
    assert call(0, None) == 1
    assert call(0, _block(env=2)) == 1                        # another env's d_in / k
    assert call(0, _block(n_envs=257)) == 1
    assert call(0, _block(steps=0)) == 1
    assert call(0, _block(env_state=None)) == 1
    assert call(0, _block(cursor=None)) == 1


def test_eval_wide_batch_rejects_before_any_hip_call(lib):
    fn = lib.xpa_small_eval_wide_batch
    keep_b, blocks = _blocks(2)
    keep_e, evals = _evals(2)
    assert fn(0, 0, blocks, P, None, None, evals, P, None) == 1        # no agent
    assert fn(0, -1, blocks, P, None, None, evals, P, None) == 1
    assert fn(0, 1 << 31, blocks, P, None, None, evals, P, None) == 1
    assert fn(7, 2, blocks, P, None, None, evals, P, None) == 1        # no such env
    assert fn(0, 2, blocks, None, None, None, evals, P, None) == 1     # an array missing
    assert fn(0, 2, blocks, P, None, None, evals, None, None) == 1
    for change in (dict(obs_clip=10.0), dict(n_envs=9), dict(steps=17), dict(use_obsnorm=0), dict(slope=0.0),
                   dict(max_episode_steps=499), dict(ld_obs=8), dict(h1=64)):
        keep_o, other = _blocks(2, **change)
        assert fn(0, 2, other, P, None, None, evals, P, None) == 1, change
    keep_o, other = _array([_block(h=(64, 64, 64)), _block(h=(64, 64, 64))])   # K32EB's widths
    assert fn(0, 2, other, P, None, None, evals, P, None) == 1
    for change in (dict(log=P + 0x1000), dict(scratch=P + 0x100000), dict(log=None), dict(log=P + 0x2000 + 4),
                   dict(scratch=None), dict(capacity=19), dict(capacity=0), dict(snap_dim=3)):
        keep_o, other = _evals(2, **change)                            # a shared log, a shared scratch, ...
        assert fn(0, 2, blocks, P, None, None, other, P, None) == 1, change
    keep_h, heads = _array([_lib.XpaSmallRolloutHead(P, 2.0), _lib.XpaSmallRolloutHead(P, 2.0)])
    assert fn(0, 2, blocks, P, heads, P, evals, P, None) == 1          # head arrays for a Categorical env
    keep_p, pblocks = _blocks(2, env=1)
    assert fn(1, 2, pblocks, P, None, None, evals, P, None) == 1       # none for the Gaussian one
    assert fn(1, 2, pblocks, P, heads, None, evals, P, None) == 1      # heads on one side only
    assert fn(1, 2, pblocks, P, None, P, evals, P, None) == 1
    keep_h, bad = _array([_lib.XpaSmallRolloutHead(P, 2.0), _lib.XpaSmallRolloutHead(None, 2.0)])
    assert fn(1, 2, pblocks, P, bad, P, evals, P, None) == 1


def test_env_reset_batch_rejects_before_any_hip_call(lib):
    fn = lib.xpa_small_env_reset_batch
    keep_b, blocks = _blocks(2)
    assert fn(0, 0, blocks, P, None) == 1                              # no agent
    assert fn(0, -1, blocks, P, None) == 1
    assert fn(0, 1 << 31, blocks, P, None) == 1
    assert fn(4, 2, blocks, P, None) == 1                              # no such env
    assert fn(-1, 2, blocks, P, None) == 1
    assert fn(0, 2, None, P, None) == 1                                # an array missing
    assert fn(0, 2, blocks, None, None) == 1
    assert fn(2, 2, blocks, P, None) == 1                              # CartPole's blocks under Acrobot's code
    for change in (dict(n_envs=9), dict(n_envs=0), dict(d_in=3), dict(k=3), dict(ld_obs=3), dict(ld_act=1),
                   dict(env_state=None), dict(env_state=P + 0x10000), dict(env_obs=None), dict(act_in=None),
                   dict(env_rew=None), dict(env_term=None), dict(env_trunc=None), dict(ep_step=None),
                   dict(ep_index=None), dict(ep_score=None), dict(ep_last_score=None), dict(ep_last_len=None)):
        keep_o, other = _blocks(2, **change)                           # differing n_envs, ..., a shared env_state
        assert fn(0, 2, other, P, None) == 1, change
    keep_o, other = _array([_block(n_envs=257, env_state=P + 0x10000), _block(n_envs=257, env_state=P + 0x20000)])
    assert fn(0, 2, other, P, None) == 1
