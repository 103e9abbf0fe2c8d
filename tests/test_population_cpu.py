"""CPU: population training's host side — the header binds the three batch entry points at the same ABI version,
plan_population accepts one shape and names what rules a population out, and the batch entry points reject an empty
population and blocks of different shapes before any HIP call (so a machine without a GPU can show it)."""
import ctypes

import pytest

from xuanpolicy_amd import _lib
from xuanpolicy_amd.population import MemberFacts, PopulationPlan, plan_population

P = 0x1000   # a fake, 16-B aligned, non-null pointer: the calls below return before anything dereferences it


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def test_header_binds_batch_entry_points(lib):
    from ctypes import c_int, c_int64, c_void_p as p
    assert _lib.ABI_VERSION == 4 and lib.xpa_abi_version() == 4
    assert _lib.SIGNATURES["xpa_small_rollout_batch"] == (c_int, [c_int, c_int64, p, p, p, p, p])
    assert _lib.SIGNATURES["xpa_small_mlp_update_batch"] == (c_int, [c_int64, p, p, p, p, p])
    assert _lib.SIGNATURES["xpa_random_permutation_batch"] == (c_int, [c_int64, c_int64, p, p, p, p])
    for name in ("xpa_small_rollout_batch", "xpa_small_mlp_update_batch", "xpa_random_permutation_batch"):
        assert hasattr(lib, name)
    # the per-agent extras of the Gaussian heads: (logstd, act_clip) and (logstd, g_logstd), 16 bytes each
    assert ctypes.sizeof(_lib.XpaSmallRolloutHead) == 16 and ctypes.sizeof(_lib.XpaSmallMlpGauss) == 16
    assert [_lib.ENV_CODES["XPA_ENV_" + n] for n in ("CARTPOLE", "PENDULUM", "ACROBOT", "MOUNTAINCAR")] == [0, 1, 2, 3]


# ---- plan_population ----------------------------------------------------------------------------------------------
def _facts(i, hidden=64, env="cartpole", n_steps=128, feed="small", world=1, **kw):
    entry, d_in, k = {"cartpole": ("xpa_small_rollout_cartpole", 4, 2),
                      "acrobot": ("xpa_small_rollout_acrobot", 6, 3)}[env]
    f = dict(driver="K32W" if hidden == 128 else "K32", feed=feed, entry=entry, chunk=min(n_steps, 128),
             dims=(d_in, hidden, hidden, hidden, k), activation=(1, 0.01), algo="ppo", n_envs=8, n_steps=n_steps,
             n_epoch=8, batch_size=8 * n_steps // 8, device="cuda:0", world=world, t=0,
             scalars=(("gamma", 0.98), ("vf_coef", 0.25)), tensors=tuple(0x100000 * (i + 1) + 256 * j for j in range(6)))
    f.update(kw)
    return MemberFacts(**f)


def test_plan_accepts_one_shape():
    plan = plan_population([_facts(i) for i in range(3)])
    assert plan == PopulationPlan(3, "xpa_small_rollout_cartpole", "XPA_ENV_CARTPOLE", False, 128)
    wide = plan_population([_facts(i, hidden=128, env="acrobot") for i in range(3)])
    assert wide.entry == "xpa_small_rollout_acrobot" and wide.env == "XPA_ENV_ACROBOT" and wide.n_agents == 3


@pytest.mark.parametrize("members, reason", [
    ([_facts(0), _facts(1, hidden=128), _facts(2)], r"member 1 differs from member 0 in dims"),
    ([_facts(0), _facts(1), _facts(2, env="acrobot")], r"member 2 differs from member 0 in entry"),
    ([_facts(0), _facts(1, n_steps=64)], r"member 1 differs from member 0 in n_steps: 64 != 128"),
    ([_facts(0), _facts(1, feed="epoch")], r"member 1: minibatch feed 'epoch'"),
    ([_facts(0, world=2), _facts(1, world=2)], r"member 0: world size 2"),
    ([_facts(0), _facts(1, driver="graph-chunk", entry=None)], r"member 1: rollout driver 'graph-chunk'"),
    ([_facts(0), _facts(1, scalars=(("gamma", 0.99), ("vf_coef", 0.25)))],
     r"member 1 differs from member 0 in gamma: 0.99 != 0.98"),
    ([_facts(0), _facts(1, tensors=_facts(0).tensors[2:3])], r"members 0 and 1 share a tensor"),
    ([], r"1 \.\. 65535 members"),
])
def test_plan_names_the_reason(members, reason):
    with pytest.raises(ValueError, match=reason):
        plan_population(members)


# ---- the entry points' host checks ---------------------------------------------------------------------------------
def _rollout_block(h=64):
    a = _lib.XpaSmallRolloutArgs()
    a.n_envs, a.horizon, a.steps, a.d_in, a.h0, a.h1, a.h2, a.k = 8, 128, 16, 4, h, h, h, 2
    a.act_code, a.use_obsnorm, a.n_slots, a.mask_returns, a.use_rewnorm, a.max_episode_steps = 1, 1, 1, 1, 1, 500
    a.slope, a.obs_clip, a.gamma, a.rew_range = 0.01, 5.0, 0.98, 5.0
    a.ld_norm = a.ld_obs = a.ld_boot = 4
    a.ld_act = 2
    for name, ctype in a._fields_:
        if ctype is ctypes.c_void_p and name != "stamps":
            setattr(a, name, P)
    return a


def _mlp_block(h=64):
    a = _lib.XpaSmallMlpArgs()
    a.batch, a.d_in, a.h0, a.h1, a.h2, a.k, a.act_code, a.algo, a.use_advnorm, a.n_sched = 20, 4, h, h, h, 2, 1, 0, 1, 256
    a.obs_ld, a.n_rows, a.n, a.n_groups = 4, 100, 9000, 1
    for name, ctype in a._fields_:
        if ctype is ctypes.c_void_p and name not in ("stamps", "grad_part", "loss_part"):
            setattr(a, name, P)
    return a


def _array(blocks):
    arr = (type(blocks[0]) * len(blocks))(*blocks)
    return arr, ctypes.addressof(arr)


def test_batch_entries_reject_before_any_hip_call(lib):
    """hipErrorInvalidValue (1) straight from the host checks: no agent, and a block 1 whose h0 is not block 0's (both
    blocks valid on their own: 32 / 64 are K32's widths, every width a K30 one).  Nothing was launched: the pointers
    are fake."""
    for h1 in (32, 64):
        keep, blocks = _array([_rollout_block(64), _rollout_block(h1)])
        assert lib.xpa_small_rollout_batch(0, 0, blocks, P, None, None, None) == 1
        assert lib.xpa_small_rollout_batch(0, -3, blocks, P, None, None, None) == 1
        if h1 != 64:
            assert lib.xpa_small_rollout_batch(0, 2, blocks, P, None, None, None) == 1
        keep, blocks = _array([_mlp_block(64), _mlp_block(h1)])
        assert lib.xpa_small_mlp_update_batch(0, blocks, P, None, None, None) == 1
        if h1 != 64:
            assert lib.xpa_small_mlp_update_batch(2, blocks, P, None, None, None) == 1
    # a scalar that differs is a shape difference too (one kernel-argument value per launch); seeds are per agent
    a, b = _rollout_block(), _rollout_block()
    b.gamma = 0.99
    keep, blocks = _array([a, b])
    assert lib.xpa_small_rollout_batch(0, 2, blocks, P, None, None, None) == 1
    # the wrong env code, a Gaussian env without its head arrays, head arrays given on one side only
    keep, blocks = _array([_rollout_block()])
    assert lib.xpa_small_rollout_batch(7, 1, blocks, P, None, None, None) == 1
    assert lib.xpa_small_rollout_batch(1, 1, blocks, P, None, None, None) == 1
    keep, blocks = _array([_mlp_block()])
    assert lib.xpa_small_mlp_update_batch(1, blocks, P, P, None, None) == 1
    assert lib.xpa_random_permutation_batch(80, 0, P, P, P, None) == 1
    assert lib.xpa_random_permutation_batch(0, 3, P, P, P, None) == 1
