"""CPU: population evaluation's host side — plan_population_test admits one shape and names the member and the field
that rule a population out; the header declares XpaSmallEval and xpa_small_eval_batch, and the bindings follow it;
the entry point refuses an empty population and mismatched members before any HIP call."""
import ctypes

import pytest

from xuanpolicy_amd import _lib
from xuanpolicy_amd.population import EvalMemberFacts, PopulationTestPlan, plan_population_test
from xuanpolicy_amd.rollout_plan import EvalFacts

P = 0x1000   # a fake, 16-B aligned, non-null pointer: the calls below return before anything dereferences it


# ---- plan_population_test ------------------------------------------------------------------------------------------
_SHAPES = {"cartpole": ("categorical", 4, 2), "pendulum": ("gaussian", 3, 1), "acrobot": ("categorical", 6, 3)}


def _facts(i, env="cartpole", hidden=64, n_envs=8, world=1, cuda=True, sync=False, **kw):
    dist, d_in, k = _SHAPES[env]
    ev = EvalFacts(cuda=cuda, env=env, dist=dist, small=(d_in, hidden, hidden, hidden, k, 1500), n_envs=n_envs,
                   obs_dim=d_in, raw_obs=False, world=world, sync_obs_rms=sync)
    f = dict(eval=ev, activation=(1, 0.01), use_obsnorm=True, obs_clip=5.0, max_episode_steps=500,
             tensors=tuple(0x100000 * (i + 1) + 256 * j for j in range(15)))
    f.update(kw)
    return EvalMemberFacts(**f)


def test_plan_admits_one_shape():
    assert plan_population_test([_facts(i) for i in range(3)]) == PopulationTestPlan(3, "XPA_ENV_CARTPOLE", False)
    assert plan_population_test([_facts(0, hidden=32)]) == PopulationTestPlan(1, "XPA_ENV_CARTPOLE", False)
    gauss = plan_population_test([_facts(i, env="pendulum") for i in range(2)])
    assert gauss == PopulationTestPlan(2, "XPA_ENV_PENDULUM", True)
    # the evaluation's action stream is per member: nothing of it is in the facts, so seeds differ freely


@pytest.mark.parametrize("members, reason", [
    # a member that does not plan "K32E": 128-wide layers (the "steps" tier), a host device, too many test envs
    ([_facts(0), _facts(1, hidden=128)], r"member 1: its test envs plan the 'steps' tier"),
    ([_facts(0, cuda=False)], r"member 0: its test envs plan the 'host' tier"),
    ([_facts(0), _facts(1), _facts(2, n_envs=300)], r"member 2: its test envs plan the 'steps' tier"),
    # one difference from member 0 per shared field
    ([_facts(0), _facts(1, env="acrobot")], r"member 1 differs from member 0 in env: 'acrobot' != 'cartpole'"),
    ([_facts(0), _facts(1)._replace(eval=_facts(1).eval._replace(dist="gaussian"))],
     r"member 1: its test envs plan the 'steps' tier"),   # (cartpole, gaussian) is no small-path pair at all
    ([_facts(0), _facts(1, hidden=32)], r"member 1 differs from member 0 in small: \(4, 32, 32, 32, 2, 1500\)"),
    ([_facts(0), _facts(1), _facts(2, n_envs=9)], r"member 2 differs from member 0 in n_envs: 9 != 8"),
    ([_facts(0), _facts(1, activation=(0, 0.0))], r"member 1 differs from member 0 in activation: \(0, 0.0\) != \(1, 0.01\)"),
    ([_facts(0), _facts(1, use_obsnorm=False)], r"member 1 differs from member 0 in use_obsnorm: False != True"),
    ([_facts(0), _facts(1, obs_clip=10.0)], r"member 1 differs from member 0 in obs_clip: 10.0 != 5.0"),
    ([_facts(0), _facts(1, max_episode_steps=200)], r"member 1 differs from member 0 in max_episode_steps: 200 != 500"),
    # two members sharing a tensor (the same test envs given twice; shared obs statistics)
    ([_facts(0), _facts(1), _facts(2, tensors=_facts(0).tensors)], r"members 0 and 2 share a tensor"),
    ([_facts(0), _facts(1, tensors=_facts(1).tensors[:14] + _facts(0).tensors[14:])],
     r"members 0 and 1 share a tensor \(data pointer 0x100e00\)"),
    # world != 1, with or without the per-step collective
    ([_facts(0), _facts(1, world=2)], r"member 1: world size 2"),
    ([_facts(0, world=2, sync=True)], r"member 0: world size 2"),
    ([], r"1 \.\. 65535 members"),
])
def test_plan_names_the_member_and_the_field(members, reason):
    with pytest.raises(ValueError, match=reason):
        plan_population_test(members)


def test_dist_difference_is_named():
    """A dist that differs while both members still plan K32E cannot be built from SMALL_ENVS' rows (an env kind has
    one head there), so the rule is exercised on the table: a second head for an env makes it reachable."""
    from xuanpolicy_amd import rollout_plan
    row = rollout_plan.SMALL_ENVS["pendulum", "gaussian"]
    extra = dict(rollout_plan.SMALL_ENVS)
    extra["cartpole", "gaussian"] = row._replace(d_in=4, k=2)
    other = _facts(1)._replace(eval=_facts(1).eval._replace(dist="gaussian"))
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(rollout_plan, "SMALL_ENVS", extra)
        with pytest.raises(ValueError, match=r"member 1 differs from member 0 in dist: 'gaussian' != 'categorical'"):
            plan_population_test([_facts(0), other])


# ---- the header and the bindings -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def test_header_declares_and_binds_the_batch_evaluation(lib):
    from ctypes import c_int, c_int64, c_void_p as p
    with open(_lib.HEADER) as f:
        text = f.read()
    assert "typedef struct XpaSmallEval {" in text and "int xpa_small_eval_batch(int env, int64_t n_agents," in text
    assert _lib.ABI_VERSION == 4 and lib.xpa_abi_version() == 4    # additions only
    assert _lib.SIGNATURES["xpa_small_eval_batch"] == (c_int, [c_int, c_int64, p, p, p, p, p, p, p])
    fn = lib.xpa_small_eval_batch
    assert fn.restype is c_int and list(fn.argtypes) == [c_int, c_int64, p, p, p, p, p, p, p]
    assert [n for n, _ in _lib.XpaSmallEval._fields_] == ["log", "scratch", "capacity", "snap_dim"]
    assert ctypes.sizeof(_lib.XpaSmallEval) == 32


# ---- the entry point's host checks ---------------------------------------------------------------------------------
def _block(h=64, n_envs=8):
    a = _lib.XpaSmallRolloutArgs()
    a.n_envs, a.horizon, a.steps, a.d_in, a.h0, a.h1, a.h2, a.k = n_envs, 1, 16, 4, h, h, h, 2
    a.act_code, a.use_obsnorm, a.max_episode_steps = 1, 1, 500
    a.slope, a.obs_clip = 0.01, 5.0
    a.ld_obs, a.ld_act = 4, 2
    for name in ("W0", "b0", "W1", "b1", "W2", "b2", "Wa", "ba", "Wc", "bc", "obs_mean", "obs_var", "obs_count",
                 "act_in", "env_state", "env_obs", "final_obs", "env_rew", "env_term", "env_trunc", "ep_step",
                 "ep_index", "ep_score", "ep_last_score", "ep_last_len", "cursor"):
        setattr(a, name, P)     # what the evaluation form reads; the training-only pointers stay NULL
    return a


def _array(items):
    arr = (type(items[0]) * len(items))(*items)
    return arr, ctypes.addressof(arr)


def _evals(n, capacity=18):
    return _array([_lib.XpaSmallEval(P + 0x1000 * (i + 1), P + 0x100000 * (i + 1), capacity, 4) for i in range(n)])


def test_batch_evaluation_rejects_before_any_hip_call(lib):
    """hipErrorInvalidValue (1) straight from the host checks — the pointers are fake, so a launch would fault."""
    fn = lib.xpa_small_eval_batch
    keep_b, blocks = _array([_block(), _block()])
    keep_e, evals = _evals(2)
    assert fn(0, 0, blocks, P, None, None, evals, P, None) == 1        # no agent
    assert fn(0, -1, blocks, P, None, None, evals, P, None) == 1
    assert fn(0, 1 << 31, blocks, P, None, None, evals, P, None) == 1
    assert fn(7, 2, blocks, P, None, None, evals, P, None) == 1        # no such env
    assert fn(0, 2, blocks, None, None, None, evals, P, None) == 1     # an array missing
    assert fn(0, 2, blocks, P, None, None, None, P, None) == 1
    assert fn(0, 2, blocks, P, None, None, evals, None, None) == 1
    keep_h, heads = _array([_lib.XpaSmallRolloutHead(P, 2.0), _lib.XpaSmallRolloutHead(P, 2.0)])
    assert fn(0, 2, blocks, P, heads, P, evals, P, None) == 1          # head arrays for a Categorical env
    assert fn(1, 2, blocks, P, None, None, evals, P, None) == 1        # none for the Gaussian one
    for change in (dict(n_envs=9), dict(steps=17), dict(h0=32), dict(use_obsnorm=0), dict(max_episode_steps=499),
                   dict(obs_clip=10.0), dict(slope=0.0), dict(ld_obs=8)):
        other = _block()
        for k, v in change.items():
            setattr(other, k, v)
        keep_b, blocks = _array([_block(), other])
        assert fn(0, 2, blocks, P, None, None, evals, P, None) == 1, change
    keep_b, blocks = _array([_block(128), _block(128)])                 # no 128-wide evaluation instantiation
    assert fn(0, 2, blocks, P, None, None, evals, P, None) == 1
    keep_b, blocks = _array([_block(), _block()])
    for i, change in enumerate((dict(log=None), dict(log=P + 4), dict(log=P + 0x1000), dict(scratch=None),
                                dict(scratch=P + 0x100000), dict(capacity=19), dict(capacity=0), dict(snap_dim=3))):
        keep_e, evals = _evals(2)
        for k, v in change.items():
            setattr(keep_e[1], k, v)
        assert fn(0, 2, blocks, P, None, None, evals, P, None) == 1, change
    keep_e, evals = _evals(2, capacity=1 << 31)
    assert fn(0, 2, blocks, P, None, None, evals, P, None) == 1
