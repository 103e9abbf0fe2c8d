"""CPU: the one statement of the small path's envs (rollout_plan.SMALL_ENVS) against the header's bindings and the
planner, and small_path's one filler of the fields the three argument structs share (no device: CPU tensors only give
addresses)."""
import ctypes

import pytest
import torch

from xuanpolicy_amd import _lib, small_path
from xuanpolicy_amd.rollout_plan import SMALL_ENVS, EvalFacts, RolloutFacts, eval_entry, plan_rollout, plan_test

PAIRS = sorted(SMALL_ENVS)   # (env, dist)


def test_every_row_names_bound_symbols_and_a_header_constant():
    assert PAIRS == [("acrobot", "categorical"), ("cartpole", "categorical"), ("mountaincar", "categorical"),
                     ("pendulum", "gaussian")]
    for row in SMALL_ENVS.values():
        assert row.rollout in _lib.SIGNATURES and row.eval in _lib.SIGNATURES and row.code in _lib.ENV_CODES
    assert len({row.code for row in SMALL_ENVS.values()}) == len(SMALL_ENVS)   # one env code per row


def test_gaussian_rows_are_the_ones_whose_signatures_take_the_head():
    cat = SMALL_ENVS["cartpole", "categorical"]
    assert not cat.gaussian
    head = [ctypes.c_void_p, ctypes.c_float]   # (logstd, act_clip), after the block
    for row in SMALL_ENVS.values():
        for name, base in ((row.rollout, cat.rollout), (row.eval, cat.eval)):
            (res, args), (res0, args0) = _lib.SIGNATURES[name], _lib.SIGNATURES[base]
            assert res is res0
            assert row.gaussian == (args == args0[:1] + head + args0[1:])
            assert (not row.gaussian) == (args == args0)


@pytest.mark.parametrize("env,dist", PAIRS)
def test_planner_and_eval_entry_return_the_rows_names(env, dist):
    row = SMALL_ENVS[env, dist]
    f = RolloutFacts(
        algo="ppo", fuse_env_step=True, fuse_post=True, fold_rms=False, fuse_value_gae=True, value_gemm=False,
        fuse_gather=True, fused_rollout=True, use_graph=True, graph_chunk=128, rollout_split=True, rollout_trunk=False,
        s3_gemms=True, cuda=True, use_obsnorm=True, raw_obs=False, atari=False, boot_from_reset=False, defer_boot=True,
        raw_defer=False, raw_mid_next=False, n_slots=1, n_steps=128, obs_dim=row.d_in, world=1, sync_obs_rms=False,
        global_advnorm=False, pending=False, env=env, env_fusable=False, obs_rows=True, shape=None, cnn=False,
        small=(row.d_in, 64, 64, 64, row.k, 2500), small_bufs=True, rows_ok=False, small_update=True,
        epoch_graphs=True, dist=dist)
    plan = plan_rollout(f)
    assert plan.driver == "K32" and plan.step_launches() == [row.rollout]
    e = EvalFacts(cuda=True, env=env, dist=dist, small=(row.d_in, 64, 64, 64, row.k, 200), n_envs=5, obs_dim=row.d_in,
                  raw_obs=False, world=1, sync_obs_rms=False)
    assert plan_test(e) == "K32E" and eval_entry(e) == row.eval


def _layers():
    torch.manual_seed(0)
    sizes = ((3, 32), (32, 64), (64, 1), (32, 32), (32, 1))   # l0, l1 (actor hidden), la, l2 (critic hidden), lc
    return tuple(torch.nn.Linear(i, o) for i, o in sizes)


@pytest.mark.parametrize("struct", ["XpaSmallRolloutArgs", "XpaSmallCloseArgs", "XpaSmallMlpArgs"])
def test_fill_writes_the_seventeen_shared_fields(struct):
    layers = l0, l1, la, l2, lc = _layers()
    policy = small_path.SmallPolicy(layers, 2, 0.25, None)
    got_layers, code, slope, logstd = policy   # callers that unpack four values
    assert got_layers is layers and (code, slope, logstd) == (2, 0.25, None)
    assert policy.dims == (3, 32, 64, 32, 1)
    assert policy.rollout_shape(5, 3, cuda=False) == (3, 32, 64, 32, 1, 0)
    blank = getattr(_lib, struct)()
    a = policy.fill(getattr(_lib, struct)())
    assert (a.d_in, a.h0, a.h1, a.h2, a.k, a.act_code, a.slope) == (3, 32, 64, 32, 1, 2, 0.25)
    want = {"W0": l0.weight, "b0": l0.bias, "W1": l1.weight, "b1": l1.bias, "W2": l2.weight, "b2": l2.bias,
            "Wa": la.weight, "ba": la.bias, "Wc": lc.weight, "bc": lc.bias}
    for name, t in want.items():
        assert getattr(a, name) == t.data_ptr() != 0, name
    shared = set(want) | {"d_in", "h0", "h1", "h2", "k", "act_code", "slope"}
    assert len(shared) == 17
    for name, _ in a._fields_:   # and nothing else
        if name not in shared:
            assert getattr(a, name) == getattr(blank, name), name


def test_small_close_args_equals_a_block_filled_by_hand():
    layers = l0, l1, la, l2, lc = _layers()
    N, T, S = 2, 4, 1
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32)   # noqa: E731
    rows, slot_t = f32((S + 1) * N, 3), torch.zeros(S * N, dtype=torch.int32)
    rew, val, term, boot, adv, ret = (f32(N, T) for _ in range(6))
    closed, vboot = torch.zeros((N, T), dtype=torch.uint8), f32((S + 1) * N)
    got = small_path.small_close_args(layers, (1, 0.01), rows, slot_t, rew, val, term, closed, boot, adv, ret, 0.99,
                                      0.95, True, vboot_out=vboot)
    a = _lib.XpaSmallCloseArgs()
    a.n_envs, a.horizon, a.d_in, a.h0, a.h1, a.h2, a.k, a.act_code, a.n_slots, a.use_gae = N, T, 3, 32, 64, 32, 1, 1, S, 1
    a.slope, a.gamma, a.gae_lambda = 0.01, 0.99, 0.95
    a.W0, a.b0, a.W1, a.b1 = l0.weight.data_ptr(), l0.bias.data_ptr(), l1.weight.data_ptr(), l1.bias.data_ptr()
    a.W2, a.b2, a.Wa, a.ba = l2.weight.data_ptr(), l2.bias.data_ptr(), la.weight.data_ptr(), la.bias.data_ptr()
    a.Wc, a.bc = lc.weight.data_ptr(), lc.bias.data_ptr()
    a.rows, a.ld_rows, a.slot_t = rows.data_ptr(), 3, slot_t.data_ptr()
    a.rew, a.val, a.term, a.closed = rew.data_ptr(), val.data_ptr(), term.data_ptr(), closed.data_ptr()
    a.boot, a.adv, a.ret, a.vboot_out = boot.data_ptr(), adv.data_ptr(), ret.data_ptr(), vboot.data_ptr()
    assert bytes(got) == bytes(a)
    from xuanpolicy_amd import ops
    assert ops.small_close_args is small_path.small_close_args
    # the dtype and contiguity checks on the weights hold off the device too
    bad = (torch.nn.Linear(3, 32).double(),) + layers[1:]
    with pytest.raises(TypeError, match="W0"):
        small_path.small_close_args(bad, (1, 0.01), rows, slot_t, rew, val, term, closed, boot, adv, ret, 0.99, 0.95)
