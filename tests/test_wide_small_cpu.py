"""CPU: the planner's side of the one-launch small path at the reference's 128-wide classic-control nets — the K32W
grant of plan_rollout (the rollout at h0 = h1 = h2 = 128), what it is not granted for, and what stays as it was (K32 at
32 / 64, the evaluation tier at 128)."""
import pytest

from xuanpolicy_amd import _lib
from xuanpolicy_amd.rollout_plan import _K32, EvalFacts, RolloutFacts, plan_rollout, plan_test

BASE = RolloutFacts(
    algo="ppo", fuse_env_step=True, fuse_post=True, fold_rms=False, fuse_value_gae=True, value_gemm=False,
    fuse_gather=True, fused_rollout=True, use_graph=True, graph_chunk=128, rollout_split=True, rollout_trunk=False,
    s3_gemms=True, cuda=True, use_obsnorm=True, raw_obs=False, atari=False, boot_from_reset=False, defer_boot=True,
    raw_defer=False, raw_mid_next=False, n_slots=1, n_steps=128, obs_dim=4, world=1, sync_obs_rms=False,
    global_advnorm=False, pending=False, env="cartpole", env_fusable=False, obs_rows=True, shape=None, cnn=False,
    small=(4, 64, 64, 64, 2, 2500), small_bufs=True, rows_ok=False, small_update=True, epoch_graphs=True)
PAIRS = sorted(_K32)   # (env, dist)


def _facts(env, dist, widths=(128, 128, 128), lds=4500):
    entry, d, k = _K32[env, dist]
    return BASE._replace(env=env, dist=dist, obs_dim=d, small=(d, *widths, k, lds))


def test_the_new_query_is_bound_and_the_abi_version_stays():
    import ctypes
    I64 = ctypes.c_int64
    assert _lib.ABI_VERSION == 4
    assert _lib.SIGNATURES["xpa_small_mlp_one_image_lds_floats"] == (I64, [I64] * 6) \
        == _lib.SIGNATURES["xpa_small_mlp_lds_floats"]


@pytest.mark.parametrize("env,dist", PAIRS)
def test_planner_grants_k32w_at_128(env, dist):
    entry = _K32[env, dist][0]
    for algo in ("ppo", "a2c"):
        p = plan_rollout(_facts(env, dist)._replace(algo=algo))
        assert p.driver == "K32W" and p.env == env and p.chunk == 128
        assert p.step_launches() == [entry]
    # K32's widths keep K32's name and the same entry point
    for h in (32, 64):
        q = plan_rollout(_facts(env, dist, (h, h, h)))
        assert q.driver == "K32" and q.step_launches() == [entry]
    assert plan_rollout(_facts(env, dist, (32, 64, 32))).driver == "K32"
    # the multi-kernel step the one launch stands for is the same plan
    sep = plan_rollout(_facts(env, dist)._replace(fused_rollout=False))
    assert sep.driver == "graph-chunk" and sep._replace(driver="K32W") == plan_rollout(_facts(env, dist))


@pytest.mark.parametrize("env,dist", PAIRS)
def test_planner_does_not_grant_k32w(env, dist):
    f = _facts(env, dist)
    _, d, k = _K32[env, dist]
    small = ("K32", "K32W")
    for widths in ((128, 128, 64), (64, 128, 128), (128, 64, 128), (256, 256, 256)):   # mixed widths, and 256
        assert plan_rollout(_facts(env, dist, widths)).driver not in small, widths
    assert plan_rollout(f._replace(small=(d + 1, 128, 128, 128, k, 4500))).driver not in small       # a wrong d_in
    assert plan_rollout(f._replace(obs_dim=d + 1)).driver not in small
    assert plan_rollout(f._replace(small=(d, 128, 128, 128, k + 1, 4500))).driver not in small       # a wrong k
    other = "gaussian" if dist == "categorical" else "categorical"
    assert plan_rollout(f._replace(dist=other)).driver not in small                                  # the other head
    assert plan_rollout(f._replace(fused_rollout=False)).driver == "graph-chunk"
    assert plan_rollout(f._replace(sync_obs_rms=True, world=2)).driver == "eager"                    # per-step merge
    assert plan_rollout(f._replace(sync_obs_rms="rollout", world=2)).driver == "K32W"                # per-rollout
    for lds in (0, -1, 16385):
        assert plan_rollout(f._replace(small=(d, 128, 128, 128, k, lds))).driver not in small, lds
    assert plan_rollout(f._replace(small=(d, 128, 128, 128, k, 16384))).driver == "K32W"
    for off in (dict(cuda=False), dict(defer_boot=False), dict(raw_obs=True), dict(small=None), dict(small_bufs=False),
                dict(env="host"), dict(env="device")):
        assert plan_rollout(f._replace(**off)).driver not in small, off


@pytest.mark.parametrize("env,dist", PAIRS)
def test_plan_test_at_128_stays_on_the_steps_tier(env, dist):
    _, d, k = _K32[env, dist]
    f = EvalFacts(cuda=True, env=env, dist=dist, small=(d, 128, 128, 128, k, 4500), n_envs=5, obs_dim=d,
                  raw_obs=False, world=1, sync_obs_rms=False)
    assert plan_test(f) == "steps"
    assert plan_test(f._replace(small=(d, 64, 64, 64, k, 200))) == "K32E"
