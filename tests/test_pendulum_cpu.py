"""CPU: the Pendulum-v1 / Gaussian small path's host side — the three entry points' bindings, the two configs, the
rollout planner's K32 grants, and the hashed reset states."""
import ctypes

import numpy as np

from xuanpolicy_amd import _lib
from xuanpolicy_amd.rollout_plan import RolloutFacts, plan_rollout

P, I32, I64, U32, F = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_float

CARTPOLE = RolloutFacts(
    algo="ppo", fuse_env_step=True, fuse_post=True, fold_rms=False, fuse_value_gae=True, value_gemm=False,
    fuse_gather=True, fused_rollout=True, use_graph=True, graph_chunk=128, rollout_split=True, rollout_trunk=False,
    s3_gemms=True, cuda=True, use_obsnorm=True, raw_obs=False, atari=False, boot_from_reset=False, defer_boot=True,
    raw_defer=False, raw_mid_next=False, n_slots=1, n_steps=128, obs_dim=4, world=1, sync_obs_rms=False,
    global_advnorm=False, pending=False, env="cartpole", env_fusable=False, obs_rows=True, shape=None, cnn=False,
    small=(4, 64, 64, 64, 2, 2500), small_bufs=True, rows_ok=False, small_update=True, epoch_graphs=True)
PENDULUM = CARTPOLE._replace(env="pendulum", obs_dim=3, small=(3, 64, 64, 64, 1, 2500), dist="gaussian")


def test_entry_points_are_bound_from_the_header():
    assert _lib.ABI_VERSION == 4
    env_step = (ctypes.c_int, [I64, P, I64, P, P, I64, P, P, P, P, P, P, P, P, P, U32, I32, P])
    assert _lib.SIGNATURES["xpa_pendulum_step"] == env_step == _lib.SIGNATURES["xpa_cartpole_step"]
    assert _lib.SIGNATURES["xpa_small_rollout_pendulum"] == (ctypes.c_int, [P, P, F, P])
    assert _lib.SIGNATURES["xpa_small_mlp_update_gauss"] == (ctypes.c_int, [P, P, P, P])


def test_configs_load_with_gaussian_policies():
    from xuanpolicy_amd.runner import get_arguments
    for method, agent in (("ppo", "PPO_Clip"), ("a2c", "A2C")):
        cfg = get_arguments(method, "classic_control", "Pendulum-v1")
        assert cfg.policy == "Gaussian_AC" and cfg.env_id == "Pendulum-v1" and cfg.env_name == "Classic Control"
        assert cfg.agent == agent and cfg.max_episode_steps == 200


def test_planner_grants_k32_per_env_and_head():
    p = plan_rollout(PENDULUM)
    assert p.driver == "K32" and p.env == "pendulum"
    assert p.step_launches() == ["xpa_small_rollout_pendulum"]
    c = plan_rollout(CARTPOLE)
    assert c.driver == "K32" and c.step_launches() == ["xpa_small_rollout_cartpole"]
    # the head must be the env's: no Gaussian K32 on CartPole, no Categorical K32 on Pendulum
    assert plan_rollout(CARTPOLE._replace(dist="gaussian")).driver != "K32"
    assert plan_rollout(PENDULUM._replace(dist="categorical")).driver != "K32"
    # nor another width: A = 2, or CartPole's observation width
    assert plan_rollout(PENDULUM._replace(small=(3, 64, 64, 64, 2, 2500))).driver != "K32"
    assert plan_rollout(PENDULUM._replace(obs_dim=4, small=(4, 64, 64, 64, 1, 2500))).driver != "K32"
    # the multi-kernel step names the env's own launch
    sep = plan_rollout(PENDULUM._replace(fused_rollout=False))
    assert sep.driver == "graph-chunk" and sep.step_launches()[-2:] == ["xpa_pendulum_step",
                                                                        "xpa_rollout_post_deferred_norm"]


def test_reset_states_are_hashed_per_env_and_episode():
    from tests import _pendulum_ref
    from xuanpolicy_amd.envs import pendulum_reset_states
    envs, eps = np.meshgrid(np.arange(64), np.arange(50), indexing="ij")
    s = pendulum_reset_states(7, envs.ravel(), eps.ravel())
    assert s.shape == (3200, 2) and s.dtype == np.float64
    np.testing.assert_array_equal(s, pendulum_reset_states(7, envs.ravel(), eps.ravel()))   # deterministic
    np.testing.assert_array_equal(s, _pendulum_ref.reset_states(7, envs.ravel(), eps.ravel()))
    assert np.all(np.abs(s[:, 0]) <= np.pi) and np.all(np.abs(s[:, 1]) <= 1.0)
    assert len(np.unique(s, axis=0)) == 3200                                               # distinct per (env, episode)
    assert not np.array_equal(s, pendulum_reset_states(8, envs.ravel(), eps.ravel()))
    # f32-exact uniforms: (th0 / pi + 1) / 2 and (thdot0 + 1) / 2 are multiples of 2^-24
    u = (s[:, 1] + 1.0) / 2.0 * 16777216.0
    np.testing.assert_array_equal(u, np.round(u))
