"""numpy f64 restatement of the device Pendulum-v1 env (K18P, csrc/pendulum_body.h): the step equations of the
header's K18P comment, every operation rounded on its own, and the hashed reset.  Test code only."""
import numpy as np

from xuanpolicy_amd.envs import _hash4, _u01

SALT = 0x9E2D0105
DT, MAX_SPEED, MAX_TORQUE = 0.05, 8.0, 2.0


def reset_states(seed, env_ids, episodes):
    """[n, 2] f64 (th0, thdot0) = ((2 u - 1) pi, 2 u - 1), u the f32-exact hashed uniform of (seed, env, episode,
    dim)."""
    e = np.asarray(env_ids, np.uint32)[:, None]
    ep = np.asarray(episodes, np.uint32)[:, None]
    d = np.arange(2, dtype=np.uint32)[None, :]
    c = 2.0 * _u01(_hash4(seed ^ SALT, e, ep, d)).astype(np.float64) - 1.0
    return np.stack([c[:, 0] * np.pi, c[:, 1]], axis=1)


def obs_of(state):
    """f32 (cos th, sin th, thdot) of f64 states [..., 2]."""
    state = np.asarray(state, np.float64)
    return np.stack([np.cos(state[..., 0]), np.sin(state[..., 0]), state[..., 1]], axis=-1).astype(np.float32)


def step(state, action):
    """One step of f64 states [n, 2] with f32 actions [n]: (new states f64 [n, 2], rewards f32 [n])."""
    state = np.asarray(state, np.float64)
    th, thdot = state[..., 0], state[..., 1]
    u = np.clip(np.asarray(action, np.float32).astype(np.float64), -MAX_TORQUE, MAX_TORQUE)
    an = np.mod(th + np.pi, 2.0 * np.pi) - np.pi          # floor modulo, as Python's %
    cost = an * an + 0.1 * (thdot * thdot) + 0.001 * (u * u)
    thdot = np.clip(thdot + (15.0 * np.sin(th) + 3.0 * u) * DT, -MAX_SPEED, MAX_SPEED)
    th = th + thdot * DT
    return np.stack([th, thdot], axis=-1), (-cost).astype(np.float32)


class PendulumRef:
    """n envs with TimeLimit(max_episode_steps) and the hashed auto-reset, stepped together."""

    def __init__(self, n, seed, max_episode_steps):
        self.n, self.seed, self.max_episode_steps = n, seed, max_episode_steps
        self.ep_index = np.zeros(n, np.int64)
        self.ep_step = np.zeros(n, np.int64)
        self.ep_score = np.zeros(n, np.float32)
        self.state = reset_states(seed, np.arange(n), self.ep_index)

    def step(self, action):
        """(final_obs, rew, trunc, next_obs, finished episodes' (length, score)); next_obs is the reset observation
        where trunc."""
        self.state, rew = step(self.state, action)
        final_obs = obs_of(self.state)
        self.ep_step += 1
        self.ep_score = (self.ep_score + rew).astype(np.float32)
        trunc = self.ep_step >= self.max_episode_steps
        last_len, last_score = self.ep_step.copy(), self.ep_score.copy()
        if trunc.any():
            self.ep_index[trunc] += 1
            self.state[trunc] = reset_states(self.seed, np.arange(self.n)[trunc], self.ep_index[trunc])
            self.ep_step[trunc] = 0
            self.ep_score[trunc] = 0.0
        return final_obs, rew, trunc, obs_of(self.state), last_len, last_score
