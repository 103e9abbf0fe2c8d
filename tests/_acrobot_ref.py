"""numpy f64 restatement of the device Acrobot-v1 env (K18A, csrc/acrobot_body.h): the "book" derivative and the RK4
step of the header's K18A comment, every operation rounded on its own and in the header's order, the wrap / clamp /
termination rules and the hashed reset.  Test code only."""
import numpy as np

from xuanpolicy_amd.envs import _hash4, _u01

SALT = 0xAC20B075
M1 = M2 = L1 = I1 = I2 = 1.0
LC1 = LC2 = 0.5
G, DT = 9.8, 0.2
MAX_VEL_1, MAX_VEL_2 = 4.0 * np.pi, 9.0 * np.pi
HALF_PI = np.pi / 2.0


def reset_states(seed, env_ids, episodes):
    """[n, 4] f64, each dim 0.2 u - 0.1, u the f32-exact hashed uniform of (seed, env, episode, dim)."""
    e = np.asarray(env_ids, np.uint32)[:, None]
    ep = np.asarray(episodes, np.uint32)[:, None]
    d = np.arange(4, dtype=np.uint32)[None, :]
    return 0.2 * _u01(_hash4(seed ^ SALT, e, ep, d)).astype(np.float64) - 0.1


def obs_of(state):
    """f32 (cos th1, sin th1, cos th2, sin th2, thdot1, thdot2) of f64 states [..., 4]."""
    s = np.asarray(state, np.float64)
    return np.stack([np.cos(s[..., 0]), np.sin(s[..., 0]), np.cos(s[..., 1]), np.sin(s[..., 1]), s[..., 2], s[..., 3]],
                    axis=-1).astype(np.float32)


def deriv(y, a):
    """f(th1, th2, thdot1, thdot2) under torque a: y [n, 4] f64, a [n] f64."""
    th1, th2, v1, v2 = y[:, 0], y[:, 1], y[:, 2], y[:, 3]
    c2, s2 = np.cos(th2), np.sin(th2)
    d1 = ((M1 * (LC1 * LC1) + M2 * (((L1 * L1) + (LC2 * LC2)) + ((2.0 * L1) * LC2) * c2)) + I1) + I2
    d2 = M2 * ((LC2 * LC2) + (L1 * LC2) * c2) + I2
    phi2 = ((M2 * LC2) * G) * np.cos((th1 + th2) - HALF_PI)
    phi1 = (((((-M2 * L1) * LC2) * (v2 * v2)) * s2 - (((((2.0 * M2) * L1) * LC2) * v2) * v1) * s2)
            + ((M1 * LC1 + M2 * L1) * G) * np.cos(th1 - HALF_PI)) + phi2
    dd2 = (((a + (d2 / d1) * phi1) - (((M2 * L1) * LC2) * (v1 * v1)) * s2) - phi2) \
        / ((M2 * (LC2 * LC2) + I2) - (d2 * d2) / d1)
    dd1 = -((d2 * dd2 + phi1) / d1)
    return np.stack([v1, v2, dd1, dd2], axis=1)


def wrap(x):
    """while x > pi: x -= 2 pi; while x < -pi: x += 2 pi, element by element.  As in the kernel (the header's K18A
    comment), an element that is not finite or lies beyond +-1e6 is left as it is, so the loops end on any input."""
    x = np.array(x, np.float64)
    live = np.abs(x) <= 1.0e6
    while (live & (x > np.pi)).any():
        x = np.where(live & (x > np.pi), x - 2.0 * np.pi, x)
    while (live & (x < -np.pi)).any():
        x = np.where(live & (x < -np.pi), x + 2.0 * np.pi, x)
    return x


def terminal_margin(state):
    """-cos th1 - cos(th2 + th1) - 1: terminated when > 0."""
    s = np.asarray(state, np.float64)
    return (-np.cos(s[..., 0]) - np.cos(s[..., 1] + s[..., 0])) - 1.0


def step(state, action):
    """One step of f64 states [n, 4] with actions [n] in {0, 1, 2}: (new states f64 [n, 4], rewards f32 [n],
    terminated [n])."""
    y = np.asarray(state, np.float64)
    a = (np.asarray(action).astype(np.int64) - 1).astype(np.float64)
    k1 = deriv(y, a)
    k2 = deriv(y + (DT / 2.0) * k1, a)
    k3 = deriv(y + (DT / 2.0) * k2, a)
    k4 = deriv(y + DT * k3, a)
    yn = y + (DT / 6.0) * (((k1 + 2.0 * k2) + 2.0 * k3) + k4)
    new = np.stack([wrap(yn[:, 0]), wrap(yn[:, 1]), np.clip(yn[:, 2], -MAX_VEL_1, MAX_VEL_1),
                    np.clip(yn[:, 3], -MAX_VEL_2, MAX_VEL_2)], axis=1)
    term = (-np.cos(new[:, 0]) - np.cos(new[:, 1] + new[:, 0])) > 1.0
    return new, np.where(term, 0.0, -1.0).astype(np.float32), term


class AcrobotRef:
    """n envs with TimeLimit(max_episode_steps) and the hashed auto-reset, stepped together."""

    def __init__(self, n, seed, max_episode_steps):
        self.n, self.seed, self.max_episode_steps = n, seed, max_episode_steps
        self.ep_index = np.zeros(n, np.int64)
        self.ep_step = np.zeros(n, np.int64)
        self.ep_score = np.zeros(n, np.float32)
        self.state = reset_states(seed, np.arange(n), self.ep_index)

    def obs(self):
        return obs_of(self.state)

    def step(self, action):
        """(final_obs, rew, term, trunc, next_obs, finished episodes' (length, score)); next_obs is the reset
        observation where done.  self.stepped: the f64 states before any reset."""
        self.state, rew, term = step(self.state, action)
        self.stepped = self.state.copy()
        final_obs = obs_of(self.state)
        self.ep_step += 1
        self.ep_score = (self.ep_score + rew).astype(np.float32)
        trunc = self.ep_step >= self.max_episode_steps
        done = term | trunc
        last_len, last_score = self.ep_step.copy(), self.ep_score.copy()
        if done.any():
            self.ep_index[done] += 1
            self.state[done] = reset_states(self.seed, np.arange(self.n)[done], self.ep_index[done])
            self.ep_step[done] = 0
            self.ep_score[done] = 0.0
        return final_obs, rew, term, trunc, obs_of(self.state), last_len, last_score
