"""numpy f64 restatement of the device MountainCar-v0 env (K18M, csrc/mountaincar_body.h): the step of the header's
K18M comment, every operation rounded on its own, the hashed reset, and the reference wrapper's stack of the last four
(position, velocity) frames.  Test code only."""
import numpy as np

from xuanpolicy_amd.envs import _hash4, _u01

SALT = 0x30CA2005
MIN_POS, MAX_POS, MAX_SPEED, GOAL_POS = -1.2, 0.6, 0.07, 0.5


def reset_states(seed, env_ids, episodes):
    """[n, 2] f64 (0.2 u - 0.6, 0), u the f32-exact hashed uniform of (seed, env, episode, 0)."""
    e = np.asarray(env_ids, np.uint32)
    ep = np.asarray(episodes, np.uint32)
    p = 0.2 * _u01(_hash4(seed ^ SALT, e, ep, np.uint32(0))).astype(np.float64) - 0.6
    return np.stack([p, np.zeros_like(p)], axis=1)


def obs_of(state):
    """The reset stack of f64 states [n, 2]: the f32 frame four times, [n, 8]."""
    return np.tile(np.asarray(state, np.float64).astype(np.float32), (1, 4))


def step(state, action):
    """One step of f64 states [n, 2] with actions [n] in {0, 1, 2}: (new states f64 [n, 2], rewards f32 [n],
    terminated [n])."""
    s = np.asarray(state, np.float64)
    pos, vel = s[:, 0], s[:, 1]
    a = (np.asarray(action).astype(np.int64) - 1).astype(np.float64)
    vel = vel + (a * 0.001 + np.cos(3.0 * pos) * (-0.0025))
    vel = np.clip(vel, -MAX_SPEED, MAX_SPEED)
    pos = pos + vel
    pos = np.clip(pos, MIN_POS, MAX_POS)
    vel = np.where((pos == MIN_POS) & (vel < 0.0), 0.0, vel)
    term = (pos >= GOAL_POS) & (vel >= 0.0)
    return np.stack([pos, vel], axis=1), np.full(pos.shape, -1.0, np.float32), term


def push(stack, state):
    """The stack [n, 8] with its columns 2..7 moved down and the f32 frame of state [n, 2] appended."""
    return np.concatenate([np.asarray(stack, np.float32)[:, 2:], np.asarray(state, np.float64).astype(np.float32)],
                          axis=1)


class MountainCarRef:
    """n envs with TimeLimit(max_episode_steps), the hashed auto-reset and the frame stack, stepped together."""

    def __init__(self, n, seed, max_episode_steps):
        self.n, self.seed, self.max_episode_steps = n, seed, max_episode_steps
        self.ep_index = np.zeros(n, np.int64)
        self.ep_step = np.zeros(n, np.int64)
        self.ep_score = np.zeros(n, np.float32)
        self.state = reset_states(seed, np.arange(n), self.ep_index)
        self.stack = obs_of(self.state)

    def obs(self):
        return self.stack.copy()

    def step(self, action):
        """(final_obs, rew, term, trunc, next_obs, finished episodes' (length, score)); next_obs is the reset stack
        where done.  self.stepped: the f64 states before any reset."""
        self.state, rew, term = step(self.state, action)
        self.stepped = self.state.copy()
        final_obs = push(self.stack, self.state)
        self.stack = final_obs.copy()
        self.ep_step += 1
        self.ep_score = (self.ep_score + rew).astype(np.float32)
        trunc = self.ep_step >= self.max_episode_steps
        done = term | trunc
        last_len, last_score = self.ep_step.copy(), self.ep_score.copy()
        if done.any():
            self.ep_index[done] += 1
            self.state[done] = reset_states(self.seed, np.arange(self.n)[done], self.ep_index[done])
            self.stack[done] = obs_of(self.state[done])
            self.ep_step[done] = 0
            self.ep_score[done] = 0.0
        return final_obs, rew, term, trunc, self.stack.copy(), last_len, last_score
