"""Device-resident synthetic vector environments for the on-policy benchmark (BASELINE.json configs).

SynthBoxVecEnv(n_envs, D, A) is the SynthBox(D, A) env of SURVEY.md §8(d), plugged in where the
reference builds envs (xuance/environment/__init__.py:76-78 NewEnv hook; DummyVecEnv_Gym contract of
xuance/environment/gym/gym_vec_env.py:148-231).  The state lives in HBM and a step is one GEMM
(X @ Wcat^T, hipBLASLt) plus the xpa_synthbox_step kernel, with auto-reset on done.

Dynamics (spec shared with the CPU checker oracle/synth_env.py; all randomness from a counter hash):
    x = W s + U clip(a, -1, 1) + NOISE * xi      (Discrete: U[:, a] via a one-hot row)
    s' = tanh(x), r = -mean(s'^2), terminated = s'[0] > TERM_THRESH, truncated at max_episode_steps
    reset s0 = RESET_SCALE * (2u - 1)
The host-facing step(actions) -> (obs, rew, term, trunc, infos) exists for the VecEnv contract and
tests; the agent's hot loop uses step_device() and never leaves the GPU.
"""
import numpy as np
import torch

from . import _lib, ops

W_GAIN, U_GAIN, NOISE, TERM_THRESH, RESET_SCALE = 1.25, 0.6, 0.35, 0.92, 0.1
SALT_W, SALT_U, SALT_RESET = 0x57A7E000, 0x0AC7E000, 0x5EED0000


def _mix32(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x85EBCA6B)
        x ^= x >> np.uint32(13)
        x *= np.uint32(0xC2B2AE35)
        x ^= x >> np.uint32(16)
    return x


def _hash4(seed, k0, k1, k2):
    h = _mix32(_mix32(np.uint32(seed & 0xFFFFFFFF)) ^ np.asarray(k0, np.uint32))
    h = _mix32(h ^ np.asarray(k1, np.uint32))
    return _mix32(h ^ np.asarray(k2, np.uint32))


def _u01(h):
    return (np.asarray(h, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def synthbox_matrices(seed, D, A, discrete=False):
    i = np.arange(D, dtype=np.uint32)[:, None]
    W = (2.0 * _u01(_hash4(seed, SALT_W, i, np.arange(D, dtype=np.uint32)[None, :])) - 1.0) * np.sqrt(3.0 / D) * W_GAIN
    gain, fan = (1.0, 1) if discrete else (U_GAIN, A)
    U = (2.0 * _u01(_hash4(seed, SALT_U, i, np.arange(A, dtype=np.uint32)[None, :])) - 1.0) * np.sqrt(3.0 / fan) * gain
    return W.astype(np.float32), U.astype(np.float32)


def synthbox_reset_states(seed, env_ids, episodes, D):
    e = np.asarray(env_ids, np.uint32)[:, None]
    ep = np.asarray(episodes, np.uint32)[:, None]
    d = np.arange(D, dtype=np.uint32)[None, :]
    return ((2.0 * _u01(_hash4(seed ^ SALT_RESET, e, ep, d)) - 1.0) * RESET_SCALE).astype(np.float32)


class _Box:
    def __init__(self, shape):
        self.shape = tuple(shape)
        self.low = -np.ones(shape, np.float32)
        self.high = np.ones(shape, np.float32)
        self.dtype = np.float32


class _Discrete:
    def __init__(self, n):
        self.n, self.shape, self.dtype = int(n), (), np.int64


class SynthBoxVecEnv:
    """n_envs SynthBox(D, A) environments resident on one GPU."""
    kind = "synthbox"   # the env's name in rollout_plan.RolloutFacts.env

    def __init__(self, n_envs, obs_dim, act_dim, seed=1, discrete=False, max_episode_steps=1000, device=None,
                 shard=0):
        self.num_envs, self.D, self.A = int(n_envs), int(obs_dim), int(act_dim)
        self.seed, self.discrete, self.max_episode_steps = int(seed), bool(discrete), int(max_episode_steps)
        self.max_episode_length = self.max_episode_steps
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        # Data-parallel shards share the dynamics (W, U from `seed`) but draw noise/reset states from a
        # per-shard stream; shard 0 is bit-identical to the CPU checker.
        self.shard = int(shard)
        self.noise_seed = (self.seed ^ ((0x9E3779B9 * self.shard) & 0xFFFFFFFF)) & 0xFFFFFFFF
        self.observation_space = _Box((self.D,))
        self.action_space = _Discrete(self.A) if discrete else _Box((self.A,))
        W, U = synthbox_matrices(self.seed, self.D, self.A, self.discrete)
        dev, N, D, A = self.device, self.num_envs, self.D, self.A
        self.Wcat_t = torch.as_tensor(np.concatenate([W, U], axis=1).T.copy(), device=dev)  # [D + A, D]
        self.X = torch.zeros((N, D + A), dtype=torch.float32, device=dev)                   # [state | action]
        self.pre = torch.empty((N, D), dtype=torch.float32, device=dev)
        self.final_obs = torch.empty((N, D), dtype=torch.float32, device=dev)
        self.rew = torch.zeros((N,), dtype=torch.float32, device=dev)
        self.term = torch.zeros((N,), dtype=torch.uint8, device=dev)
        self.trunc = torch.zeros((N,), dtype=torch.uint8, device=dev)
        self.ep_step = torch.zeros((N,), dtype=torch.int32, device=dev)
        self.ep_index = torch.zeros((N,), dtype=torch.int32, device=dev)  # read as uint32 by the kernel
        self.ep_score = torch.zeros((N,), dtype=torch.float32, device=dev)
        self.ep_last_score = torch.zeros((N,), dtype=torch.float32, device=dev)
        self.ep_last_len = torch.zeros((N,), dtype=torch.int32, device=dev)
        self.reset()

    @property
    def obs(self):
        """Current observation [N, D] (a strided view of X)."""
        return self.X[:, :self.D]

    @property
    def act_in(self):
        """Env action input [N, A] (a strided view of X): clipped action or one-hot."""
        return self.X[:, self.D:]

    @property
    def buf_obs(self):
        return self.obs

    def reset(self):
        self.resets = getattr(self, "resets", 0) + 1   # agents re-arm a folded obs-RMS merge (K8R)
        ids = np.arange(self.num_envs)
        s0 = synthbox_reset_states(self.noise_seed, ids, np.zeros(self.num_envs), self.D)
        self.X.zero_()
        self.X[:, :self.D] = torch.as_tensor(s0, device=self.device)
        for t in (self.ep_step, self.ep_index, self.ep_score, self.ep_last_score, self.ep_last_len, self.rew,
                  self.term, self.trunc):
            t.zero_()
        return self.obs.clone(), [{} for _ in range(self.num_envs)]

    def fusable_with_policy_step(self, dist):
        """True when the rollout's K14 can run this env's step in the same launch
        (ops.rollout_policy_head_synthbox): continuous actions and at most 64 state dims."""
        return dist == "gaussian" and not self.discrete and self.D <= 64

    def step_device(self):
        """One env step for all envs from the action already written into act_in."""
        torch.mm(self.X, self.Wcat_t, out=self.pre)
        _lib.call(ops.lib().xpa_synthbox_step, self.num_envs, self.D, ops._p(self.pre), self.noise_seed,
                  self.max_episode_steps, NOISE, TERM_THRESH, RESET_SCALE, ops._p(self.X), self.X.stride(0),
                  ops._p(self.final_obs), ops._p(self.rew), ops._p(self.term), ops._p(self.trunc), ops._p(self.ep_step),
                  ops._p(self.ep_index), ops._p(self.ep_score), ops._p(self.ep_last_score), ops._p(self.ep_last_len),
                  ops._stream(self.device))

    def step(self, actions):
        """VecEnv contract (gym_vec_env.py:201-212): returns host copies of (obs, rew, term, trunc, infos)
        with infos[i]['reset_obs'] for done envs."""
        a = torch.as_tensor(np.asarray(actions) if not isinstance(actions, torch.Tensor) else actions,
                            device=self.device)
        if self.discrete:
            self.act_in.zero_()
            self.act_in.scatter_(1, a.long().reshape(-1, 1), 1.0)
        else:
            self.act_in.copy_(torch.clamp(a.float().reshape(self.num_envs, self.A), -1.0, 1.0))
        self.step_device()
        obs = self.final_obs.cpu().numpy()
        rew = self.rew.cpu().numpy()
        term = self.term.cpu().numpy().astype(bool)
        trunc = self.trunc.cpu().numpy().astype(bool)
        nxt = self.obs.cpu().numpy()
        lens, scores = self.ep_step.cpu().numpy(), self.ep_score.cpu().numpy()
        last_len, last_score = self.ep_last_len.cpu().numpy(), self.ep_last_score.cpu().numpy()
        infos = []
        for i in range(self.num_envs):
            done = term[i] or trunc[i]
            info = {"episode_step": int(last_len[i] if done else lens[i]),
                    "episode_score": float(last_score[i] if done else scores[i])}
            if done:
                info["reset_obs"] = nxt[i].copy()
            infos.append(info)
        return obs, rew, term, trunc, infos

    def close(self):
        pass


class _ImageBox:
    def __init__(self, shape):
        self.shape = tuple(shape)
        self.low = np.zeros(shape, np.uint8)
        self.high = np.full(shape, 255, np.uint8)
        self.dtype = np.uint8


class SynthAtariVecEnv:
    """n_envs SynthAtari envs (uint8 4x84x84 frame stacks, Discrete(n_actions), reward sign, lives) resident
    on one GPU — the C3 / C5 shapes of BASELINE.json.  Spec and CPU checker: oracle/synth_env.py
    (SynthAtariEnv); kernel: csrc/atari.hip (K15).  Same interface as SynthBoxVecEnv: obs, act_in,
    final_obs, rew/term/trunc, step_device(), host step() with the DummyVecEnv_Atari contract."""

    kind = "synthatari"
    HW, STACK = 84, 4

    def __init__(self, n_envs, n_actions=6, seed=1, max_episode_steps=27000, device=None, shard=0):
        self.num_envs, self.n_actions = int(n_envs), int(n_actions)
        self.seed, self.max_episode_steps = int(seed), int(max_episode_steps)
        self.max_episode_length = self.max_episode_steps
        # the reference's Atari flag rules (gym_env.py:193-209): a game over or the step limit sets terminated AND
        # truncated, so a truncation never needs a bootstrap value (finish_path(0)) — the agent then evaluates the
        # critic only on the last step's observations, once per rollout
        self.truncation_implies_terminal = True
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.shard = int(shard)
        self.noise_seed = (self.seed ^ ((0x9E3779B9 * self.shard) & 0xFFFFFFFF)) & 0xFFFFFFFF
        shape = (self.HW, self.HW, self.STACK)
        self.observation_space = _ImageBox(shape)
        self.action_space = _Discrete(self.n_actions)
        dev, N = self.device, self.num_envs
        self.stack = torch.zeros((N,) + shape, dtype=torch.uint8, device=dev)
        self.final_obs = torch.zeros((N,) + shape, dtype=torch.uint8, device=dev)
        self._act = torch.zeros((N, self.n_actions), dtype=torch.float32, device=dev)
        self.rew = torch.zeros((N,), dtype=torch.float32, device=dev)
        self.term = torch.zeros((N,), dtype=torch.uint8, device=dev)
        self.trunc = torch.zeros((N,), dtype=torch.uint8, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.ep_step, self.ep_index = torch.zeros((N,), **i32), torch.zeros((N,), **i32)
        self.lives, self.paddle = torch.zeros((N,), **i32), torch.zeros((N,), **i32)
        self.ep_last_len = torch.zeros((N,), **i32)
        self.ep_score = torch.zeros((N,), dtype=torch.float32, device=dev)
        self.ep_last_score = torch.zeros((N,), dtype=torch.float32, device=dev)
        self.err = torch.zeros((1,), dtype=torch.int32, device=dev)   # steps taken with no action set (K15)
        self.reset()

    @property
    def obs(self):
        return self.stack

    @property
    def act_in(self):
        return self._act

    @property
    def buf_obs(self):
        return self.stack

    def reset(self):
        self.resets = getattr(self, "resets", 0) + 1   # agents re-arm a folded obs-RMS merge (K8R)
        for t in (self.ep_step, self.ep_index, self.ep_score, self.ep_last_score, self.ep_last_len, self.rew,
                  self.term, self.trunc, self._act):
            t.zero_()
        self.lives.fill_(5)
        self.paddle.fill_(38)
        _lib.call(ops.lib().xpa_synthatari_reset, self.num_envs, self.noise_seed, ops._p(self.stack),
                  ops._p(self.ep_index), ops._stream(self.device))
        return self.stack.clone(), [{} for _ in range(self.num_envs)]

    def step_device(self):
        _lib.call(ops.lib().xpa_synthatari_step, self.num_envs, self.n_actions, ops._p(self._act), self._act.stride(0),
                  self.noise_seed, self.max_episode_steps, ops._p(self.stack), ops._p(self.final_obs), ops._p(self.rew),
                  ops._p(self.term), ops._p(self.trunc), ops._p(self.ep_step), ops._p(self.ep_index),
                  ops._p(self.lives), ops._p(self.paddle), ops._p(self.ep_score), ops._p(self.ep_last_score),
                  ops._p(self.ep_last_len), ops._p(self.err), ops._stream(self.device))

    def step(self, actions):
        """DummyVecEnv_Atari contract (gym_vec_env.py:201-212): host copies of (obs, rew, term, trunc, infos);
        infos[i]['reset_obs'] after a game over."""
        a = torch.as_tensor(np.asarray(actions) if not isinstance(actions, torch.Tensor) else actions,
                            device=self.device).long().reshape(-1, 1)
        self._act.zero_()
        self._act.scatter_(1, a, 1.0)
        self.step_device()
        obs = self.final_obs.cpu().numpy()
        rew = self.rew.cpu().numpy()
        term = self.term.cpu().numpy().astype(bool)
        trunc = self.trunc.cpu().numpy().astype(bool)
        nxt = self.stack.cpu().numpy()
        lens, scores = self.ep_step.cpu().numpy(), self.ep_score.cpu().numpy()
        last_len, last_score = self.ep_last_len.cpu().numpy(), self.ep_last_score.cpu().numpy()
        infos = []
        for i in range(self.num_envs):
            info = {"episode_step": int(last_len[i] if trunc[i] else lens[i]),
                    "episode_score": float(last_score[i] if trunc[i] else scores[i])}
            if trunc[i]:
                info["reset_obs"] = nxt[i].copy()
            infos.append(info)
        return obs, rew, term, trunc, infos

    def close(self):
        pass


# ---- CartPole-v1 (BASELINE.json configs[0]) -------------------------------------------------------------------
SALT_CARTPOLE = 0xCA27B01E


def cartpole_reset_states(seed, env_ids, episodes):
    """uniform(-0.05, 0.05) per dim from the counter hash (f32-exact uniform, then f64), as K18 draws them."""
    e = np.asarray(env_ids, np.uint32)[:, None]
    ep = np.asarray(episodes, np.uint32)[:, None]
    d = np.arange(4, dtype=np.uint32)[None, :]
    return _u01(_hash4(seed ^ SALT_CARTPOLE, e, ep, d)).astype(np.float64) * 0.1 - 0.05


class CartPoleVecEnv:
    """n_envs CartPole-v1 envs resident on one GPU (K18 xpa_cartpole_step, csrc/classic.hip): gym 0.26.2's
    dynamics with TimeLimit(500), f64 state, f32 observations, Discrete(2) actions read from the one-hot env
    input the rollout kernels write.  Same interface as SynthBoxVecEnv (obs, act_in, final_obs, rew / term /
    trunc, step_device(), host step() with DummyVecEnv_Gym's contract).  CPU checker:
    oracle/synth_env.CartPoleEnv."""
    kind = "cartpole"   # rollout_plan: K32 steps this env inside the fused rollout step

    def __init__(self, n_envs, seed=1, max_episode_steps=500, device=None, shard=0):
        self.num_envs, self.seed, self.max_episode_steps = int(n_envs), int(seed), int(max_episode_steps)
        self.max_episode_length = self.max_episode_steps
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.shard = int(shard)
        self.noise_seed = (self.seed ^ ((0x9E3779B9 * self.shard) & 0xFFFFFFFF)) & 0xFFFFFFFF
        self.observation_space = _Box((4,))
        self.observation_space.low = np.full(4, -np.inf, np.float32)
        self.observation_space.high = np.full(4, np.inf, np.float32)
        self.action_space = _Discrete(2)
        dev, N = self.device, self.num_envs
        self.state = torch.zeros((N, 4), dtype=torch.float64, device=dev)
        self._obs = torch.zeros((N, 4), dtype=torch.float32, device=dev)
        self._act = torch.zeros((N, 2), dtype=torch.float32, device=dev)
        self.final_obs = torch.zeros((N, 4), dtype=torch.float32, device=dev)
        self.rew = torch.zeros((N,), dtype=torch.float32, device=dev)
        self.term = torch.zeros((N,), dtype=torch.uint8, device=dev)
        self.trunc = torch.zeros((N,), dtype=torch.uint8, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.ep_step, self.ep_index, self.ep_last_len = (torch.zeros((N,), **i32) for _ in range(3))
        self.ep_score = torch.zeros((N,), dtype=torch.float32, device=dev)
        self.ep_last_score = torch.zeros((N,), dtype=torch.float32, device=dev)
        self.reset()

    @property
    def obs(self):
        return self._obs

    @property
    def act_in(self):
        """Env action input [N, 2]: the one-hot of the sampled action (K3 / K14 write it)."""
        return self._act

    @property
    def buf_obs(self):
        return self._obs

    def reset_host(self):
        """reset()'s host-only half, for a caller whose device half ran in small_path.env_reset_batch's launch."""
        self.resets = getattr(self, "resets", 0) + 1   # agents re-arm a folded obs-RMS merge (K8R)

    def reset(self):
        self.reset_host()
        s0 = cartpole_reset_states(self.noise_seed, np.arange(self.num_envs), np.zeros(self.num_envs))
        self.state.copy_(torch.as_tensor(s0, device=self.device))
        self._obs.copy_(self.state.float())
        for t in (self.ep_step, self.ep_index, self.ep_score, self.ep_last_score, self.ep_last_len, self.rew,
                  self.term, self.trunc):
            t.zero_()
        return self._obs.clone(), [{} for _ in range(self.num_envs)]

    def fusable_with_policy_step(self, dist):
        return False

    def step_device(self):
        _lib.call(ops.lib().xpa_cartpole_step, self.num_envs, ops._p(self._act), self._act.stride(0),
                  ops._p(self.state), ops._p(self._obs), self._obs.stride(0), ops._p(self.final_obs), ops._p(self.rew),
                  ops._p(self.term), ops._p(self.trunc), ops._p(self.ep_step), ops._p(self.ep_index),
                  ops._p(self.ep_score), ops._p(self.ep_last_score), ops._p(self.ep_last_len), self.noise_seed,
                  self.max_episode_steps, ops._stream(self.device))

    def step(self, actions):
        """VecEnv contract (gym_vec_env.py:201-212): host copies of (obs, rew, term, trunc, infos)."""
        a = torch.as_tensor(np.asarray(actions) if not isinstance(actions, torch.Tensor) else actions,
                            device=self.device).long().reshape(-1, 1)
        self._act.zero_()
        self._act.scatter_(1, a, 1.0)
        self.step_device()
        obs = self.final_obs.cpu().numpy()
        rew = self.rew.cpu().numpy()
        term = self.term.cpu().numpy().astype(bool)
        trunc = self.trunc.cpu().numpy().astype(bool)
        nxt = self._obs.cpu().numpy()
        lens, scores = self.ep_step.cpu().numpy(), self.ep_score.cpu().numpy()
        last_len, last_score = self.ep_last_len.cpu().numpy(), self.ep_last_score.cpu().numpy()
        infos = []
        for i in range(self.num_envs):
            done = term[i] or trunc[i]
            info = {"episode_step": int(last_len[i] if done else lens[i]),
                    "episode_score": float(last_score[i] if done else scores[i])}
            if done:
                info["reset_obs"] = nxt[i].copy()
            infos.append(info)
        return obs, rew, term, trunc, infos

    def close(self):
        pass


# ---- Pendulum-v1 (the reference's configs/ppo|a2c/classic_control/Pendulum-v1.yaml) ------------------------------
SALT_PENDULUM = 0x9E2D0105


def pendulum_reset_states(seed, env_ids, episodes):
    """[n, 2] f64 (th0, thdot0) = ((2 u - 1) pi, 2 u - 1) from the counter hash (f32-exact uniforms, then f64), as
    K18P draws them."""
    e = np.asarray(env_ids, np.uint32)[:, None]
    ep = np.asarray(episodes, np.uint32)[:, None]
    d = np.arange(2, dtype=np.uint32)[None, :]
    c = 2.0 * _u01(_hash4(seed ^ SALT_PENDULUM, e, ep, d)).astype(np.float64) - 1.0
    c[:, 0] = c[:, 0] * np.pi
    return c


class PendulumVecEnv:
    """n_envs Pendulum-v1 envs resident on one GPU (K18P xpa_pendulum_step, csrc/classic.hip): the equations of the
    header's K18P comment with TimeLimit(200), f64 state (th, thdot), f32 observations (cos th, sin th, thdot), one
    torque in [-2, 2] read from the clipped env input the Gaussian rollout kernels write.  Same interface as
    CartPoleVecEnv.  CPU checker: tests/_pendulum_ref.py."""
    kind = "pendulum"   # rollout_plan: K32 steps this env inside the fused rollout step
    MAX_SPEED, MAX_TORQUE = 8.0, 2.0

    def __init__(self, n_envs, seed=1, max_episode_steps=200, device=None, shard=0):
        self.num_envs, self.seed, self.max_episode_steps = int(n_envs), int(seed), int(max_episode_steps)
        self.max_episode_length = self.max_episode_steps
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.shard = int(shard)
        self.noise_seed = (self.seed ^ ((0x9E3779B9 * self.shard) & 0xFFFFFFFF)) & 0xFFFFFFFF
        self.observation_space = _Box((3,))
        self.observation_space.high = np.array([1.0, 1.0, self.MAX_SPEED], np.float32)
        self.observation_space.low = -self.observation_space.high
        self.action_space = _Box((1,))
        self.action_space.high = np.full(1, self.MAX_TORQUE, np.float32)
        self.action_space.low = -self.action_space.high
        dev, N = self.device, self.num_envs
        self.state = torch.zeros((N, 2), dtype=torch.float64, device=dev)
        self._obs = torch.zeros((N, 3), dtype=torch.float32, device=dev)
        self._act = torch.zeros((N, 1), dtype=torch.float32, device=dev)
        self.final_obs = torch.zeros((N, 3), dtype=torch.float32, device=dev)
        self.rew = torch.zeros((N,), dtype=torch.float32, device=dev)
        self.term = torch.zeros((N,), dtype=torch.uint8, device=dev)
        self.trunc = torch.zeros((N,), dtype=torch.uint8, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.ep_step, self.ep_index, self.ep_last_len = (torch.zeros((N,), **i32) for _ in range(3))
        self.ep_score = torch.zeros((N,), dtype=torch.float32, device=dev)
        self.ep_last_score = torch.zeros((N,), dtype=torch.float32, device=dev)
        self.reset()

    @property
    def obs(self):
        return self._obs

    @property
    def act_in(self):
        """Env action input [N, 1]: the clipped torque (K3 / K14 / K32 write it)."""
        return self._act

    @property
    def buf_obs(self):
        return self._obs

    def reset_host(self):
        """reset()'s host-only half, for a caller whose device half ran in small_path.env_reset_batch's launch."""
        self.resets = getattr(self, "resets", 0) + 1   # agents re-arm a folded obs-RMS merge (K8R)

    def reset(self):
        self.reset_host()
        s0 = pendulum_reset_states(self.noise_seed, np.arange(self.num_envs), np.zeros(self.num_envs))
        self.state.copy_(torch.as_tensor(s0, device=self.device))
        o0 = np.stack([np.cos(s0[:, 0]), np.sin(s0[:, 0]), s0[:, 1]], axis=1).astype(np.float32)
        self._obs.copy_(torch.as_tensor(o0, device=self.device))
        for t in (self.ep_step, self.ep_index, self.ep_score, self.ep_last_score, self.ep_last_len, self.rew,
                  self.term, self.trunc, self._act):
            t.zero_()
        return self._obs.clone(), [{} for _ in range(self.num_envs)]

    def fusable_with_policy_step(self, dist):
        return False

    def step_device(self):
        _lib.call(ops.lib().xpa_pendulum_step, self.num_envs, ops._p(self._act), self._act.stride(0),
                  ops._p(self.state), ops._p(self._obs), self._obs.stride(0), ops._p(self.final_obs), ops._p(self.rew),
                  ops._p(self.term), ops._p(self.trunc), ops._p(self.ep_step), ops._p(self.ep_index),
                  ops._p(self.ep_score), ops._p(self.ep_last_score), ops._p(self.ep_last_len), self.noise_seed,
                  self.max_episode_steps, ops._stream(self.device))

    def step(self, actions):
        """VecEnv contract (gym_vec_env.py:201-212): host copies of (obs, rew, term, trunc, infos)."""
        a = torch.as_tensor(np.asarray(actions) if not isinstance(actions, torch.Tensor) else actions,
                            device=self.device)
        self._act.copy_(torch.clamp(a.float().reshape(self.num_envs, 1), -self.MAX_TORQUE, self.MAX_TORQUE))
        self.step_device()
        obs = self.final_obs.cpu().numpy()
        rew = self.rew.cpu().numpy()
        term = self.term.cpu().numpy().astype(bool)
        trunc = self.trunc.cpu().numpy().astype(bool)
        nxt = self._obs.cpu().numpy()
        lens, scores = self.ep_step.cpu().numpy(), self.ep_score.cpu().numpy()
        last_len, last_score = self.ep_last_len.cpu().numpy(), self.ep_last_score.cpu().numpy()
        infos = []
        for i in range(self.num_envs):
            done = term[i] or trunc[i]
            info = {"episode_step": int(last_len[i] if done else lens[i]),
                    "episode_score": float(last_score[i] if done else scores[i])}
            if done:
                info["reset_obs"] = nxt[i].copy()
            infos.append(info)
        return obs, rew, term, trunc, infos

    def close(self):
        pass


# ---- Acrobot-v1 and MountainCar-v0 (the reference's configs/ppo|a2c/classic_control/{Acrobot-v1,MountainCar-v0}.yaml) --
SALT_ACROBOT = 0xAC20B075
SALT_MOUNTAINCAR = 0x30CA2005


def acrobot_reset_states(seed, env_ids, episodes):
    """[n, 4] f64 (th1, th2, thdot1, thdot2), each 0.2 u - 0.1 from the counter hash (f32-exact uniforms, then f64), as
    K18A draws them."""
    e = np.asarray(env_ids, np.uint32)[:, None]
    ep = np.asarray(episodes, np.uint32)[:, None]
    d = np.arange(4, dtype=np.uint32)[None, :]
    return 0.2 * _u01(_hash4(seed ^ SALT_ACROBOT, e, ep, d)).astype(np.float64) - 0.1


def mountaincar_reset_states(seed, env_ids, episodes):
    """[n, 2] f64 (position, velocity) = (0.2 u - 0.6, 0) from the counter hash (f32-exact uniform, then f64), as K18M
    draws them."""
    e = np.asarray(env_ids, np.uint32)
    ep = np.asarray(episodes, np.uint32)
    p = 0.2 * _u01(_hash4(seed ^ SALT_MOUNTAINCAR, e, ep, np.uint32(0))).astype(np.float64) - 0.6
    return np.stack([p, np.zeros_like(p)], axis=1)


class _Discrete3VecEnv:
    """What AcrobotVecEnv and MountainCarVecEnv share: n_envs envs resident on one GPU with an f64 state, f32
    observations, Discrete(3) actions read from the one-hot env input [N, 3] the Categorical rollout kernels write, and
    a step kernel of K18's contract.  Same interface as CartPoleVecEnv.  A subclass names its kind, step entry point,
    state width, spaces, default time limit, hashed reset states and their observation."""

    def __init__(self, n_envs, seed=1, max_episode_steps=None, device=None, shard=0):
        self.num_envs, self.seed = int(n_envs), int(seed)
        self.max_episode_steps = int(self.TIME_LIMIT if max_episode_steps is None else max_episode_steps)
        self.max_episode_length = self.max_episode_steps
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.shard = int(shard)
        self.noise_seed = (self.seed ^ ((0x9E3779B9 * self.shard) & 0xFFFFFFFF)) & 0xFFFFFFFF
        self.observation_space = self._observation_space()
        self.action_space = _Discrete(3)
        dev, N, D = self.device, self.num_envs, self.observation_space.shape[0]
        self.state = torch.zeros((N, self.STATE_DIM), dtype=torch.float64, device=dev)
        self._obs = torch.zeros((N, D), dtype=torch.float32, device=dev)
        self._act = torch.zeros((N, 3), dtype=torch.float32, device=dev)
        self.final_obs = torch.zeros((N, D), dtype=torch.float32, device=dev)
        self.rew = torch.zeros((N,), dtype=torch.float32, device=dev)
        self.term = torch.zeros((N,), dtype=torch.uint8, device=dev)
        self.trunc = torch.zeros((N,), dtype=torch.uint8, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.ep_step, self.ep_index, self.ep_last_len = (torch.zeros((N,), **i32) for _ in range(3))
        self.ep_score = torch.zeros((N,), dtype=torch.float32, device=dev)
        self.ep_last_score = torch.zeros((N,), dtype=torch.float32, device=dev)
        self.reset()

    @property
    def obs(self):
        return self._obs

    @property
    def act_in(self):
        """Env action input [N, 3]: the one-hot of the sampled action (K3 / K14 / K32 write it)."""
        return self._act

    @property
    def buf_obs(self):
        return self._obs

    def reset_host(self):
        """reset()'s host-only half, for a caller whose device half ran in small_path.env_reset_batch's launch."""
        self.resets = getattr(self, "resets", 0) + 1   # agents re-arm a folded obs-RMS merge (K8R)

    def reset(self):
        self.reset_host()
        s0 = self.reset_states(self.noise_seed, np.arange(self.num_envs), np.zeros(self.num_envs))
        self.state.copy_(torch.as_tensor(s0, device=self.device))
        self._obs.copy_(torch.as_tensor(self.obs_of_reset(s0), device=self.device))
        for t in (self.ep_step, self.ep_index, self.ep_score, self.ep_last_score, self.ep_last_len, self.rew,
                  self.term, self.trunc, self._act):
            t.zero_()
        return self._obs.clone(), [{} for _ in range(self.num_envs)]

    def fusable_with_policy_step(self, dist):
        return False

    def step_device(self):
        _lib.call(getattr(ops.lib(), self.STEP), self.num_envs, ops._p(self._act), self._act.stride(0),
                  ops._p(self.state), ops._p(self._obs), self._obs.stride(0), ops._p(self.final_obs), ops._p(self.rew),
                  ops._p(self.term), ops._p(self.trunc), ops._p(self.ep_step), ops._p(self.ep_index),
                  ops._p(self.ep_score), ops._p(self.ep_last_score), ops._p(self.ep_last_len), self.noise_seed,
                  self.max_episode_steps, ops._stream(self.device))

    def step(self, actions):
        """VecEnv contract (gym_vec_env.py:201-212): host copies of (obs, rew, term, trunc, infos)."""
        a = torch.as_tensor(np.asarray(actions) if not isinstance(actions, torch.Tensor) else actions,
                            device=self.device).long().reshape(-1, 1)
        self._act.zero_()
        self._act.scatter_(1, a, 1.0)
        self.step_device()
        obs = self.final_obs.cpu().numpy()
        rew = self.rew.cpu().numpy()
        term = self.term.cpu().numpy().astype(bool)
        trunc = self.trunc.cpu().numpy().astype(bool)
        nxt = self._obs.cpu().numpy()
        lens, scores = self.ep_step.cpu().numpy(), self.ep_score.cpu().numpy()
        last_len, last_score = self.ep_last_len.cpu().numpy(), self.ep_last_score.cpu().numpy()
        infos = []
        for i in range(self.num_envs):
            done = term[i] or trunc[i]
            info = {"episode_step": int(last_len[i] if done else lens[i]),
                    "episode_score": float(last_score[i] if done else scores[i])}
            if done:
                info["reset_obs"] = nxt[i].copy()
            infos.append(info)
        return obs, rew, term, trunc, infos

    def close(self):
        pass


class AcrobotVecEnv(_Discrete3VecEnv):
    """n_envs Acrobot-v1 envs (K18A xpa_acrobot_step, csrc/classic.hip): the equations of the header's K18A comment
    ("book" dynamics, one RK4 step of dt 0.2) with TimeLimit(500), f64 state (th1, th2, thdot1, thdot2), f32
    observations (cos th1, sin th1, cos th2, sin th2, thdot1, thdot2), torque action - 1.  CPU checker:
    tests/_acrobot_ref.py."""
    kind = "acrobot"   # rollout_plan: K32 steps this env inside the fused rollout step
    STEP, STATE_DIM, TIME_LIMIT = "xpa_acrobot_step", 4, 500
    MAX_VEL_1, MAX_VEL_2 = 4 * np.pi, 9 * np.pi
    reset_states = staticmethod(acrobot_reset_states)

    def _observation_space(self):
        box = _Box((6,))
        box.high = np.array([1.0, 1.0, 1.0, 1.0, self.MAX_VEL_1, self.MAX_VEL_2], np.float32)
        box.low = -box.high
        return box

    @staticmethod
    def obs_of_reset(s):
        return np.stack([np.cos(s[:, 0]), np.sin(s[:, 0]), np.cos(s[:, 1]), np.sin(s[:, 1]), s[:, 2], s[:, 3]],
                        axis=1).astype(np.float32)


class MountainCarVecEnv(_Discrete3VecEnv):
    """n_envs MountainCar-v0 envs behind the reference's MountainCar wrapper (K18M xpa_mountaincar_step,
    csrc/classic.hip): the equations of the header's K18M comment with TimeLimit(200), f64 state (position, velocity),
    and the observation the wrapper gives (gym_env.py:52-85) — the last four f32 (position, velocity) frames, oldest
    first, the reset frame four times after a reset.  The stack lives in `obs` itself.  CPU checker:
    tests/_mountaincar_ref.py."""
    kind = "mountaincar"   # rollout_plan: K32 steps this env inside the fused rollout step
    STEP, STATE_DIM, TIME_LIMIT = "xpa_mountaincar_step", 2, 200
    reset_states = staticmethod(mountaincar_reset_states)

    def _observation_space(self):
        box = _Box((8,))
        box.low = np.array([-1.2, -0.07] * 4, np.float32)
        box.high = np.array([0.6, 0.07] * 4, np.float32)
        return box

    @staticmethod
    def obs_of_reset(s):
        return np.tile(s.astype(np.float32), (1, 4))
