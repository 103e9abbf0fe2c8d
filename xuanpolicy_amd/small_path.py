"""The host side of the one-launch small path (K32 / K32W rollout, K32E evaluation, K33 closing, K30 update and their
population forms): one record of the policy's five layers, one filler for the fields the three argument structs share,
the block builders, and one function per launch ("Where the small path's envs and blocks are stated").
Which env / head pair a launch serves comes from rollout_plan.SMALL_ENVS alone.  ops re-exports the closing's and the
evaluation's functions, so this module reaches ops' argument checks inside the functions that use them."""
import ctypes
import functools
from typing import NamedTuple

import torch

from . import _lib
from .rollout_plan import SMALL_BY_ENTRY, SMALL_ENVS

_p = torch.Tensor.data_ptr


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class SmallPolicy(NamedTuple):
    """learner.small_policy_layers(): the policy in the shape K30, K32 and K33 take."""
    layers: tuple    # (l0, l1, la, l2, lc): representation, actor hidden, actor out (logits / mu), critic hidden and out
    code: int        # the activation's code ...
    slope: float     # ... and slope, shared by the three hidden layers
    logstd: object   # the Gaussian head's parameter (None: Categorical)

    @property
    def dims(self):
        """(d_in, h0, h1, h2, k)"""
        l0, l1, la, l2, _ = self.layers
        return l0.in_features, l0.out_features, l1.out_features, l2.out_features, la.out_features

    def rollout_shape(self, n_envs, obs_dim, cuda):
        """RolloutFacts.small / EvalFacts.small: dims + K32's LDS floats at n_envs envs (0 off the device)."""
        lds = int(_lib.load().xpa_small_rollout_lds_floats(n_envs, obs_dim, *self.dims[1:])) if cuda else 0
        return self.dims + (lds,)

    def fill(self, a):
        """Write the fields XpaSmallRolloutArgs, XpaSmallCloseArgs and XpaSmallMlpArgs share into block a; returns a."""
        l0, l1, la, l2, lc = self.layers
        a.d_in, a.h0, a.h1, a.h2, a.k = self.dims
        a.act_code, a.slope = int(self.code), float(self.slope)
        a.W0, a.b0, a.W1, a.b1, a.W2 = _p(l0.weight), _p(l0.bias), _p(l1.weight), _p(l1.bias), _p(l2.weight)
        a.b2, a.Wa, a.ba, a.Wc, a.bc = _p(l2.bias), _p(la.weight), _p(la.bias), _p(lc.weight), _p(lc.bias)
        return a


# ---- the argument blocks (built at plan time; they hold addresses: plan() rebuilds them when a tensor moves) ----------
def env_block(agent, policy, env, n_envs, horizon, seed, cursor):
    """An XpaSmallRolloutArgs with what the rollout and the evaluation block share: the policy, the observation
    statistics, the env's tensors and episode fields, the action stream.  As it is (horizon 1) K32E's block over test
    envs: the training-only pointers (buffer, returns, slots) stay NULL."""
    a = policy.fill(_lib.XpaSmallRolloutArgs())
    a.n_envs, a.horizon, a.steps, a.use_obsnorm = int(n_envs), int(horizon), 1, int(agent.use_obsnorm)
    a.max_episode_steps, a.obs_clip = int(env.max_episode_steps), float(agent._obs_clip())
    a.seed, a.env_seed = int(seed) & 0xFFFFFFFF, int(env.noise_seed) & 0xFFFFFFFF
    a.obs_mean, a.obs_var, a.obs_count = _p(agent.obs_mean), _p(agent.obs_var), _p(agent.obs_count)
    a.act_in, a.ld_act = _p(env.act_in), env.act_in.stride(0)
    a.env_state, a.env_obs, a.ld_obs = _p(env.state), _p(env.obs), env.obs.stride(0)
    a.final_obs, a.env_rew, a.env_term, a.env_trunc = _p(env.final_obs), _p(env.rew), _p(env.term), _p(env.trunc)
    a.ep_step, a.ep_index, a.ep_score = _p(env.ep_step), _p(env.ep_index), _p(env.ep_score)
    a.ep_last_score, a.ep_last_len, a.cursor = _p(env.ep_last_score), _p(env.ep_last_len), _p(cursor)
    return a


def rollout(agent):
    """K32 / K32W for an agent whose plan's driver is one of them: (block, launch, head).  launch() launches the block
    as it then stands (the caller sets block.steps); head is the agent's entry of xpa_small_rollout_batch's head array
    (None for a Categorical row).  The entry point and the head's extra arguments are resolved here, once per block."""
    mem, policy = agent.memory, agent.learner.small_policy_layers()
    a = env_block(agent, policy, agent.envs, agent.n_envs, agent.n_steps, agent.seed, agent.cursor)
    a.n_slots, a.mask_returns, a.use_rewnorm = int(agent.n_slots), int(agent.algo == "ppo"), int(agent.use_rewnorm)
    a.slot_reset_obs, a.gamma, a.rew_range = int(agent.boot_from_reset), float(agent.gamma), float(agent.rewnorm_range)
    a.obs_norm, a.ld_norm = _p(agent.obs_norm), agent.obs_norm.stride(0)
    logp_buf = mem.auxiliary_infos["old_logp"] if agent.algo == "ppo" else agent.logp_scratch
    a.buf_obs, a.buf_act, a.buf_logp, a.buf_val = _p(mem.observations), _p(mem.actions), _p(logp_buf), _p(mem.values)
    a.buf_rew, a.buf_term, a.buf_closed, a.buf_boot = _p(mem.rewards), _p(mem.terminals), _p(mem.closed), _p(mem.boot)
    a.returns, a.ret_mean, a.ret_var = _p(agent.returns), _p(agent.ret_mean), _p(agent.ret_var)
    a.ret_count, a.slot_obs, a.slot_t = _p(agent.ret_count), _p(agent.slot_obs), _p(agent.slot_t)
    a.overflow, a.boot_norm, a.ld_boot = _p(agent.slot_overflow), _p(agent.boot_obs), agent.boot_obs.stride(0)
    row = SMALL_ENVS[agent.envs.kind, agent.dist]
    fn, ref, device = getattr(_lib.load(), row.rollout), ctypes.byref(a), agent.device
    head = (_p(policy.logstd), float(agent._act_clip())) if row.gaussian else ()
    return a, (lambda: _lib.call(fn, ref, *head, _stream(device))), _lib.XpaSmallRolloutHead(*head) if head else None


def small_close_args(layers, act, rows, slot_t, rew, val, term, closed, boot, adv, ret, gamma, gae_lambda,
                     use_gae=True, vboot_out=None):
    """K33's argument block (XpaSmallCloseArgs) of one agent.  layers: the five Linear modules (representation, actor
    hidden, actor out, critic hidden, critic out) of learner.small_policy_layers, act = (code, slope); rows
    [(S + 1) N, d_in] the normalised deferred bootstrap rows (slot-major, then the last-step rows; row-strided allowed);
    slot_t [S N]; rew / val / term / boot / adv / ret float32 [N, T], closed uint8 [N, T]; vboot_out (optional)
    float32 [(S + 1) N].  The block holds the tensors' addresses and, as a Python object, references that keep them
    alive (a byte copy of it does not)."""
    from . import ops
    N, T = rew.shape
    req = functools.partial(ops._req, cuda=rew.is_cuda)   # off the device: a block to look at, never to launch
    S = ops._n_slots(slot_t, N, rew.is_cuda)
    for name, t in (("rew", rew), ("val", val), ("term", term), ("boot", boot), ("adv", adv), ("ret", ret)):
        req(t, name, torch.float32, (N, T))
    req(closed, "closed", torch.uint8, (N, T))
    req(rows, "rows", torch.float32, contiguous=False)
    ld = ops._row_stride(rows, "rows", layers[0].in_features)
    if rows.shape[0] != (S + 1) * N:
        raise ValueError("rows must hold (n_slots + 1) x n_envs rows")
    if vboot_out is not None:
        req(vboot_out, "vboot_out", torch.float32, ((S + 1) * N,))
    for name, lin in zip("01a2c", layers):
        req(lin.weight, "W" + name, torch.float32)
        req(lin.bias, "b" + name, torch.float32)
    a = SmallPolicy(tuple(layers), act[0], act[1], None).fill(_lib.XpaSmallCloseArgs())
    a.n_envs, a.horizon, a.n_slots, a.use_gae = N, T, S, int(bool(use_gae))
    a.gamma, a.gae_lambda = float(gamma), float(gae_lambda)
    a.rows, a.ld_rows, a.slot_t = _p(rows), ld, _p(slot_t)
    a.rew, a.val, a.term, a.closed = _p(rew), _p(val), _p(term), _p(closed)
    a.boot, a.adv, a.ret, a.vboot_out = _p(boot), _p(adv), _p(ret), None if vboot_out is None else _p(vboot_out)
    a._keep = (layers, rows, slot_t, rew, val, term, closed, boot, adv, ret, vboot_out)
    return a


# ---- the launches (the single-agent rollout's: rollout()) -------------------------------------------------------------
def _head_arrays(heads):   # a batch launch's (host, device) head arguments; heads: (ctypes array, device copy) | None
    return (ctypes.addressof(heads[0]), heads[1].data_ptr()) if heads else (None, None)


def rollout_batch(code, n_agents, blocks, heads, device):
    """xpa_small_rollout_batch: n_agents agents' K32 / K32W launches in one.  code: the SMALL_ENVS row's; blocks (and
    heads, for a Gaussian row; else None): (ctypes array, its copy in device memory as a uint8 tensor)."""
    _lib.call(_lib.load().xpa_small_rollout_batch, _lib.ENV_CODES[code], n_agents, ctypes.addressof(blocks[0]),
              blocks[1].data_ptr(), *_head_arrays(heads), _stream(device))


def small_eval(entry, args, log, capacity, snap_dim, scratch, logstd=None, act_clip=1.0):
    """K32E (a SMALL_ENVS row's eval entry): up to args.steps evaluation steps in one launch, the finished episodes
    into the log.  args: an XpaSmallRolloutArgs whose seed / cursor are the evaluation's; scratch f32 [3 * n_envs]."""
    from .ops import _eval_log_dims, _req
    _eval_log_dims(log, capacity, snap_dim)
    _req(scratch, "scratch", torch.float32, (3 * int(args.n_envs),))
    row = SMALL_BY_ENTRY.get(entry)
    if row is None or entry != row.eval:
        raise _lib.XpaError("no one-launch evaluation entry point named %r" % (entry,))
    head = (_p(_req(logstd, "logstd", torch.float32, (1,))), float(act_clip)) if row.gaussian else ()
    _lib.call(getattr(_lib.load(), entry), ctypes.byref(args), *head, log.data_ptr(), int(capacity), int(snap_dim),
              scratch.data_ptr(), _stream(log.device))


def small_eval_batch(code, n_agents, blocks, heads, evals, device):
    """K32EB (xpa_small_eval_batch): n_agents agents' K32E launches in one, each into its own log.  code: the
    SMALL_ENVS row's; blocks, heads (None for a Categorical row) and evals (XpaSmallEval: log, scratch, capacity,
    snap_dim per agent) as rollout_batch's: (ctypes array, its copy in device memory as a uint8 tensor)."""
    _lib.call(_lib.load().xpa_small_eval_batch, _lib.ENV_CODES[code], n_agents, ctypes.addressof(blocks[0]),
              blocks[1].data_ptr(), *_head_arrays(heads), ctypes.addressof(evals[0]), evals[1].data_ptr(),
              _stream(device))


def small_eval_wide(code, args, log, capacity, snap_dim, scratch, logstd=None, act_clip=1.0):
    """K32WE (xpa_small_eval_wide): small_eval at K32W's widths (h0 = h1 = h2 = 128).  code: the SMALL_ENVS row's; the
    other arguments as small_eval's (logstd / act_clip: a Gaussian row's head)."""
    from .ops import _eval_log_dims, _req
    _eval_log_dims(log, capacity, snap_dim)
    _req(scratch, "scratch", torch.float32, (3 * int(args.n_envs),))
    row = next((r for r in SMALL_ENVS.values() if r.code == code), None)
    if row is None:
        raise _lib.XpaError("no one-launch evaluation for the env code %r" % (code,))
    head = None
    if row.gaussian:
        head = ctypes.byref(_lib.XpaSmallRolloutHead(_p(_req(logstd, "logstd", torch.float32, (1,))), float(act_clip)))
    _lib.call(_lib.load().xpa_small_eval_wide, _lib.ENV_CODES[code], ctypes.byref(args), head, log.data_ptr(),
              int(capacity), int(snap_dim), scratch.data_ptr(), _stream(log.device))


def small_eval_wide_batch(code, n_agents, blocks, heads, evals, device):
    """K32WEB (xpa_small_eval_wide_batch): small_eval_batch at K32W's widths; the same arguments."""
    _lib.call(_lib.load().xpa_small_eval_wide_batch, _lib.ENV_CODES[code], n_agents, ctypes.addressof(blocks[0]),
              blocks[1].data_ptr(), *_head_arrays(heads), ctypes.addressof(evals[0]), evals[1].data_ptr(),
              _stream(device))


def env_reset_batch(code, n_agents, blocks, device):
    """xpa_small_env_reset_batch: the device half of env.reset() for n_agents env sets in one launch, over the blocks an
    evaluation launch takes ((ctypes array, its copy in device memory as a uint8 tensor)); the caller owes each env
    its host half (env.reset_host())."""
    _lib.call(_lib.load().xpa_small_env_reset_batch, _lib.ENV_CODES[code], n_agents, ctypes.addressof(blocks[0]),
              blocks[1].data_ptr(), _stream(device))


def small_close(block, device):
    """K33 (xpa_small_close): one agent's closing — the deferred bootstraps' critic with K32's arithmetic, the
    fixup's writes and the advantage scan — in one launch.  block: small_close_args'."""
    _lib.call(_lib.load().xpa_small_close, ctypes.byref(block), _stream(device))


def small_close_batch(n_agents, host_blocks, dev_blocks, device):
    """K33 for a population (xpa_small_close_batch): host_blocks a ctypes array of XpaSmallCloseArgs, dev_blocks its
    copy in device memory (a uint8 tensor)."""
    _lib.call(_lib.load().xpa_small_close_batch, n_agents, ctypes.addressof(host_blocks), _p(dev_blocks), _stream(device))


def update(block, logstd, device):
    """K30 (xpa_small_mlp_update; with logstd, SmallPolicy.logstd of a Gaussian head, xpa_small_mlp_update_gauss: la is
    the mu layer, act [n_rows, A]); capturable."""
    lib, head = _lib.load(), () if logstd is None else (_p(logstd), _p(logstd.grad))
    _lib.call(lib.xpa_small_mlp_update_gauss if head else lib.xpa_small_mlp_update, ctypes.byref(block), *head,
              _stream(device))


def update_batch(n_agents, blocks, heads, device):
    """xpa_small_mlp_update_batch: one minibatch update of every agent in one launch (capturable); blocks / heads as
    rollout_batch's, the heads XpaSmallMlpGauss."""
    _lib.call(_lib.load().xpa_small_mlp_update_batch, n_agents, ctypes.addressof(blocks[0]), blocks[1].data_ptr(),
              *_head_arrays(heads), _stream(device))
