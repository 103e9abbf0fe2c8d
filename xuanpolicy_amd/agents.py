"""PPO-Clip and A2C agents: the reference's on-policy training loop, device-resident on one GPU.

Mirrors (reference paths):
  Agent base            xuance/torch/agents/agent.py:7-141 (obs/reward normalisation, logging, save/load)
  PPOCLIP_Agent.train   xuance/torch/agents/policy_gradient/ppoclip_agent.py:59-111
  A2C_Agent.train       xuance/torch/agents/policy_gradient/a2c_agent.py:57-107
  REGISTRY              xuance/torch/agents/__init__.py:68-111 ("PPO_Clip", "A2C")
Same constructor (config, envs, policy, optimizer, scheduler, device) and config keys
(n_steps, n_epoch, n_minibatch, gamma, gae_lambda, use_gae, use_advnorm, use_obsnorm, use_rewnorm,
obsnorm_range, rewnorm_range, vf_coef, ent_coef, clip_range, clip_grad_norm / clip_grad, ...).

One env step of the hot loop (device env, no host sync):
   K5  RunningMeanStd.update(obs) + normalise -> policy input and buffer column
   --  policy heads forward (PyTorch-ROCm GEMMs, no autograd)
   K3  sample action, log-prob, store act/logp/value
   K7  env step (GEMM + xpa_synthbox_step, auto-reset)
   K5c normalise the final obs with the same statistics -> critic forward (truncation bootstrap)
   K8  reward norm, return tracker, ret_rms, terminals, path closures; cursor += 1
When the buffer is full: K1 GAE over [n_envs, n_steps]; then n_epoch x n_minibatch updates of
K4 gather -> heads forward -> K2 loss fwd+bwd -> autograd backward -> [all-reduce] -> clip -> Adam.
Host-side envs (numpy VecEnvs) are supported through the same kernels with per-step H2D/D2H copies.

Semantic notes: action sampling uses the counter-hash RNG on device, not torch's
CPU generator; the truncation bootstrap value V(norm(final obs)) is computed for every env each step
(the reference recomputes a full batch once per truncated env, ppoclip_agent.py:99-100); ret_rms merges
all finished envs of a step in one Chan update (mathematically equal to the reference's sequential
single-value updates).
"""
import json
import os
import time

import numpy as np
import torch

from . import _lib, graphs, ops, small_path
from .buffer import DummyOnPolicyBuffer, DummyOnPolicyBuffer_Atari
from .fused_mlp import FusedActorCritic, Rows, _no_form
from .learners import A2C_Learner, PerDQN_Learner, PPOCLIP_Learner
from .policies import policy_discrete, policy_heads, space_shape
from .rollout_plan import (EVAL_TIERS, K32_DRIVERS, SMALL_ENVS, EvalFacts, RolloutFacts, eval_entry, plan_rollout,
                           plan_test)

FLOAT_MAX = 3.0e38
# test_device's action stream: the counter hash keyed by seed ^ EVAL_SALT and a step counter of its own
EVAL_SALT = 0x7E57E9A1


def _cfg(config, name, default):
    return getattr(config, name, default)


# r05: fold the next step's obs_rms.update into K8 on the device-env path (xpa_rollout_post_deferred_norm_rms).
# Measured neutral at C2 (profiles/r05/r05fold: rollout 5.70 / 5.68 ms on vs 5.68 / 5.69 off — the merge chain moves
# into K8, 6.5 + 7.7 -> 15.0 us), so it is an opt-in (bench.py --fold-rms on); off keeps the reference's update order
# exactly, also around test() calls (which update obs_rms with the test observations, ppoclip_agent.py:125)
FOLD_RMS = False
# r06: K8's post step (and, with per-rank obs statistics, the next step's obs_rms.update) inside the env-fused K14 launch
# (K14F, ops.rollout_policy_head_synthbox(post=)): a C2 env step in three launches instead of five
FUSE_POST = True
# r06 (opt-in, XPA_VALUE_GEMM=1 / bench --gae-form k40v): the deferred bootstrap rows' critic on K40V (split GEMM +
# value-head epilogue) feeding the compact GAE scan.  The scan is faster (5.3 vs 6.0 us) but K40V's launch, 64 blocks
# each streaming all of B, costs 25.6 us against the library GEMM's 15.1 for the value form: 30.9 vs 21.1 us per
# iteration, so the value-fused scan (K1V) stays the default
VALUE_GEMM = os.environ.get("XPA_VALUE_GEMM", "0") == "1"


def _space_clip(space):
    """The one symmetric bound of a Box action space (what the device samplers clip a Gaussian action to)."""
    lo, hi = (np.asarray(getattr(space, k), np.float64).reshape(-1) for k in ("low", "high"))
    assert hi.size and np.all(hi == hi[0]) and np.all(lo == -hi) and np.isfinite(hi[0]) and hi[0] > 0, \
        "the device samplers clip to one symmetric bound: action_space low %r high %r" % (lo, hi)
    return float(hi[0])


def rms_rollout_sync(start, end, all_reduce_sum):
    """sync_obs_rms = "rollout" (r06): the rank's rows of a rollout recovered from its running statistics — end = start
    (+) B, Chan's merge being associative over the per-step merges (statistic_tools.py:86-112) — as (n, sum, sum of squares)
    in f64, SUM-reduced over the ranks, and merged into start: the statistics one RunningMeanStd over every rank's rows
    would hold, up to the f32 rounding of the stored mean / var.  start / end = (mean f32 [D], var f32 [D], count f64 [1]);
    returns (mean f32, var f32, count f64)."""
    m0, v0, c0 = start[0].double(), start[1].double(), start[2].double()
    m1, v1, c1 = end[0].double(), end[1].double(), end[2].double()
    n = c1 - c0
    s1 = m1 * c1 - m0 * c0                                       # the rows' sum
    mb = s1 / n
    m2 = v1 * c1 - v0 * c0 - (mb - m0) ** 2 * c0 * n / c1       # the rows' squared deviations about their own mean
    red = torch.cat([n, s1, m2 + s1 * mb])                      # (n, sum, sum of squares)
    all_reduce_sum(red)
    D = m0.shape[0]
    N, S1, Q = red[:1], red[1:1 + D], red[1 + D:]
    mB = S1 / N
    m2B = torch.clamp(Q - S1 * mB, min=0.0)
    tot = c0 + N
    delta = mB - m0
    mean = m0 + delta * N / tot
    var = (v0 * c0 + m2B + delta * delta * c0 * N / tot) / tot
    return mean.float(), var.float(), tot

class _OnPolicyAgent:
    algo = "ppo"

    def __init__(self, config, envs, policy, optimizer, scheduler=None, device=None):
        self.config = config
        self.envs = envs
        self.policy = policy
        self.render = _cfg(config, "render", False)
        self.n_envs = envs.num_envs
        self.n_steps = config.n_steps
        self.n_minibatch = config.n_minibatch
        self.n_epoch = config.n_epoch
        self.gamma = config.gamma
        self.gae_lam = config.gae_lambda
        self.atari = _cfg(config, "env_name", "") == "Atari"
        self.observation_space = envs.observation_space
        self.action_space = envs.action_space
        self.device = next(policy.parameters()).device
        self.discrete = policy_discrete(policy)
        self.dist = "categorical" if self.discrete else "gaussian"
        self.auxiliary_info_shape = {"old_logp": ()} if self.algo == "ppo" else {}
        Buffer = DummyOnPolicyBuffer_Atari if self.atari else DummyOnPolicyBuffer
        self.buffer_size = self.n_envs * self.n_steps
        self.batch_size = self.buffer_size // self.n_minibatch
        self.memory = Buffer(self.observation_space, self.action_space, self.auxiliary_info_shape, self.n_envs,
                             self.n_steps, _cfg(config, "use_gae", True), _cfg(config, "use_advnorm", True),
                             self.gamma, self.gae_lam, device=self.device)
        self.learner = self._make_learner(config, policy, optimizer, scheduler)
        # A2C bootstraps a mid-rollout truncation with V(norm(reset_obs)): a2c_agent.py:88-95 writes obs[i] =
        # reset_obs into next_obs before its critic call (PPO calls the critic first, ppoclip_agent.py:95-101, and
        # both use the final observations for the full-buffer closures).  False: the final observation for A2C too.
        self.boot_from_reset = self.algo == "a2c" and bool(_cfg(config, "a2c_reset_bootstrap", True))
        self.use_obsnorm = bool(_cfg(config, "use_obsnorm", False))
        self.use_rewnorm = bool(_cfg(config, "use_rewnorm", False))
        self.obsnorm_range = float(_cfg(config, "obsnorm_range", 5))
        self.rewnorm_range = float(_cfg(config, "rewnorm_range", 5))
        dev, N, T = self.device, self.n_envs, self.n_steps
        self.obs_shape = space_shape(self.observation_space)
        D = int(np.prod(self.obs_shape)) if len(self.obs_shape) else 1
        self.obs_dim = D
        f32 = dict(dtype=torch.float32, device=dev)
        # RunningMeanStd state (statistic_tools.py:35-60): mean 0, var 1, count 1e-4
        self.obs_mean = torch.zeros((D,), **f32)
        self.obs_var = torch.ones((D,), **f32)
        self.obs_count = torch.full((1,), 1e-4, dtype=torch.float64, device=dev)
        self.ret_mean = torch.zeros((1,), **f32)
        self.ret_var = torch.ones((1,), **f32)
        self.ret_count = torch.full((1,), 1e-4, dtype=torch.float64, device=dev)
        self.returns = torch.zeros((N,), **f32)
        self.cursor = ops.new_cursor(dev)
        self.post_ws = ops.post_workspace(N, dev)
        # Raw observations (uint8 Atari frames without obs normalisation, DummyOnPolicyBuffer_Atari): stored
        # and fed to the policy as they are (AC_CNN_Atari scales by 1/255 on device).
        self.raw_obs = self.memory.observations.dtype == torch.uint8 and not self.use_obsnorm
        self.obs_norm = None if self.raw_obs else torch.empty((N, D), **f32)
        self.boot_obs = None if self.raw_obs else torch.empty((N, D), **f32)
        self.rms_part = (torch.empty((2 * ops.rms_num_partials(N), D), dtype=torch.float64, device=dev)
                         if self.use_obsnorm else None)
        self._rms_ticket = torch.zeros((1,), dtype=torch.int32, device=dev)   # xpa_rms_update's arrival count
        self._policy_in = self.obs_norm
        self.logp_scratch = None if self.algo == "ppo" else torch.zeros((N, T), **f32)
        self.obs_mb = None
        self.adv_part = None
        self._adv_parts = {}   # gather partials -> [g, 2] f64 advantage moments (one per minibatch size)
        self._mb_bufs = {}     # (rows, dtype, row shape) -> (obs_mb, adv_part) of the gathered-minibatch feeds
        self._mid_obs = self._env_in = self._raw_vb = self._raw_slots = self._vboot = None   # made on first use
        self.seed = int(_cfg(config, "seed", 1))
        self._perm_counter = 0
        self._perm_buf = None
        self.device_env = hasattr(envs, "step_device")
        self._act_clip_v = None   # _act_clip's bound, read from the action space on first use
        # The switches below, read after construction too: plan() is their one reader (rollout_plan.plan_rollout)
        self.fuse_env_step = True   # device SynthBox env stepped inside K14 when possible (_env_fused)
        self.fuse_value_gae = True  # deferred bootstraps' value head inside the GAE scan (xpa_gae_scan_value)
        # r06 (K40V): with fuse_value_gae, the deferred bootstraps' critic to the value on the split GEMM (the value head in
        # its epilogue) and the compact GAE scan on exactly SURVEY.md §8(d)'s bytes, where it applies
        self.value_gemm = VALUE_GEMM
        self.fuse_gather = True     # minibatch gather + adv moments inside the update's K13 (fused_mlp.Rows)
        # r05: the next step's obs_rms.update folded into K8 (xpa_rollout_post_deferred_norm_rms) on the device-env
        # path; _rms_pending: the current observation's statistics are not merged yet (the first step, or after
        # anything but a folded step produced env.obs), so that step runs the standalone update first.  An env reset
        # (envs.reset bumps envs.resets) re-arms it.  test() does not: its obs_rms.update merges other rows, and the
        # folded merge of env.obs already happened (the Chan merge is order-independent up to rounding)
        self.fold_rms = FOLD_RMS
        self.fuse_post = FUSE_POST
        self._k14f_ws = None
        self._rms_pending = True
        self._rms_resets = getattr(envs, "resets", 0)
        self._rms_fold_part = None
        # K32: whole device env steps (RMS, normalise, forward, sample, env, post) in one launch (plan().driver)
        self.fused_rollout = bool(_cfg(config, "fused_rollout", True))
        self._k32 = None                      # K32's argument block (small_path.rollout), rebuilt with the plan
        # K33 (opt-in, plan().gae == "K33"): a one-launch small-path rollout closes in one launch, its bootstraps in
        # K32's own arithmetic
        self.small_close = bool(_cfg(config, "small_close", False))
        self._k33 = None                      # K33's argument block, rebuilt with the plan
        self._plan = self._plan_key = None
        self._eval_cursor = None              # test_device's step counter (made on first use; continues across calls)
        self.last_test_log = None             # test_device's decoded episode log (ops.eval_log_decode)
        self._params = list(policy.parameters())   # re-homing (flat.FlatState) moves their data, not the objects
        self.current_step = 0
        self.current_episode = np.zeros((N,), np.int32)
        self.iterations = 0
        self.last_info = None
        self.infos = []          # host copies, one dict per buffer-full phase
        self.log_hook = None     # optional callable(info: dict, step: int) (tensorboard/wandb adapter)
        self.timers = {"rollout": 0.0, "update": 0.0}
        self.phase_events = None
        self.update_log = None   # a list: every update's device loss scalars are appended (tests / diagnostics)
        self._t = 0
        self._host_obs = None
        self.use_graph = bool(_cfg(config, "cuda_graph", True)) and self.device.type == "cuda"
        # Data-parallel normalisation variants; default = per-shard statistics with one
        # gradient all-reduce per minibatch.
        #   sync_obs_rms:   SUM the per-step RMS partials across ranks (identical obs statistics everywhere)
        #   global_advnorm: AVG each minibatch's advantage moments across ranks (global adv-norm)
        self.world = 1
        import torch.distributed as tdist
        if tdist.is_available() and tdist.is_initialized():
            self.world = tdist.get_world_size()
        #   sync_obs_rms = "rollout" (r06): per-rank statistics inside a rollout (graph-captured, folded into K14F), merged
        #                   across ranks once per rollout, before the update (rms_rollout_sync)
        sync_mode = _cfg(config, "sync_obs_rms", False)
        dp_rms = self.world > 1 and self.use_obsnorm
        self.sync_obs_rms_rollout = dp_rms and isinstance(sync_mode, str) and sync_mode.lower() == "rollout"
        self.sync_obs_rms = dp_rms and bool(sync_mode) and not self.sync_obs_rms_rollout
        self._rms_c0 = None
        self.global_advnorm = bool(_cfg(config, "global_advnorm", False)) and self.world > 1
        if self.sync_obs_rms:
            self.use_graph = False  # the per-step collective runs outside a captured graph
        # Deferred truncation bootstraps: the critic runs once per iteration on [truncation slots;
        # last-step obs] instead of on every env at every step.  Only the device envs qualify: their one truncation
        # source is the time limit, so an env truncates at most ceil((T - 1) / max_episode_steps) times before the
        # rollout's last step, and K8 keeps that many slots per env (1 when max_episode_steps >= n_steps, the C1 / C2
        # / C4 case); a host VecEnv may truncate for other reasons (per-step bootstraps).
        max_ep = int(getattr(envs, "max_episode_steps", getattr(envs, "max_episode_length", 0)) or 0)
        self.defer_boot = (bool(_cfg(config, "defer_bootstrap", True)) and not self.raw_obs
                           and hasattr(envs, "step_device") and max_ep > 0)
        self.n_slots = 0
        if self.defer_boot:
            S = max(1, -(-(T - 1) // max_ep))
            self.n_slots = S
            # [truncation slots (slot-major, S x N rows); last-step observations] as one buffer: the deferred critic
            # pass reads it whole (no concatenation launch)
            pair = torch.zeros(((S + 1) * N, D), **f32)
            self.slot_obs, self.boot_obs = pair[:S * N], pair[S * N:]
            self._boot_pair = pair
            self.slot_t = torch.full((S * N,), -1, dtype=torch.int32, device=dev)
            self.slot_overflow = torch.zeros((1,), dtype=torch.int32, device=dev)
            self._overflow_host = self._overflow_event = None
        # Raw-frame device envs whose truncations are always terminal (SynthAtari): K8 gets no per-step bootstrap
        # values (every mid-rollout close is terminal, boot 0) and the last step's are formed after the rollout —
        # one critic forward per iteration instead of one per env step (a2c_agent.py:66-72, 86-98).
        self.raw_defer = (self.raw_obs and self.device_env and bool(_cfg(config, "defer_bootstrap", True))
                          and bool(getattr(envs, "truncation_implies_terminal", False)))
        self._zero_vboot = torch.zeros((N,), **f32) if self.raw_defer else None
        # A2C over raw-frame device envs without that contract: a truncation at step t < T - 1 bootstraps with
        # V(reset frames) = V(obs of step t + 1), which is exactly the value the rollout stores in column t + 1 (the
        # same frames through the same critic forward, weights unchanged inside a rollout), so it is read from there
        # after the rollout (_raw_mid_from_next) instead of a second critic forward over every env at every step
        self.raw_mid_next = (self.raw_obs and self.device_env and self.boot_from_reset and not self.raw_defer
                             and bool(_cfg(config, "defer_bootstrap", True)))
        self._graph = None
        self._graph_pool = None
        # device env steps per replayed graph (train() falls back to single-step replays at chunk boundaries it
        # cannot meet); 1 = per-step graphs
        self.graph_chunk = int(_cfg(config, "graph_chunk", min(self.n_steps, 128)))
        self._chunk_graph = self._chunk_key = None
        # Model / log directories and the logger (agent.py:33-70).  model_dir_save is seed_<seed>_<time>
        # under model_dir, model_dir_load is model_dir itself (what load_model searches); both are created
        # when first written, not at construction (tests and benches build many agents).
        time_string = time.asctime().replace(" ", "").replace(":", "_")
        seed_tag = "seed_%d_" % self.seed
        model_dir = _cfg(config, "model_dir", "./models/")
        self.log_dir = _cfg(config, "log_dir", "./logs/")
        self.model_dir_save = os.path.join(os.getcwd(), model_dir, seed_tag + time_string)
        self.model_dir_load = model_dir
        self.writer = _make_writer(_cfg(config, "logger", "none"), os.path.join(os.getcwd(), self.log_dir,
                                                                               seed_tag + time_string))
        self.use_wandb = False
        # The reference's runner hands over the policy and a torch Adam; the hot path re-homes the parameters
        # into flat buffers (learner.enable_fast_path) so the fused kernels own the update.
        if bool(_cfg(config, "fast_path", True)) and self.device.type == "cuda":
            if bool(_cfg(config, "tunableop", True)):
                from .runner import enable_tuned_gemms
                enable_tuned_gemms()
            self.learner.enable_fast_path(fused_optimizer=bool(_cfg(config, "fused_adam", True)))
            # small minibatches: one hipGraph per minibatch slot (learners._graphed_mlp_update); the agent loop's
            # inputs are persistent buffers, which the graphs need (the drop-in learner.update path keeps it off)
            self.learner.graph_updates = bool(_cfg(config, "graph_update", True))

    def _make_learner(self, config, policy, optimizer, scheduler):
        raise NotImplementedError

    # ---- normalisation (agent.py:104-123) -----------------------------------------------------------
    def _obs_clip(self):
        return self.obsnorm_range if self.use_obsnorm else FLOAT_MAX

    def _act_clip(self):
        """The bound the samplers clip a Gaussian action to on its way into a device env's input: the action space's
        (one symmetric bound for every dimension; _Box's default is 1).  A host env takes the raw actions and clips
        them itself: its env input is scratch."""
        if self.discrete or not self.device_env:
            return 1.0
        if self._act_clip_v is not None:
            return self._act_clip_v
        lo, hi = (np.asarray(getattr(self.action_space, k), np.float64).reshape(-1) for k in ("low", "high"))
        assert hi.size and np.all(hi == hi[0]) and np.all(lo == -hi) and np.isfinite(hi[0]) and hi[0] > 0, \
            "the device samplers clip to one symmetric bound: action_space low %r high %r" % (lo, hi)
        self._act_clip_v = float(hi[0])
        return self._act_clip_v

    def _normalize_into(self, x, out, to_buffer):
        mem = self.memory
        if to_buffer:
            T, D = self.n_steps, self.obs_dim
            ops.obs_normalize(x, self.obs_mean, self.obs_var, self._obs_clip(), out, col_out=mem.observations,
                              col_ld=T * D, cursor=self.cursor)
        else:
            ops.obs_normalize(x, self.obs_mean, self.obs_var, self._obs_clip(), out)

    # ---- the iteration's forms ("Where the rollout's forms are decided") ------------------------
    def _rollout_mlp(self):
        """The learner's FusedActorCritic when it can drive the rollout forward (K14), else None."""
        fm = self.learner._fused_mlp()
        return fm if fm is not None and fm.rollout_ok else None

    def _rollout_cnn(self):
        """The learner's explicit CNN forward (fused_cnn.FusedCNNActorCritic) for raw-frame policies, else None."""
        return self.learner._fused_cnn() if self.raw_obs else None

    def plan(self, obs=None):
        """The RolloutPlan of this agent as it stands, cached under every switch's value, the parameter and buffer
        pointers, env.obs's geometry (obs: env.obs where the caller holds it) and the pending flag: a switch flipped
        after construction takes effect, and a steady step pays this key and one comparison."""
        L, fm = self.learner, self._rollout_mlp()
        F = FusedActorCritic if fm is None else fm
        if obs is None and self.device_env:
            obs = self.envs.obs
        key = (self.fuse_env_step, self.fuse_post, self.fold_rms, self.fuse_value_gae, self.value_gemm,
               self.fuse_gather, self.fused_rollout, self.small_close, self.use_graph, self.graph_chunk, F.ROLLOUT_SPLIT,
               F.ROLLOUT_TRUNK, F.WIDE_TRUNK, ops.S3_GEMMS, L.small_updates, L.small_split, L.graph_updates, L.grad_sync is None,
               bool(self.memory._pending), None if obs is None else (obs.shape, obs.stride()),
               self.memory.observations.data_ptr(), self.memory.actions.data_ptr(),
               *[p.data_ptr() for p in self._params])
        if key != self._plan_key:
            self._plan = plan_rollout(self._facts(fm, F, obs))
            self._k32, self._k32_launch, self._k32_head = \
                small_path.rollout(self) if self._plan.driver in K32_DRIVERS else (None, None, None)
            self._k33 = self._build_small_close() if self._plan.gae == "K33" else None
            self._plan_key = key
        return self._plan

    def _facts(self, fm, F, obs):
        """What plan_rollout decides from (rollout_plan.RolloutFacts), gathered when plan()'s key changes."""
        L, env, mem = self.learner, self.envs, self.memory
        policy = L.small_policy_layers()
        small = policy and policy.rollout_shape(self.n_envs, self.obs_dim, self.device.type == "cuda")
        bufs = (mem.observations, mem.actions, mem.values, mem.rewards, mem.terminals, mem.boot)
        obs_flat = mem.observations.reshape((self.buffer_size,) + tuple(mem.observations.shape[2:]))
        fusable = getattr(env, "fusable_with_policy_step", None)
        return RolloutFacts(
            algo=self.algo, fuse_env_step=self.fuse_env_step, fuse_post=self.fuse_post, fold_rms=self.fold_rms,
            fuse_value_gae=self.fuse_value_gae, value_gemm=self.value_gemm, fuse_gather=self.fuse_gather,
            fused_rollout=self.fused_rollout, use_graph=self.use_graph, graph_chunk=self.graph_chunk,
            rollout_split=F.ROLLOUT_SPLIT, rollout_trunk=F.ROLLOUT_TRUNK, s3_gemms=bool(ops.S3_GEMMS),
            cuda=self.device.type == "cuda", use_obsnorm=self.use_obsnorm, raw_obs=self.raw_obs, atari=self.atari,
            boot_from_reset=self.boot_from_reset, defer_boot=self.defer_boot, raw_defer=self.raw_defer,
            raw_mid_next=self.raw_mid_next, n_slots=self.n_slots, n_steps=self.n_steps, obs_dim=self.obs_dim,
            world=self.world, global_advnorm=self.global_advnorm, pending=bool(mem._pending),
            sync_obs_rms=True if self.sync_obs_rms else "rollout" if self.sync_obs_rms_rollout else False,
            env=getattr(env, "kind", "device") if self.device_env else "host",
            env_fusable=bool(fusable is not None and fusable(self.dist)),
            obs_rows=obs is not None and obs.dim() == 2 and obs.stride(1) == 1,
            shape=None if fm is None else fm.rollout_shape(), cnn=self._rollout_cnn() is not None, small=small,
            small_bufs=(all(b.dtype == torch.float32 and b.is_contiguous() for b in bufs)
                        and mem.closed.is_contiguous()),
            rows_ok=fm is not None and fm.rows_ok(obs_flat), small_update=L.small_update_ok(obs_flat, self.batch_size),
            epoch_graphs=bool(L.graph_updates), dist=self.dist, small_close=bool(self.small_close))

    def _env_fused(self, fm=None):
        """True when the device env's step runs inside the rollout's K14 launch (ops.rollout_policy_head_synthbox);
        fuse_env_step = False keeps the separate env GEMM + K7 launches."""
        return self.plan().env == "in-head"

    # ---- one env step ---------------------------------------------------------------------------------
    def _sample_into_buffer(self, plan, raw_x=None):
        """The policy step in the plan's forms.  raw_x (obs "trunk"): the raw observations, normalised inside the fused
        trunk.  Heads K14E / K14F also step the device env in the launch, K14F runs K8's post step there too (the
        caller then skips env.step_device() / _post)."""
        mem = self.memory
        logp_buf = mem.auxiliary_infos["old_logp"] if self.algo == "ppo" else self.logp_scratch
        env_in = self.envs.act_in if self.device_env else self._act_scratch()
        if plan.head == "K3":
            head, logstd, v = self._heads(plan.trunk, self._policy_in)
            ops.rollout_sample(self.dist, head.contiguous(), logstd, v.contiguous(), self.cursor, self.seed,
                               mem.actions, logp_buf, mem.values, env_in, act_clip=self._act_clip())
            return
        if plan.head not in ("K14", "K14E", "K14F"):
            _no_form("the rollout's head", plan.head)
        norm = None
        if raw_x is not None:
            norm = (self.obs_mean, self.obs_var, self._obs_clip(), self.obs_norm, mem.observations,
                    self.n_steps * self.obs_dim, self.cursor)
        self._rollout_mlp().rollout_act(self._policy_in if raw_x is None else raw_x, self.dist, self.cursor, self.seed,
                                        mem.actions, logp_buf, mem.values, env_in, act_clip=self._act_clip(), norm=norm,
                                        env=self.envs if plan.head != "K14" else None,
                                        post=self._k14f_post(plan) if plan.head == "K14F" else None,
                                        trunk=plan.trunk, pair=plan.pair)

    @torch.no_grad()
    def _heads(self, form, x):
        """(head, logstd, v) of x through the module form of the plan's trunk: the explicit CNN forward or the policy."""
        if form == "cnn":
            return self._rollout_cnn().heads(x)
        if form != "policy":
            _no_form("the policy module's forward", form)
        return policy_heads(self.policy, x)

    def _act_scratch(self):
        if self._env_in is None:
            A = self.action_space.n if self.discrete else int(np.prod(self.action_space.shape))
            self._env_in = torch.zeros((self.n_envs, A), dtype=torch.float32, device=self.device)
        return self._env_in

    def _k8_args(self):
        """What every form of K8 takes after its cursor (ops.rollout_post's keywords, K14F's post dict)."""
        mem = self.memory
        return dict(ret_mean=self.ret_mean, ret_var=self.ret_var, ret_count=self.ret_count, returns=self.returns,
                    buf_rew=mem.rewards, buf_term=mem.terminals, buf_closed=mem.closed, buf_boot=mem.boot,
                    gamma=self.gamma, mask_returns=(self.algo == "ppo"), use_rewnorm=self.use_rewnorm,
                    rew_range=self.rewnorm_range, atari_lifeloss=self.atari)

    def _post(self, plan, rew, term, trunc, final_obs):
        if plan.post == "K8-deferred":
            # final-obs normalisation folded into K8: kept truncation rows and, at the last step, every env's
            # normalised final observation (boot_obs) — no separate normalise launch per step; rms "fold-K8": also the
            # next step's obs_rms.update (its statistics then merged once this step's normalisations are done)
            rms = None
            if plan.rms == "fold-K8":
                if self._rms_fold_part is None:
                    self._rms_fold_part = torch.empty((2 * int(ops.lib().xpa_rollout_post_num_blocks(self.n_envs)),
                                                       self.obs_dim), dtype=torch.float64, device=self.device)
                rms = (self.envs.obs, self.obs_count, self._rms_fold_part)
            ops.rollout_post(rew, term, trunc, None, self.cursor, **self._k8_args(),
                             deferred=(final_obs, self.slot_obs, self.slot_t, self.slot_overflow, self.obs_mean,
                                       self.obs_var, self._obs_clip(), self.boot_obs)
                             + ((self.envs.obs,) if plan.mid == "slots-from-next" else ()),
                             workspace=self.post_ws, rms=rms)
            return
        if plan.post != "K8":
            _no_form("the post step", plan.post)
        # per-step bootstrap values; mid "critic": A2C over a device env stepped per step (replayed graphs: the host
        # does not know which column is the last) gives both, K8 takes V(next obs) for closures before the last step
        v_boot = self._zero_vboot if plan.boot == "zero" else self._step_values(plan, final_obs, self.boot_obs)
        v_mid = None
        if plan.mid == "critic":
            if self._mid_obs is None and not self.raw_obs:
                self._mid_obs = torch.empty_like(self.boot_obs)
            v_mid = self._step_values(plan, self.envs.obs, self._mid_obs).contiguous()
        ops.rollout_post(rew, term, trunc, v_boot.contiguous(), self.cursor, **self._k8_args(),
                         workspace=self.post_ws, v_boot_mid=v_mid)

    def _step_values(self, plan, x, norm_out):
        """V(x) for K8's per-step bootstraps: raw frames as they are, else normalised into norm_out first."""
        if plan.obs == "raw":
            return self._heads(plan.value_trunk, x)[2]
        self._normalize_into(x, norm_out, False)
        return self._values(plan, norm_out)

    def _values(self, plan, x):
        """The critic alone on normalised rows x in the plan's value_trunk form."""
        if plan.value_trunk in ("K13", "chain"):
            return self._rollout_mlp().rollout_value(x, trunk=plan.value_trunk)
        return self._heads(plan.value_trunk, x)[2]

    def _k14f_post(self, plan):
        """K14F's post-step arguments (ops.rollout_policy_head_synthbox(post=)) — the deferred, normalised K8 call of
        _post, with the next step's obs_rms.update where rms is "fold-K14F"."""
        rms = plan.rms == "fold-K14F"
        if self._k14f_ws is None or self._k14f_ws[0] != rms:   # graph-capture safe: allocated on the first (eager) step
            self._k14f_ws = (rms, ops.rollout_step_workspace(self.n_envs, self.obs_dim, rms, self.device))
        return dict(slot_obs=self.slot_obs, slot_t=self.slot_t, overflow=self.slot_overflow,
                    slot_from_next=plan.mid == "slots-from-next", obs_mean=self.obs_mean, obs_var=self.obs_var,
                    obs_count=self.obs_count if rms else None, obs_clip=self._obs_clip(), boot_norm=self.boot_obs,
                    workspace=self._k14f_ws[1], **self._k8_args())

    def _rms_update(self, x):
        if self.sync_obs_rms:
            import torch.distributed as tdist
            ops.rms_update(x, self.obs_mean, self.obs_var, self.obs_count, partials=self.rms_part,
                           reduce_partials=lambda t: tdist.all_reduce(t, op=tdist.ReduceOp.SUM), world=self.world)
        else:
            ops.rms_update(x, self.obs_mean, self.obs_var, self.obs_count, partials=self.rms_part,
                           ticket=self._rms_ticket)

    def _sync_rms_rollout(self):
        """sync_obs_rms = "rollout": every rank's rollout rows merged into the common start statistics (rms_rollout_sync,
        one all-reduce of 2 D + 1 doubles per rollout), so every rank leaves the rollout with the same obs_rms."""
        import torch.distributed as tdist
        m, v, c = rms_rollout_sync(self._rms_c0, (self.obs_mean, self.obs_var, self.obs_count),
                                   lambda t: tdist.all_reduce(t, op=tdist.ReduceOp.SUM))
        self.obs_mean.copy_(m)
        self.obs_var.copy_(v)
        self.obs_count.copy_(c)
        self._rms_c0 = None

    def _build_small_close(self):
        """K33's argument block (xpa_small_close) for a plan whose gae form is "K33": the policy's layers, the deferred
        bootstrap rows and the buffer's tensors; plan() rebuilds it with K32's block."""
        mem = self.memory
        layers, code, slope, _ = self.learner.small_policy_layers()
        return small_path.small_close_args(layers, (code, slope), self._boot_pair, self.slot_t, mem.rewards, mem.values,
                                    mem.terminals, mem.closed, mem.boot, mem._advantages, mem._returns, mem.gamma,
                                    mem.gae_lam, mem.use_gae)

    def _small_close_block(self):
        """K33's block for a launch now: the scan's scalars are the buffer's as they stand, as every other closing
        reads them (the tensors' addresses are the plan's: plan() rebuilds the block when they move)."""
        a, mem = self._k33, self.memory
        a.gamma, a.gae_lambda, a.use_gae = float(mem.gamma), float(mem.gae_lam), int(bool(mem.use_gae))
        return a

    def _small_rollout_launch(self, steps):
        self._k32.steps = int(steps)
        self._k32_launch()

    def _rollout_step_device(self):
        env = self.envs
        x = env.obs
        plan = self.plan(x)
        if plan.driver in K32_DRIVERS:
            self._small_rollout_launch(1)
            return
        if plan.rms is not None:
            if getattr(env, "resets", 0) != self._rms_resets:
                self._rms_resets, self._rms_pending = getattr(env, "resets", 0), True
            if self._rms_pending or plan.rms in ("standalone", "all-reduce"):
                self._rms_update(x)
                self._rms_pending = False
        if plan.obs == "raw":
            ops.store_column(x, self.memory.observations, self.cursor)
            self._policy_in = x
        elif plan.obs == "K5N":
            self._normalize_into(x, self.obs_norm, True)
        elif plan.obs != "trunk":
            _no_form("the observation store", plan.obs)
        self._sample_into_buffer(plan, raw_x=x if plan.obs == "trunk" else None)
        if plan.env != "in-head":
            env.step_device()
        if plan.post != "K14F":
            self._post(plan, env.rew, env.term, env.trunc, env.final_obs)

    def _rollout_step_graph(self):
        """The device env step captured once into a hipGraph and replayed: every per-step argument
        (buffer column, RNG step) lives in the device cursor, so the same graph serves all steps."""
        if self.plan().driver in K32_DRIVERS:   # one launch per step: nothing to capture
            self._rollout_step_device()
            return
        key = tuple(p.data_ptr() for p in self._params)
        if self._graph is not None and key != self._graph_key:
            self._graph = None  # parameters were re-homed (e.g. flat buffers attached): re-capture
        if self._graph is None:
            self._graph_key = key
            side = torch.cuda.Stream(self.device)
            side.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(side):
                self._rollout_step_device()        # a real step (also warms up BLAS handles)
            torch.cuda.current_stream(self.device).wait_stream(side)
            self._graph, _ = graphs.capture(self._rollout_step_device, self._graph_pool)   # recorded, not executed
            return
        self._graph.replay()

    def _rollout_chunk_graph(self, k):
        """k consecutive device env steps captured into ONE hipGraph (k x 5 kernels) and replayed as a unit: a
        per-step replay leaves the GPU idle ~8 us between graphs while the host launches the next (r02 trace:
        127 such gaps = 1.0 ms of a 72 ms iteration).  Same replay invariance as _rollout_step_graph."""
        if self.plan().driver in K32_DRIVERS:   # the k steps as one K32 launch
            self._small_rollout_launch(k)
            return k
        key = (k,) + tuple(p.data_ptr() for p in self._params)
        if self._chunk_graph is not None and key != self._chunk_key:
            self._chunk_graph = None
        if self._chunk_graph is None:
            if self._graph is None:
                self._rollout_step_graph()   # a real first step + the single-step graph (warm-up, BLAS handles)
                return 1
            self._chunk_key = key
            self._chunk_graph, _ = graphs.capture(lambda: [self._rollout_step_device() for _ in range(k)],
                                                  self._graph_pool)   # k steps recorded, not executed
        self._chunk_graph.replay()
        return k

    def _rollout_step_host(self):
        """One step of ppoclip_agent.py:59-111 / a2c_agent.py:57-107 over a host VecEnv (numpy in / out, reset_obs
        in infos; gym_vec_env.py:148-231): the same kernels with per-step H2D / D2H copies, and the loop's host
        semantics kept as they are (checked step for step against oracle.cpu_ref.VecAgentRef,
        tests/test_gpu_hostenv.py):
          * a train() call starts from envs.buf_obs (ppoclip_agent.py:60): a row whose env ended on the previous
            call's last step still holds its final observation there;
          * without obs-norm the reference stores `obs` after envs.step, and on a call's first step that is
            envs.buf_obs itself: the column holds what that array holds after the step (DummyVecEnv writes it in
            place, SubprocVecEnv rebinds it — the object kept here is read either way);
          * done envs continue from infos[i]["reset_obs"]; with env_name "Atari" a life loss (terminal, not
            truncated) keeps the path and the observation (ppoclip_agent.py:93-94);
          * A2C's mid-rollout truncation bootstraps are V(norm(reset_obs)) (a2c_agent.py:88-95, boot_from_reset)."""
        env, dev, plan = self.envs, self.device, self.plan()
        dt = np.uint8 if self.raw_obs else np.float32
        shape = (self.n_envs,) + (tuple(self.obs_shape) if self.raw_obs else (-1,))
        alias = None
        if self._host_obs is None:
            self._host_obs = np.array(env.buf_obs, dt, copy=True).reshape(shape)
            if not self.use_obsnorm:
                alias = env.buf_obs
        x = torch.as_tensor(self._host_obs, device=dev)
        if plan.obs == "raw":
            ops.store_column(x.contiguous(), self.memory.observations, self.cursor)
            self._policy_in = x
        else:
            if plan.rms is not None:
                self._rms_update(x)
            self._normalize_into(x, self.obs_norm, True)
        self._sample_into_buffer(plan)
        t = self._t
        acts = (self.memory.actions[:, t]).cpu().numpy()
        if self.discrete:
            acts = acts.astype(np.int64)
        next_obs, rews, terms, truncs, infos = env.step(acts)
        if alias is not None:   # the stored column is what the vec env's buf_obs holds now
            col = self.memory.observations[:, t]
            col.copy_(torch.as_tensor(np.asarray(alias, dt).reshape(col.shape), device=dev))
        next_obs = np.asarray(next_obs, dt).reshape(shape)
        obs = next_obs.copy()
        for i in range(self.n_envs):
            if terms[i] or truncs[i]:
                if self.atari and not truncs[i]:
                    continue
                obs[i] = np.asarray(infos[i]["reset_obs"], dt).reshape(obs[i].shape)
                self.current_episode[i] += 1
        # K8 reads the bootstrap rows where a path closes: the final observations, except A2C's mid-rollout
        # truncations (reset_obs); the last step's closures use the final observations for every algorithm
        boot_src = obs if (self.boot_from_reset and t < self.n_steps - 1) else next_obs
        self._post(plan, torch.as_tensor(np.asarray(rews, np.float32), device=dev),
                   torch.as_tensor(np.asarray(terms, np.uint8), device=dev),
                   torch.as_tensor(np.asarray(truncs, np.uint8), device=dev), torch.as_tensor(boot_src, device=dev))
        self._host_obs = obs

    # ---- buffer-full phase ------------------------------------------------------------------------------
    def epoch_permutation(self, n, counter=None):
        """The minibatch permutation of the next epoch (ppoclip_agent.py:76-81): a device Feistel
        permutation keyed by (config.seed, epoch counter) — one launch instead of a sort."""
        if counter is not None:   # an explicit epoch (tests, replays): a fresh tensor, no live buffer touched
            return ops.random_permutation(n, self.seed, counter,
                                          out=torch.empty(n, dtype=torch.int64, device=self.device))
        counter = self._perm_counter
        self._perm_counter += 1
        if self._perm_buf is None or self._perm_buf.shape[0] != n:
            self._perm_buf = torch.empty(n, dtype=torch.int64, device=self.device)
        return ops.random_permutation(n, self.seed, counter, out=self._perm_buf)

    def _deferred_bootstraps(self, plan):
        """V([truncation slots; last-step final obs]) in one critic pass ([(S + 1) N] values)."""
        return self._values(plan, self._boot_pair).contiguous().reshape(-1)

    def _raw_last_bootstraps(self, plan):
        """raw_defer: V(final frames of the last step) for the last column's bootstraps (0 where terminal), written
        by xpa_rollout_bootstrap_fixup; a mid-rollout non-terminal close (which would have needed its own value)
        contradicts the env's truncation_implies_terminal contract and raises."""
        mem = self.memory
        T = self.n_steps
        bad = bool(((mem.closed[:, :T - 1] != 0) & (mem.terminals[:, :T - 1] == 0)).any())
        if bad:
            raise RuntimeError("a non-terminal truncation inside the rollout: the env breaks truncation_implies_"
                               "terminal; set config.defer_bootstrap = False")
        N = self.n_envs
        if self._raw_vb is None:
            self._raw_vb = torch.zeros((2 * N,), dtype=torch.float32, device=self.device)
            self._raw_slots = torch.full((N,), -1, dtype=torch.int32, device=self.device)
        self._raw_vb[N:].copy_(self._heads(plan.value_trunk, self.envs.final_obs)[2])
        ops.bootstrap_fixup(self._raw_vb, self._raw_slots, mem.terminals, mem.boot)

    def _raw_mid_from_next(self):
        """raw_mid_next: the bootstrap of every non-terminal close before the last step is V(reset frames) =
        values[:, t + 1] (a2c_agent.py:88-95: obs[i] = reset_obs, then the critic on next_obs); K8 wrote V(final
        frames) there, which only the last column keeps."""
        mem = self.memory
        T = self.n_steps
        if T < 2:
            return
        mid = (mem.closed[:, :T - 1] != 0) & (mem.terminals[:, :T - 1] == 0)
        b = mem.boot[:, :T - 1]
        b.copy_(torch.where(mid, mem.values[:, 1:T], b))

    def _check_overflow(self):
        # More truncations per env than slots cannot happen for the device envs (their one truncation source is the
        # time limit, and __init__ sizes n_slots from it), so this guard of the env contract is checked without a
        # host sync: copied to pinned memory here and read one iteration later.
        if self._overflow_host is None:
            self._overflow_host = torch.zeros((1,), dtype=torch.int32, pin_memory=True)
            self._overflow_event = torch.cuda.Event()
        elif self._overflow_event.query() and int(self._overflow_host[0]):
            raise RuntimeError("an env truncated more often than its time limit allows within one rollout (device env "
                               "contract broken); set config.defer_bootstrap = False")
        self._overflow_host.copy_(self.slot_overflow, non_blocking=True)
        self._overflow_event.record()

    def _gathered_update(self, feed, obs_flat, idx, act_flat, adv_flat, ret_flat, logp_flat, use_advnorm, batches):
        """One minibatch through K4's gather in the "epoch" (appended to batches, None returned), "slot" or "all-reduce"
        feed; returns the update's loss scalars."""
        # one (obs_mb, adv_part) pair per minibatch size: a ragged last minibatch keeps its own buffers, so
        # the pointers the learner's slot graphs are keyed by stay stable across epochs
        key = (idx.shape[0], obs_flat.dtype, tuple(obs_flat.shape[1:]))
        bufs = self._mb_bufs.get(key)
        if bufs is None:
            bufs = self._mb_bufs[key] = (
                torch.empty(key[:1] + key[2], dtype=obs_flat.dtype, device=self.device),
                torch.empty((ops.gather_num_partials(key[0]), 2), dtype=torch.float64, device=self.device))
        self.obs_mb, self.adv_part = bufs
        part = self.adv_part if use_advnorm else None

        def gather(idx=idx, obs_out=self.obs_mb):
            return ops.gather_minibatch(idx, obs_flat, adv=adv_flat if use_advnorm else None, obs_out=obs_out,
                                        adv_partials=part)
        if feed == "epoch":
            batches.append((self.obs_mb, idx, act_flat, adv_flat, ret_flat, logp_flat, part, gather))
            return None
        if feed == "slot":
            # the gather rides in the learner's slot graph when the update is graphed (writes obs_mb / adv_part)
            return self.learner.update_fused(self.obs_mb, idx, act_flat, adv_flat, ret_flat, logp_flat, part,
                                             pre=gather)
        obs_mb, part = gather()
        if part is not None:
            import torch.distributed as tdist
            tdist.all_reduce(part, op=tdist.ReduceOp.SUM)   # (sum, sumsq) over all ranks' minibatches,
            part.div_(self.world)                           # averaged: mean / var of the global minibatch
        return self.learner.update_fused(obs_mb, idx, act_flat, adv_flat, ret_flat, logp_flat, part)

    def _close_rollout(self):
        """The end of a full rollout, up to the first minibatch: the bootstrap values (one critic pass over the
        deferred rows) and the advantage scan, in the plan's forms."""
        plan, mem = self.plan(), self.memory
        mem.size = self.n_steps
        if plan.close == "raw-last":
            self._raw_last_bootstraps(plan)
        elif plan.close == "raw-mid-next":
            self._raw_mid_from_next()
        gae = plan.gae
        if gae == "scan":
            mem.compute_advantages()
        elif gae == "K33":
            # one launch: the deferred rows' critic in K32's arithmetic, the fixup's writes and the advantage scan
            small_path.small_close(self._small_close_block(), self.device)
            self._closed_small()
        elif gae == "value":
            # one launch: the critic's output layer, the fixup's bootstrap writes and the compact GAE scan
            fm = self._rollout_mlp()
            lin_co = fm.critic[-1][0]
            _, code, slope = fm.critic[-2]
            zc = fm.rollout_value_hidden(self._boot_pair, trunk=plan.value_trunk)
            ops.gae_scan_value(mem.rewards, mem.values, mem.terminals, self.slot_t, zc, (code, slope), lin_co.weight,
                               lin_co.bias, mem.gamma, mem.gae_lam, mem.use_gae, adv=mem._advantages,
                               ret=mem._returns, boot=mem.boot)
            mem._dirty = False
            self.gae_form = "value"
        elif gae in ("K40V+compact", "compact", "fixup+scan"):
            if gae == "K40V+compact":   # the deferred bootstrap rows' critic on the split GEMM
                if self._vboot is None:
                    self._vboot = torch.empty(self._boot_pair.shape[0], dtype=torch.float32, device=self.device)
                vboot = self._rollout_mlp().rollout_value_split(self._boot_pair, out=self._vboot,
                                                                trunk=plan.value_trunk)
            else:
                vboot = self._deferred_bootstraps(plan)
            if gae == "fixup+scan":
                ops.bootstrap_fixup(vboot, self.slot_t, mem.terminals, mem.boot)
                mem.compute_advantages()
            else:
                # one launch: the fixup's bootstrap writes fused into the compact-closure GAE scan
                ops.gae_scan_compact(mem.rewards, mem.values, mem.terminals, self.slot_t, vboot, mem.gamma,
                                     mem.gae_lam, mem.use_gae, adv=mem._advantages, ret=mem._returns, boot=mem.boot)
                mem._dirty = False
                self.gae_form = "compact"
        else:
            _no_form("the advantage scan", gae)

    def _closed_small(self):
        """The host state a K33 launch (the agent's own, or the population's batch launch) leaves."""
        self.memory.size = self.n_steps
        self.memory._dirty = False
        self.gae_form = "K33"

    def _flat_rows(self):
        """The closed rollout as the minibatch updates read it: (obs, act, adv, ret, old_logp) flat over env x step."""
        mem, NT = self.memory, self.buffer_size
        obs_flat = mem.observations.reshape((NT,) + tuple(mem.observations.shape[2:]))
        act_flat = mem.actions.reshape(-1)
        adv_flat = mem.advantages.reshape(-1)
        ret_flat = mem.returns.reshape(-1)
        logp_flat = mem.auxiliary_infos["old_logp"].reshape(-1) if self.algo == "ppo" else None
        return obs_flat, act_flat, adv_flat, ret_flat, logp_flat

    def _update_phase(self):
        self._close_rollout()
        if self.phase_events is not None:   # measurement hook: closing | epochs split of the update
            self.phase_events.append(("close_end", torch.cuda.Event(enable_timing=True)))
            self.phase_events[-1][1].record()
        plan, mem = self.plan(), self.memory
        NT, B = self.buffer_size, self.batch_size
        obs_flat, act_flat, adv_flat, ret_flat, logp_flat = self._flat_rows()
        use_advnorm = mem.use_advnorm
        scalars = None
        feed, log = plan.feed, self.update_log
        if feed not in ("rows", "small", "epoch", "slot", "all-reduce"):
            _no_form("the minibatch feed", feed)
        for _ in range(self.n_epoch):
            perm = self.epoch_permutation(NT)
            if feed == "small":
                # K30: the whole small-MLP update (gather + forward + loss + backward + clip + Adam) in one launch per
                # minibatch, an epoch of them one captured graph (learners.small_epoch)
                batches = [(perm[s:s + B], act_flat, adv_flat, ret_flat, logp_flat) for s in range(0, NT, B)]
                outs = self.learner.small_epoch(obs_flat, batches, use_advnorm, keep_all=log is not None)
                scalars = outs[-1]
                if log is not None:
                    log.extend(outs)
                continue
            batches = []
            for start in range(0, NT, B):
                idx = perm[start:start + B]
                b = idx.shape[0]
                if feed == "rows":
                    # K4 folded into K13: the update reads the minibatch rows (and forms the adv moments) through idx
                    g = ops.gather_num_partials(b)
                    if g not in self._adv_parts:   # one per minibatch size (a ragged last minibatch keeps its own)
                        self._adv_parts[g] = torch.empty((g, 2), dtype=torch.float64, device=self.device)
                    self.adv_part = self._adv_parts[g]
                    scalars = self.learner.update_fused(Rows(obs_flat, idx), idx, act_flat, adv_flat, ret_flat,
                                                        logp_flat, self.adv_part if use_advnorm else None)
                else:
                    scalars = self._gathered_update(feed, obs_flat, idx, act_flat, adv_flat, ret_flat, logp_flat,
                                                    use_advnorm, batches)
                if log is not None and scalars is not None:
                    log.append(scalars.clone())
            if batches:
                # graphed small-batch updates (C1): the epoch's minibatches go to the learner as one list, which replays
                # them as one captured graph once every slot is captured (learners.update_epoch)
                outs = self.learner.update_epoch(batches, keep_all=log is not None)
                scalars = outs[-1]
                if log is not None:
                    log.extend(outs)
        self._end_update(scalars)

    def _end_update(self, scalars):
        """After an iteration's last minibatch update is enqueued; scalars: that update's loss scalars."""
        self.last_info = scalars
        self.iterations += 1
        if self.defer_boot:
            # after the whole update is enqueued: a D2H copy here no longer holds the host back before the critic
            # pass + GAE (issued right after the rollout graph, it made the GPU idle 30-100 us before K1V)
            self._check_overflow()

    def log_infos(self, info, x_index):
        """agent.py:81-94: every entry to the logger (tensorboard when importable, else JSON lines in
        log_dir) and to log_hook."""
        if self.log_hook is not None:
            self.log_hook(info, x_index)
        if self.writer is not None:
            self.writer.write(info, x_index)

    def _host_info(self):
        info = self.learner._info(self.last_info)
        info["iteration"] = self.iterations
        info["step"] = self.current_step
        return info

    # ---- public API (ppoclip_agent.py:59-111) -------------------------------------------------------------
    def train(self, train_steps, log=True):
        plan = self.plan()
        step_fn = {"host": self._rollout_step_host, "graph-chunk": self._rollout_step_graph,
                   "graph-step": self._rollout_step_graph}.get(plan.driver, self._rollout_step_device)
        if plan.driver == "host":
            self._host_obs = None   # every call starts from envs.buf_obs (ppoclip_agent.py:60)
        chunk = plan.chunk
        left = train_steps
        while left > 0:
            t0 = time.perf_counter()
            if self._t == 0:
                self._begin_rollout()
            if chunk > 1 and left >= chunk and self._t % chunk == 0 and self.n_steps - self._t >= chunk:
                k = self._rollout_chunk_graph(chunk)
            else:
                step_fn()
                k = 1
            left -= k
            self._advance(k)
            t1 = time.perf_counter()
            self.timers["rollout"] += t1 - t0
            if self._t == self.n_steps:
                if self.sync_obs_rms_rollout and self._rms_c0 is not None:
                    self._sync_rms_rollout()
                if self.phase_events is not None:   # measurement hook (bench.py): rollout | update split
                    self.phase_events.append(("rollout_end", torch.cuda.Event(enable_timing=True)))
                    self.phase_events[-1][1].record()
                self._update_phase()
                if self.phase_events is not None:
                    self.phase_events.append(("update_end", torch.cuda.Event(enable_timing=True)))
                    self.phase_events[-1][1].record()
                self._end_iteration(log)
                self.timers["update"] += time.perf_counter() - t1

    def _begin_rollout(self):
        """Ahead of a rollout's first step, outside any captured graph."""
        if self.sync_obs_rms_rollout:   # the common statistics every rank starts this rollout from
            self._rms_c0 = (self.obs_mean.clone(), self.obs_var.clone(), self.obs_count.clone())
        fc = self._rollout_cnn()
        if fc is not None:
            fc.refresh()   # outside any captured graph: the replays read the refreshed weight copy
        pair = self.plan().pair
        if pair is not None:
            self._rollout_mlp().rollout_refresh(pair)   # K40R's weight planes (same: outside the graphs)

    def _advance(self, k):
        """The host's view of k device env steps just enqueued."""
        self._t += k
        self.memory.ptr = self._t % self.n_steps
        self.memory.size = min(self.memory.size + k, self.n_steps)
        self.current_step += self.n_envs * k

    def _end_iteration(self, log):
        """After the update phase: the buffer starts over and the iteration's info is logged."""
        self._t = 0
        self.memory.ptr, self.memory.size = 0, 0
        if log:
            info = self._host_info()
            self.infos.append(info)
            self.log_infos(info, self.current_step)

    def save_model(self, model_name):
        """agent.py:74-76: the policy's state_dict to model_dir_save/model_name."""
        os.makedirs(self.model_dir_save, exist_ok=True)
        self.learner.save_model(self.model_dir_save + "/" + model_name)

    def load_model(self, path, seed=1):
        """agent.py:78-79 -> learner.py:27-48 (newest file of the seed_<seed> directory under path)."""
        self.learner.load_model(path, seed)

    # ---- test (ppoclip_agent.py:113-165, a2c_agent.py:109-160) ----------------------------------------
    @torch.no_grad()
    def _test_action(self, x):
        head, logstd, _ = policy_heads(self.policy, x)
        if self.discrete:
            a = torch.distributions.Categorical(logits=head).sample()
        else:
            a = head + logstd.exp() * torch.randn_like(head)   # stochastic_sample of Normal(mu, exp(logstd))
        return a.cpu().numpy()

    def _test_obs(self, obs):
        """The reference updates obs_rms in test() too (ppoclip_agent.py:125) and normalises with it."""
        x = obs if isinstance(obs, torch.Tensor) else torch.as_tensor(np.asarray(obs))
        if self.raw_obs:
            return x.to(self.device)
        x = x.to(device=self.device, dtype=torch.float32).reshape(x.shape[0], -1).contiguous()
        if self.use_obsnorm:
            ops.rms_update(x, self.obs_mean, self.obs_var, self.obs_count)
        out = torch.empty_like(x)
        ops.obs_normalize(x, self.obs_mean, self.obs_var, self._obs_clip(), out)
        return out

    # ---- test on the device (config.device_test; DESIGN.md §3, "Evaluation on the device") ----------------------
    def _eval_facts(self, test_envs):
        """What plan_test decides from (rollout_plan.EvalFacts) for these test envs."""
        device = hasattr(test_envs, "step_device")
        n = int(test_envs.num_envs)
        policy = self.learner.small_policy_layers()
        small = policy and policy.rollout_shape(n, self.obs_dim, self.device.type == "cuda")
        return EvalFacts(cuda=self.device.type == "cuda", env=getattr(test_envs, "kind", "device") if device else "host",
                         dist=self.dist, small=small, n_envs=n, obs_dim=self.obs_dim, raw_obs=self.raw_obs,
                         world=self.world, sync_obs_rms=True if self.sync_obs_rms else
                         "rollout" if self.sync_obs_rms_rollout else False,
                         wide_eval=bool(_cfg(self.config, "device_test_wide", False)))

    def _eval_stream(self, rng):
        """(seed, cursor) of the evaluation's action stream: seed ^ EVAL_SALT and a step counter of its own that
        continues across calls — the training stream (self.seed, self.cursor) is neither replayed nor advanced;
        rng = (seed, step) replaces both for one call (tests)."""
        if rng is not None:
            cur = ops.new_cursor(self.device)
            step = int(rng[1]) & 0xFFFFFFFF
            cur[1] = step - (1 << 32) if step >= (1 << 31) else step   # the uint32 step counter's bits
            return int(rng[0]) & 0xFFFFFFFF, cur
        if self._eval_cursor is None:
            self._eval_cursor = ops.new_cursor(self.device)
        return (int(self.seed) ^ EVAL_SALT) & 0xFFFFFFFF, self._eval_cursor

    def _eval_scalars(self, env):
        """(snap_dim, act_clip) of an evaluation on env: the log's snapshot width and the sampler's action clip."""
        return (0 if self.raw_obs or not self.use_obsnorm else self.obs_dim,
                1.0 if self.discrete else _space_clip(env.action_space))

    def _build_small_eval(self, env, seed, cursor):
        """K32E's argument block over the test envs (small_path.env_block) and the Gaussian head's logstd (or None)."""
        policy = self.learner.small_policy_layers()
        return small_path.env_block(self, policy, env, env.num_envs, 1, seed, cursor), policy.logstd

    @torch.no_grad()
    def _eval_step(self, env, ws, log, capacity, snap_dim, seed, cursor, act_clip):
        """One evaluation step of the "steps" tier, eager on the current stream, no host synchronisation: the host
        loop's obs_rms.update + normalise + policy forward, K3 with horizon 1 into scratch columns and the test envs'
        action input, the env's step, xpa_eval_post."""
        x = env.obs
        stats = None
        if not self.raw_obs:
            if self.use_obsnorm:
                ops.rms_update(x, self.obs_mean, self.obs_var, self.obs_count, partials=ws["part"], ticket=ws["ticket"])
                stats = (self.obs_mean, self.obs_var, self.obs_count)
            x = ops.obs_normalize(x, self.obs_mean, self.obs_var, self._obs_clip(), ws["norm"])
        head, logstd, v = policy_heads(self.policy, x)
        ops.rollout_sample(self.dist, head.contiguous(), logstd, v.contiguous(), cursor, seed, ws["act"], ws["logp"],
                           ws["val"], env.act_in, act_clip=act_clip)
        env.step_device()
        ops.eval_post(log, capacity, snap_dim, env.term, env.trunc, env.ep_last_score, env.ep_last_len, self.atari,
                      cursor, stats=stats)

    def plan_test(self, test_envs):
        """The tier test_device would evaluate these envs on: "K32E" | "K32WE" | "steps" | "host"
        (rollout_plan.plan_test)."""
        return plan_test(self._eval_facts(test_envs))

    def test_device(self, test_envs, test_episode, chunk=None, rng=None):
        """test()'s loop on the device: the scores of the episodes that end on test_envs, in the order the reference's
        loop appends them (step-major, ascending env index), up to and including the first step at which test_episode
        of them have ended; obs_rms ends as it stands after that many updates, and nothing else of the agent changes.
        Actions come from the counter-hash sampler on the evaluation's own stream (_eval_stream).
          tier "K32E"   xpa_small_eval_*: `chunk` steps per launch (default 128, a training K32 launch), the log's
                        header read after each launch; the kernel stops at the completing step itself
          tier "K32WE"  xpa_small_eval_wide: K32E at 128-wide layers (config.device_test_wide), run the same way
          tier "steps"  _eval_step, `chunk` steps (default 8) between header reads; steps past the completing one
                        still update obs_rms, which is then restored from the log's snapshot.  The eager step is
                        bound by the host's launch rate (~250 us at C2's nets), so a read every 8 steps waits for
                        nothing and at most 7 steps run past the stop (with 32, a 34-step evaluation paid for 64)
        A log that is not complete after (test_episode // N + 2) * max_episode_steps steps raises."""
        f = self._eval_facts(test_envs)
        tier = plan_test(f)
        if tier == "host":
            raise ValueError("test_device: these test envs plan the host loop (no step_device, a CPU device, or a "
                             "per-step obs_rms collective); use test()")
        env, dev = test_envs, self.device
        N, target = int(env.num_envs), int(test_episode)
        max_ep = int(getattr(env, "max_episode_steps", 0) or 0)
        if target < 1 or max_ep < 1:
            raise ValueError("test_device: test_episode >= 1 and time-limited test envs (max_episode_steps)")
        env.reset()
        seed, cursor = self._eval_stream(rng)
        snap_dim, act_clip = self._eval_scalars(env)
        capacity = target + N
        log = ops.eval_log_new(target, N, snap_dim, dev)
        bound = (target // N + 2) * max_ep
        if tier in EVAL_TIERS:
            chunk = 128 if chunk is None else int(chunk)
            args, logstd = self._build_small_eval(env, seed, cursor)
            args.steps, entry = chunk, eval_entry(f)
            scratch = torch.empty((3 * N,), dtype=torch.float32, device=dev)
            code = SMALL_ENVS[f.env, f.dist].code

            def step():
                if tier == "K32WE":
                    small_path.small_eval_wide(code, args, log, capacity, snap_dim, scratch, logstd, act_clip)
                else:
                    small_path.small_eval(entry, args, log, capacity, snap_dim, scratch, logstd, act_clip)
        else:
            chunk = 8 if chunk is None else int(chunk)
            A = env.act_in.shape[1]
            f32 = dict(dtype=torch.float32, device=dev)
            ws = {"act": torch.empty((N, 1, A) if not self.discrete else (N, 1), **f32),
                  "logp": torch.empty((N, 1), **f32), "val": torch.empty((N, 1), **f32)}
            if not self.raw_obs:
                ws["norm"] = torch.empty((N, self.obs_dim), **f32)
                ws["part"] = torch.empty((2 * ops.rms_num_partials(N), self.obs_dim), dtype=torch.float64, device=dev)
                ws["ticket"] = torch.zeros((1,), dtype=torch.int32, device=dev)

            def step():
                for _ in range(chunk):
                    self._eval_step(env, ws, log, capacity, snap_dim, seed, cursor, act_clip)
        if chunk < 1:
            raise ValueError("test_device: chunk >= 1")
        issued = 0
        while True:
            step()
            issued += chunk
            h = ops.eval_log_header(log)
            if h["overflow"]:
                raise _lib.XpaError("test_device: the episode log overflowed (%d entries, capacity %d)"
                                    % (h["count"], capacity))
            if h["done"]:
                break
            if issued >= bound:
                raise RuntimeError("test_device: %d of %d episodes ended in %d steps (bound %d = (test_episode // N + 2)"
                                   " * max_episode_steps)" % (h["count"], target, h["steps_run"], bound))
        if tier == "steps" and snap_dim and issued > h["steps_run"]:
            cnt, mean, var = ops.eval_log_snapshot(log, snap_dim)   # obs_rms as it stood after steps_run updates
            self.obs_count.copy_(cnt)
            self.obs_mean.copy_(mean)
            self.obs_var.copy_(var)
        self.last_test_log = ops.eval_log_decode(log.cpu().numpy())
        return [float(s) for s in self.last_test_log["score"]]

    def test(self, env_fn, test_episode):
        """Run the current policy (stochastic actions) on env_fn()'s envs until test_episode episodes have
        ended; returns their scores (infos[i]['episode_score']).  config.device_test: on the device (test_device)
        where plan_test allows it."""
        test_envs = env_fn()
        if bool(_cfg(self.config, "device_test", False)) and self.plan_test(test_envs) != "host":
            return self._finish_test(test_envs, self.test_device(test_envs, test_episode))
        num_envs = test_envs.num_envs
        current_episode, scores = 0, []
        obs, _ = test_envs.reset()
        obs = obs.cpu().numpy() if isinstance(obs, torch.Tensor) else np.asarray(obs)
        verbose = bool(_cfg(self.config, "test_mode", False))
        while current_episode < test_episode:
            acts = self._test_action(self._test_obs(obs))
            if self.discrete:
                acts = acts.astype(np.int64)
            next_obs, rewards, terminals, truncations, infos = test_envs.step(acts)
            obs = np.array(next_obs, copy=True)
            for i in range(num_envs):
                if terminals[i] or truncations[i]:
                    if self.atari and not truncations[i]:   # life loss: the game goes on
                        continue
                    obs[i] = infos[i]["reset_obs"]
                    scores.append(infos[i]["episode_score"])
                    current_episode += 1
                    if verbose:
                        print("Episode: %d, Score: %.2f" % (current_episode, infos[i]["episode_score"]))
        return self._finish_test(test_envs, scores, listed=True)

    def _finish_test(self, test_envs, scores, listed=False):
        """test()'s tail, shared by the host loop, the device path and Population.test: the scores printed under
        config.test_mode (listed: the host loop printed each episode as it ended), the two test infos logged at
        current_step, the test envs closed; returns scores."""
        if bool(_cfg(self.config, "test_mode", False)):
            for i, s in enumerate(() if listed else scores):
                print("Episode: %d, Score: %.2f" % (i + 1, s))
            print("Best Score: %.2f" % max(scores, default=-np.inf))
        self.log_infos({"Test-Episode-Rewards/Mean-Score": float(np.mean(scores)),
                        "Test-Episode-Rewards/Std-Score": float(np.std(scores))}, self.current_step)
        test_envs.close()
        return scores

    def finish(self):
        if self.writer is not None:
            self.writer.close()


class PPOCLIP_Agent(_OnPolicyAgent):
    algo = "ppo"

    def _make_learner(self, config, policy, optimizer, scheduler):
        return PPOCLIP_Learner(policy, optimizer, scheduler, _cfg(config, "device", None), _cfg(config, "model_dir", "./"),
                               vf_coef=config.vf_coef, ent_coef=config.ent_coef, clip_range=config.clip_range,
                               clip_grad_norm=config.clip_grad_norm, use_grad_clip=_cfg(config, "use_grad_clip", True))


class A2C_Agent(_OnPolicyAgent):
    algo = "a2c"

    def _make_learner(self, config, policy, optimizer, scheduler):
        return A2C_Learner(policy, optimizer, scheduler, _cfg(config, "device", None), _cfg(config, "model_dir", "./"),
                           config.vf_coef, config.ent_coef, config.clip_grad)


class PerDQN_Agent:
    """perdqn_agent.py:4-95 (BASELINE.json configs[4]): e-greedy DQN with prioritized replay, device-resident.

    Same constructor and train(train_steps) loop as the reference: each step stores (obs, act, rew, term, next)
    in the PER buffer (K6 store: the new leaf at max priority), and every training_frequency steps after
    start_training samples a batch (K6 sample: stratified prefix-sum descent + IS weights; K4 gathers the uint8
    frames), runs PerDQN_Learner.update (Q forwards / backward on PyTorch-ROCm, K19 TD / loss / gradient /
    priorities) and writes the |TD| priorities back (K6 update) without leaving the GPU.  PER_beta and the
    e-greedy rate follow perdqn_agent.py:74-95.  With a device env (step_device / act_in, e.g. the SynthAtari
    vec env with 18 actions) the loop never copies frames to the host; the coin flip of the e-greedy choice is
    the reference's np.random draw (one host draw per step, no sync)."""

    def __init__(self, config, envs, policy, optimizer, scheduler=None, device=None):
        from .per import PerOffPolicyBuffer
        self.config = config
        self.envs = envs
        self.policy = policy
        self.device = torch.device(device if device is not None else _cfg(config, "device", "cuda:0"))
        self.n_envs = envs.num_envs
        self.gamma = config.gamma
        self.train_frequency = config.training_frequency
        self.start_training = config.start_training
        self.start_greedy, self.end_greedy = config.start_greedy, config.end_greedy
        self.egreedy = config.start_greedy
        self.decay_step_greedy = _cfg(config, "decay_step_greedy", 1)
        self.observation_space, self.action_space = envs.observation_space, envs.action_space
        self.PER_beta0 = self.PER_beta = config.PER_beta0
        self.atari = _cfg(config, "env_name", "") == "Atari"
        obs_dtype = torch.uint8 if self.atari else torch.float32
        self.memory = PerOffPolicyBuffer(self.observation_space, self.action_space, {}, self.n_envs, config.n_size,
                                         config.batch_size, config.PER_alpha, device=self.device,
                                         seed=_cfg(config, "seed", 1), obs_dtype=obs_dtype)
        self.learner = PerDQN_Learner(policy, optimizer, scheduler, self.device, _cfg(config, "model_dir", "./"),
                                      config.gamma, config.sync_frequency)
        self.device_env = hasattr(envs, "step_device")
        self.current_step = 0
        self.current_episode = np.zeros(self.n_envs, np.int32)
        self.infos = []
        # perdqn_agent.py:57-66: train() starts from `obs = self.envs.buf_obs` and stores `obs` after envs.step, so the
        # first store of every train() call holds whatever that array holds after the step: the step's frames for a
        # vec env that writes buf_obs in place (DummyVecEnv, gym_vec_env.py:228), the pre-step ones for one that
        # rebinds it (SubprocVecEnv, gym_vec_env.py:101).  A host vec env is handled by keeping that object and
        # storing its contents; the device envs model the in-place DummyVecEnv (their final_obs).  Reproduced by
        # default (a drop-in stores what the reference stores); False stores the pre-step frames.
        self.alias_first_obs = bool(_cfg(config, "alias_first_obs", True))
        # optional callable() -> uniforms [n_envs, batch / n_envs] for the next PER sample (e.g. the reference's
        # recorded random.random() draws, memory_tools.py:415); None: the buffer's counter-hash uniforms
        self.uniform_source = None

    def _action(self, obs, egreedy=0.0):
        """perdqn_agent.py:47-54: argmax of the eval Q row, or (with probability egreedy, one draw for all envs)
        uniform random actions from np.random, as the reference draws them."""
        q = self.learner.q_values(obs)
        argmax_action = q.argmax(dim=-1)
        random_action = np.random.choice(self.action_space.n, self.n_envs)
        if np.random.rand() < egreedy:
            return torch.as_tensor(random_action, device=self.device)
        return argmax_action

    def _env_step(self, acts):
        """(next observation to store, rew, term, trunc); the observation the policy sees next is env.obs (device
        env: the kernel already continued done envs from their reset state) or self._host_obs."""
        env = self.envs
        if self.device_env:
            env.act_in.zero_()
            env.act_in.scatter_(1, acts.long().reshape(-1, 1), 1.0)
            env.step_device()
            return env.final_obs, env.rew, env.term, env.trunc
        nxt, rew, term, trunc, infos = env.step(acts.cpu().numpy())
        self._host_obs = np.array(nxt, copy=True)
        for i in range(self.n_envs):   # perdqn_agent.py:76-83: continue from reset_obs (not on an Atari life loss)
            if (term[i] or trunc[i]) and not (self.atari and not trunc[i]):
                self._host_obs[i] = infos[i]["reset_obs"]
        return nxt, rew, term, trunc

    def train(self, train_steps, sync_info=False):
        """perdqn_agent.py:56-95.  A host vec env: every call starts from envs.buf_obs (perdqn_agent.py:57), whose rows
        of envs that ended on the previous call's last step still hold their final frames."""
        env = self.envs
        buf0 = None
        if not self.device_env:
            buf0 = env.buf_obs
            self._host_obs = np.array(buf0, copy=True)
        for k in range(train_steps):
            obs = env.obs.clone() if self.device_env else self._host_obs
            acts = self._action(obs, self.egreedy)
            nxt, rew, term, trunc = self._env_step(acts)
            first = obs
            if k == 0 and self.alias_first_obs:
                first = nxt if self.device_env else np.array(buf0, copy=True)
            self.memory.store(first, acts, rew, term, nxt)
            if self.current_step > self.start_training and self.current_step % self.train_frequency == 0:
                u = self.uniform_source() if self.uniform_source is not None else None
                o, a, r, d, n, w, idxes = self.memory.sample(self.PER_beta, uniforms=u)
                td_abs, info = self.learner.update(o, a, r, n, d, sync_info=sync_info)
                self.memory.update_priorities(idxes, td_abs, check=False)
                info["epsilon-greedy"] = self.egreedy
                self.infos.append(info)
            self.PER_beta += (1 - self.PER_beta0) / train_steps
            self.egreedy = self.egreedy - (self.start_greedy - self.end_greedy) / train_steps
            self.current_step += self.n_envs
            if self.egreedy > self.end_greedy:
                self.egreedy = self.egreedy - (self.start_greedy - self.end_greedy) / self.decay_step_greedy


    def check_errors(self):
        """The device loop's error words since the last call (one host sync): PER sample draws clamped past the
        stored leaves, gathered indices outside the replay buffer, env steps without an action, actions outside
        [0, n) in the TD kernel, max-pool argmax outside the window.  All 0 unless something upstream is corrupt."""
        out = dict(zip(("per_sample", "gather"), self.memory.check_errors()))
        for name, t in (("env", getattr(self.envs, "err", None)), ("td_action", self.learner._err)):
            out[name] = int(t.item()) if t is not None else 0
            if t is not None:
                t.zero_()
        fq = self.learner._fused_q()
        e = getattr(fq.eval_trunk, "err", None) if fq is not None else None
        out["maxpool"] = int(e.item()) if e is not None else 0
        if e is not None:
            e.zero_()
        return out


REGISTRY = {"PPO_Clip": PPOCLIP_Agent, "A2C": A2C_Agent, "PerDQN": PerDQN_Agent}
Agent = _OnPolicyAgent


def get_total_iters(agent_name, args):
    """agent.py:144-145: the LinearLR horizon the runner and the examples use."""
    return args.running_steps


class _JsonlWriter:
    """Scalar sink for log_infos when no tensorboard / wandb is importable: one JSON object per line."""

    def __init__(self, log_dir):
        self.path = os.path.join(log_dir, "scalars.jsonl")
        self._f = None

    def write(self, info, step):
        if self._f is None:
            os.makedirs(os.path.dirname(self.path), exist_ok=True)
            self._f = open(self.path, "a")
        rec = {"step": int(step)}
        for k, v in info.items():
            if isinstance(v, dict):
                rec.update({"%s/%s" % (k, kk): float(vv) for kk, vv in v.items()})
            elif isinstance(v, (int, float, np.floating, np.integer)):
                rec[k] = float(v)
        self._f.write(json.dumps(rec) + "\n")

    def close(self):
        if self._f is not None:
            self._f.close()
            self._f = None


class _TensorboardWriter:
    def __init__(self, writer):
        self.w = writer

    def write(self, info, step):
        for k, v in info.items():
            if isinstance(v, dict):
                self.w.add_scalars(k, v, step)
            else:
                self.w.add_scalar(k, v, step)

    def close(self):
        self.w.close()


def _make_writer(logger, log_dir):
    """config.logger: 'tensorboard' / 'wandb' (the reference's choices) or 'none'.  tensorboard and wandb
    are optional: without them the scalars go to log_dir/scalars.jsonl."""
    if logger in (None, "none", "None", False):
        return None
    if logger == "tensorboard":
        try:
            from torch.utils.tensorboard import SummaryWriter
            os.makedirs(log_dir, exist_ok=True)
            return _TensorboardWriter(SummaryWriter(log_dir))
        except ImportError:
            pass
    return _JsonlWriter(log_dir)
