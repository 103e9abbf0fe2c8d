"""The kernel form of every stage of one on-policy iteration outside the minibatch update: chosen once by plan_rollout
from a facts record (host logic alone: no tensor, no device), run by the agent's stages, which dispatch on the plan's
fields and test no capability of their own ("Where the rollout's forms are decided")."""
from typing import NamedTuple


class RolloutShape(NamedTuple):
    """The policy shape as FusedActorCritic.rollout_shape reports it (the agent passes None where no FusedActorCritic
    drives the rollout: another representation, no paired hidden layer, raw frames)."""
    thin0: bool       # the first representation layer is K13's (d_in <= 64 -> 256)
    n_rep: int        # representation layers
    d_in: int         # the first layer's input width
    pair256: bool     # both heads' hidden layers are Linear(256, 256) on the head kernels' GEMM form: K40R's shape
    critic256: bool   # the critic is Linear(256, 256) + act -> Linear(256, 1): K40V's shape


class RolloutFacts(NamedTuple):
    """What plan_rollout decides from.  _OnPolicyAgent.plan gathers it."""
    algo: str                 # "ppo" | "a2c"
    # the switches
    fuse_env_step: bool
    fuse_post: bool
    fold_rms: bool
    fuse_value_gae: bool
    value_gemm: bool
    fuse_gather: bool
    fused_rollout: bool
    use_graph: bool
    graph_chunk: int
    rollout_split: bool       # FusedActorCritic.ROLLOUT_SPLIT
    rollout_trunk: bool       # FusedActorCritic.ROLLOUT_TRUNK
    s3_gemms: bool            # ops.S3_GEMMS
    # the agent
    cuda: bool
    use_obsnorm: bool
    raw_obs: bool
    atari: bool
    boot_from_reset: bool
    defer_boot: bool
    raw_defer: bool
    raw_mid_next: bool
    n_slots: int              # deferred truncation slots per env (0 without defer_boot)
    n_steps: int
    obs_dim: int
    world: int
    sync_obs_rms: object      # False | True (a collective per step) | "rollout" (one merge per rollout)
    global_advnorm: bool
    pending: bool             # host closures (buffer.finish_path) wait for the scan
    # the env
    env: str                  # "synthbox" | "synthatari" | "cartpole" | "pendulum" | "acrobot" | "mountaincar" |
                              # "device" (another one) | "host"
    env_fusable: bool         # env.fusable_with_policy_step(dist)
    obs_rows: bool            # env.obs is [N, D] with unit column stride
    # the policy and the learner
    shape: object             # RolloutShape | None
    cnn: bool                 # the learner's explicit CNN forward serves raw frames
    small: object             # K32's shape (d_in, h0, h1, h2, k, LDS floats) of learner.small_policy_layers, or None
    small_bufs: bool          # the rollout buffers are contiguous f32 (K32 writes them by index)
    rows_ok: bool             # the update takes fused_mlp.Rows of the flat observations
    small_update: bool        # learner.small_update_ok (K30)
    epoch_graphs: bool        # learner.graph_updates
    dist: str = "categorical"  # the head's distribution: "categorical" | "gaussian" (K32's instantiation)
    small_close: bool = False  # the switch: a one-launch small-path rollout closes in one launch (K33)


_RMS = {None: (), "standalone": ("xpa_rms_update",), "all-reduce": ("xpa_rms_partials", "xpa_rms_merge"),
        "fold-K8": (), "fold-K14F": ()}
_OBS = {"raw": ("xpa_store_column",), "K5N": ("xpa_obs_normalize",), "trunk": ()}
# cnn: the CNN forward's own launches (fused_cnn's plan) are not listed; policy: the torch module
_TRUNK = {"K40T": ("xpa_s3_gemm_rows_pair_trunk",), "K13-norm": ("xpa_thin_linear_act_fwd_norm",),
          "K13": ("xpa_thin_linear_act_fwd",), "chain": (), "cnn": (), "policy": ()}
_PAIR = {"K40R": ("xpa_s3_gemm_rows_pair",), "linear": (), None: ()}
_HEAD = {"K14F": ("xpa_rollout_step_synthbox",), "K14E": ("xpa_rollout_policy_head_synthbox",),
         "K14": ("xpa_rollout_policy_head",), "K3": ("xpa_rollout_sample",)}
_ENV = {"in-head": (), "synthbox": ("xpa_synthbox_step",), "synthatari": ("xpa_synthatari_step",),
        "cartpole": ("xpa_cartpole_step",), "device": (), "host": ()}
# step_launches' env table: _ENV (whose keys test_rollout_plan_cpu's invariants enumerate over its env kinds) and the
# device envs added since
_ENV_STEP = dict(_ENV, pendulum=("xpa_pendulum_step",), acrobot=("xpa_acrobot_step",),
                 mountaincar=("xpa_mountaincar_step",))


class SmallEnv(NamedTuple):
    """One env / head pair of the one-launch small path (K32, K32W, K32E, the population's batch launch): a row of
    SMALL_ENVS, the only statement of them on the host."""
    d_in: int        # the env's observation width
    k: int           # the head's width
    rollout: str     # K32's single-agent entry point
    eval: str        # K32E's entry point
    code: str        # xpa_small_rollout_batch's env code: the XPA_ENV_* constant's name
    gaussian: bool   # the entry points take (logstd, act_clip) after the block, the batch launch its head arrays


SMALL_ENVS = {   # by (env kind, the head's distribution)
    ("cartpole", "categorical"): SmallEnv(4, 2, "xpa_small_rollout_cartpole", "xpa_small_eval_cartpole",
                                          "XPA_ENV_CARTPOLE", False),
    ("pendulum", "gaussian"): SmallEnv(3, 1, "xpa_small_rollout_pendulum", "xpa_small_eval_pendulum",
                                       "XPA_ENV_PENDULUM", True),
    ("acrobot", "categorical"): SmallEnv(6, 3, "xpa_small_rollout_acrobot", "xpa_small_eval_acrobot",
                                         "XPA_ENV_ACROBOT", False),
    ("mountaincar", "categorical"): SmallEnv(8, 3, "xpa_small_rollout_mountaincar", "xpa_small_eval_mountaincar",
                                             "XPA_ENV_MOUNTAINCAR", False)}
SMALL_BY_ENTRY = {e: row for row in SMALL_ENVS.values() for e in (row.rollout, row.eval)}   # the row of an entry point
_K32 = {key: (row.rollout, row.d_in, row.k) for key, row in SMALL_ENVS.items()}   # a view of the table tests read
K32_DRIVERS = ("K32", "K32W")   # the one-launch rollout's drivers: the same entry points, run the same way
_VALUE_HEAD = {"K13": ("xpa_value_head",), "chain": ("xpa_value_head",), "cnn": (), "policy": ()}
_POST = {"K14F": (), "K8-deferred": ("xpa_rollout_post_deferred_norm",), "K8": ("xpa_rollout_post",)}
_CLOSE = {None: (), "raw-last": ("xpa_rollout_bootstrap_fixup",), "raw-mid-next": ()}
_GAE = {"K40V+compact": ("xpa_s3_gemm_value", "xpa_gae_scan_compact"), "value": ("xpa_gae_scan_value",),
        "compact": ("xpa_gae_scan_compact",), "fixup+scan": ("xpa_rollout_bootstrap_fixup", "xpa_gae_scan"),
        "scan": ("xpa_gae_scan",)}
# close_launches' scan table: _GAE (whose keys test_rollout_plan_cpu's invariants require the planner to emit over its
# own product of switches) and the opt-in form added since
_GAE_CLOSE = dict(_GAE, K33=("xpa_small_close",))
_FEED = {"rows": (), "small": (), "epoch": (), "slot": (), "all-reduce": ("xpa_gather_minibatch",)}


class RolloutPlan(NamedTuple):
    """One iteration's forms.  With driver "K32" / "K32W" the step fields name the multi-kernel step the one launch
    stands for."""
    driver: str        # "K32" | "K32W" (K32 at 128-wide layers) | "graph-chunk" | "graph-step" | "eager" | "host"
    chunk: int         # device env steps per replayed graph, or per K32 launch under use_graph (1: single steps)
    obs: str           # "raw" (store_column) | "K5N" (normalise + column store) | "trunk" (inside the first layer)
    rms: object        # None | "standalone" | "all-reduce" | "fold-K8" | "fold-K14F"
    trunk: str         # "K40T" | "K13-norm" | "K13" | "chain" | "cnn" | "policy"
    value_trunk: str   # the critic-only passes' trunk: "K13" | "chain" | "cnn" | "policy"
    pair: object       # "K40R" | "linear" | None
    head: str          # "K14F" | "K14E" | "K14" | "K3"
    env: str           # "in-head" | "synthbox" | "synthatari" | "cartpole" | "pendulum" | "acrobot" | "mountaincar" |
                       # "device" | "host"
    post: str          # "K14F" | "K8-deferred" | "K8"
    boot: str          # "slots" | "per-step" | "zero"
    mid: object        # A2C's mid-rollout bootstraps: None | "critic" | "next-column" | "slots-from-next"
    close: object      # None | "raw-last" | "raw-mid-next"
    gae: str           # "K40V+compact" | "value" | "compact" | "fixup+scan" | "scan" | "K33" (small_close: the critic
                       # pass, the fixup and the scan in one launch)
    feed: str          # "rows" | "small" | "epoch" | "slot" | "all-reduce"

    def _values(self):
        """One critic-only pass (FusedActorCritic.rollout_value, or the module's)."""
        return _TRUNK[self.value_trunk] + _VALUE_HEAD[self.value_trunk]

    def start_launches(self):
        """The library entry points ahead of a rollout's first step (rollout_refresh: K40R's planes)."""
        return ["xpa_s3_split_batch"] if self.pair == "K40R" else []

    def step_launches(self, pending=False):
        """The library entry points of one steady device env step, in order (hipBLASLt / torch launches are not
        counted).  pending: the step after a reset, which runs the standalone obs_rms update whatever the form."""
        if self.driver in K32_DRIVERS:
            return [row.rollout for (env, _), row in SMALL_ENVS.items() if env == self.env]
        out = list(_RMS["standalone"] if pending and self.rms in ("fold-K8", "fold-K14F") else _RMS[self.rms])
        out += _OBS[self.obs] + _TRUNK[self.trunk]
        if self.trunk != "K40T":
            out += _PAIR[self.pair]
        out += _HEAD[self.head] + _ENV_STEP[self.env]
        if self.post == "K8":
            one = (() if self.obs == "raw" else _OBS["K5N"]) + self._values()
            out += (() if self.boot == "zero" else one) + (one if self.mid == "critic" else ())
        out += ("xpa_rollout_post_deferred_norm_rms",) if (self.post, self.rms) == ("K8-deferred", "fold-K8") \
            else _POST[self.post]
        return out

    def close_launches(self):
        """The library entry points from the end of the last step up to the first update call."""
        out = list(_CLOSE[self.close])
        if self.gae == "K33":   # the deferred rows' critic pass is inside the launch
            return out + list(_GAE_CLOSE[self.gae]) + ["xpa_random_permutation"] + list(_FEED[self.feed])
        if self.gae in ("K40V+compact", "value"):   # (value: + the critic's hidden layer, a library GEMM)
            out += _TRUNK[self.value_trunk]
        elif self.boot == "slots":
            out += self._values()
        out += _GAE_CLOSE[self.gae]
        out.append("xpa_random_permutation")
        return out + list(_FEED[self.feed])


def plan_rollout(f):
    """The RolloutPlan of facts f: the only place a rollout-side switch is read or a capability tested."""
    sh = None if f.raw_obs else f.shape
    device = f.env != "host"
    collective = f.sync_obs_rms is True and f.world > 1 and f.use_obsnorm
    # K32: a CartPole (Categorical, 2 actions), Pendulum (Gaussian, 1 torque), Acrobot or MountainCar (Categorical, 3
    # actions) device env with deferred bootstraps, no per-step collective, the small_policy_layers shape
    k32 = (f.fused_rollout and f.cuda and (f.env, f.dist) in SMALL_ENVS and f.defer_boot and not f.raw_obs and not collective
           and f.algo in ("ppo", "a2c") and f.small is not None and f.small_bufs)
    wide = False
    if k32:
        d_in, h0, h1, h2, k, lds = f.small
        wide = (h0, h1, h2) == (128, 128, 128)   # K32W: the forward's own layout, everything else K32's
        k32 = ((wide or (h0 in (32, 64) and h1 in (32, 64) and h2 in (32, 64)))
               and (d_in, k) == SMALL_ENVS[f.env, f.dist][:2] and d_in == f.obs_dim and 0 < lds <= 16384)
    chunk = max(1, f.graph_chunk) if f.use_graph and device and not collective else 1
    driver = ("host" if not device else ("K32W" if wide else "K32") if k32
              else "eager" if not (f.use_graph and not collective) else "graph-chunk" if chunk > 1 else "graph-step")
    fused = sh is not None and device and f.fuse_env_step and f.env_fusable
    k14f = fused and f.fuse_post and f.defer_boot
    head = "K3" if sh is None else "K14F" if k14f else "K14E" if fused else "K14"
    # the next step's obs_rms.update in the step's last launch: per-rank statistics, deferred bootstraps, D <= 64
    fold = ((f.fold_rms or k14f) and device and f.use_obsnorm and not collective and f.defer_boot and not f.raw_obs
            and f.obs_dim <= 64 and f.obs_rows)
    rms = (None if f.raw_obs or not f.use_obsnorm else ("fold-K14F" if k14f else "fold-K8") if fold
           else "all-reduce" if collective else "standalone")
    pair = None if sh is None else "K40R" if f.rollout_split and f.s3_gemms and sh.pair256 else "linear"
    thin = sh is not None and device and sh.thin0 and f.obs_rows
    module = "cnn" if f.raw_obs and f.cnn else "policy"
    if sh is None:
        trunk = value_trunk = module
    else:
        value_trunk = "K13" if sh.thin0 else "chain"
        k40t = f.rollout_trunk and pair == "K40R" and sh.n_rep == 1 and sh.d_in <= 18
        trunk = value_trunk if not thin else "K40T" if k40t else "K13-norm"
    obs = "raw" if f.raw_obs else "trunk" if thin else "K5N"
    post = "K14F" if k14f else "K8-deferred" if f.defer_boot else "K8"
    boot = "slots" if f.defer_boot else "zero" if f.raw_defer else "per-step"
    mid = None
    if f.boot_from_reset and device:
        mid = ("slots-from-next" if f.defer_boot else None if f.raw_defer else "next-column" if f.raw_mid_next
               else "critic")
    close = "raw-last" if f.raw_defer else "raw-mid-next" if f.raw_mid_next else None
    # the fused scans take one deferred truncation per env, no Atari life-loss handling, nothing pending
    one = f.defer_boot and f.n_slots == 1 and not f.atari and not f.pending
    scan_v = one and f.fuse_value_gae and sh is not None
    if scan_v and f.value_gemm and pair == "K40R" and sh.critic256:
        gae = "K40V+compact"
    elif scan_v and f.n_steps % 4 == 0 and f.n_steps >= 36:   # xpa_gae_scan_value's horizons (ops.gae_value_ok)
        gae = "value"
    else:
        gae = "compact" if one else "fixup+scan" if f.defer_boot else "scan"
    # K33 (opt-in): the closing of a one-launch small-path rollout in one launch, the bootstraps in K32's arithmetic
    if f.small_close and driver in K32_DRIVERS and f.defer_boot and not f.atari and not f.pending and close is None:
        gae = "K33"
    if f.global_advnorm and f.world > 1:
        feed = "all-reduce"
    else:
        feed = ("rows" if sh is not None and f.fuse_gather and f.rows_ok else "small" if f.small_update
                else "epoch" if f.epoch_graphs else "slot")
    return RolloutPlan(driver, chunk, obs, rms, trunk, value_trunk, pair, head, "host" if not device else
                       "in-head" if fused else f.env, post, boot, mid, close, gae, feed)


# ---- evaluation (agent.test) ------------------------------------------------------------------------------------------
class EvalFacts(NamedTuple):
    """What plan_test decides from.  _OnPolicyAgent._eval_facts gathers it for one set of test envs."""
    cuda: bool
    env: str                  # the test envs' kind ("cartpole", ...), "device" (another one) or "host" (no step_device)
    dist: str                 # the head's distribution: "categorical" | "gaussian"
    small: object             # K32's shape (d_in, h0, h1, h2, k, LDS floats at the test envs' count), or None
    n_envs: int               # test_envs.num_envs
    obs_dim: int
    raw_obs: bool
    world: int
    sync_obs_rms: object      # as RolloutFacts.sync_obs_rms
    wide_eval: bool = False   # the switch (config.device_test_wide): 128-wide nets evaluate in one launch (K32WE)


def plan_test(f):
    """The tier agent.test_device evaluates on: "K32E" (whole steps in one launch: xpa_small_eval_*), "K32WE" (the same
    at K32W's widths, xpa_small_eval_wide; opt-in: wide_eval), "steps" (the multi-kernel step, eager, + xpa_eval_post)
    or "host" (the reference's Python loop).  The only place it is decided."""
    if not f.cuda or f.env == "host" or (f.sync_obs_rms is True and f.world > 1):   # the per-step collective
        return "host"
    if (f.env, f.dist) in SMALL_ENVS and not f.raw_obs and 0 < f.n_envs <= 256 and f.small is not None:
        d_in, h0, h1, h2, k, lds = f.small
        if (d_in, k) == SMALL_ENVS[f.env, f.dist][:2] and d_in == f.obs_dim and 0 < lds <= 16384:
            if h0 in (32, 64) and h1 in (32, 64) and h2 in (32, 64):
                return "K32E"
            if f.wide_eval and (h0, h1, h2) == (128, 128, 128):
                return "K32WE"
    return "steps"


EVAL_TIERS = ("K32E", "K32WE")   # the one-launch evaluation's tiers: the same body, run the same way


def eval_entry(f):
    """K32E's entry point for facts that plan "K32E"."""
    return SMALL_ENVS[f.env, f.dist].eval
