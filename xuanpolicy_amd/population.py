"""P classic-control agents trained side by side: one launch per stage for the whole population (DESIGN.md §3,
"Population training").

The one-launch small path (K32 / K32W rollout, K30 update) is one workgroup per agent — ten at most in the split update
— on a chip of 256 CUs.  Population puts "agent" on a grid dimension of those kernels: xpa_small_rollout_batch,
xpa_random_permutation_batch and xpa_small_mlp_update_batch run P members' rollout chunk, epoch permutation and
minibatch update in one launch each, every workgroup reading its own agent's argument block from device memory and
computing exactly what the single-agent launch computes.  So Population.train means `for a in agents: a.train(...)`
bit for bit, and a member stays an ordinary agent before, between and after.

plan_population decides eligibility from a facts record per member (host logic alone: no tensor, no device), in the
style of rollout_plan.plan_rollout; there is no sequential fallback: an ineligible population raises.

Evaluation is the same idea ("Population evaluation (K32EB)"): Population.test_device runs every member's
test episodes through xpa_small_eval_batch — one launch per chunk for all members, each into its own row of one log
tensor, and one read of the P headers — and means `[a.test_device(e, ...) for a, e in zip(agents, test_envs)]` bit for
bit; plan_population_test decides its eligibility, and Population.test falls back to the loop over agent.test."""
import ctypes
from typing import NamedTuple

from .rollout_plan import EVAL_TIERS, K32_DRIVERS, SMALL_BY_ENTRY, SMALL_ENVS, plan_test

MAX_AGENTS = 65535   # the y extent of a launch grid (the update's agent dimension); not a function of the CU count


class MemberFacts(NamedTuple):
    """What plan_population decides from, one record per member.  Population._facts gathers it."""
    driver: str          # the member's RolloutPlan.driver
    feed: str            # the member's RolloutPlan.feed
    entry: str           # the single-agent rollout entry point its plan launches (None without a K32 driver)
    chunk: int           # RolloutPlan.chunk: env steps per rollout launch
    dims: tuple          # (d_in, h0, h1, h2, k) of learner.small_policy_layers (None: another policy shape)
    activation: tuple    # (activation code, slope)
    algo: str            # "ppo" | "a2c"
    n_envs: int
    n_steps: int
    n_epoch: int
    batch_size: int      # minibatch rows
    device: str
    world: int
    t: int               # steps of the current rollout already taken
    scalars: tuple       # ((name, value), ...): the hyper-parameters that are kernel-argument scalars
    tensors: tuple       # data pointers of every tensor the launches write for this member
    gae: str = None      # the member's RolloutPlan.gae: the closing's form ("K33": one batch launch for the population)


class PopulationPlan(NamedTuple):
    n_agents: int
    entry: str           # the single-agent entry point the batch launch stands for
    env: str             # its XPA_ENV_* constant's name
    gaussian: bool       # the head arrays (logstd, act_clip / logstd, g_logstd) are passed
    chunk: int
    close_batch: bool = False   # the closing is one xpa_small_close_batch launch (every member plans gae "K33")


_SHARED = ("gae", "entry", "dims", "activation", "algo", "n_envs", "n_steps", "n_epoch", "batch_size", "device", "chunk",
           "t")


def plan_population(facts):
    """The PopulationPlan of the members' facts, or ValueError naming the first thing that rules the population out.
    The only place eligibility is decided."""
    facts = list(facts)
    if not 1 <= len(facts) <= MAX_AGENTS:
        raise ValueError("a population has 1 .. %d members, not %d" % (MAX_AGENTS, len(facts)))
    for i, f in enumerate(facts):
        if f.world != 1:
            raise ValueError("member %d: world size %d (a population trains in one process: world must be 1)"
                             % (i, f.world))
        if f.driver not in K32_DRIVERS or f.entry not in SMALL_BY_ENTRY:
            raise ValueError("member %d: rollout driver %r is not the one-launch small path %s"
                             % (i, f.driver, "/".join(K32_DRIVERS)))
        if f.feed != "small":
            raise ValueError("member %d: minibatch feed %r is not the one-launch update (\"small\")" % (i, f.feed))
        if f.dims is None:
            raise ValueError("member %d: the policy is not the small-path shape" % i)
    f0 = facts[0]
    for i, f in enumerate(facts[1:], 1):
        for name in _SHARED:
            if getattr(f, name) != getattr(f0, name):
                raise ValueError("member %d differs from member 0 in %s: %r != %r"
                                 % (i, name, getattr(f, name), getattr(f0, name)))
        if f.scalars != f0.scalars:
            d0 = dict(f0.scalars)
            name, v = next((n, v) for n, v in f.scalars if d0.get(n, v) != v or n not in d0)
            raise ValueError("member %d differs from member 0 in %s: %r != %r (a kernel-argument scalar: one value "
                             "per launch)" % (i, name, v, d0.get(name)))
    seen = {}
    for i, f in enumerate(facts):
        for ptr in f.tensors:
            if ptr in seen and seen[ptr] != i:
                raise ValueError("members %d and %d share a tensor (data pointer 0x%x)" % (seen[ptr], i, ptr))
            seen[ptr] = i
    row = SMALL_BY_ENTRY[f0.entry]
    return PopulationPlan(len(facts), f0.entry, row.code, row.gaussian, f0.chunk, f0.gae == "K33")


class EvalMemberFacts(NamedTuple):
    """What plan_population_test decides from, one record per member and its test envs.  Population._test_facts
    gathers it."""
    eval: object             # the member's rollout_plan.EvalFacts for its test envs
    activation: tuple        # (activation code, slope)
    use_obsnorm: bool
    obs_clip: float
    max_episode_steps: int   # the test envs' time limit
    tensors: tuple           # data pointers of the test envs' tensors and the member's obs statistics


class PopulationTestPlan(NamedTuple):
    n_agents: int
    code: str            # the SMALL_ENVS row's XPA_ENV_* constant's name
    gaussian: bool       # the head array (logstd, act_clip) is passed
    wide: bool = False   # every member plans "K32WE": the launch is xpa_small_eval_wide_batch (K32WEB)


# the fields every member shares with member 0: (name in the error text, where it is read)
_TEST_SHARED = (("env", lambda f: f.eval.env), ("dist", lambda f: f.eval.dist), ("small", lambda f: f.eval.small),
                ("n_envs", lambda f: f.eval.n_envs), ("activation", lambda f: f.activation),
                ("use_obsnorm", lambda f: f.use_obsnorm), ("obs_clip", lambda f: f.obs_clip),
                ("max_episode_steps", lambda f: f.max_episode_steps))


def plan_population_test(facts):
    """The PopulationTestPlan of the members' evaluation facts (one K32EB launch serves them all; K32WEB where they all
    plan "K32WE"), or ValueError naming the first thing that rules it out.  The only place the population evaluation's
    eligibility is decided."""
    facts = list(facts)
    if not 1 <= len(facts) <= MAX_AGENTS:
        raise ValueError("a population has 1 .. %d members, not %d" % (MAX_AGENTS, len(facts)))
    for i, f in enumerate(facts):
        if f.eval.world != 1:
            raise ValueError("member %d: world size %d (a population is evaluated in one process: world must be 1)"
                             % (i, f.eval.world))
        tier = plan_test(f.eval)
        if tier not in EVAL_TIERS:
            raise ValueError("member %d: its test envs plan the %r tier, not the one-launch evaluation \"K32E\""
                             % (i, tier))
    f0 = facts[0]
    tier0 = plan_test(f0.eval)
    for i, f in enumerate(facts[1:], 1):
        if plan_test(f.eval) != tier0:
            raise ValueError("member %d: its test envs plan the %r tier, member 0's the %r tier (one launch serves one "
                             "tier)" % (i, plan_test(f.eval), tier0))
    for i, f in enumerate(facts[1:], 1):
        for name, get in _TEST_SHARED:
            if get(f) != get(f0):
                raise ValueError("member %d differs from member 0 in %s: %r != %r" % (i, name, get(f), get(f0)))
    seen = {}
    for i, f in enumerate(facts):
        for ptr in f.tensors:
            if ptr in seen:
                raise ValueError("members %d and %d share a tensor (data pointer 0x%x)" % (seen[ptr], i, ptr))
        seen.update((ptr, i) for ptr in f.tensors)
    row = SMALL_ENVS[f0.eval.env, f0.eval.dist]
    return PopulationTestPlan(len(facts), row.code, row.gaussian, tier0 == "K32WE")


def _block_array(struct, blocks):
    arr = (struct * len(blocks))()
    for i, b in enumerate(blocks):
        ctypes.memmove(ctypes.addressof(arr) + i * ctypes.sizeof(struct), ctypes.addressof(b), ctypes.sizeof(struct))
    return arr


class _DeviceBlocks:
    """Argument-block arrays in device memory, uploaded once per distinct content (outside any capture) and kept
    alive with their host copies for the launches and graphs that hold their addresses."""

    def __init__(self, device):
        self.device, self._cache = device, {}

    def get(self, arr):
        import torch
        raw = bytes(arr)
        ent = self._cache.get(raw)
        if ent is None:
            if len(self._cache) >= 64:   # a caller whose layouts never repeat: do not grow without bound
                self._cache.clear()
            dev = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(self.device)
            ent = self._cache[raw] = (arr, dev)
        return ent


def update_blocks(learners, rows, idxs, scalars, cache):
    """xpa_small_mlp_update_batch's arguments for one minibatch of every learner: (blocks, heads), each a (host array,
    device copy) pair, heads None for Categorical heads.  rows[p] = (obs_flat, act, adv, ret, old_logp, use_advnorm) and
    idxs[p] (int64 row indices) are learner p's, scalars[p] the 8 floats its loss scalars go to; each block is the
    learner's own (learner._small_args), cache a _DeviceBlocks."""
    from . import _lib
    blocks, heads = [], []
    for p, L in enumerate(learners):
        obs_flat, act, adv, ret, old_logp, use_advnorm = rows[p]
        blocks.append(L._small_args(obs_flat, idxs[p], act, adv, ret, old_logp, use_advnorm, scalars=scalars[p])[0])
        logstd = L._fused_mlp().logstd
        if logstd is not None:
            heads.append(_lib.XpaSmallMlpGauss(logstd.data_ptr(), logstd.grad.data_ptr()))
    if heads and len(heads) != len(blocks):
        raise ValueError("Categorical and Gaussian heads in one batch update")
    return (cache.get(_block_array(_lib.XpaSmallMlpArgs, blocks)),
            cache.get(_block_array(_lib.XpaSmallMlpGauss, heads)) if heads else None)


def small_update_batch(learners, rows, idxs, scalars, cache=None):
    """learner.small_update (one eager K30 update and the host bookkeeping of the step) for every learner, the device
    part as one batch launch.  Arguments as update_blocks'; returns scalars."""
    from . import small_path
    device = scalars.device
    for L in learners:
        if not L.fused_opt.sched_enabled:
            L.fused_opt.enable_sched()   # the blocks hold the schedule's and the cursor's addresses
    slot = update_blocks(learners, rows, idxs, scalars, _DeviceBlocks(device) if cache is None else cache)
    for L in learners:
        L.fused_opt.ensure_window(L.scheduler)
        L.iterations += 1
    small_path.update_batch(len(learners), *slot, device)
    for L in learners:
        L._host_steps(1)
    return scalars


class Population:
    """Population(agents): P PPOCLIP_Agent / A2C_Agent members of one shape (plan_population) trained in lockstep.

    train(train_steps, log) is `for a in agents: a.train(train_steps, log)` for every member's parameters, Adam state,
    schedule cursor, statistics, env state, buffers and host counters; the members' own `timers` are not advanced (the
    population's `timers` are).  The schedule cursor agrees for members that have taken all their updates in the same
    way (alone or in this population); after a mix of the two the table may be refilled at another update, which
    changes the cursor's value and nothing a launch computes."""

    def __init__(self, agents):
        from .agents import _OnPolicyAgent
        self.agents = list(agents)
        for i, a in enumerate(self.agents):
            if not isinstance(a, _OnPolicyAgent):
                raise ValueError("member %d: a population's members are PPOCLIP_Agent / A2C_Agent objects, not %s"
                                 % (i, type(a).__name__))
        self.timers = {"rollout": 0.0, "update": 0.0}
        self.phase_events = None   # a list: ("rollout_end" | "close_end" | "update_end", event) per iteration
        self._plan = self._plan_key = None
        self.plan()
        a0 = self.agents[0]
        self.device = a0.device
        self._blocks = _DeviceBlocks(self.device)
        self._eval_blocks = _DeviceBlocks(self.device)   # test_device's arrays (they change with every set of test envs)
        self._perm = self._perm_keys = self._perm_host = None   # [P, n] permutations; (seeds, counters) on the device
        self._epochs = {}          # epoch key -> ["warm" | graph, per-slot launch arguments, their loss scalars]
        self._graph_pool = None
        self._graph_failed = False

    # ---- eligibility --------------------------------------------------------------------------------------------
    @staticmethod
    def _facts(a):
        plan, L, env, mem = a.plan(), a.learner, a.envs, a.memory
        policy = L.small_policy_layers()
        k32 = plan.driver in K32_DRIVERS
        dims, act = (policy.dims, (int(policy.code), float(policy.slope))) if policy else (None, None)
        tensors = ()
        if k32 and plan.feed == "small":
            fused = L.fused_opt
            ts = [fused.fs.param, fused.fs.flat, fused.exp_avg, fused.exp_avg_sq, mem.observations, mem.actions,
                  mem.values, mem.rewards, mem.terminals, mem.closed, mem.boot, env.state, env.obs, env.act_in,
                  a.obs_mean, a.obs_var, a.obs_count, a.ret_mean, a.ret_var, a.ret_count, a.returns, a.cursor,
                  a.obs_norm, a._boot_pair, a.slot_t, mem._advantages, mem._returns]
            tensors = tuple(int(t.data_ptr()) for t in ts)
        g = L.optimizer.param_groups[0]
        scalars = (("use_obsnorm", a.use_obsnorm), ("use_rewnorm", a.use_rewnorm), ("obs_clip", float(a._obs_clip())),
                   ("rewnorm_range", float(a.rewnorm_range)), ("gamma", float(a.gamma)), ("n_slots", int(a.n_slots)),
                   ("max_episode_steps", int(getattr(env, "max_episode_steps", 0) or 0)),
                   ("boot_from_reset", bool(a.boot_from_reset)), ("use_advnorm", bool(mem.use_advnorm)),
                   ("clip_range", float(getattr(L, "clip_range", 0.0) or 0.0)), ("vf_coef", float(L.vf_coef)),
                   ("ent_coef", float(L.ent_coef)),
                   ("max_norm", float(L._max_norm) if L._use_clip else -1.0), ("betas", tuple(map(float, g["betas"]))),
                   ("eps", float(g["eps"])), ("small_split", bool(L.small_split)),
                   ("graph_updates", bool(L.graph_updates)))
        if plan.gae == "K33":   # K33's scalars: one value per batch launch
            scalars += (("gae_lam", float(mem.gae_lam)), ("use_gae", bool(mem.use_gae)))
        entry = plan.step_launches()[0] if k32 else None
        return MemberFacts(plan.driver, plan.feed, entry, plan.chunk, dims, act, a.algo, a.n_envs, a.n_steps, a.n_epoch,
                           a.batch_size, str(a.device), a.world, a._t, scalars, tensors, plan.gae)

    def plan(self):
        """The PopulationPlan of the members as they stand (cached under the members' own plans and positions)."""
        for a in self.agents:
            a.plan()   # refreshes the member's own plan, its key and its K32 block when what they rest on changed
        key = tuple((id(a), a._plan_key) for a in self.agents)
        if key != self._plan_key or any(a._t != self.agents[0]._t for a in self.agents):
            self._plan = plan_population([self._facts(a) for a in self.agents])
            self._plan_key = key
        return self._plan

    # ---- the batch launches ---------------------------------------------------------------------------------------
    def _rollout_launch(self, plan, steps):
        """`steps` env steps of every member in one launch (xpa_small_rollout_batch) over the members' own blocks."""
        from . import _lib, small_path
        for a in self.agents:
            a._k32.steps = int(steps)
        blocks = self._blocks.get(_block_array(_lib.XpaSmallRolloutArgs, [a._k32 for a in self.agents]))
        heads = plan.gaussian and self._blocks.get(_block_array(_lib.XpaSmallRolloutHead,
                                                                [a._k32_head for a in self.agents]))
        small_path.rollout_batch(plan.env, len(self.agents), blocks, heads, self.device)

    def _close_launch(self):
        """Every member's closing (agent._close_rollout's "K33" form) in one launch (xpa_small_close_batch) over the
        members' own blocks, then the host state each member's own launch leaves."""
        from . import _lib, small_path
        host, dev = self._blocks.get(_block_array(_lib.XpaSmallCloseArgs, [a._small_close_block() for a in self.agents]))
        small_path.small_close_batch(len(self.agents), host, dev, self.device)
        for a in self.agents:
            a._closed_small()

    def _permutations(self, n):
        """Row p: member p's next epoch permutation (agent.epoch_permutation), all in one launch."""
        import numpy as np
        import torch
        from . import ops
        P = len(self.agents)
        if self._perm is None or self._perm.shape[1] != n:
            self._perm = torch.empty((P, n), dtype=torch.int64, device=self.device)
        want = [(int(a.seed) & 0xFFFFFFFF, int(a._perm_counter) & 0xFFFFFFFF) for a in self.agents]
        if self._perm_host != want:
            # (seed, counter) per member on the device; the counters then advance there, one add per epoch, and are
            # uploaded again only when a member's own counter moved some other way (it trained alone in between)
            keys = np.asarray(want, dtype=np.uint32).T.copy().view(np.int32)
            self._perm_keys = torch.from_numpy(keys).to(self.device)
        ops.random_permutation_batch(n, self._perm_keys[0], self._perm_keys[1], out=self._perm)
        self._perm_keys[1].add_(1)
        for a in self.agents:
            a._perm_counter += 1
        self._perm_host = [(s, (c + 1) & 0xFFFFFFFF) for s, c in want]
        return self._perm

    def _epoch_args(self, rows, perm, NT, B):
        """The launch arguments of one epoch's minibatch slots (the blocks built by the members' own learners) and
        the [P, slots, 8] tensor their loss scalars go to."""
        import torch
        starts = list(range(0, NT, B))
        scalars = torch.zeros((len(self.agents), len(starts), 8), dtype=torch.float32, device=self.device)
        learners = [a.learner for a in self.agents]
        return [update_blocks(learners, rows, [perm[p, s:s + B] for p in range(len(learners))], scalars[:, j],
                              self._blocks) for j, s in enumerate(starts)], scalars

    def _epoch_key(self, rows, NT, B):
        """What an epoch's launches (and their captured graph) bake in besides the permutation buffer: every member's
        learners.small_epoch key.  Formed once per update phase: nothing of it can change between two epochs."""
        from .learners import _ptr
        return (NT, B) + tuple(
            (_ptr(r[0]), tuple(r[0].shape), _ptr(r[1]), _ptr(r[2]), _ptr(r[3]), _ptr(r[4]), bool(r[5]),
             float(a.learner.clip_range), float(a.learner.vf_coef), float(a.learner.ent_coef),
             bool(a.learner.small_split)) + a.learner._step_key() for r, a in zip(rows, self.agents))

    def _epoch(self, rows, perm, NT, B, key):
        """One epoch of minibatch updates for every member: learners.small_epoch's legs over the batch launches —
        eager the first time a layout is seen, then captured once as one linear graph and replayed.  Returns the
        [P, slots, 8] loss scalars of the epoch's updates."""
        from . import graphs, small_path
        learners = [a.learner for a in self.agents]
        n_slots = -(-NT // B)
        key = (perm.data_ptr(),) + key
        for L in learners:
            if not L.fused_opt.sched_enabled:
                L.fused_opt.enable_sched()
        cache = self._epochs
        ent = cache.get(key)
        W = learners[0].fused_opt.SCHED_WINDOW
        graphed = (all(L.graph_updates for L in learners) and not self._graph_failed and n_slots <= W
                   and (ent is not None or len(cache) < learners[0].graph_max_slots))
        if ent is None or not graphed:
            slots, scalars = self._epoch_args(rows, perm, NT, B) if ent is None else ent[1:]
            for slot in slots:
                for L in learners:
                    L.fused_opt.ensure_window(L.scheduler)
                    L.iterations += 1
                small_path.update_batch(len(learners), *slot, self.device)
                for L in learners:
                    L._host_steps(1)
            if graphed:
                cache[key] = ["warm", slots, scalars]
            return scalars
        for L in learners:
            L.fused_opt.ensure_window(L.scheduler, need=n_slots)
        if ent[0] == "warm":
            import torch
            if self._graph_pool is None:
                self._graph_pool = torch.cuda.graph_pool_handle()
            try:
                ent[0], _ = graphs.capture(
                    lambda: [small_path.update_batch(len(learners), *s, self.device) for s in ent[1]], self._graph_pool)
            except Exception:
                torch.cuda.synchronize()   # nothing of an aborted capture ran: stay eager from here on
                self._graph_failed = True
                del cache[key]
                return self._epoch(rows, perm, NT, B, key[1:])
        ent[0].replay()
        for L in learners:
            L.iterations += n_slots
            L._host_steps(n_slots)
        return ent[2]

    def _update_phase(self):
        """agent._update_phase for every member: each closes its own rollout (bootstrap critic pass + GAE, the code it
        runs alone) or, where every member plans the "K33" closing, one batch launch closes them all; then per epoch
        one permutation launch and the minibatch slots' batch launches."""
        import torch
        agents = self.agents
        if self._plan.close_batch:   # train()'s plan of this iteration
            self._close_launch()
        else:
            for a in agents:
                a._close_rollout()
        if self.phase_events is not None:
            self.phase_events.append(("close_end", torch.cuda.Event(enable_timing=True)))
            self.phase_events[-1][1].record()
        a0 = agents[0]
        NT, B = a0.buffer_size, a0.batch_size
        rows = [a._flat_rows() + (a.memory.use_advnorm,) for a in agents]
        n_slots = -(-NT // B)
        key = self._epoch_key(rows, NT, B)
        for _ in range(a0.n_epoch):
            perm = self._permutations(NT)
            scalars = self._epoch(rows, perm, NT, B, key)
            for p, a in enumerate(agents):
                if a.update_log is not None:
                    a.update_log.extend(scalars[p, j].clone() for j in range(n_slots))
        for p, a in enumerate(agents):
            a._end_update(scalars[p, n_slots - 1])

    # ---- evaluation ("Population evaluation (K32EB)") ------------------------------------------------
    @staticmethod
    def _test_facts(a, env):
        f = a._eval_facts(env)
        policy = a.learner.small_policy_layers()
        tensors = ()
        if plan_test(f) in EVAL_TIERS:
            ts = [env.state, env.obs, env.act_in, env.final_obs, env.rew, env.term, env.trunc, env.ep_step, env.ep_index,
                  env.ep_score, env.ep_last_score, env.ep_last_len, a.obs_mean, a.obs_var, a.obs_count]
            tensors = tuple(int(t.data_ptr()) for t in ts)
        return EvalMemberFacts(f, (int(policy.code), float(policy.slope)) if policy else None, bool(a.use_obsnorm),
                               float(a._obs_clip()), int(getattr(env, "max_episode_steps", 0) or 0), tensors)

    def plan_test(self, test_envs):
        """The PopulationTestPlan of the members over test_envs (one set of test envs per member), or ValueError."""
        envs = list(test_envs)
        if len(envs) != len(self.agents):
            raise ValueError("test_envs: one set of test envs per member (%d members, %d sets)"
                             % (len(self.agents), len(envs)))
        return plan_population_test([self._test_facts(a, e) for a, e in zip(self.agents, envs)])

    def test_device(self, test_envs, test_episode, chunk=None, rngs=None, batch_reset=False):
        """[a.test_device(e, test_episode, chunk, rng) for a, e, rng in zip(agents, test_envs, rngs)] with every
        member's steps in ONE launch per chunk (xpa_small_eval_batch; xpa_small_eval_wide_batch for members that plan
        "K32WE") and one read of the P log headers after it:
        each member's returned scores, last_test_log, obs statistics, test-env state and evaluation cursor are its own
        call's, and nothing else of a member changes.  test_envs: one set of device envs per member; rngs: None or one
        (seed, step) per member.  A member whose log is complete sits out the later launches (its workgroup returns at
        once).  batch_reset: the members' env.reset() calls are one xpa_small_env_reset_batch launch over the
        evaluation's own blocks plus each env's host half (reset_host), leaving every env as reset() does.  One stream,
        no graph capture; an ineligible population raises ValueError (plan_population_test): there is no sequential
        fallback in here."""
        import torch
        from . import _lib, ops, small_path
        agents, envs = self.agents, list(test_envs)
        P = len(agents)
        rngs = [None] * P if rngs is None else list(rngs)
        if len(rngs) != P:
            raise ValueError("rngs: None or one (seed, step) per member (%d members, %d given)" % (P, len(rngs)))
        plan = self.plan_test(envs)
        N, target = int(envs[0].num_envs), int(test_episode)
        max_ep = int(getattr(envs[0], "max_episode_steps", 0) or 0)
        if target < 1 or max_ep < 1:
            raise ValueError("test_device: test_episode >= 1 and time-limited test envs (max_episode_steps)")
        chunk = 128 if chunk is None else int(chunk)
        if chunk < 1:
            raise ValueError("test_device: chunk >= 1")
        dev = self.device
        snap_dim = agents[0]._eval_scalars(envs[0])[0]   # one value: use_obsnorm and the observation width are shared
        capacity = target + N
        logs = ops.eval_logs_new([target] * P, N, snap_dim, dev)
        scratch = torch.empty((P, 3 * N), dtype=torch.float32, device=dev)
        blocks, heads, evals, cursors = [], [], [], []
        for p, (a, env, rng) in enumerate(zip(agents, envs, rngs)):
            if not batch_reset:
                env.reset()
            seed, cursor = a._eval_stream(rng)
            args, logstd = a._build_small_eval(env, seed, cursor)
            args.steps = chunk
            blocks.append(args)
            cursors.append(cursor)   # an rng's cursor is this call's alone: alive until the last launch has run
            if plan.gaussian:
                heads.append(_lib.XpaSmallRolloutHead(logstd.data_ptr(), float(a._eval_scalars(env)[1])))
            evals.append(_lib.XpaSmallEval(logs[p].data_ptr(), scratch[p].data_ptr(), capacity, snap_dim))
        cache = self._eval_blocks
        arrays = (cache.get(_block_array(_lib.XpaSmallRolloutArgs, blocks)),
                  plan.gaussian and cache.get(_block_array(_lib.XpaSmallRolloutHead, heads)),
                  cache.get(_block_array(_lib.XpaSmallEval, evals)))
        if batch_reset:
            small_path.env_reset_batch(plan.code, P, arrays[0], dev)
            for env in envs:
                env.reset_host()
        launch = small_path.small_eval_wide_batch if plan.wide else small_path.small_eval_batch
        bound = (target // N + 2) * max_ep
        issued = 0
        while True:
            launch(plan.code, P, *arrays, dev)
            issued += chunk
            head = ops.eval_log_headers(logs)   # [P, 8]: count, target, done, steps_run, overflow
            for p in range(P):
                if head[p, 4]:
                    raise _lib.XpaError("test_device: member %d: the episode log overflowed (%d entries, capacity %d)"
                                        % (p, head[p, 0], capacity))
            if head[:, 2].all():
                break
            if issued >= bound:
                p = int((head[:, 2] == 0).argmax())
                raise RuntimeError("test_device: member %d: %d of %d episodes ended in %d steps (bound %d = "
                                   "(test_episode // N + 2) * max_episode_steps)"
                                   % (p, head[p, 0], target, head[p, 3], bound))
        words = logs.cpu().numpy()
        del cursors
        scores = []
        for p, a in enumerate(agents):
            a.last_test_log = ops.eval_log_decode(words[p])
            scores.append([float(s) for s in a.last_test_log["score"]])
        return scores

    def test(self, env_fn, test_episode):
        """[a.test(env_fn, test_episode) for a in agents]: one env_fn() call per member, in member order.  Where every
        member's config has device_test and plan_population_test admits the members over their test envs, the
        evaluation is test_device's batch launches, followed by each member's own printing, log_infos and
        test_envs.close() (agent._finish_test); otherwise it is that loop itself.  128-wide members take the batch
        launches where every member's config has device_test_wide (a member's own flag decides its tier, so a
        population that mixes them is not admitted and loops); where every member's config has device_test_batch_reset
        the batch path resets the members' test envs in one launch (test_device's batch_reset)."""
        from .agents import _cfg
        agents = self.agents
        if not all(bool(_cfg(a.config, "device_test", False)) for a in agents):
            return [a.test(env_fn, test_episode) for a in agents]
        envs = [env_fn() for _ in agents]
        try:
            self.plan_test(envs)
        except ValueError:
            return [a.test(lambda e=e: e, test_episode) for a, e in zip(agents, envs)]
        batch_reset = all(bool(_cfg(a.config, "device_test_batch_reset", False)) for a in agents)
        scores = self.test_device(envs, test_episode, batch_reset=batch_reset)
        return [a._finish_test(e, s) for a, e, s in zip(agents, envs, scores)]

    # ---- public API -------------------------------------------------------------------------------------------------
    def train(self, train_steps, log=True):
        """agent.train(train_steps, log) for every member, in lockstep (see the class docstring)."""
        import time
        import torch
        agents = self.agents
        a0 = agents[0]
        left = train_steps
        while left > 0:
            plan = self.plan()
            chunk, t = plan.chunk, a0._t
            t0 = time.perf_counter()
            if t == 0:
                for a in agents:
                    a._begin_rollout()
            k = chunk if chunk > 1 and left >= chunk and t % chunk == 0 and a0.n_steps - t >= chunk else 1
            self._rollout_launch(plan, k)
            left -= k
            for a in agents:
                a._advance(k)
            t1 = time.perf_counter()
            self.timers["rollout"] += t1 - t0
            if a0._t == a0.n_steps:
                if self.phase_events is not None:
                    self.phase_events.append(("rollout_end", torch.cuda.Event(enable_timing=True)))
                    self.phase_events[-1][1].record()
                self._update_phase()
                if self.phase_events is not None:
                    self.phase_events.append(("update_end", torch.cuda.Event(enable_timing=True)))
                    self.phase_events[-1][1].record()
                for a in agents:
                    a._end_iteration(log)
                self.timers["update"] += time.perf_counter() - t1
