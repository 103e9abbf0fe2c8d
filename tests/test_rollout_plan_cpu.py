"""The rollout's planner on the host alone: plan_rollout is a pure function of RolloutFacts, so every form of an
iteration outside the minibatch update is decided (and checked) without a device.

The expected plans of the named cases are written out from the predicates the planner replaced (_rms_fold_ok, _k14f_on,
_env_fused, _small_rollout, rollout_refresh / _rollout_pair / _rollout_trunk_pair / rollout_value_split and
_update_phase's conditions), not from the planner's output."""
import itertools

import pytest
import torch

from oracle import cpu_ref
from xuanpolicy_amd import rollout_plan as rp
from xuanpolicy_amd.rollout_plan import RolloutFacts, RolloutPlan, RolloutShape, plan_rollout

# C2: PPO over SynthBox(17, 6), hidden 256, 4096 envs x 128 steps, every switch at its default
C2 = RolloutFacts(
    algo="ppo", fuse_env_step=True, fuse_post=True, fold_rms=False, fuse_value_gae=True, value_gemm=False,
    fuse_gather=True, fused_rollout=True, use_graph=True, graph_chunk=128, rollout_split=True, rollout_trunk=False,
    s3_gemms=True, cuda=True, use_obsnorm=True, raw_obs=False, atari=False, boot_from_reset=False, defer_boot=True,
    raw_defer=False, raw_mid_next=False, n_slots=1, n_steps=128, obs_dim=17, world=1, sync_obs_rms=False,
    global_advnorm=False, pending=False, env="synthbox", env_fusable=True, obs_rows=True,
    shape=RolloutShape(thin0=True, n_rep=1, d_in=17, pair256=True, critic256=True), cnn=False, small=None,
    small_bufs=True, rows_ok=True, small_update=False, epoch_graphs=True)
C2_PLAN = RolloutPlan(driver="graph-chunk", chunk=128, obs="trunk", rms="fold-K14F", trunk="K13-norm", value_trunk="K13",
                      pair="K40R", head="K14F", env="in-head", post="K14F", boot="slots", mid=None, close=None,
                      gae="value", feed="rows")
# the step with the env outside K14 (categorical actions, fuse_env_step off): K14, the env's own step, K8 deferred
SEPARATE = dict(head="K14", env="synthbox", post="K8-deferred", rms="standalone")

CATEGORICAL = C2._replace(env_fusable=False, small=(17, 256, 256, 256, 6, 1 << 20))
A2C = C2._replace(algo="a2c", boot_from_reset=True, use_obsnorm=False)
WIDE = C2._replace(obs_dim=376, env_fusable=False, shape=RolloutShape(False, 1, 376, True, True))
# C1: PPO over CartPole, hidden 64 (no paired 256 layer: no FusedActorCritic drives the rollout), K30 updates
CARTPOLE = C2._replace(env="cartpole", env_fusable=False, obs_dim=4, shape=None, small=(4, 64, 64, 64, 2, 2500),
                       rows_ok=False, small_update=True)
CARTPOLE_PLAN = C2_PLAN._replace(driver="K32", obs="K5N", rms="standalone", trunk="policy", value_trunk="policy",
                                 pair=None, head="K3", env="cartpole", post="K8-deferred", gae="compact", feed="small")
# C3: A2C over SynthAtari frames (uint8, the CNN policy), truncations always terminal
ATARI = C2._replace(algo="a2c", use_obsnorm=False, raw_obs=True, atari=True, boot_from_reset=True, defer_boot=False,
                    raw_defer=True, n_slots=0, obs_dim=4 * 84 * 84, env="synthatari", env_fusable=False, obs_rows=False,
                    shape=None, cnn=True, rows_ok=False)
ATARI_PLAN = RolloutPlan(driver="graph-chunk", chunk=128, obs="raw", rms=None, trunk="cnn", value_trunk="cnn", pair=None,
                         head="K3", env="synthatari", post="K8", boot="zero", mid=None, close="raw-last", gae="scan",
                         feed="epoch")
# a host VecEnv with C2's policy: per-step copies, per-step bootstraps
HOST = C2._replace(env="host", env_fusable=False, obs_rows=False, defer_boot=False, n_slots=0)
HOST_PLAN = C2_PLAN._replace(driver="host", chunk=1, obs="K5N", rms="standalone", trunk="K13", head="K14", env="host",
                             post="K8", boot="per-step", gae="scan")

CASES = {
    "c2_default": (C2, C2_PLAN),
    "c2_categorical": (CATEGORICAL, C2_PLAN._replace(**SEPARATE)),
    "fuse_post_off": (C2._replace(fuse_post=False),
                      C2_PLAN._replace(head="K14E", post="K8-deferred", rms="standalone")),
    "fuse_post_off_fold_rms": (C2._replace(fuse_post=False, fold_rms=True),
                               C2_PLAN._replace(head="K14E", post="K8-deferred", rms="fold-K8")),
    "fuse_env_step_off": (C2._replace(fuse_env_step=False), C2_PLAN._replace(**SEPARATE)),
    "value_gemm_off": (C2._replace(value_gemm=False), C2_PLAN),
    "value_gemm_on": (C2._replace(value_gemm=True), C2_PLAN._replace(gae="K40V+compact")),
    "fuse_value_gae_off": (C2._replace(fuse_value_gae=False), C2_PLAN._replace(gae="compact")),
    "short_horizon": (C2._replace(n_steps=16, graph_chunk=16), C2_PLAN._replace(chunk=16, gae="compact")),
    "four_slots": (C2._replace(n_slots=4), C2_PLAN._replace(gae="fixup+scan")),
    "rollout_split_off": (C2._replace(rollout_split=False, value_gemm=True), C2_PLAN._replace(pair="linear")),
    "rollout_trunk_on": (C2._replace(rollout_trunk=True), C2_PLAN._replace(trunk="K40T")),
    "a2c_synthbox": (A2C, C2_PLAN._replace(rms=None, mid="slots-from-next")),
    "cartpole_k32": (CARTPOLE, CARTPOLE_PLAN),
    "cartpole_fused_rollout_off": (CARTPOLE._replace(fused_rollout=False), CARTPOLE_PLAN._replace(driver="graph-chunk")),
    "wide_trunk_376_17": (WIDE, C2_PLAN._replace(obs="K5N", trunk="chain", value_trunk="chain", **SEPARATE)),
    "atari_a2c_trunc_terminal": (ATARI, ATARI_PLAN),
    "atari_a2c_mid_next": (ATARI._replace(raw_defer=False, raw_mid_next=True),
                           ATARI_PLAN._replace(boot="per-step", mid="next-column", close="raw-mid-next")),
    "host_ppo": (HOST, HOST_PLAN),
    "host_a2c": (HOST._replace(algo="a2c", boot_from_reset=True, use_obsnorm=False), HOST_PLAN._replace(rms=None)),
    # the per-step collective runs outside a captured graph; K14F keeps the post step, not the statistics
    "sync_obs_rms_world2": (C2._replace(world=2, sync_obs_rms=True, use_graph=False),
                            C2_PLAN._replace(driver="eager", chunk=1, rms="all-reduce")),
    "sync_obs_rms_rollout_world2": (C2._replace(world=2, sync_obs_rms="rollout"), C2_PLAN),
    "global_advnorm": (C2._replace(world=2, global_advnorm=True), C2_PLAN._replace(feed="all-reduce")),
    "pending_host_closures": (C2._replace(pending=True), C2_PLAN._replace(gae="fixup+scan")),
}


@pytest.mark.parametrize("name", list(CASES))
def test_named_facts_give_the_expected_plan(name):
    facts, want = CASES[name]
    assert plan_rollout(facts) == want


SWITCHES = ("fuse_env_step", "fuse_post", "fold_rms", "fuse_value_gae", "value_gemm", "fuse_gather", "fused_rollout",
            "use_graph", "rollout_split", "rollout_trunk", "s3_gemms")
KINDS = (C2, CATEGORICAL, A2C, WIDE, C2._replace(n_slots=4), CARTPOLE, CARTPOLE._replace(algo="a2c", boot_from_reset=True),
         ATARI, ATARI._replace(raw_defer=False, raw_mid_next=True), HOST, HOST._replace(algo="a2c", boot_from_reset=True),
         C2._replace(obs_dim=72, shape=RolloutShape(False, 1, 72, True, True)),    # env fusable by its own word, D > 64
         C2._replace(shape=RolloutShape(True, 2, 17, True, False)),               # a deeper trunk, another critic
         C2._replace(global_advnorm=True), CARTPOLE._replace(small_update=False, epoch_graphs=False))


def _product():
    for kind in KINDS:
        for vals in itertools.product((False, True), repeat=len(SWITCHES)):
            f = kind._replace(**dict(zip(SWITCHES, vals)))
            for sync, pending in itertools.product((False, True, "rollout"), (False, True)):
                yield f._replace(world=2 if sync or f.global_advnorm else 1, sync_obs_rms=sync, pending=pending)


def test_invariants_over_every_switch_and_env_kind():
    tables = {"rms": rp._RMS, "obs": rp._OBS, "trunk": rp._TRUNK, "value_trunk": rp._VALUE_HEAD, "pair": rp._PAIR,
              "head": rp._HEAD, "env": rp._ENV, "post": rp._POST, "close": rp._CLOSE, "gae": rp._GAE, "feed": rp._FEED}
    seen = set()
    for f in _product():
        p = plan_rollout(f)
        seen.add(p)
        collective = f.sync_obs_rms is True and f.world > 1 and f.use_obsnorm
        if p.head == "K14F":
            assert f.env_fusable and p.env == "in-head" and p.boot == "slots" and p.post == "K14F"
        assert (p.post == "K14F") == (p.head == "K14F")
        assert (p.env == "in-head") == (p.head in ("K14E", "K14F"))
        if p.rms in ("fold-K8", "fold-K14F"):
            assert f.use_obsnorm and not collective and f.obs_dim <= 64 and f.defer_boot and p.boot == "slots"
            assert (p.rms == "fold-K14F") == (p.head == "K14F")
        assert (p.rms == "all-reduce") == (collective and not f.raw_obs)
        if p.gae in ("K40V+compact", "value", "compact"):
            assert f.n_slots == 1 and not f.atari and not f.pending
        if p.gae == "K40V+compact":
            assert p.pair == "K40R" and f.value_gemm and f.shape.critic256
        if p.driver == "K32":
            assert f.env == "cartpole" and f.defer_boot and f.obs_dim == 4 and not collective and f.fused_rollout
        if p.trunk == "K40T":
            assert p.pair == "K40R" and p.obs == "trunk" and f.shape.d_in <= 18
        assert (p.obs == "trunk") == (p.trunk in ("K40T", "K13-norm"))
        assert (p.driver == "host") == (f.env == "host") == (p.env == "host")
        assert p.chunk == 1 or (f.use_graph and p.driver in ("graph-chunk", "K32"))
        assert (p.pair is None) == (p.head == "K3")
        # every form is a key of the launch tables, and the lists build
        for field, table in tables.items():
            assert getattr(p, field) in table, (field, getattr(p, field))
        assert isinstance(p.start_launches() + p.step_launches() + p.step_launches(pending=True) + p.close_launches(),
                          list)
    assert len(seen) > 60   # the product reaches the forms, it does not collapse onto a few plans
    for field, table in tables.items():   # and every form of the tables is one the planner emits
        emitted = {getattr(p, field) for p in seen}
        assert emitted == set(table) - ({"device"} if field == "env" else set()), (field, emitted)


def test_launch_lists_of_the_named_plans():
    """The tables spelled out for the two ends: C2's three-launch step, and the five-launch step it replaced."""
    assert C2_PLAN.start_launches() == ["xpa_s3_split_batch"]
    assert C2_PLAN.step_launches() == ["xpa_thin_linear_act_fwd_norm", "xpa_s3_gemm_rows_pair",
                                       "xpa_rollout_step_synthbox"]
    assert C2_PLAN.step_launches(pending=True) == ["xpa_rms_update"] + C2_PLAN.step_launches()
    assert C2_PLAN.close_launches() == ["xpa_thin_linear_act_fwd", "xpa_gae_scan_value", "xpa_random_permutation"]
    sep = C2_PLAN._replace(**SEPARATE)
    assert sep.step_launches() == ["xpa_rms_update", "xpa_thin_linear_act_fwd_norm", "xpa_s3_gemm_rows_pair",
                                   "xpa_rollout_policy_head", "xpa_synthbox_step", "xpa_rollout_post_deferred_norm"]
    assert sep.step_launches(pending=True) == sep.step_launches()
    assert CARTPOLE_PLAN.step_launches() == ["xpa_small_rollout_cartpole"]
    assert HOST_PLAN.step_launches() == ["xpa_rms_update", "xpa_obs_normalize", "xpa_thin_linear_act_fwd",
                                         "xpa_s3_gemm_rows_pair", "xpa_rollout_policy_head", "xpa_obs_normalize",
                                         "xpa_thin_linear_act_fwd", "xpa_value_head", "xpa_rollout_post"]
    assert ATARI_PLAN.close_launches() == ["xpa_rollout_bootstrap_fixup", "xpa_gae_scan", "xpa_random_permutation"]


def test_a_stage_handed_an_unknown_form_raises():
    """RuntimeError from the stage itself (a raise, not an assert), before it touches a buffer."""
    from xuanpolicy_amd.agents import PPOCLIP_Agent
    from xuanpolicy_amd.fused_mlp import FusedActorCritic
    fm = FusedActorCritic(cpu_ref.build_actor_critic_ref(17, 6, [256], [256], [256]))
    x = torch.zeros(8, 17)
    with pytest.raises(RuntimeError, match="no form"):
        fm._rep_forward(x, "K99")
    with pytest.raises(RuntimeError, match="no form"):
        fm.rollout_value(x, trunk="K99")
    with pytest.raises(RuntimeError, match="no form"):
        fm._rollout_pair(torch.zeros(8, 256), "K99")
    with pytest.raises(RuntimeError, match="K40R's planes"):   # planned on planes no refresh made
        fm._rollout_pair(torch.zeros(8, 256), "K40R")
    agent = object.__new__(PPOCLIP_Agent)   # the stages check the form before they read any state
    with pytest.raises(RuntimeError, match="no form"):
        agent._post(C2_PLAN._replace(post="K99"), None, None, None, None)
    with pytest.raises(RuntimeError, match="no form"):
        agent._heads("K99", x)
    with pytest.raises(RuntimeError, match="no form"):
        agent._values(C2_PLAN._replace(value_trunk="K99"), x)
