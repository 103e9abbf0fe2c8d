"""The rollout runs what its plan says: one eager iteration (cuda_graph off, so every step is visible; 256 envs x 16
steps, one epoch of two minibatches) with every library call recorded.  The entry points of each env step must equal
RolloutPlan.step_launches() — the first step also carries the pending standalone obs_rms update — and those from the
end of the last step to the first update call RolloutPlan.close_launches(); both lists are built from the plan's
fields alone.  max_episode_steps 19 keeps one truncation slot per env, 5 gives three (the slot rows, the two RMS
ticket levels and a ragged K14F block are all exercised at this size)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N, T = 256, 16

# (name, builder, builder overrides, agents / FusedActorCritic switches, agent attributes set after construction,
#  the plan fields the case is about)
CASES = [
    ("c2_default", "box", {}, {}, {}, dict(driver="eager", obs="trunk", rms="fold-K14F", trunk="K13-norm", pair="K40R",
                                           head="K14F", post="K14F", gae="compact", feed="rows")),
    ("categorical", "box", {"discrete": True}, {}, {},
     dict(head="K14", env="synthbox", post="K8-deferred", rms="standalone")),
    ("fuse_post_off", "box", {}, {"FUSE_POST": False}, {}, dict(head="K14E", post="K8-deferred", rms="standalone")),
    ("fuse_post_off_fold_rms", "box", {}, {"FUSE_POST": False, "FOLD_RMS": True}, {},
     dict(head="K14E", post="K8-deferred", rms="fold-K8")),
    ("three_slots", "box", {"max_episode_steps": 5}, {}, {}, dict(head="K14F", boot="slots", gae="fixup+scan")),
    ("a2c", "box", {"agent": "A2C"}, {}, {}, dict(head="K14F", rms=None, mid="slots-from-next", gae="compact")),
    ("value_gemm_off", "box", {}, {}, {"value_gemm": False}, dict(gae="compact")),
    ("value_gemm_on", "box", {}, {}, {"value_gemm": True}, dict(gae="K40V+compact")),
    ("fuse_value_gae_off", "box", {}, {}, {"fuse_value_gae": False, "value_gemm": True}, dict(gae="compact")),
    ("rollout_split_off", "box", {}, {"ROLLOUT_SPLIT": False}, {"value_gemm": True}, dict(pair="linear", gae="compact")),
    ("value_scan_64_steps", "box", {"n_steps": 64, "max_episode_steps": 67}, {}, {}, dict(gae="value")),
    # (a minibatch of 2048 rows is past K30's LDS budget: the slot-graph feed, as learner.small_update_ok says)
    ("cartpole_k32", "cartpole", {}, {}, {}, dict(driver="K32", feed="epoch")),
    ("cartpole_k32_off", "cartpole", {"fused_rollout": False}, {}, {},
     dict(driver="eager", obs="K5N", trunk="policy", head="K3", env="cartpole", post="K8-deferred", gae="compact")),
    ("wide_trunk_376_17", "box", {"obs_dim": 376, "act_dim": 17}, {}, {},
     dict(obs="K5N", rms="standalone", trunk="chain", pair="K40R", head="K14", env="synthbox", post="K8-deferred")),
]


@pytest.mark.parametrize("name,builder,over,switches,attrs,want", CASES, ids=[c[0] for c in CASES])
def test_iteration_launches_what_its_plan_declares(name, builder, over, switches, attrs, want, monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import xuanpolicy_amd.agents as ag
    from xuanpolicy_amd import _lib
    from xuanpolicy_amd.fused_mlp import FusedActorCritic
    from xuanpolicy_amd.runner import build_cartpole_ppo, build_synthbox_ppo
    for k, v in switches.items():
        monkeypatch.setattr(FusedActorCritic if k.startswith("ROLLOUT") else ag, k, v)
    kw = dict(n_envs=N, n_steps=T, n_epoch=1, n_minibatch=2, seed=5, device=DEV, cuda_graph=False, max_episode_steps=19)
    if builder == "box":
        kw.update(obs_dim=17, act_dim=6, hidden=256)
        agent = build_synthbox_ppo(**dict(kw, **over))
    else:
        agent = build_cartpole_ppo(**dict(kw, hidden=64, **over))
    for k, v in attrs.items():
        setattr(agent, k, v)
    steps = agent.n_steps
    plan = agent.plan()
    assert {k: getattr(plan, k) for k in want} == want
    assert plan.chunk == 1

    log = []
    real_call, real_step, learner = _lib.call, agent._rollout_step_device, agent.learner
    monkeypatch.setattr(_lib, "call", lambda fn, *a: (log.append(fn.__name__), real_call(fn, *a))[1])
    monkeypatch.setattr(agent, "_rollout_step_device", lambda: (log.append("STEP"), real_step())[1])
    for entry in ("update_fused", "small_epoch", "update_epoch"):
        def logged(*a, _real=getattr(learner, entry), **k):
            log.append("UPDATE")
            return _real(*a, **k)
        monkeypatch.setattr(learner, entry, logged)
    agent.train(steps, log=False)
    torch.cuda.synchronize()
    assert agent.plan() == plan and agent.iterations == 1

    segs, cur = [], []
    for e in log:
        if e == "STEP":
            segs.append(cur)
            cur = []
        else:
            cur.append(e)
    segs.append(cur)
    assert len(segs) == steps + 1
    step = plan.step_launches()
    assert segs[0] == plan.start_launches()
    assert segs[1] == plan.step_launches(pending=True)
    for t in range(2, steps):
        assert segs[t] == step, t
    last = segs[steps]
    assert last[:len(step)] == step
    assert "UPDATE" in last
    assert last[len(step):last.index("UPDATE")] == plan.close_launches()
