"""The minibatch update runs what its plan says: one eager learner.update_fused on a Rows minibatch (N x T = 512 x 64,
B = 8192, the end-to-end shape) with every library call recorded; the ordered entry points up to the clip + Adam step
must equal UpdatePlan.launches(), which is built from the plan's fields alone."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

CASES = [
    # (name, obs width, act width, ops switches, class switches, (heads, dw_hidden, trunk_fwd, trunk_bwd))
    ("c2_default", 17, 6, {}, {}, ("K16Q-mask", "K41P", "K13-gather-sign", "K42C")),
    ("c2_crit_off", 17, 6, {}, {"CRIT_FACTORED": False}, ("K16Q", "K41V", "K13-gather-sign", "K42S")),
    ("c2_f32", 17, 6, {"S3_GEMMS": False}, {}, ("K16", "splitk", "K13-gather", "mm+chain")),
    ("c4_direct", 376, 17, {}, {"WIDE_TRUNK": True, "WIDE_DIRECT": True}, ("K16Q-mask", "K41P", "K40F-idx", "K42C-dz")),
    ("c4_gather", 376, 17, {}, {"WIDE_TRUNK": True, "WIDE_DIRECT": False},
     ("K16Q-mask", "K41P", "K40F-pitched", "K42C-dz")),
]


@pytest.mark.parametrize("name,D,A,ops_sw,cls_sw,want", CASES, ids=[c[0] for c in CASES])
def test_update_launches_what_its_plan_declares(name, D, A, ops_sw, cls_sw, want, monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from xuanpolicy_amd import _lib, ops
    from xuanpolicy_amd.fused_mlp import FusedActorCritic, Rows
    from xuanpolicy_amd.runner import build_synthbox_ppo
    for k, v in ops_sw.items():
        monkeypatch.setattr(ops, k, v)
    for k, v in cls_sw.items():
        monkeypatch.setattr(FusedActorCritic, k, v)
    N, T, n_mb = 512, 64, 4
    agent = build_synthbox_ppo(n_envs=N, n_steps=T, obs_dim=D, act_dim=A, hidden=256, n_epoch=2, n_minibatch=n_mb,
                               seed=5, device=DEV, max_episode_steps=T + 17)
    learner, mem = agent.learner, agent.memory
    fm = learner._fused_mlp()
    assert fm is not None and fm.fused_heads and fm.pair is not None
    gen = torch.Generator(device=DEV).manual_seed(7)
    for t in (mem.observations, mem.actions, mem._advantages, mem._returns):
        t.copy_(torch.randn(t.shape, device=DEV, generator=gen))
    mem.auxiliary_infos["old_logp"].fill_(-1.0 * A)
    NT, B = N * T, N * T // n_mb
    obs_flat = mem.observations.reshape(NT, D)
    assert fm.rows_ok(obs_flat)
    idx = torch.randperm(NT, device=DEV, generator=gen)[:B]
    part = torch.empty((ops.gather_num_partials(B), 2), dtype=torch.float64, device=DEV)

    log = []
    real_call, real_step = _lib.call, learner._sync_clip_step
    monkeypatch.setattr(_lib, "call", lambda fn, *a: (log.append(fn.__name__), real_call(fn, *a))[1])
    monkeypatch.setattr(learner, "_sync_clip_step", lambda *a, **k: (log.append("STEP"), real_step(*a, **k))[1])
    scalars = learner.update_fused(Rows(obs_flat, idx), idx, mem.actions.reshape(-1), mem._advantages.reshape(-1),
                                   mem._returns.reshape(-1), mem.auxiliary_infos["old_logp"].reshape(-1), part)
    torch.cuda.synchronize()
    assert torch.isfinite(scalars).all()
    plan = fm.last_plan
    assert plan == fm.plan(Rows(obs_flat, idx))
    assert (plan.heads, plan.dw_hidden, plan.trunk_fwd, plan.trunk_bwd) == want
    assert log[:log.index("STEP")] == plan.launches(adv_moments=True)
