"""No GPU: the host side of the device evaluation (agent.test_device) — the tier decision (rollout_plan.plan_test), the
episode log's decoder against a literal transcription of the reference's test loop, and the three entry points'
declarations in the C header."""
import ctypes

import numpy as np
import pytest

from xuanpolicy_amd import _lib, ops
from xuanpolicy_amd.rollout_plan import EvalFacts, eval_entry, plan_test

# C1's shape on CartPole: (d_in, h0, h1, h2, k, LDS floats)
BASE = EvalFacts(cuda=True, env="cartpole", dist="categorical", small=(4, 64, 64, 64, 2, 200), n_envs=3, obs_dim=4,
                 raw_obs=False, world=1, sync_obs_rms=False)


def test_plan_test_base_cases():
    assert plan_test(BASE) == "K32E" and eval_entry(BASE) == "xpa_small_eval_cartpole"
    pend = BASE._replace(env="pendulum", dist="gaussian", small=(3, 32, 64, 32, 1, 200), obs_dim=3)
    assert plan_test(pend) == "K32E" and eval_entry(pend) == "xpa_small_eval_pendulum"


@pytest.mark.parametrize("change,tier", [
    (dict(cuda=False), "host"),
    (dict(env="host"), "host"),                          # no step_device
    (dict(sync_obs_rms=True, world=2), "host"),          # the per-step collective
    (dict(sync_obs_rms=True, world=1), "K32E"),
    (dict(sync_obs_rms="rollout", world=2), "K32E"),
    (dict(env="synthbox"), "steps"),                     # (kind, dist) not one of K32's
    (dict(env="device"), "steps"),
    (dict(dist="gaussian"), "steps"),
    (dict(env="pendulum"), "steps"),                     # Pendulum with a Categorical head
    (dict(small=None), "steps"),                         # no small_policy_layers
    (dict(small=(4, 128, 64, 64, 2, 200)), "steps"),     # widths outside 32 / 64
    (dict(small=(4, 64, 128, 64, 2, 200)), "steps"),
    (dict(small=(4, 64, 64, 48, 2, 200)), "steps"),
    (dict(small=(4, 32, 32, 32, 2, 200)), "K32E"),
    (dict(small=(3, 64, 64, 64, 2, 200)), "steps"),      # d_in is not the env's
    (dict(small=(4, 64, 64, 64, 3, 200)), "steps"),      # k is not the env's
    (dict(obs_dim=5), "steps"),
    (dict(small=(4, 64, 64, 64, 2, -1)), "steps"),       # the library found no LDS layout
    (dict(small=(4, 64, 64, 64, 2, 16385)), "steps"),
    (dict(n_envs=256), "K32E"),
    (dict(n_envs=257), "steps"),
    (dict(raw_obs=True), "steps"),
])
def test_plan_test_truth_table(change, tier):
    assert plan_test(BASE._replace(**change)) == tier


def _reference_loop(term, trunc, score, test_episode, atari):
    """ppoclip_agent.py:113-165's collection, literally: per step, envs in ascending order; a terminal without
    truncation is skipped under env_name "Atari"; the loop ends after the first step with enough episodes."""
    current_episode, scores, where, steps = 0, [], [], 0
    while current_episode < test_episode:
        terminals, truncations = term[steps], trunc[steps]
        for i in range(term.shape[1]):
            if terminals[i] or truncations[i]:
                if atari and not truncations[i]:
                    continue
                scores.append(score[steps, i])
                where.append((steps, i))
                current_episode += 1
        steps += 1
    return scores, where, steps


def _write_log(term, trunc, score, length, test_episode, atari, capacity=None, snap_dim=2):
    """What the device writers leave: the log's int32 words, built with numpy from the header's layout."""
    S, N = term.shape
    capacity = test_episode + N if capacity is None else capacity
    ent0, total = ops.eval_log_layout(capacity, snap_dim)
    w = np.zeros((total,), np.int32)
    w[1], w[5], w[6] = test_episode, capacity, snap_dim
    for s in range(S):
        if w[2]:
            break
        for i in range(N):
            if (term[s, i] or trunc[s, i]) and not (atari and not trunc[s, i]):
                if w[0] < capacity:
                    e = ent0 + 4 * int(w[0])
                    w[e], w[e + 1], w[e + 3] = s, i, length[s, i]
                    w[e + 2:e + 3] = np.float32(score[s, i]).reshape(1).view(np.int32)
                else:
                    w[4] = 1
                w[0] += 1
        w[3] += 1
        if w[0] >= test_episode:
            w[2] = 1
            snap = w[ops.EVAL_LOG_HEADER:ent0]
            snap[:2] = np.array([1e-4 + (s + 1) * N], np.float64).view(np.int32)
            snap[2:2 + snap_dim] = np.arange(1, 1 + snap_dim, dtype=np.float32).view(np.int32)
            snap[2 + snap_dim:2 + 2 * snap_dim] = np.arange(5, 5 + snap_dim, dtype=np.float32).view(np.int32)
    return w


def _synthetic(seed, S, N, p_term, p_trunc):
    rng = np.random.default_rng(seed)
    term, trunc = rng.random((S, N)) < p_term, rng.random((S, N)) < p_trunc
    return term, trunc, rng.standard_normal((S, N)).astype(np.float32), rng.integers(1, 500, (S, N)).astype(np.int32)


@pytest.mark.parametrize("atari", [False, True])
@pytest.mark.parametrize("case", ["same-step", "first-step", "sparse"])
def test_log_decoder_matches_reference_loop(case, atari):
    S, N, test_episode = 12, 7, 5
    term, trunc, score, length = _synthetic(3, S, N, 0.08, 0.05)
    if case == "same-step":      # four envs end together at the step that completes the log: the list is longer
        term[:4], trunc[:4] = False, False
        trunc[2, :3] = True
        trunc[4, 1:5] = True
        term[4, 2] = True
    elif case == "first-step":   # an episode ends in the very first step
        trunc[0, 3] = True
        term[0, 5] = True        # under the Atari flag a life loss: no entry
    trunc[-1] = True             # the log always completes inside the window
    ref_scores, ref_where, ref_steps = _reference_loop(term, trunc, score, test_episode, atari)
    log = ops.eval_log_decode(_write_log(term, trunc, score, length, test_episode, atari))
    assert log["done"] and not log["overflow"] and log["target"] == test_episode
    assert log["steps_run"] == ref_steps and log["count"] == len(ref_scores) >= test_episode
    assert [s.tobytes() for s in log["score"]] == [np.float32(s).tobytes() for s in ref_scores]
    assert list(zip(log["step"].tolist(), log["env"].tolist())) == ref_where
    assert log["length"].tolist() == [int(length[s, i]) for s, i in ref_where]
    assert log["obs_count"] == 1e-4 + ref_steps * N
    np.testing.assert_array_equal(log["obs_mean"], [1.0, 2.0])
    np.testing.assert_array_equal(log["obs_var"], [5.0, 6.0])
    if case == "same-step":
        assert ref_steps == 5 and len(ref_scores) > test_episode
    if case == "first-step":
        assert ref_where[0] == (0, 3) and ((0, 5) in ref_where) == (not atari)
    if atari and case != "same-step":
        lifeloss = term & ~trunc
        assert lifeloss[:ref_steps].any() and not any(lifeloss[s, i] for s, i in ref_where)


def test_log_decoder_overflow_and_layout():
    term, trunc, score, length = _synthetic(5, 4, 6, 0.0, 0.0)
    trunc[1] = True
    w = _write_log(term, trunc, score, length, 3, False, capacity=5)
    log = ops.eval_log_decode(w)
    assert log["overflow"] and log["count"] == 6 and log["done"] and len(log["score"]) == 5
    assert log["env"].tolist() == [0, 1, 2, 3, 4]
    for cap, D in ((1, 0), (9, 4), (300, 17)):
        ent0, total = ops.eval_log_layout(cap, D)
        assert ent0 % 4 == 0 and ent0 >= ops.EVAL_LOG_HEADER + 2 + 2 * D and total == ent0 + 4 * cap
    with pytest.raises(ValueError):
        ops.eval_log_decode(w[:-1])


def test_header_declares_the_entry_points():
    P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    with open(_lib.HEADER) as f:
        sigs, structs, consts = _lib.parse_header(f.read())
    assert consts["XPA_ABI_VERSION"] == 4 and "XpaSmallRolloutArgs" in structs
    for table in (sigs, _lib.SIGNATURES):
        assert table["xpa_small_eval_cartpole"] == (I, [P, P, L, L, P, P])
        assert table["xpa_small_eval_pendulum"] == (I, [P, P, F, P, L, L, P, P])
        assert table["xpa_eval_post"] == (I, [P, L, L, L, P, P, P, P, I, P, P, P, P, P])
        assert table["xpa_eval_log_ints"] == (L, [L, L])
