"""No device needed: tests/_rollout_step_ref.py — the references the K5 / K8 / K3 GPU tests use — against the reference
project's semantics as oracle/cpu_ref.py restates them, negative controls on the comparators (a wrong reference must
be rejected by the assertion helpers the GPU tests call), and the conditions the chosen inputs must meet."""
import numpy as np
import pytest

from oracle import cpu_ref
from tests import _rollout_step_ref as R

F32, F64 = np.float32, np.float64


# ---------------------------------------------------------------------------------------------- K5
@pytest.mark.parametrize("n,dim", [(1, 1), (257, 6), (300, 65)])
def test_rms_reference_agrees_with_running_mean_std(n, dim):
    rms = cpu_ref.RunningMeanStdRef((dim,))
    mean, var, count = R.rms_initial(dim)
    for X in R.rms_case(n, dim):
        x = X[:, :dim]
        assert np.isnan(X[:, dim:]).all() and np.isfinite(x).all()
        m64, v64, count = R.rms_update_ref64(mean, var, count, x)
        rms.update(x.astype(F64))
        np.testing.assert_allclose(m64, rms.mean, rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(v64, rms.var, rtol=1e-6, atol=1e-9)
        assert count == rms.count
        mean, var = m64.astype(F32), v64.astype(F32)
        R.check_ulp(mean, m64, "own rounding")           # a correctly rounded result passes its own check


@pytest.mark.parametrize("n,dim", R.RMS_FAR_SHAPES)
def test_far_shift_ratio_is_about_1e3(n, dim):
    """|batch mean - running mean| / batch std of the first batch: large enough that an f32 or unshifted accumulation
    shows (1e6 ulps of cancellation in the variance), and not beyond 1e3-ish, so that the f64 one-pass variance's own
    cancellation (ratio^2 * 2^-53 ~ 1e-10) stays far below an f32 ulp."""
    X = R.rms_case(n, dim, far=True)[0][:, :dim].astype(F64)
    ratio = np.abs(X.mean(0) - 0.0) / X.std(0)
    assert 500 < ratio.min() and ratio.max() < 2000, (ratio.min(), ratio.max())
    # the unshifted f32 accumulation this case is for: rejected by the comparator
    m64, v64, _ = R.rms_update_ref64(*R.rms_initial(dim), X.astype(F32))
    x32 = X.astype(F32)
    naive = (np.square(x32).mean(0, dtype=F32) - np.square(x32.mean(0, dtype=F32))).astype(F32)
    with pytest.raises(AssertionError):
        R.check_ulp(naive, v64, "f32 one-pass variance")


def test_negative_control_row_dropped_from_a_sum():
    n, dim = 257, 6
    mean, var, count = R.rms_initial(dim)
    x = R.rms_case(n, dim)[0][:, :dim]
    m64, v64, _ = R.rms_update_ref64(mean, var, count, x)
    got_m, got_v = m64.astype(F32), v64.astype(F32)
    R.check_ulp(got_m, m64, "mean")
    R.check_ulp(got_v, v64, "var")
    wm, wv, _ = R.rms_update_ref64(mean, var, count, x, drop_row=n - 1)
    with pytest.raises(AssertionError):
        R.check_ulp(got_m, wm, "mean against the sum without its last row")
    with pytest.raises(AssertionError):
        R.check_ulp(got_v, wv, "var against the sum without its last row")


def test_normalize_reference_agrees_with_process_observation():
    X, mean, var, clip = R.normalize_case(257, 6)
    x = X[:, :6]
    rms = cpu_ref.RunningMeanStdRef((6,))
    rms.mean, rms.var = mean.astype(F64), var.astype(F64)
    want = cpu_ref.process_observation(x.astype(F64), rms, obs_range=clip)
    got = R.obs_normalize_ref32(x, mean, var, clip)
    assert got.dtype == F32
    np.testing.assert_allclose(got, want, rtol=3e-7, atol=1e-7)
    assert (got == clip).any() and (got == -clip).any() and got[2, 0] == 0.0 and np.isfinite(got).all()


# ---------------------------------------------------------------------------------------------- K8
@pytest.mark.parametrize("algo,atari,mid", [("ppo", False, False), ("a2c", False, False), ("ppo", True, False),
                                            ("a2c", False, True)])
def test_post_reference_agrees_with_the_reference_rules(algo, atari, mid):
    """tests/test_gpu_kernels.py test_rollout_post_matches_reference_rules' loop (agent.py:118-123,
    ppoclip_agent.py:69-101 / a2c_agent.py:84), with its per-env sequential ret_rms.update, against post_step_ref run
    on its own rounded outputs."""
    rng = np.random.default_rng(3)
    N, T = 300, 5
    returns = rng.normal(0, 1, N).astype(F32)
    ret_rms = cpu_ref.RunningMeanStdRef(())
    ret_rms.mean, ret_rms.var, ret_rms.count = F32(0.3), F32(2.0), 17.0
    st = dict(T=T, ptr=0, step=0, ret_mean=F32(0.3), ret_var=F32(2.0), ret_count=17.0, returns=returns.copy())
    for t in range(T):
        rew = rng.normal(0, 2, N).astype(F32)
        term = rng.random(N) < 0.2
        trunc = rng.random(N) < 0.1
        vb = rng.normal(0, 1, N).astype(F32)
        vm = rng.normal(0, 1, N).astype(F32)
        exp_rew = cpu_ref.process_reward(rew, ret_rms, rew_range=5.0)
        if algo == "ppo":
            returns = (1 - term) * 0.99 * returns + rew
        else:
            returns = 0.99 * returns + rew
        done = term | trunc
        for i in np.nonzero(done)[0]:
            ret_rms.update(returns[i:i + 1])
        returns = np.where(done, 0, returns).astype(F32)
        last = t == T - 1
        close = np.full(N, True) if last else (done & ~(atari & ~trunc))
        exp_boot = np.where(close, np.where(term, 0, vm if (mid and not last) else vb), 0)
        ref = R.post_step_ref(st, rew, term, trunc, gamma=0.99, form="plain", v_boot=vb, v_boot_mid=vm if mid else None,
                              mask_returns=(algo == "ppo"), atari_lifeloss=atari)
        np.testing.assert_allclose(ref["buf_rew"], exp_rew, rtol=1e-6, atol=1e-7)
        np.testing.assert_array_equal(ref["buf_term"], term.astype(F32))
        np.testing.assert_array_equal(ref["buf_closed"].astype(bool), close)
        np.testing.assert_array_equal(ref["buf_boot"], exp_boot.astype(F32))
        np.testing.assert_allclose(ref["returns64"], returns, rtol=1e-6, atol=1e-6)
        assert ref["ret_count"] == pytest.approx(ret_rms.count, abs=1e-9)
        for form, (m64, v64) in ref["ret64"].items():
            assert m64 == pytest.approx(float(ret_rms.mean), rel=1e-6, abs=1e-7), form
            assert v64 == pytest.approx(float(ret_rms.var), rel=1e-5), form
        m64, v64 = ref["ret64"]["two"] if ref["ret64"] else (st["ret_mean"], st["ret_var"])
        st = R.post_advance(st, ref, ref["returns64"].astype(F32), F32(m64), F32(v64))
    assert st["ptr"] == 0 and st["step"] == T


def _defer_step(form="norm", slot_src=True, **kw):
    N, D, S = 257, 17, 3
    steps = R.post_case(N, 2, D)
    st = R.post_initial(N, 3, "mid", D, S)
    s = steps[1]                                  # every env finishes: the truncated ones are kept
    return st, s, R.post_step_ref(st, s["rew"], s["term"], s["trunc"], gamma=R.POST_GAMMA, form=form,
                                  final_obs=s["final_obs"], slot_src=s["slot_src"] if slot_src else None, **kw)


def test_negative_control_slot_row_from_the_wrong_source():
    st, s, good = _defer_step()
    assert good["n_kept"] > 50 and np.isfinite(good["slot_obs"]).all()
    R.check_exact(good["slot_obs"].copy(), good["slot_obs"], "slot_obs")
    R.check_exact(good["slot_t"].copy(), good["slot_t"], "slot_t")
    for slot_src in (True, False):
        _, _, good = _defer_step(slot_src=slot_src)
        _, _, wrong = _defer_step(slot_src=slot_src, wrong_slot_source=True)
        R.check_exact(good["slot_t"], wrong["slot_t"], "slot_t")          # the same rows are kept ...
        with pytest.raises(AssertionError):
            R.check_exact(good["slot_obs"], wrong["slot_obs"], "slot_obs")   # ... from another source
    # one single slot row taken from the other source
    one = good["slot_obs"].copy()
    k = int(np.flatnonzero(good["slot_t"] >= 0)[0])
    one[k] = R.obs_normalize_ref32(s["slot_src"][k % 257, :17], st["obs_mean"], st["obs_var"], 5.0)
    with pytest.raises(AssertionError):
        R.check_exact(one, good["slot_obs"], "slot_obs")


def test_post_reference_slot_rules():
    """The overflow rule (count it, reuse the last slot), the old-statistics normalisation and the untouched ret_rms."""
    for S in (1, 3):
        N, D = 5, 3
        st = R.post_initial(N, 3, "mid", D, S)
        hits = []
        for i, s in enumerate(R.post_case(N, 7, D)):
            ref = R.post_step_ref(st, s["rew"], s["term"], s["trunc"], gamma=R.POST_GAMMA, form="fold",
                                  final_obs=s["final_obs"], rms_x=s["rms_x"])
            if i == 0:
                assert ref["n_finished"] == 0 and not ref["ret64"] and ref["ret_count"] == st["ret_count"]
                R.check_ret_rms(st["ret_mean"], st["ret_var"], st["ret_count"], ref, "c == 0")
                with pytest.raises(AssertionError):
                    R.check_ret_rms(np.nextafter(st["ret_mean"], F32(9)), st["ret_var"], st["ret_count"], ref, "c == 0")
            if i == 1:
                assert ref["n_finished"] == N
            if st["ptr"] != 2 and s["trunc"][0] and not s["term"][0]:
                hits.append(i)
                row = R.obs_normalize_ref32(s["final_obs"][0, :D], st["obs_mean"], st["obs_var"], 5.0)
                k = min(len(hits), S) - 1
                assert ref["slot_t"][k * N] == st["ptr"]
                R.check_exact(ref["slot_obs"][k * N], row, "env 0's kept row")
            if st["ptr"] == 2:
                assert ref["boot_norm"] is not None and ref["buf_closed"].all()
            m, v = ref["ret64"]["fma"] if ref["ret64"] else (st["ret_mean"], st["ret_var"])
            st = R.post_advance(st, ref, ref["returns64"].astype(F32), m, v,
                                (ref["obs_mean64"].astype(F32), ref["obs_var64"].astype(F32)))
        # env 0 alone overflows once its S + 1-th row arrives (S = 3: the 4th, at step 6)
        assert hits == [1, 3, 4, 6] and st["overflow"] >= len(hits) - S >= 1


def test_post_cases_take_both_rstd_clamps_and_the_reward_clip():
    for ret_state, want in (("lo", 0.1), ("hi", 100.0)):
        st = R.post_initial(257, 3, ret_state)
        s = R.post_case(257, 1)[0]
        ref = R.post_step_ref(st, s["rew"], s["term"], s["trunc"], gamma=R.POST_GAMMA, v_boot=s["v_boot"])
        assert ref["rstd"] == F32(want) and np.sqrt(F32(st["ret_var"])) != F32(want)
        assert (np.abs(ref["buf_rew"]) == 5.0).any()
    both = [(s["term"] & s["trunc"]).any() for s in R.post_case(257, 7)]
    assert both[1] and both[5]
    assert R.POST_BIG_N > 1024 * 256 and (R.POST_BIG_N + 255) // 256 == 1025


def test_tracker_bound_holds_for_both_f32_evaluations():
    rng = np.random.default_rng(0)
    R0 = rng.normal(0, 30, 100000).astype(F32)
    r = rng.normal(0, 2, 100000).astype(F32)
    g = F32(0.99)
    ref = F64(g) * R0.astype(F64) + r.astype(F64)
    R.check_tracker((g * R0 + r).astype(F32), ref, F64(g) * R0.astype(F64), "two roundings")
    R.check_tracker(ref.astype(F32), ref, F64(g) * R0.astype(F64), "one rounding")
    with pytest.raises(AssertionError):
        R.check_tracker((F32(0.99000007) * R0 + r).astype(F32), ref, F64(g) * R0.astype(F64), "gamma one ulp off")


def test_bootstrap_fixup_reference():
    values, slot_t, buf_term, buf_boot = R.fixup_case()
    N, T, S = R.FIXUP_SHAPE
    boot, st = R.bootstrap_fixup_ref(values, slot_t, buf_term, buf_boot)
    assert (st == -1).all() and boot.dtype == F32
    want = buf_boot.copy()
    for n in range(N):
        for k in range(S):
            t = slot_t[k * N + n]
            if 0 <= t < T:
                want[n, t] = values[k * N + n]
        want[n, T - 1] = 0.0 if buf_term[n, T - 1] else values[S * N + n]
    R.check_exact(boot, want, "buf_boot")


# ---------------------------------------------------------------------------------------------- K3
def test_sample_reference_is_a_standard_normal_and_the_softmax():
    mu, logstd, _ = R.sample_case("gaussian", 4099, 6)
    r = R.sample_ref("gaussian", mu, logstd, R.SAMPLE_SEED, 5)
    assert abs(r["eps"].mean()) < 0.02 and abs(r["eps"].std() - 1.0) < 0.02
    assert (r["u1"] > 0).all() and (r["u1"] <= 1).all() and (r["u2"] >= 0).all() and (r["u2"] < 1).all()
    import torch
    lp = torch.distributions.Normal(torch.from_numpy(mu).double(), torch.from_numpy(logstd).double().exp()).log_prob(
        torch.from_numpy(r["act"])).sum(-1).numpy()
    np.testing.assert_allclose(r["logp"], lp, rtol=1e-9, atol=1e-9)
    z, _, _ = R.sample_case("categorical", 4099, 18)
    c = R.sample_ref("categorical", z, None, R.SAMPLE_SEED, 0x80000123)
    p = torch.softmax(torch.from_numpy(z).double(), -1).numpy()
    np.testing.assert_allclose(c["cdf"], np.cumsum(p, axis=1), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(c["logp_all"], np.log(p), rtol=1e-9, atol=1e-9)
    assert c["pick"][1] == 9 and (np.bincount(c["pick"], minlength=18) > 0).sum() >= 16
    # a step above 2^31 and its low 31 bits draw differently (the key is the full uint32)
    c2 = R.sample_ref("categorical", z, None, R.SAMPLE_SEED, 0x00000123)
    assert (c["u"] != c2["u"]).mean() > 0.99


def test_negative_control_draw_keyed_with_a_instead_of_2a():
    mu, logstd, _ = R.sample_case("gaussian", 257, 6)
    r64 = R.sample_ref("gaussian", mu, logstd, R.SAMPLE_SEED, 5, F64)
    r32 = R.sample_ref("gaussian", mu, logstd, R.SAMPLE_SEED, 5, F32)
    bad = R.sample_ref("gaussian", mu, logstd, R.SAMPLE_SEED, 5, F32, wrong_key=True)
    np.testing.assert_array_equal(bad["eps"][:, 0], r32["eps"][:, 0])      # a = 0: 2a == a
    for name in ("act", "logp", "eps"):
        got = r64[name].astype(F32)           # a correctly rounded kernel passes
        assert R.check_within_f32([got], [r32[name]], [r64[name]], name).ratio <= 1.0 + 1e-9 or name == "logp"
        with pytest.raises(AssertionError):
            R.check_within_f32([bad[name]], [r32[name]], [r64[name]], name)
    # and the Categorical key
    z, _, _ = R.sample_case("categorical", 257, 3)
    c64 = R.sample_ref("categorical", z, None, R.SAMPLE_SEED, 5, F64)
    c32 = R.sample_ref("categorical", z, None, R.SAMPLE_SEED, 5, F32)
    wrong = R.sample_ref("categorical", z, None, R.SAMPLE_SEED, 5, F32, wrong_key=True)
    delta = R.cat_delta(c64, c32)
    R.check_cat_picks(c32["pick"], c64, delta, "the f32 baseline's picks")
    with pytest.raises(AssertionError):
        R.check_cat_picks(wrong["pick"], c64, delta, "picks from key 1")


@pytest.mark.parametrize("K", R.SAMPLE_K)
@pytest.mark.parametrize("n_envs", R.SAMPLE_N)
def test_categorical_cases_leave_out_at_most_one_percent(n_envs, K):
    """delta = MARGIN x the f32 baseline's worst CDF error; the envs whose uniform lies within delta of a boundary are
    left out of the pick comparison: at most 1 % of a case (expected share ~ 2 K delta)."""
    z, _, _ = R.sample_case("categorical", n_envs, K)
    pool = R.sample_pool_e32("categorical", K)
    assert 0 < pool["cdf"] < 1e-6 and 0 < pool["logp"] < 4e-6, pool
    for _, step in R.SAMPLE_CURSORS:
        c64 = R.sample_ref("categorical", z, None, R.SAMPLE_SEED, step, F64)
        c32 = R.sample_ref("categorical", z, None, R.SAMPLE_SEED, step, F32)
        delta = R.cat_delta(c64, c32, e32_pool=pool["cdf"])
        assert delta < 1e-5, delta
        out = R.cat_near(c64, delta).any(axis=1)
        assert out.sum() <= R.CAT_CAP * n_envs, (int(out.sum()), n_envs, delta)
        R.check_cat_picks(c32["pick"], c64, delta, "baseline", cap=R.CAT_CAP)
    if n_envs > 1:
        np.testing.assert_allclose(c64["cdf"][0], np.arange(1, K + 1) / K, rtol=1e-12)
        assert c64["cdf"][1, K // 2] - c64["cdf"][1, K // 2 - 1] >= 1 - 1e-12        # the dominant logit
