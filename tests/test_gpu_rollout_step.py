"""GPU: the per-step rollout kernels of csrc/rollout.hip — K5 (xpa_rms_partials / _merge / _update, xpa_obs_normalize),
K8 (xpa_rollout_post and its three deferred forms, xpa_rollout_bootstrap_fixup) and K3 (xpa_rollout_sample) — through
xuanpolicy_amd.ops against the numpy restatements of tests/_rollout_step_ref.py, at every launch geometry.  K14F, K32,
K32W and K33 are tested as "equal to these kernels"; these are tested against an independent reference.

What is asserted (the comparators live in tests/_rollout_step_ref.py and have negative controls in
tests/test_rollout_step_ref_cpu.py):
  * single correctly rounded f32 operations (obs_normalize / obs_norm1, the reward scaling and its clamps): bit equal;
  * integers, flags and copies (closed, term, boot, slot_t, overflow, cursor, counts, tickets back at 0): exact;
  * f64-accumulated statistics (obs mean / var of K5 and of the fold, ret mean / var): within one f32 ulp of the f64
    reference, count exact, ret_rms bitwise untouched when no env finished; the fold also within one ulp of
    ops.rms_update on the same rows;
  * the return tracker: |got - f64| <= 2^-24 (|gamma R| + |f64|);
  * K3 Gaussian: eps, action and log-prob within tests/_small_ref.py's within_f32 bound (MARGIN 4 x the error of the
    same restatement run in numpy f32, + 2^-24 of the scale); env_in the exact f32 clamp; repeated launches bit equal;
  * K3 Categorical: the pick equals the f64 inverse CDF's wherever the uniform is at least delta (4 x the f32
    baseline's worst CDF error) from every boundary, at most 1 % of a case left out and those picks beside the near
    boundary; the log-prob of the kernel's pick within within_f32; exact one-hot rows.

Shapes, and the branch each is there for:
  K5 update (ticketed one-launch form and partials + merge, x row-strided with NaN pads, three updates from
  count = 1e-4):  (1, 1) smallest | (255, 3) 85 row groups, thread 255 idle | (256, 4) one full row block | (257, 6)
  second block of one row | (300, 64) last 1-D width | (300, 65) first 2-D width, second column block of one column |
  (513, 128) 2-D over three row blocks | (4096, 64) np * dim * 2 == 2048, staged merge | (4097, 64) unstaged merge |
  (1000, 376) C4.  Far shift (first batch 1e3 batch-std from the running mean): (257, 6) 1-D, (300, 65) 2-D.
  obs_normalize:  (1, 1) | (257, 6) strided, into buffer column 0 and T - 1 | (4099, 257) above 4096 x 256 elements, the
  grid-stride loop; var = 0 in column 0, both clip edges.
  K8 (horizon 3; 4 steps plain, 7 steps deferred so that env 0 fills n_slots + 1 rows; one workspace per run):
  n_envs 1 | 255 last thread idle | 256 one full block | 257 second block of one env | 1000; plain form at 262145
  envs = 1025 blocks (the unstaged partial sum), horizon 2.  Events: a step finishing no env (the c == 0 merge), one
  finishing all, term and trunc both set, atari_lifeloss / mask_returns on and off, use_rewnorm off, ret_var 1e-4 and
  1e6 (both rstd clamps), rewards of +-1000 (the rew_range clip).  Deferred: obs_dim 1 | 17 | 64, n_slots 1 | 3,
  slot_src on and off, NaN-padded sources, slot overflow.  Fold: obs_dim 1 | 15 | 16 (one full tile) | 17 (tile + 1)
  | 33 | 64 x n_envs 1 | 255 | 257 (ragged block: the break) | 1000.
  bootstrap_fixup: 257 envs, 2 slots, used / unused / out-of-range slots, terminal last steps.
  K3: n_envs 1 | 255 | 257 | 4099; Gaussian A 1 | 6 | 17; Categorical K 2 | 3 | 18; cursor.ptr 0 and T - 1, cursor.step
  small and above 2^31; ld_env above A; equal logits and a dominant (+80) logit.

E32 of the K3 bounds is pooled over every case of one width (_rollout_step_ref.sample_pool_e32): the one-env cases hold
1 .. 17 elements, and on its own such a case's baseline can round luckily (E32 = 0.2 ulp of the log-sum-exp at K = 18,
where the kernel's honest 3.6 ulp then missed 4 E32).  The pool is computed from the references alone.

Measured on an MI355X (the margin used is 4 everywhere; every test prints its figures).  No kernel defect was found.
  K5, both forms, all shapes and the far shift: worst distance from the f64 reference 0.500 f32 ulp (the bound is 1),
    the one-launch and the two-launch form bit equal.
  K8: every flag, copy, reward and kept row exact; ret_rms and the fold's obs_rms inside one ulp in every step.  In
    some steps only the merge of the two-rounding tracker lay inside the ulp (check_ret_rms tries the fused one first
    and reports the form it matched), so both forms of post_step_ref's ret64 are needed.
  K3 Gaussian, worst |err| / E32 over the 12 cases: eps 1.03, action 1.30, log-prob 1.06.
  K3 Categorical, worst log-prob |err| / E32 over the 12 cases: 0.90; envs left out of the pick comparison: 1 of
    16396 at (4099, 18), none elsewhere; every pick equal to the f64 inverse CDF's.
A library with five in-bounds defects (u1 keyed with a; the inverse CDF's pick off by one; the fold's ragged block one
row short; the unstaged merge reading a neighbouring partial; the overflow reusing slot 0) failed 61 of these 101
cases, each defect exactly where its branch is taken: K5 only at (4097, 64) and (1000, 376), the Gaussian sampler at
A = 6 and 17 but not at A = 1 (2a == a), every Categorical, deferred and fold case.
"""
import numpy as np
import pytest
import torch

from tests import _rollout_step_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from xuanpolicy_amd import _lib
    _lib.load()


def _d(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def _h(t):
    return t.detach().cpu().numpy().copy()


def _cursor(ptr, step):
    s = int(step) & 0xFFFFFFFF
    return torch.tensor([ptr, s - (1 << 32) if s >= (1 << 31) else s, 0, 0], dtype=torch.int32, device=DEV)


def _cursor_of(cur):
    c = _h(cur)
    return int(c[0]), int(c[1]) & 0xFFFFFFFF, int(c[2]), int(c[3])


# ---------------------------------------------------------------------------------------------- K5
def _rms_run(n, dim, far):
    from xuanpolicy_amd import ops
    m0, v0, c0 = R.rms_initial(dim)
    st = {f: (_d(m0), _d(v0), torch.tensor([c0], dtype=torch.float64, device=DEV)) for f in ("ticket", "two")}
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    worst = 0.0
    for k, X in enumerate(R.rms_case(n, dim, far)):
        x = _d(X)[:, :dim]
        assert x.stride(0) == dim + R.RMS_PAD
        refs = {f: R.rms_update_ref64(_h(s[0]), _h(s[1]), float(s[2]), X[:, :dim]) for f, s in st.items()}
        ops.rms_update(x, *st["two"])
        ops.rms_update(x, *st["ticket"], ticket=ticket)
        assert int(ticket.item()) == 0, "ticket not reset"
        for f, (mean, var, cnt) in st.items():
            rm, rv, rc = refs[f]
            what = "rms (%d, %d) update %d %s" % (n, dim, k, f)
            worst = max(worst, R.check_ulp(_h(mean), rm, what + " mean"), R.check_ulp(_h(var), rv, what + " var"))
            assert float(cnt) == rc, (what, float(cnt), rc)
        for a, b in zip(st["ticket"], st["two"]):
            assert torch.equal(a, b), "the one-launch and the two-launch form differ"
    print("K5 (%d, %d)%s: worst distance %.3f ulp" % (n, dim, " far" if far else "", worst))


@pytest.mark.parametrize("n,dim", R.RMS_SHAPES)
def test_rms_update_matches_f64(n, dim):
    _rms_run(n, dim, False)


@pytest.mark.parametrize("n,dim", R.RMS_FAR_SHAPES)
def test_rms_update_far_shift_matches_f64(n, dim):
    _rms_run(n, dim, True)


@pytest.mark.parametrize("n,dim,ptr", [(1, 1, None), (257, 6, 0), (257, 6, 3), (4099, 257, None)])
def test_obs_normalize_bit_equal(n, dim, ptr):
    from xuanpolicy_amd import ops
    X, mean, var, clip = R.normalize_case(n, dim)
    exp = R.obs_normalize_ref32(X[:, :dim], mean, var, clip)
    assert (exp == clip).any() and (n < 2 or (exp == -clip).any()) and (n < 3 or exp[2, 0] == 0)
    T = 4
    out = torch.full((n, dim + 1), -9.0, device=DEV)
    col = torch.full((n, T, dim), -9.0, device=DEV) if ptr is not None else None
    cur = _cursor(ptr, 3) if ptr is not None else None
    ops.obs_normalize(_d(X)[:, :dim], _d(mean), _d(var), clip, out[:, :dim], col_out=col, col_ld=T * dim, cursor=cur)
    R.check_exact(_h(out[:, :dim]), exp, "obs_normalize out")
    assert bool((out[:, dim] == -9.0).all()), "pad column written"
    if ptr is not None:
        want = np.full((n, T, dim), -9.0, F32)
        want[:, ptr] = exp
        R.check_exact(_h(col), want, "obs_normalize buffer column")
        assert _cursor_of(cur) == (ptr, 3, 0, 0)


# ---------------------------------------------------------------------------------------------- K8
SENT = -3.0


class _PostRun:
    """The device side of one K8 run and its step-by-step comparison with post_step_ref."""

    def __init__(self, N, T, ret_state, D=0, S=0, fold=False):
        from xuanpolicy_amd import ops
        self.ops, self.N, self.T, self.D, self.S = ops, N, T, D, S
        self.st = R.post_initial(N, T, ret_state, D, S)
        st = self.st
        self.cur = _cursor(st["ptr"], st["step"])
        self.rm, self.rv = _d(np.array([st["ret_mean"]], F32)), _d(np.array([st["ret_var"]], F32))
        self.rc = torch.tensor([st["ret_count"]], dtype=torch.float64, device=DEV)
        self.rt = _d(st["returns"])
        self.bufs = {k: torch.full((N, T), SENT, device=DEV) for k in ("rew", "term", "boot")}
        self.closed = torch.full((N, T), 9, dtype=torch.uint8, device=DEV)
        self.shadow = {k: np.full((N, T), SENT, F32) for k in ("rew", "term", "boot")}
        self.shadow["closed"] = np.full((N, T), 9, np.uint8)
        self.ws = ops.post_workspace(N, DEV)
        self.forms = set()
        if S:
            self.slot_obs, self.slot_t = _d(st["slot_obs"]), _d(st["slot_t"])
            self.over = torch.zeros(1, dtype=torch.int32, device=DEV)
            self.boot_norm = torch.full((N, D + 2), SENT, device=DEV)
            self.bn_shadow = np.full((N, D + 2), SENT, F32)
        if D:
            self.om, self.ov = _d(st["obs_mean"]), _d(st["obs_var"])
            self.oc = torch.tensor([st["obs_count"]], dtype=torch.float64, device=DEV)
        if fold:
            self.rpart = torch.zeros(2 * int(ops.lib().xpa_rollout_post_num_blocks(N)), D, dtype=torch.float64,
                                     device=DEV)

    def step(self, s, form, what, gamma=R.POST_GAMMA, mask_returns=True, use_rewnorm=True, atari=False, mid=False,
             slot_src=False, rew_range=5.0):
        ops, N, D = self.ops, self.N, self.D
        t = self.st["ptr"]
        kw = dict(gamma=gamma, form=form, mask_returns=mask_returns, use_rewnorm=use_rewnorm, rew_range=rew_range,
                  atari_lifeloss=atari)
        deferred, rms = None, None
        if form == "plain":
            kw.update(v_boot=s["v_boot"], v_boot_mid=s["v_boot_mid"] if mid else None)
        else:
            kw.update(final_obs=s["final_obs"], slot_src=s["slot_src"] if slot_src else None, obs_clip=5.0)
            deferred = (_d(s["final_obs"])[:, :D], self.slot_obs, self.slot_t, self.over)
            if form != "deferred":
                deferred += (self.om, self.ov, 5.0, self.boot_norm[:, :D])
            if slot_src:
                assert form != "deferred"
                deferred += (_d(s["slot_src"])[:, :D],)
        if form == "fold":
            kw.update(rms_x=s["rms_x"])
            rx = _d(s["rms_x"])[:, :D]
            rms = (rx, self.oc, self.rpart)
            twin = (self.om.clone(), self.ov.clone(), self.oc.clone())     # ops.rms_update on the same rows
            ops.rms_update(rx, *twin)
        ref = R.post_step_ref(self.st, s["rew"], s["term"], s["trunc"], **kw)
        ops.rollout_post(_d(s["rew"]), _d(s["term"]), _d(s["trunc"]), _d(s["v_boot"]) if form == "plain" else None,
                         self.cur, self.rm, self.rv, self.rc, self.rt, self.bufs["rew"], self.bufs["term"], self.closed,
                         self.bufs["boot"], gamma, mask_returns=mask_returns, use_rewnorm=use_rewnorm,
                         rew_range=rew_range, atari_lifeloss=atari, deferred=deferred, workspace=self.ws,
                         v_boot_mid=_d(s["v_boot_mid"]) if (mid and form == "plain") else None, rms=rms)
        assert int(self.ws[1].item()) == 0, (what, "ticket not reset")
        for k in ("rew", "term", "boot", "closed"):
            self.shadow[k][:, t] = ref["buf_" + k]
        for k in ("rew", "term", "boot"):
            R.check_exact(_h(self.bufs[k]), self.shadow[k], what + " buf_" + k)
        R.check_exact(_h(self.closed), self.shadow["closed"], what + " buf_closed")
        assert _cursor_of(self.cur) == (ref["ptr"], ref["step"], 0, 0), (what, _cursor_of(self.cur))
        got_rt = _h(self.rt)
        R.check_tracker(got_rt, ref["returns64"], ref["gamma_r64"], what + " returns")
        assert not got_rt[ref["done"]].any(), (what, "a finished env's return is not 0")
        self.forms.add(R.check_ret_rms(_h(self.rm)[0], _h(self.rv)[0], float(self.rc), ref, what))
        if form != "plain":
            R.check_exact(_h(self.slot_t), ref["slot_t"], what + " slot_t")
            R.check_exact(_h(self.slot_obs), ref["slot_obs"], what + " slot_obs")
            assert int(self.over.item()) == ref["overflow"], (what, "overflow", int(self.over.item()), ref["overflow"])
            if ref["boot_norm"] is not None:
                self.bn_shadow[:, :D] = ref["boot_norm"]
            R.check_exact(_h(self.boot_norm), self.bn_shadow, what + " boot_norm")
        got_obs = None
        if form == "fold":
            got_obs = (_h(self.om), _h(self.ov))
            R.check_ulp(got_obs[0], ref["obs_mean64"], what + " obs_mean")
            R.check_ulp(got_obs[1], ref["obs_var64"], what + " obs_var")
            assert float(self.oc) == ref["obs_count"] == float(twin[2]), (what, "obs_count")
            R.check_ulp(got_obs[0], _h(twin[0]).astype(np.float64), what + " obs_mean vs ops.rms_update")
            R.check_ulp(got_obs[1], _h(twin[1]).astype(np.float64), what + " obs_var vs ops.rms_update")
        elif D and form != "deferred":
            R.check_exact(_h(self.om), self.st["obs_mean"], what + " obs_mean untouched")
            R.check_exact(_h(self.ov), self.st["obs_var"], what + " obs_var untouched")
        self.st = R.post_advance(self.st, ref, got_rt, _h(self.rm)[0], _h(self.rv)[0], got_obs)
        return ref


@pytest.mark.parametrize("cfg", R.POST_CONFIGS, ids=lambda c: "mask%d-atari%d-norm%d-mid%d-%s" % tuple(c))
@pytest.mark.parametrize("n_envs", R.POST_N)
def test_post_plain_matches_reference(n_envs, cfg):
    mask, atari, rewnorm, mid, ret_state = cfg
    run = _PostRun(n_envs, 3, ret_state)
    seen = set()
    for i, s in enumerate(R.post_case(n_envs, 4)):
        ref = run.step(s, "plain", "plain N=%d step %d" % (n_envs, i), mask_returns=mask, use_rewnorm=rewnorm,
                       atari=atari, mid=mid)
        seen.add(float(ref["rstd"]))
    if ret_state != "mid" and rewnorm:
        assert (0.1 if ret_state == "lo" else 100.0) in {round(x, 6) for x in seen}, ("rstd clamp not taken", seen)
    print("K8 plain N=%d %s: ret_rms matched the tracker forms %s" % (n_envs, cfg, sorted(run.forms)))


def test_post_plain_above_1024_blocks():
    """262145 envs = 1025 blocks: the last block sums the partials from global memory (unstaged)."""
    N = R.POST_BIG_N
    run = _PostRun(N, 2, "mid")
    for i, s in enumerate(R.post_case(N, 3)):
        run.step(s, "plain", "plain N=%d step %d" % (N, i))
    print("K8 plain N=%d: ret_rms matched the tracker forms %s" % (N, sorted(run.forms)))


# (form, n_slots, slot_src) run at every (n_envs, obs_dim) of the deferred test
DEFERRED_RUNS = [("deferred", 1, False), ("deferred", 3, False), ("norm", 1, False), ("norm", 3, True),
                 ("norm", 3, False), ("norm", 1, True)]


@pytest.mark.parametrize("obs_dim", [1, 17, 64])
@pytest.mark.parametrize("n_envs", R.POST_N)
def test_post_deferred_forms_match_reference(n_envs, obs_dim):
    steps = R.post_case(n_envs, 7, obs_dim)
    for j, (form, S, slot_src) in enumerate(DEFERRED_RUNS):
        mask, atari, rewnorm, _, ret_state = R.POST_CONFIGS[j % len(R.POST_CONFIGS)]
        run = _PostRun(n_envs, 3, ret_state, obs_dim, S)
        kept = 0
        for i, s in enumerate(steps):
            ref = run.step(s, form, "%s N=%d D=%d S=%d src=%d step %d" % (form, n_envs, obs_dim, S, slot_src, i),
                           mask_returns=mask, use_rewnorm=rewnorm, atari=atari, slot_src=slot_src)
            kept += ref["n_kept"]
        # env 0 kept n_slots + 1 rows by step 1 (S = 1: steps 1, 3) / step 6 (S = 3: steps 1, 3, 4, 6)
        assert kept >= S + 1 and run.st["overflow"] >= 1, (kept, run.st["overflow"])
        assert run.st["slot_t"][(S - 1) * n_envs] == 0, "env 0's reused last slot holds the last truncation's t"


@pytest.mark.parametrize("obs_dim", [1, 15, 16, 17, 33, 64])
@pytest.mark.parametrize("n_envs", [1, 255, 257, 1000])
def test_post_fold_matches_reference(n_envs, obs_dim):
    """xpa_rollout_post_deferred_norm_rms: K8 deferred + normalised with the next observation's obs_rms merge; the rows
    it keeps and boot_norm are normalised with the statistics from BEFORE the merge."""
    steps = R.post_case(n_envs, 7, obs_dim)
    j = (n_envs + obs_dim) % len(R.POST_CONFIGS)
    mask, atari, rewnorm, _, ret_state = R.POST_CONFIGS[j]
    run = _PostRun(n_envs, 3, ret_state, obs_dim, 3, fold=True)
    for i, s in enumerate(steps):
        run.step(s, "fold", "fold N=%d D=%d step %d" % (n_envs, obs_dim, i), mask_returns=mask, use_rewnorm=rewnorm,
                 atari=atari, slot_src=bool(obs_dim % 2))
    assert run.st["overflow"] >= 1


def test_bootstrap_fixup_exact():
    from xuanpolicy_amd import ops
    values, slot_t, buf_term, buf_boot = R.fixup_case()
    N, T, S = R.FIXUP_SHAPE
    assert (slot_t >= 0).any() and (slot_t < 0).any() and buf_term[:, T - 1].any() and not buf_term[:, T - 1].all()
    exp_boot, exp_t = R.bootstrap_fixup_ref(values, slot_t, buf_term, buf_boot)
    d_t, d_boot, d_term = _d(slot_t), _d(buf_boot), _d(buf_term)
    ops.bootstrap_fixup(_d(values), d_t, d_term, d_boot)
    R.check_exact(_h(d_boot), exp_boot, "buf_boot")
    R.check_exact(_h(d_t), exp_t, "slot_t")
    R.check_exact(_h(d_term), buf_term, "buf_term")


# ---------------------------------------------------------------------------------------------- K3
def _sample_launch(dist, head, logstd, v, ptr, step, A):
    from xuanpolicy_amd import ops
    N, T = head.shape[0], R.SAMPLE_T
    cur = _cursor(ptr, step)
    act = torch.full((N, T, A) if dist == "gaussian" else (N, T), SENT, device=DEV)
    logp, val = torch.full((N, T), SENT, device=DEV), torch.full((N, T), SENT, device=DEV)
    env_in = torch.full((N, A + 2), SENT, device=DEV)
    ops.rollout_sample(dist, _d(head), _d(logstd) if logstd is not None else None, _d(v), cur, R.SAMPLE_SEED, act, logp,
                       val, env_in[:, :A], act_clip=1.0)
    assert _cursor_of(cur) == (ptr, int(step) & 0xFFFFFFFF, 0, 0), "K3 must not move the cursor"
    act, logp, val, env_in = _h(act), _h(logp), _h(val), _h(env_in)
    other = [c for c in range(T) if c != ptr]
    for name, b in (("act", act), ("logp", logp), ("val", val)):
        assert (b[:, other] == SENT).all(), (name, "another buffer column was written")
    assert (env_in[:, A:] == SENT).all(), "env_in pad columns written"
    R.check_exact(val[:, ptr], v, "buf_val")
    return act[:, ptr], logp[:, ptr], env_in[:, :A]


@pytest.mark.parametrize("A", R.SAMPLE_A)
@pytest.mark.parametrize("n_envs", R.SAMPLE_N)
def test_sample_gaussian_matches_f64(n_envs, A):
    mu, logstd, v = R.sample_case("gaussian", n_envs, A)
    pool = R.sample_pool_e32("gaussian", A)
    worst = {}
    for ptr, step in R.SAMPLE_CURSORS:
        act, logp, env_in = _sample_launch("gaussian", mu, logstd, v, ptr, step, A)
        act2, logp2, env_in2 = _sample_launch("gaussian", mu, logstd, v, ptr, step, A)
        for a, b, name in ((act, act2, "act"), (logp, logp2, "logp"), (env_in, env_in2, "env_in")):
            R.check_exact(a, b, "repeated launch " + name)
        R.check_exact(env_in, np.fmin(np.fmax(act, F32(-1.0)), F32(1.0)), "env_in = clamp(act)")
        r64 = R.sample_ref("gaussian", mu, logstd, R.SAMPLE_SEED, step, np.float64)
        r32 = R.sample_ref("gaussian", mu, logstd, R.SAMPLE_SEED, step, np.float32)
        what = "gaussian N=%d A=%d ptr=%d step=%#x " % (n_envs, A, ptr, step)
        sets = {"eps": ([R.gauss_eps_of(act, mu, logstd)], [R.gauss_eps_of(r32["act"], mu, logstd)], [r64["eps"]]),
                "act": ([act], [r32["act"]], [r64["act"]]), "logp": ([logp], [r32["logp"]], [r64["logp"]])}
        for name, (got, base, ref) in sets.items():
            w = R.check_within_f32(got, base, ref, what + name, e32_pool=pool[name])
            worst[name] = max(worst.get(name, 0.0), w.ratio)
    print("K3 gaussian N=%d A=%d: worst |err| / E32: %s" % (n_envs, A, {k: round(x, 3) for k, x in worst.items()}))


@pytest.mark.parametrize("K", R.SAMPLE_K)
@pytest.mark.parametrize("n_envs", R.SAMPLE_N)
def test_sample_categorical_matches_f64(n_envs, K):
    z, _, v = R.sample_case("categorical", n_envs, K)
    pool = R.sample_pool_e32("categorical", K)
    worst, left = 0.0, 0
    for ptr, step in R.SAMPLE_CURSORS:
        act, logp, onehot = _sample_launch("categorical", z, None, v, ptr, step, K)
        act2, logp2, onehot2 = _sample_launch("categorical", z, None, v, ptr, step, K)
        R.check_exact(act, act2, "repeated launch act")
        R.check_exact(logp, logp2, "repeated launch logp")
        pick = act.astype(np.int64)
        assert (pick == act).all() and (pick >= 0).all() and (pick < K).all()
        R.check_exact(onehot, np.eye(K, dtype=F32)[pick], "one-hot rows")
        r64 = R.sample_ref("categorical", z, None, R.SAMPLE_SEED, step, np.float64)
        r32 = R.sample_ref("categorical", z, None, R.SAMPLE_SEED, step, np.float32)
        what = "categorical N=%d K=%d ptr=%d step=%#x" % (n_envs, K, ptr, step)
        left += R.check_cat_picks(pick, r64, R.cat_delta(r64, r32, e32_pool=pool["cdf"]), what, cap=R.CAT_CAP)
        rows = np.arange(n_envs)
        w = R.check_within_f32([logp], [r32["logp_all"][rows, pick]], [r64["logp_all"][rows, pick]], what + " logp",
                               e32_pool=pool["logp"])
        worst = max(worst, w.ratio)
    print("K3 categorical N=%d K=%d: worst log-prob |err| / E32 %.3f, envs left out %d of %d"
          % (n_envs, K, worst, left, 4 * n_envs))
