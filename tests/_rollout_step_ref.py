"""Test helper (numpy only, no device needed): plain restatements of the per-step rollout kernels of csrc/rollout.hip —
K5 (RunningMeanStd update, obs_normalize), K8 (the post step in its four forms, bootstrap_fixup) and K3 (the sampler) —
the comparators the GPU tests hold the kernels to, and the deterministic inputs both test modules use.

Every reference takes the kernel's own f32 inputs and f32 / f64 state:

  * rms_update_ref64      statistic_tools.py:86-112 in f64 from the f32 state (two-pass batch variance), unrounded.
  * obs_normalize_ref32   obs_normalize_kernel's arithmetic, one correctly rounded f32 operation after another.
  * post_step_ref         one K8 step of any form: f32 reward scaling, the buffer column, closed / boot, kept slot rows
                          with the overflow rule, boot_norm at the last step, the return tracker in f64, the ret_rms
                          merge in f64 from the finished envs' (count, sum, sumsq) and, for the fold form, the next
                          observation's obs_rms merge (the normalisation uses the OLD statistics).
  * bootstrap_fixup_ref
  * sample_ref            K3 from oracle.synth_env's hash4 / u01 with the kernel's salt and keys, in f64 or in f32
                          (the f32 run is the baseline of the within_f32 bound).

The f32 return tracker feeds ret_rms: an env that finishes contributes its f32 running return R' = fl(gamma R + r).  The
device may form R' with one rounding (a fused multiply-add) or with two; both are f32 evaluations of the same
expression and both satisfy the tracker bound, but the moments of the finished envs differ with them by about an ulp
of R', which is not small against an ulp of a mean near zero.  post_step_ref therefore returns the merged ret_rms
statistics for both (`ret64["fma"]`, `ret64["two"]`) and check_ret_rms accepts the one the stored values match.
"""
import functools

import numpy as np

from oracle.synth_env import hash4, u01

F32, F64 = np.float32, np.float64
SALT_ACT = 0xAC7105ED          # rollout.hip kSaltAct
MARGIN = 4.0                   # tests/_small_ref.py MARGIN
LOG_SQRT_2PI = 0.91893853320467274178


# ---------------------------------------------------------------------------------------------- comparators
def ulp32(x):
    """The spacing of f32 at |x| (x: f64 values)."""
    return np.spacing(np.abs(np.asarray(x, F64)).astype(F32)).astype(F64)


def check_ulp(got32, ref64, what, ulps=1.0):
    """Every stored f32 within `ulps` f32 ulp of the f64 reference value; returns the worst distance in ulps."""
    got, ref = np.asarray(got32), np.asarray(ref64, F64)
    assert got.dtype == F32 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    assert np.isfinite(got).all(), (what, "non-finite")
    d = np.abs(got.astype(F64) - ref) / ulp32(ref)
    worst = float(d.max()) if d.size else 0.0
    assert worst <= ulps, (what, "f32 ulps from the f64 reference", worst, int(np.argmax(d)))
    return worst


def check_exact(got, ref, what):
    """Bit equality (floats are compared as their bit patterns: -0.0 != 0.0, NaN == the same NaN)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    g = got.view(np.uint32) if got.dtype == F32 else got
    r = ref.view(np.uint32) if ref.dtype == F32 else ref
    bad = np.flatnonzero(g.ravel() != r.ravel())
    assert bad.size == 0, (what, "elements differ", int(bad.size), "first", int(bad[0]),
                           got.ravel()[bad[0]], ref.ravel()[bad[0]])


def check_tracker(got32, ref64, gamma_r64, what):
    """|got - ref64| <= 2^-24 (|gamma R| + |ref64|): one rounding of the product and one of the sum, or one fused."""
    got = np.asarray(got32)
    assert got.dtype == F32, what
    err = np.abs(got.astype(F64) - ref64)
    tol = 2.0 ** -24 * (np.abs(gamma_r64) + np.abs(ref64))
    bad = np.flatnonzero(~(err <= tol))
    assert bad.size == 0, (what, int(bad.size), "first", int(bad[0]), float(err[bad[0]]), float(tol[bad[0]]))


def check_ret_rms(got_mean, got_var, got_count, ref, what):
    """ret_rms after a K8 step against post_step_ref's output: untouched bit for bit when no env finished, else the
    count exact and (mean, var) within one f32 ulp of the f64 merge of one of the two f32 trackers.  Returns the
    tracker form matched."""
    assert float(got_count) == ref["ret_count"], (what, "ret_count", float(got_count), ref["ret_count"])
    if ref["n_finished"] == 0:
        check_exact(np.asarray(got_mean, F32).reshape(1), ref["ret_mean_in"].reshape(1), what + " ret_mean untouched")
        check_exact(np.asarray(got_var, F32).reshape(1), ref["ret_var_in"].reshape(1), what + " ret_var untouched")
        return "none"
    errs = {}
    for form, (m64, v64) in ref["ret64"].items():
        try:
            check_ulp(np.asarray(got_mean, F32).reshape(1), np.reshape(m64, 1), what + " ret_mean")
            check_ulp(np.asarray(got_var, F32).reshape(1), np.reshape(v64, 1), what + " ret_var")
            return form
        except AssertionError as e:
            errs[form] = e.args
    raise AssertionError(what, "ret_rms matches the f64 merge under neither f32 tracker", errs)


class Within:
    """tests/_small_ref.py's within_f32 on numpy arrays: pooled E32 = max |base32 - ref64|, scale = max |ref64|;
    every element of got within margin * E32 + 2^-24 * scale of ref64."""

    def __init__(self, got, base32, ref64, margin=MARGIN, e32_pool=0.0):
        f = lambda a: np.asarray(a, F64).ravel()   # noqa: E731
        got, base32, ref64 = [f(a) for a in got], [f(a) for a in base32], [f(a) for a in ref64]
        assert len(got) == len(base32) == len(ref64) > 0
        for g, b, r in zip(got, base32, ref64):
            assert g.shape == b.shape == r.shape, (g.shape, b.shape, r.shape)
        self.e32 = max([float(np.abs(b - r).max()) for b, r in zip(base32, ref64)] + [float(e32_pool)])
        self.scale = max(float(np.abs(r).max()) for r in ref64)
        self.tol = margin * self.e32 + 2.0 ** -24 * self.scale
        errs = [float(np.abs(g - r).max()) if np.isfinite(g).all() else float("inf") for g, r in zip(got, ref64)]
        self.err = max(errs)
        self.bad = [i for i, e in enumerate(errs) if not e <= self.tol]
        self.ok = not self.bad
        self.ratio = self.err / max(self.e32, 1e-300)


def check_within_f32(got, base32, ref64, what, e32_pool=0.0):
    """e32_pool: the baseline's error over a wider pool of the same computation (sample_pool_e32), so that a case of
    one env — one element — cannot make E32 vanish by a lucky rounding."""
    w = Within(got, base32, ref64, e32_pool=e32_pool)
    assert w.ok, (what, "err", w.err, "tol", w.tol, "E32", w.e32, "scale", w.scale, "tensors", w.bad)
    return w


# ---------------------------------------------------------------------------------------------- K5
def rms_update_ref64(mean32, var32, count, x, drop_row=None):
    """RunningMeanStd.update(x) (statistic_tools.py:86-112) in f64 from the f32 state: (mean64, var64, count) before the
    final rounding.  drop_row: a negative control — that row is left out of the sums (the count is not changed)."""
    x = np.asarray(x)
    assert x.dtype == F32 and x.ndim == 2
    n = x.shape[0]
    x64 = x.astype(F64)
    if drop_row is not None:
        x64 = np.delete(x64, drop_row, axis=0)
    m0, v0, c0 = np.asarray(mean32, F32).astype(F64), np.asarray(var32, F32).astype(F64), float(count)
    bm = x64.sum(axis=0) / n
    bvar = np.square(x64 - bm).sum(axis=0) / n
    tot = c0 + n
    delta = bm - m0
    new_mean = m0 + delta * n / tot
    m2 = v0 * c0 + bvar * n + np.square(delta) * c0 * n / tot
    return new_mean, m2 / tot, tot


def obs_normalize_ref32(x, mean, var, clip):
    """obs_normalize_kernel / obs_norm1: sqrtf, + 1e-8f, subtract, divide, fmaxf / fminf, each in f32."""
    x, mean, var = np.asarray(x), np.asarray(mean), np.asarray(var)
    assert x.dtype == F32 and mean.dtype == F32 and var.dtype == F32
    sd = np.sqrt(var)
    y = (x - mean) / (sd + F32(1e-8))
    c = F32(clip)
    y = np.fmin(np.fmax(y, -c), c)
    assert y.dtype == F32
    return y


# ---------------------------------------------------------------------------------------------- K8
def _ret_merge64(m0, v0, c0, rk):
    """ret_rms.update_from_moments over the finished envs' f32 returns rk, in f64 (two-pass variance)."""
    c = float(rk.size)
    r = rk.astype(F64)
    bm = r.sum() / c
    bvar = np.square(r - bm).sum() / c
    tot = c0 + c
    delta = bm - m0
    return m0 + delta * c / tot, (v0 * c0 + bvar * c + delta * delta * c0 * c / tot) / tot


def post_step_ref(state, rew, term, trunc, *, gamma, form="plain", v_boot=None, v_boot_mid=None, mask_returns=True,
                  use_rewnorm=True, rew_range=5.0, atari_lifeloss=False, final_obs=None, slot_src=None, obs_clip=5.0,
                  rms_x=None, wrong_slot_source=False):
    """One K8 step.  form: "plain" (xpa_rollout_post), "deferred" (final_obs arrives normalised), "norm" (the kernel
    normalises final_obs / slot_src with obs_mean / obs_var) or "fold" (norm + the obs_rms merge of rms_x).

    state (numpy, the kernel's values BEFORE the step; not modified): ptr, step (ints), T, ret_mean / ret_var (f32
    scalars), ret_count (float), returns f32 [N]; deferred forms: slot_t int32 [S N], slot_obs f32 [S N, D], overflow
    (int); norm / fold: obs_mean, obs_var f32 [D]; fold: obs_count.

    Returns a dict: the step's buffer column (buf_rew, buf_term f32; buf_closed uint8; buf_boot f32), returns64 /
    gamma_r64 (the f64 tracker and |gamma R| for check_tracker; finished envs' returns64 is 0), done, ptr / step after,
    ret_count, n_finished, ret64 {"fma", "two"} -> (mean64, var64), and by form slot_t / slot_obs / overflow, boot_norm
    (None before the last step), obs_mean64 / obs_var64 / obs_count.
    wrong_slot_source: a negative control — kept rows are taken from the other source."""
    rew = np.asarray(rew)
    assert rew.dtype == F32
    N = rew.shape[0]
    te, tr = np.asarray(term).astype(bool), np.asarray(trunc).astype(bool)
    T, t = int(state["T"]), int(state["ptr"])
    last = t == T - 1
    out = {}
    # reward scaling: rstd and the quotient are single f32 operations
    rstd = np.fmin(np.fmax(np.sqrt(F32(state["ret_var"])), F32(0.1)), F32(100.0))
    if use_rewnorm:
        out["buf_rew"] = np.fmin(np.fmax(rew / rstd, -F32(rew_range)), F32(rew_range)).astype(F32)
    else:
        out["buf_rew"] = rew.copy()
    out["rstd"] = rstd
    out["buf_term"] = te.astype(F32)
    done = te | tr
    close = np.ones(N, bool) if last else (done & ~(bool(atari_lifeloss) & ~tr))
    out["buf_closed"] = close.astype(np.uint8)
    if form == "plain":
        vb = np.asarray(v_boot_mid if (v_boot_mid is not None and not last) else v_boot)
        assert vb.dtype == F32
    else:
        vb = np.zeros(N, F32)
    out["buf_boot"] = np.where(close & ~te, vb, F32(0)).astype(F32)
    # kept truncation rows
    if form != "plain":
        slot_t = np.asarray(state["slot_t"], np.int32).copy()
        slot_obs = np.asarray(state["slot_obs"], F32).copy()
        S, D = slot_t.size // N, slot_obs.shape[1]
        keep = np.flatnonzero(close & ~te & (not last))
        st2 = slot_t.reshape(S, N)
        free = st2[:, keep] < 0
        k = np.where(free.any(axis=0), free.argmax(axis=0), S)
        over = int((k == S).sum())
        k = np.minimum(k, S - 1)       # every slot taken: counted, the last slot is reused
        use_src = (slot_src is not None) != bool(wrong_slot_source)
        src = np.asarray(slot_src if (use_src and slot_src is not None) else final_obs)
        if wrong_slot_source and slot_src is None:
            src = np.roll(src, 1, axis=0)
        rows = src[keep, :D]
        if form in ("norm", "fold"):
            rows = obs_normalize_ref32(rows, state["obs_mean"], state["obs_var"], obs_clip)
        sl = k * N + keep
        slot_t[sl] = t
        slot_obs[sl] = rows
        out.update(slot_t=slot_t, slot_obs=slot_obs, overflow=int(state["overflow"]) + over, n_kept=int(keep.size))
        out["boot_norm"] = None
        if form in ("norm", "fold") and last:
            out["boot_norm"] = obs_normalize_ref32(np.asarray(final_obs)[:, :D], state["obs_mean"], state["obs_var"],
                                                   obs_clip)
    # the return tracker: f64 for the bound, and the two f32 evaluations that can feed ret_rms
    R = np.asarray(state["returns"])
    assert R.dtype == F32
    g32 = F32(gamma)
    gr64 = F64(g32) * R.astype(F64)          # exact in f64: 24 x 24 bits
    if mask_returns:
        gr64 = np.where(te, 0.0, gr64)
    rk64 = gr64 + rew.astype(F64)
    rk_fma = rk64.astype(F32)
    gr32 = (g32 * R).astype(F32)
    if mask_returns:
        gr32 = np.where(te, F32(0), gr32)
    rk_two = (gr32 + rew).astype(F32)
    out["returns64"] = np.where(done, 0.0, rk64)
    out["gamma_r64"] = np.where(done, 0.0, gr64)
    out["done"] = done
    out["n_finished"] = int(done.sum())
    m0, v0, c0 = F64(F32(state["ret_mean"])), F64(F32(state["ret_var"])), float(state["ret_count"])
    out["ret_mean_in"], out["ret_var_in"] = np.asarray(state["ret_mean"], F32), np.asarray(state["ret_var"], F32)
    out["ret_count"] = c0 + float(done.sum()) if done.any() else c0
    out["ret64"] = {}
    if done.any():
        out["ret64"] = {"fma": _ret_merge64(m0, v0, c0, rk_fma[done]), "two": _ret_merge64(m0, v0, c0, rk_two[done])}
    if form == "fold":
        D = np.asarray(state["obs_mean"]).shape[0]
        out["obs_mean64"], out["obs_var64"], out["obs_count"] = rms_update_ref64(
            state["obs_mean"], state["obs_var"], state["obs_count"], np.ascontiguousarray(np.asarray(rms_x)[:, :D]))
    out["ptr"] = (t + 1) % T
    out["step"] = (int(state["step"]) + 1) & 0xFFFFFFFF
    return out


def bootstrap_fixup_ref(values, slot_t, buf_term, buf_boot):
    """bootstrap_fixup_kernel: (buf_boot, slot_t) after — every used slot's value at its (env, t), slots reset to -1,
    then the last column = 0 where the last step was terminal, else V(last-step rows)."""
    boot = np.asarray(buf_boot, F32).copy()
    N, T = boot.shape
    st = np.asarray(slot_t, np.int32).reshape(-1, N)
    S = st.shape[0]
    v = np.asarray(values, F32)
    for k in range(S):        # in slot order: a later slot with the same t overwrites
        n = np.flatnonzero((st[k] >= 0) & (st[k] < T))
        boot[n, st[k, n]] = v[k * N + n]
    boot[:, T - 1] = np.where(np.asarray(buf_term)[:, T - 1] != 0, F32(0), v[S * N:(S + 1) * N])
    return boot, np.full(S * N, -1, np.int32)


# ---------------------------------------------------------------------------------------------- K3
def sample_ref(dist, head, logstd, seed, step, dtype=F64, act_clip=1.0, wrong_key=False):
    """K3 at one (seed, cursor.step): the draws from hash4(seed ^ salt, step, env, key) — keys 2a (u1) and 2a + 1 (u2)
    for Gaussian dimension a, key 0 for Categorical — and the arithmetic of gauss_sample_store_at /
    cat_sample_store_at in `dtype`.  head: the kernel's f32 mu [N, A] or logits [N, K].
    Gaussian: dict(eps, act, logp, u1, u2).  Categorical: dict(u, cdf [N, K], lse, logp_all, pick).
    wrong_key: a negative control — u1 of dimension a keyed with a instead of 2a."""
    head = np.asarray(head)
    assert head.dtype == F32 and head.ndim == 2
    N, A = head.shape
    s = (int(seed) ^ SALT_ACT) & 0xFFFFFFFF
    step = np.uint32(int(step) & 0xFFFFFFFF)
    env = np.arange(N, dtype=np.uint32)
    z = head.astype(dtype)
    if dist == "gaussian":
        a = np.arange(A, dtype=np.uint32)
        k1 = (a if wrong_key else 2 * a)[None, :]
        u1 = F32(1.0) - u01(hash4(s, step, env[:, None], k1))           # (0, 1], exact in f32
        u2 = u01(hash4(s, step, env[:, None], (2 * a + 1)[None, :]))
        two_pi = dtype(6.28318530717958647692)
        eps = np.sqrt(dtype(-2.0) * np.log(u1.astype(dtype))) * np.cos(two_pi * u2.astype(dtype))
        sc = np.exp(np.asarray(logstd, F32).astype(dtype))[None, :]
        x = z + sc * eps
        diff = x - z
        terms = -(diff * diff) / (dtype(2.0) * sc * sc) - np.log(sc) - dtype(LOG_SQRT_2PI)
        logp = np.zeros(N, dtype)
        for j in range(A):        # the kernel's order of accumulation
            logp = logp + terms[:, j]
        assert eps.dtype == dtype and x.dtype == dtype and logp.dtype == dtype
        return dict(eps=eps, act=x, logp=logp, u1=u1, u2=u2)
    assert dist == "categorical"
    m = z.max(axis=1)
    se = np.zeros(N, dtype)
    for k in range(A):
        se = se + np.exp(z[:, k] - m)
    lse = m + np.log(se)
    u = u01(hash4(s, step, env, np.uint32(1 if wrong_key else 0)))
    p = np.exp(z - lse[:, None])
    cdf = np.zeros((N, A), dtype)
    acc = np.zeros(N, dtype)
    for k in range(A):
        acc = acc + p[:, k]
        cdf[:, k] = acc
    below = u.astype(dtype)[:, None] < cdf
    pick = np.where(below.any(axis=1), below.argmax(axis=1), A - 1)
    assert cdf.dtype == dtype and lse.dtype == dtype
    return dict(u=u, cdf=cdf, lse=lse, logp_all=z - lse[:, None], pick=pick)


def gauss_eps_of(act32, mu32, logstd32):
    """The eps a stored f32 action stands for: (x - mu) / exp(logstd) in f64 (|x - mu| is exact or within an ulp of x)."""
    return (np.asarray(act32, F32).astype(F64) - np.asarray(mu32, F32).astype(F64)) / \
        np.exp(np.asarray(logstd32, F32).astype(F64))[None, :]


def cat_delta(ref64, base32, margin=MARGIN, e32_pool=0.0):
    """The distance from a CDF boundary inside which an f32 inverse CDF may pick the neighbour: margin x the f32
    baseline's worst CDF error (never taken from the kernel under test), pooled with e32_pool as in check_within_f32."""
    return margin * max(float(np.abs(base32["cdf"].astype(F64) - ref64["cdf"]).max()), float(e32_pool))


def cat_near(ref64, delta):
    """near [N, K - 1]: the uniform lies within delta of boundary k (the last boundary, 1, decides nothing)."""
    u = ref64["u"].astype(F64)[:, None]
    return np.abs(u - ref64["cdf"][:, :-1]) < delta


def check_cat_picks(pick, ref64, delta, what, cap=0.01):
    """The kernel's picks against the f64 inverse CDF: equal wherever the uniform is at least delta from every boundary;
    elsewhere one of the two actions beside a near boundary; at most `cap` of the envs are left out.  Returns the
    number left out."""
    pick = np.asarray(pick)
    N, K = ref64["cdf"].shape
    assert pick.shape == (N,)
    near = cat_near(ref64, delta)
    out = near.any(axis=1)
    assert out.sum() <= cap * N, (what, "envs left out", int(out.sum()), N)
    bad = np.flatnonzero(~out & (pick != ref64["pick"]))
    assert bad.size == 0, (what, "picks differ from the f64 inverse CDF", int(bad.size), "first env", int(bad[0]),
                           int(pick[bad[0]]), int(ref64["pick"][bad[0]]))
    for n in np.flatnonzero(out):
        b = np.flatnonzero(near[n])
        allowed = set(b.tolist()) | set((b + 1).tolist()) | {int(ref64["pick"][n])}
        assert int(pick[n]) in allowed, (what, "env", int(n), "pick", int(pick[n]), "allowed", sorted(allowed))
    return int(out.sum())


# ---------------------------------------------------------------------------------------------- the cases
# K5: (n, dim) -> the branch it is there for
RMS_SHAPES = [
    (1, 1),         # the smallest case: one row, one column, 255 idle threads
    (255, 3),       # 85 row groups of 3 columns, thread 255 idle
    (256, 4),       # exactly one full row block
    (257, 6),       # the second row block holds one row; 256 / 6 not integral
    (300, 64),      # the last width of the 1-D kernel
    (300, 65),      # the first width of the 2-D kernel; the second column block holds one column
    (513, 128),     # the 2-D kernel over three row blocks, the last of one row
    (4096, 64),     # np * dim * 2 == 2048: the merge's LDS staging limit
    (4097, 64),     # one more partial: the unstaged merge
    (1000, 376),    # C4's width
]
RMS_FAR_SHAPES = [(257, 6), (300, 65)]      # the far-shift batch through the 1-D and the 2-D kernel
RMS_PAD = 3


def rms_case(n, dim, far=False):
    """Three batches [n, dim + RMS_PAD] (pad columns NaN) of rescaled, re-centred data.  far: the first batch sits
    ~1e3 batch standard deviations from the initial running mean (0)."""
    rng = np.random.default_rng(1000 * n + dim + (7 if far else 0))
    base = rng.normal(0.0, 1.0, (n, dim))
    off = rng.uniform(0.5, 3.0, dim) * rng.choice([-1.0, 1.0], dim)
    out = []
    for k, (scale, shift) in enumerate([(3.0, 1.0), (0.25, -2.0), (11.0, 0.5)]):
        if far and k == 0:
            scale, shift = 1.0, 1000.0 / np.maximum(np.abs(off), 1e-9)
        X = np.full((n, dim + RMS_PAD), np.nan, F32)
        X[:, :dim] = (base * scale + off * shift).astype(F32)
        out.append(X)
        base = rng.normal(0.0, 1.0, (n, dim))
    return out


def rms_initial(dim):
    return np.zeros(dim, F32), np.ones(dim, F32), 1e-4


def normalize_case(n, dim, pad=2):
    """x [n, dim + pad] (NaN pads), mean, var, clip: var[0] = 0 (x / 1e-8 clips either way or is exactly 0), and values
    beyond both clip edges in every column."""
    rng = np.random.default_rng(77 * n + dim)
    X = np.full((n, dim + pad), np.nan, F32)
    X[:, :dim] = rng.normal(0.5, 4.0, (n, dim)).astype(F32)
    mean = rng.normal(0.5, 0.5, dim).astype(F32)
    var = rng.uniform(0.3, 3.0, dim).astype(F32)
    var[0] = 0.0
    X[0, :dim] = mean + F32(100.0)
    if n > 1:
        X[1, :dim] = mean - F32(100.0)
    if n > 2:
        X[2, 0] = mean[0]          # (x - mean) = 0 over sqrt(0) + 1e-8: exactly 0
    return X, mean, var, 5.0


# K8: the ret_rms state a run starts from -> which rstd clamp its steps take
RET_STATES = {"mid": (0.3, 2.0, 17.0), "lo": (0.01, 1e-4, 1e5), "hi": (5.0, 1e6, 1e5)}
POST_N = [1, 255, 256, 257, 1000]
POST_BIG_N = 262145                      # 1025 blocks: the unstaged partial sum
# (mask_returns, atari_lifeloss, use_rewnorm, v_boot_mid, ret state)
POST_CONFIGS = [(True, False, True, False, "mid"), (False, False, True, True, "lo"), (True, True, True, False, "hi"),
                (False, True, False, True, "mid")]
POST_GAMMA = 0.99


def post_case(n_envs, n_steps, obs_dim=0, seed=0, pad=3):
    """The steps of a K8 run (horizon 3): step 0 finishes no env; step 1 finishes every env (term, trunc or both in
    turn; env 0 trunc only); from step 1 on env 0 truncates at every step (with horizon 3 and n_slots slots that is
    n_slots + 1 kept rows by step 1 / step 6) and has term and trunc both set at step 5 (a last step); the other envs
    finish at random.  One reward per step lies beyond rew_range.  obs_dim > 0: final_obs / slot_src / rms_x [N, D + pad]
    with NaN pads, re-centred every step so that the fold's statistics move."""
    rng = np.random.default_rng(31 * n_envs + 7 * n_steps + obs_dim + 1000 * seed)
    steps = []
    N = n_envs
    for i in range(n_steps):
        s = dict(rew=rng.normal(0.2, 2.0, N).astype(F32), v_boot=rng.normal(0, 1, N).astype(F32),
                 v_boot_mid=rng.normal(0, 1, N).astype(F32))
        s["rew"][(3 * i) % N] = F32(1000.0 if i % 2 else -1000.0)
        if i == 0:
            te, tr = np.zeros(N, bool), np.zeros(N, bool)
        elif i == 1:
            kind = np.arange(N) % 3
            te, tr = kind != 1, kind != 0          # 0: term, 1: trunc, 2: both
            te[0], tr[0] = False, True
        else:
            te, tr = rng.random(N) < 0.2, rng.random(N) < 0.3
            te[0], tr[0] = (i == 5), True
        s["term"], s["trunc"] = te.astype(np.uint8), tr.astype(np.uint8)
        if obs_dim:
            for name, loc in (("final_obs", 0.3 * i), ("slot_src", -0.2 * i), ("rms_x", 1.0 + 0.7 * i)):
                X = np.full((N, obs_dim + pad), np.nan, F32)
                X[:, :obs_dim] = rng.normal(loc, 1.0 + 0.5 * i, (N, obs_dim)).astype(F32)
                s[name] = X
        steps.append(s)
    return steps


def post_initial(n_envs, horizon, ret_state, obs_dim=0, n_slots=0, seed=0):
    rng = np.random.default_rng(5 + n_envs + seed)
    m, v, c = RET_STATES[ret_state]
    st = dict(T=horizon, ptr=0, step=0xFFFFFFFE, ret_mean=F32(m), ret_var=F32(v), ret_count=float(c),
              returns=rng.normal(0.5, 1.5, n_envs).astype(F32))
    if n_slots:
        st.update(slot_t=np.full(n_slots * n_envs, -1, np.int32), slot_obs=np.full((n_slots * n_envs, obs_dim), -7.0, F32),
                  overflow=0)
    if obs_dim:
        st.update(obs_mean=rng.normal(0, 0.3, obs_dim).astype(F32), obs_var=rng.uniform(0.5, 2.0, obs_dim).astype(F32),
                  obs_count=37.0)
    return st


def post_advance(state, out, got_returns, got_ret_mean, got_ret_var, got_obs=None):
    """The state the next step's reference starts from: the reference's exact outputs and the KERNEL's rounded
    statistics and returns (each reference step takes the kernel's own f32 state)."""
    st = dict(state)
    st.update(ptr=out["ptr"], step=out["step"], ret_count=out["ret_count"], returns=np.asarray(got_returns, F32).copy(),
              ret_mean=F32(got_ret_mean), ret_var=F32(got_ret_var))
    if "slot_t" in out:
        st.update(slot_t=out["slot_t"], slot_obs=out["slot_obs"], overflow=out["overflow"])
    if got_obs is not None:
        st.update(obs_mean=np.asarray(got_obs[0], F32).copy(), obs_var=np.asarray(got_obs[1], F32).copy(),
                  obs_count=out["obs_count"])
    return st


FIXUP_SHAPE = (257, 4, 2)     # envs, horizon, slots


def fixup_case():
    N, T, S = FIXUP_SHAPE
    rng = np.random.default_rng(12)
    slot_t = np.where(rng.random(S * N) < 0.5, rng.integers(0, T - 1, S * N), -1).astype(np.int32)
    slot_t[3] = T            # out of range: ignored, still reset
    values = rng.normal(0, 1, (S + 1) * N).astype(F32)
    buf_term = (rng.random((N, T)) < 0.3).astype(F32)
    buf_boot = rng.normal(0, 1, (N, T)).astype(F32)
    return values, slot_t, buf_term, buf_boot


# K3
SAMPLE_N = [1, 255, 257, 4099]
SAMPLE_A = [1, 6, 17]
SAMPLE_K = [2, 3, 18]
SAMPLE_T = 3
SAMPLE_CURSORS = [(0, 5), (SAMPLE_T - 1, 0x80000123), (0, 0xFFFFFFFF), (SAMPLE_T - 1, 77)]   # (ptr, step)
SAMPLE_SEED = 0x9E3779B9
CAT_CAP = 0.01


def sample_case(dist, n_envs, a):
    """head f32 [N, a], logstd f32 [a] (None for Categorical), v f32 [N].  Categorical: row 0 has equal logits and row 1
    a dominant one (+80) wherever those rows exist."""
    rng = np.random.default_rng(100 * n_envs + a + (0 if dist == "gaussian" else 50))
    v = rng.normal(0, 1, n_envs).astype(F32)
    if dist == "gaussian":
        return rng.normal(0, 0.7, (n_envs, a)).astype(F32), rng.uniform(-1.5, 0.4, a).astype(F32), v
    z = rng.normal(0, 1.5, (n_envs, a)).astype(F32)
    if n_envs > 1:
        z[0] = F32(0.37)
        z[1, a // 2] += F32(80.0)
    return z, None, v


@functools.lru_cache(maxsize=None)
def sample_pool_e32(dist, a):
    """The f32 baseline's worst error against the f64 restatement, per quantity, over EVERY case of this width (all of
    SAMPLE_N x SAMPLE_CURSORS): E32 is a property of f32 arithmetic at these inputs' scale, and the one-env cases have
    1 .. 17 elements, too few to show it (a single lucky rounding of the log-sum-exp gave E32 = 0.2 ulp).  Computed
    from the references alone."""
    e = {}

    def put(name, b, r):
        e[name] = max(e.get(name, 0.0), float(np.abs(np.asarray(b, F64) - r).max()))
    for n in SAMPLE_N:
        head, logstd, _ = sample_case(dist, n, a)
        for _, step in SAMPLE_CURSORS:
            r64 = sample_ref(dist, head, logstd, SAMPLE_SEED, step, F64)
            r32 = sample_ref(dist, head, logstd, SAMPLE_SEED, step, F32)
            if dist == "gaussian":
                put("eps", gauss_eps_of(r32["act"], head, logstd), r64["eps"])
                put("act", r32["act"], r64["act"])
                put("logp", r32["logp"], r64["logp"])
            else:
                put("cdf", r32["cdf"], r64["cdf"])
                # without the dominant-logit row: its unpicked log-probs are ~ -80 and carry an ulp of 80
                rows = np.arange(n) != (1 if n > 1 else -1)
                put("logp", r32["logp_all"][rows], r64["logp_all"][rows])
    return e
