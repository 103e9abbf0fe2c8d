"""GPU: K9 (csrc/optim.hip: global-norm clip + Adam over flat buffers) against torch f64 at every launch geometry and
through every entry point, and FusedClipAdam's host side (flat.py).

tests/test_gpu_kernels.py's test_fused_clip_adam_matches_torch stays as it is: it covers FusedClipAdam.step() on an
832-parameter net for six chained updates against torch's f32 Adam (rtol 1e-5 / 1e-4), with state_dict() describing the
moments.  That is one block in both kernels, no grid-stride trip, no n % 4 tail, one entry point.  This module covers
the rest:

  A1. xpa_clip_adam_step, _partials and _sched called through the C ABI on plain tensors at n = 1, 3, 4, 7 (tails),
      1027 (two norm blocks + tail), 524288 + 5 (past the norm pass's 512-block cap) and 2097152 + 1029 (past the Adam
      pass's 2048-block cap); max_norm none / 0.5 (active) / 1e9 (inactive) / 0.0; Adam steps 1, 2, 3, 300, 100000.
  A2. The scheduled form's cursor: ticket logic at 1, several and 2048 blocks, the clamp-and-flag overflow, and one
      captured launch replayed with the cursor advancing on the device.
  A3. Negative controls on the reference side (step + 1; the clip coefficient applied twice) and the argument checks.
  A4. FusedClipAdam: scheduled stepping against host-argument stepping, ensure_window's invalidation rules and `need`,
      and optimizer.load_state_dict() (the post hook in flat.py; without it the kernels went on from the old moments).

Reference, baseline, bound (tests/_small_ref.py, nothing fitted here): clip_adam_ref in f64 on the device is the
reference, the same function in f32 on the device the baseline (A4's state round trip: torch's own clip_grad_norm_ +
Adam), within_f32 with MARGIN the bound, pooled per set: the parameter step p_new - p_old (formed exactly, in f64), exp_avg,
exp_avg_sq and the clipped gradient K9 writes back.  total_norm_out is held to the f64 norm at 1e-5 (the K30 tail
test's).  Forms that share arithmetic are held to bit equality.  Reference and baseline get the betas the kernel
receives, f32(0.9) and f32(0.999) (tests/test_gpu_small_envelope.py's docstring: they cross the ABI as `float`).

Each comparison is ONE step from a common f32 state: the kernel's output is the start of the next step for kernel,
baseline and reference alike, so errors do not compound and a failure names its step.  Below 64 elements a case runs
ceil(64 / n) independent launches of that n and pools them (within_f32's own reason for pooling: a one-element set
can make the baseline's error vanish by luck).

Measured on an MI355X, the largest printed |err| / E32 per set (the margin is 4 everywhere; nothing needed more):
  test_k9_entry_points_match_f64        step 2.14 (n 2097152 + 1029, max_norm 0.0, step 1), exp_avg 1.48 (n 3, 0.5),
                                        exp_avg_sq 2.16 (n 4, none, step 3), grad 1.17 (n 3, 0.5); most cases print
                                        1.0 (K9's worst element is the baseline's); total_norm within 5.8e-8 (relative)
                                        of the f64 norm at every size, exactly equal at n = 1
  test_k9_partials_resplit_matches_f64  step 1.54, exp_avg 1.0, exp_avg_sq 1.0, grad 1.13; total_norm within 3.9e-8
  test_fused_adam_takes_a_loaded_optimizer_state   step 1.0, exp_avg 1.0, exp_avg_sq 1.0, grad 1.0 (both forms); on
                                        flat.py without the load hook the step set is 8.6e4 (host arguments) and 8.2e4
                                        (scheduled) x E32 off, in all four parameter tensors
  test_the_checker_rejects_k9_against_wrong_references   past the bound by a factor of 2.5e3 (step 2 held to step 3), 47
                                        (step 300 to 301), and 574 / 7.0e4 / 701 / 1.8e7 (step, exp_avg, exp_avg_sq,
                                        grad) with the clip coefficient applied twice
No kernel defect was found: every bit-equality between the forms held, at every size.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import _small_ref as sr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

B1, B2 = float(np.float32(0.9)), float(np.float32(0.999))   # the betas as they cross the C ABI
LR, EPS = 4e-4, 1e-5
SETS = ("step", "exp_avg", "exp_avg_sq", "grad")
NORM_CAP = 512 * 256 * 4      # optim.hip: kMaxNormBlocks x kOptThreads x 4 floats
ADAM_CAP = 2048 * 256 * 4     # optim.hip: the Adam pass's 2048-block cap
SIZES = (1, 3, 4, 7, 1027, NORM_CAP + 5, ADAM_CAP + 1029)
MAX_NORMS = (-1.0, 0.5, 1e9, 0.0)
STEPS = (1, 2, 3, 300, 100000)


@pytest.fixture(scope="module", autouse=True)
def _setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from xuanpolicy_amd import ops
    ops.lib()


# ---- the entry points on plain tensors ------------------------------------------------------------------------------------
def _L():
    from xuanpolicy_amd import ops
    return ops.lib()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _n_partials(n):
    return int(_L().xpa_grad_norm_num_partials(n))


def k9_host(st, partials, max_norm, lr, step, norm_out, n=None):
    from xuanpolicy_amd import _lib
    p, g, m, v = st
    _lib.call(_L().xpa_clip_adam_step, _ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel() if n is None else n, _ptr(partials),
              max_norm, lr, B1, B2, EPS, step, _ptr(norm_out), _stream())


def k9_partials(st, sq, n_sq, max_norm, lr, step, norm_out, n=None):
    from xuanpolicy_amd import _lib
    p, g, m, v = st
    _lib.call(_L().xpa_clip_adam_step_partials, _ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel() if n is None else n,
              _ptr(sq), n_sq, max_norm, lr, B1, B2, EPS, step, _ptr(norm_out), _stream())


def k9_sched(st, partials, max_norm, sched, n_sched, cursor, norm_out, n=None):
    from xuanpolicy_amd import _lib
    p, g, m, v = st
    _lib.call(_L().xpa_clip_adam_step_sched, _ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel() if n is None else n,
              _ptr(partials), max_norm, B1, B2, EPS, _ptr(sched), n_sched, _ptr(cursor), _ptr(norm_out), _stream())


def sched_table(entries):
    """The device table of [(lr, step), ...], each entry made by xpa_adam_sched_entry."""
    out2 = (ctypes.c_float * 2)()
    vals = []
    for lr, step in entries:
        _L().xpa_adam_sched_entry(lr, B1, B2, step, ctypes.addressof(out2))
        vals += [out2[0], out2[1]]
    return torch.tensor(vals, dtype=torch.float32, device=DEV)


# ---- states, gradients, the reference -----------------------------------------------------------------------------------
def _zero_run(n):
    """The 64-element run with p = g = m = v = 0 (FlatState's padding, flat.py), off every 4- and 256-element boundary;
    None below 128 elements."""
    return None if n < 128 else slice(n // 2 + 1, n // 2 + 65)


def fresh_grad(n, gen, max_norm):
    """Random, every 11th element exactly 0, the zero run 0; for max_norm 0.5 scaled to norm 3 so the clip is active."""
    g = torch.randn(n, device=DEV, generator=gen) * 0.1
    g[10::11] = 0.0
    if _zero_run(n) is not None:
        g[_zero_run(n)] = 0.0
    if max_norm == 0.5:
        g *= 3.0 / float(g.double().norm())
    return g


def fresh_state(n, gen, max_norm, moments=False):
    """(p, g, m, v): p ~ 0.1 N(0, 1); zero moments (an optimizer's first step) unless `moments`."""
    p = torch.randn(n, device=DEV, generator=gen) * 0.1
    m = torch.randn(n, device=DEV, generator=gen) * 0.05 if moments else torch.zeros(n, device=DEV)
    v = torch.rand(n, device=DEV, generator=gen) * 1e-2 if moments else torch.zeros(n, device=DEV)
    if _zero_run(n) is not None:
        for t in (p, m, v):
            t[_zero_run(n)] = 0.0
    return [p, fresh_grad(n, gen, max_norm), m, v]


def clone(st):
    return [t.clone() for t in st]


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def clipped(g, norm, max_norm):
    """clip_grad_norm_'s in-place result, in g's dtype (clip_adam_ref's coefficient, which it does not return)."""
    if max_norm < 0:
        return g.clone()
    return g * torch.clamp(max_norm / (norm + 1e-6), max=1.0)


def reference(st, step, lr, max_norm, dtype, coef_twice=False):
    """clip_adam_ref on one (p, g, m, v) in `dtype` on the device: {set: tensor} and the pre-clip norm.  The step is
    formed in f64 from the rounded new parameter, exactly.  coef_twice: clip_adam_ref's negative control; the gradient
    such a kernel would write back is clipped a second time as well."""
    p, g, m, v = (t.to(dtype) for t in st)
    P, M, V, norm = sr.clip_adam_ref([p], [g], [m], [v], step, lr, max_norm, (B1, B2), EPS, coef_twice=coef_twice)
    grad = clipped(g, norm, max_norm)
    return {"step": P[0].double() - p.double(), "exp_avg": M[0], "exp_avg_sq": V[0],
            "grad": clipped(grad, norm, max_norm) if coef_twice else grad}, norm


def kernel_sets(before, after):
    return {"step": after[0].double() - before[0].double(), "exp_avg": after[2], "exp_avg_sq": after[3],
            "grad": after[1]}


def check_sets(tag, befores, afters, step, lr, max_norm, worst=None, **kw):
    """within_f32 per set, pooled over the replicas of one case; prints each ratio; returns {set: Bound}."""
    got = [kernel_sets(b, a) for b, a in zip(befores, afters)]
    base = [reference(b, step, lr, max_norm, torch.float32, **kw)[0] for b in befores]
    ref = [reference(b, step, lr, max_norm, torch.float64, **kw)[0] for b in befores]
    out = {}
    for name in SETS:
        res = sr.within_f32([x[name] for x in got], [x[name] for x in base], [x[name] for x in ref])
        print("%s %s: worst |err| / E32 %.3g (E32 %.3g, scale %.3g)" % (tag, name, res.ratio, res.e32, res.scale))
        out[name] = res
        if worst is not None:
            worst[name] = max(worst.get(name, 0.0), res.ratio)
    return out


def check_norm(tag, norm_out, st, worst=None):
    want = float(st[1].double().norm())
    got = float(norm_out)
    dev = abs(got - want) / max(want, 1e-300)
    print("%s total_norm: %.9g against f64 %.9g (relative deviation %.3g)" % (tag, got, want, dev))
    np.testing.assert_allclose(got, want, rtol=1e-5, err_msg=tag)
    if worst is not None:
        worst["total_norm"] = max(worst.get("total_norm", 0.0), dev)


def check_zero_run(tag, st):
    run = _zero_run(st[0].numel())
    if run is not None:
        for name, t in zip("pgmv", st):
            assert int(t[run].view(torch.int32).abs().max()) == 0, (tag, name)


# ---- A1. the three entry points against f64 ----------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", MAX_NORMS, ids=["none", "0.5", "1e9", "0.0"])
@pytest.mark.parametrize("n", SIZES)
def test_k9_entry_points_match_f64(n, max_norm):
    """Steps 1, 2, 3, 300 and 100000 with the carried moments and a fresh gradient per step, lr 4e-4, eps 1e-5.  Per
    step, from one common state: xpa_clip_adam_step within the bound of f64 on all four sets and its norm within 1e-5;
    _partials fed the partials that launch left behind, and _sched fed xpa_adam_sched_entry's entry, equal it bit for
    bit (all four buffers and the norm); the zero run stays bitwise zero.  max_norm 0.0 starts from non-zero moments:
    g becomes exactly 0, m and v decay, p moves by the decayed m."""
    reps = 1 if n >= 64 else -(-64 // n)
    gen = torch.Generator(device=DEV).manual_seed(9000 + n)
    states = [fresh_state(n, gen, max_norm, moments=(max_norm == 0.0)) for _ in range(reps)]
    nb = _n_partials(n)
    assert nb == min(512, max(1, -(-(n // 4) // 256)))
    worst = {}
    for step in STEPS:
        tag = "n %d max_norm %g step %d" % (n, max_norm, step)
        afters = []
        for st in states:
            host, part, sch = clone(st), clone(st), clone(st)
            partials = torch.full((nb,), float("nan"), dtype=torch.float64, device=DEV)
            norms = torch.full((3,), float("nan"), device=DEV)
            k9_host(host, partials, max_norm, LR, step, norms[0:1])
            k9_partials(part, partials.clone(), nb, max_norm, LR, step, norms[1:2])
            cursor = torch.zeros(4, dtype=torch.int32, device=DEV)
            k9_sched(sch, torch.empty_like(partials), max_norm, sched_table([(LR, step)]), 1, cursor, norms[2:3])
            assert same_bits(host, part) and same_bits(host, sch), tag
            assert same_bits([norms[0:1]], [norms[1:2]]) and same_bits([norms[0:1]], [norms[2:3]]), tag
            assert cursor.tolist() == [1, 0, 0, 0], tag
            check_norm(tag, norms[0], st, worst)
            check_zero_run(tag, host)
            afters.append(host)
        res = check_sets(tag, states, afters, step, LR, max_norm, worst)
        for name in SETS:
            assert res[name].ok, (tag, name, res[name])
        for st, after in zip(states, afters):
            want_norm = float(st[1].double().norm())
            if max_norm == 0.5:
                assert want_norm > 2.9 and not torch.equal(after[1], st[1]), tag      # the clip is active
            elif max_norm == 0.0:
                assert torch.equal(after[1], torch.zeros_like(after[1])), tag        # g is exactly 0 ...
                assert float(st[2].abs().max()) > 0 and float(st[3].max()) > 0, tag   # ... and the moments were not
                assert float((after[0] - st[0]).abs().max()) > 0, tag
            else:
                assert same_bits([after[1]], [st[1]]), tag                            # no clip: g untouched
        states = [[a[0], fresh_grad(n, gen, max_norm), a[2], a[3]] for a in afters]
    print("n %d max_norm %g: worst %s" % (n, max_norm, ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("n_sq", [1, 7, 64, 65, 1000])
@pytest.mark.parametrize("n", [7, 1027, NORM_CAP + 5])
def test_k9_partials_resplit_matches_f64(n, n_sq):
    """xpa_clip_adam_step_partials fed |g|^2 (f64) re-split into n_sq partials (the kernel re-reduces them with 64 lanes:
    fewer than, exactly, one more than and many times a wave): within the bound on all four sets, the norm within
    1e-5.  Step 2 from non-zero moments, max_norm 0.5 active."""
    reps = 1 if n >= 64 else -(-64 // n)
    gen = torch.Generator(device=DEV).manual_seed(100 * n_sq + n % 97)
    states = [fresh_state(n, gen, 0.5, moments=True) for _ in range(reps)]
    tag = "n %d n_sq %d" % (n, n_sq)
    afters = []
    for st in states:
        w = torch.rand(n_sq, dtype=torch.float64, device=DEV, generator=gen) + 0.01
        sq = (st[1].double() ** 2).sum() * (w / w.sum())
        assert abs(float(sq.sum()) / float((st[1].double() ** 2).sum()) - 1.0) < 1e-14
        after, norm = clone(st), torch.full((1,), float("nan"), device=DEV)
        k9_partials(after, sq, n_sq, 0.5, LR, 2, norm)
        check_norm(tag, norm[0], st)
        check_zero_run(tag, after)
        afters.append(after)
    res = check_sets(tag, states, afters, 2, LR, 0.5)
    for name in SETS:
        assert res[name].ok, (tag, name, res[name])


# ---- A2. the cursor -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 1027 * 4, ADAM_CAP + 1029], ids=["1-block", "5-blocks", "2048-blocks"])
def test_k9_sched_cursor_and_overflow(n):
    """A 3-entry table, five launches with fresh gradients: launches 0-2 equal xpa_clip_adam_step with entries 0-2 bit for
    bit, launches 3 and 4 use entry 2 (the clamp) and raise cursor[2]; after launch k cursor[0] == k + 1 and the block
    ticket cursor[1] is back at 0."""
    entries = [(4e-4, 1), (3e-4, 2), (1e-4, 300)]
    table = sched_table(entries)
    assert min(2048, max(1, -(-(n // 4) // 256))) == {7: 1, 4108: 5, ADAM_CAP + 1029: 2048}[n]
    gen = torch.Generator(device=DEV).manual_seed(77 + n)
    st = fresh_state(n, gen, 0.5)
    twin = clone(st)
    nb = _n_partials(n)
    partials, partials_t = (torch.zeros(nb, dtype=torch.float64, device=DEV) for _ in range(2))
    cursor = torch.zeros(4, dtype=torch.int32, device=DEV)
    norms = torch.zeros(2, device=DEV)
    for k in range(5):
        if k:
            st[1] = fresh_grad(n, gen, 0.5)
            twin[1] = st[1].clone()
        lr, step = entries[min(k, 2)]
        k9_sched(st, partials, 0.5, table, 3, cursor, norms[0:1])
        k9_host(twin, partials_t, 0.5, lr, step, norms[1:2])
        assert same_bits(st, twin) and same_bits([norms[0:1]], [norms[1:2]]), (n, k)
        assert cursor.tolist() == [k + 1, 0, 1 if k >= 3 else 0, 0], (n, k, cursor.tolist())


def test_k9_sched_captured_replays_advance_the_cursor():
    """One scheduled launch captured (xuanpolicy_amd.graphs.capture) after an eager warm-up launch, replayed four times
    with the gradient buffer rewritten in between: every replay equals the eager host-argument twin bit for bit and the
    cursor advances by one per replay.  The graph is the norm pass followed by the Adam pass: one chain."""
    from xuanpolicy_amd import graphs
    n = 1027 * 4
    entries = [(4e-4 * (1.0 - 0.1 * k), k + 1) for k in range(8)]
    table = sched_table(entries)
    gen = torch.Generator(device=DEV).manual_seed(5)
    st = fresh_state(n, gen, 0.5)
    twin = clone(st)
    nb = _n_partials(n)
    partials, partials_t = (torch.zeros(nb, dtype=torch.float64, device=DEV) for _ in range(2))
    cursor = torch.zeros(4, dtype=torch.int32, device=DEV)
    norms = torch.zeros(2, device=DEV)

    def launch():
        k9_sched(st, partials, 0.5, table, 8, cursor, norms[0:1])
    launch()                                                   # eager warm-up: entry 0
    k9_host(twin, partials_t, 0.5, *entries[0], norms[1:2])
    torch.cuda.synchronize()
    assert same_bits(st, twin) and cursor.tolist() == [1, 0, 0, 0]
    graph, _ = graphs.capture(launch)
    torch.cuda.synchronize()
    assert same_bits(st, twin) and cursor.tolist() == [1, 0, 0, 0]   # recorded, not executed
    for k in range(1, 5):
        new_g = fresh_grad(n, gen, 0.5)
        st[1].copy_(new_g)                                     # the captured pointer
        twin[1] = new_g.clone()
        graph.replay()
        k9_host(twin, partials_t, 0.5, *entries[k], norms[1:2])
        torch.cuda.synchronize()
        assert same_bits(st, twin) and same_bits([norms[0:1]], [norms[1:2]]), k
        assert cursor.tolist() == [k + 1, 0, 0, 0], (k, cursor.tolist())


# ---- A3. negative controls and rejections ------------------------------------------------------------------------------
def _factor(res):
    """How far past the bound the worst element of a within_f32 result is."""
    return res.ratio * res.e32 / (sr.MARGIN * res.e32 + 2.0 ** -24 * res.scale)


def test_the_checker_rejects_k9_against_wrong_references():
    """The kernel is not modified; the reference side (f64 reference and f32 baseline alike) is.  K9's output at step 2
    and at step 300 passes against clip_adam_ref at that step and is rejected against it at step + 1 (the bias
    corrections: only the parameter step depends on them), and at step 2 against a reference whose clip coefficient is
    applied twice (every set)."""
    n = 1027
    gen = torch.Generator(device=DEV).manual_seed(31)
    st = fresh_state(n, gen, 0.5, moments=True)
    partials = torch.zeros(_n_partials(n), dtype=torch.float64, device=DEV)
    norm = torch.zeros(1, device=DEV)
    for step in (2, 300):
        after = clone(st)
        k9_host(after, partials, 0.5, LR, step, norm)
        good = check_sets("control step %d, right reference" % step, [st], [after], step, LR, 0.5)
        assert all(good[name].ok for name in SETS), good
        wrong = check_sets("control step %d against step %d" % (step, step + 1), [st], [after], step + 1, LR, 0.5)
        print("control step %d against step %d: the parameter step is %.3g x the bound off" %
              (step, step + 1, _factor(wrong["step"])))
        assert not wrong["step"].ok and _factor(wrong["step"]) > 10, (step, wrong["step"])
        assert all(wrong[name].ok for name in ("exp_avg", "exp_avg_sq", "grad")), wrong   # they do not depend on step
    after = clone(st)
    k9_host(after, partials, 0.5, LR, 2, norm)
    wrong = check_sets("control coefficient twice", [st], [after], 2, LR, 0.5, coef_twice=True)
    for name in SETS:
        print("control coefficient twice: %s is %.3g x the bound off" % (name, _factor(wrong[name])))
        assert not wrong[name].ok and _factor(wrong[name]) > 10, (name, wrong[name])


def test_k9_rejects_bad_arguments():
    """n <= 0, step < 1, a parameter / gradient / moment pointer 4 bytes off 16-B alignment, n_sq <= 0, n_sched <= 0, a
    null schedule or cursor: every call returns an error and launches nothing (the buffers keep their bits)."""
    from xuanpolicy_amd import _lib
    n = 64
    gen = torch.Generator(device=DEV).manual_seed(1)
    big = [torch.randn(n + 4, device=DEV, generator=gen).abs() for _ in range(4)]
    st = [t[:n] for t in big]
    keep = clone(big)
    partials = torch.full((1,), 3.0, dtype=torch.float64, device=DEV)
    norm = torch.full((1,), -7.0, device=DEV)
    table = sched_table([(LR, 1)])
    cursor = torch.zeros(4, dtype=torch.int32, device=DEV)
    bad = {}
    for nn in (0, -4):
        bad["n %d" % nn] = lambda nn=nn: k9_host(st, partials, 0.5, LR, 1, norm, n=nn)
        bad["n %d, partials" % nn] = lambda nn=nn: k9_partials(st, partials, 1, 0.5, LR, 1, norm, n=nn)
        bad["n %d, sched" % nn] = lambda nn=nn: k9_sched(st, partials, 0.5, table, 1, cursor, norm, n=nn)
    for step in (0, -1):
        bad["step %d" % step] = lambda step=step: k9_host(st, partials, 0.5, LR, step, norm)
        bad["step %d, partials" % step] = lambda step=step: k9_partials(st, partials, 1, 0.5, LR, step, norm)
    for i, which in enumerate(("param", "grad", "exp_avg", "exp_avg_sq")):   # each in turn, 4 bytes on
        off = [t[1:n + 1] if j == i else t[:n] for j, t in enumerate(big)]
        assert off[i].data_ptr() % 16 == 4
        bad[which + " + 4 B"] = lambda off=off: k9_host(off, partials, 0.5, LR, 1, norm)
        bad[which + " + 4 B, partials"] = lambda off=off: k9_partials(off, partials, 1, 0.5, LR, 1, norm)
        bad[which + " + 4 B, sched"] = lambda off=off: k9_sched(off, partials, 0.5, table, 1, cursor, norm)
    for n_sq in (0, -1):
        bad["n_sq %d" % n_sq] = lambda n_sq=n_sq: k9_partials(st, partials, n_sq, 0.5, LR, 1, norm)
    for n_sched in (0, -1):
        bad["n_sched %d" % n_sched] = lambda n_sched=n_sched: k9_sched(st, partials, 0.5, table, n_sched, cursor, norm)
    bad["null schedule"] = lambda: k9_sched(st, partials, 0.5, None, 1, cursor, norm)
    bad["null cursor"] = lambda: k9_sched(st, partials, 0.5, table, 1, None, norm)
    assert len(bad) == 28
    for label, f in bad.items():
        try:
            f()
        except _lib.XpaError:
            continue
        pytest.fail("accepted: " + label)
    torch.cuda.synchronize()
    assert same_bits(big, keep) and float(partials) == 3.0 and float(norm) == -7.0 and cursor.tolist() == [0, 0, 0, 0]


# ---- A4. FusedClipAdam's host side ---------------------------------------------------------------------------------------
WINDOW = 8


def _net(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(17, 33), torch.nn.LeakyReLU(), torch.nn.Linear(33, 7)).to(DEV)


def _linear_lr(opt):
    return torch.optim.lr_scheduler.LinearLR(opt, start_factor=1.0, end_factor=0.25, total_iters=40)


class _Fused:
    """A small two-layer net on a FlatState with FusedClipAdam and LinearLR."""

    def __init__(self, src=None, sched=False):
        from xuanpolicy_amd.flat import FlatState, FusedClipAdam
        self.net = _net(0)
        if src is not None:
            self.net.load_state_dict(src.state_dict())
        self.opt = torch.optim.Adam(self.net.parameters(), LR, betas=(B1, B2), eps=EPS)
        self.fs = FlatState(self.net.parameters())
        self.fused = FusedClipAdam(self.opt, self.fs)
        self.scheduler = _linear_lr(self.opt)
        self.refills = []
        if sched:
            self.fused.enable_sched()

    def buffers(self):
        return [self.fs.param, self.fs.flat, self.fused.exp_avg, self.fused.exp_avg_sq]

    def step_host(self, max_norm=0.5):
        self.fused.step(max_norm)
        self.scheduler.step()

    def step_sched(self, max_norm=0.5, need=1):
        f = self.fused
        before = getattr(f, "_sched_start", None)
        f.ensure_window(self.scheduler, need=need)
        if f._sched_start != before:   # a refill starts the window at the current update, which no earlier one did
            assert f._sched_start == f.step_count
            self.refills.append(f.step_count)
        f.launch_sched(max_norm)
        f.host_step()
        self.scheduler.step()


def _grads_from(x, a, others):
    """The gradient of a's net on x, written into a's flat buffer by autograd and copied into the others' (the pairs
    differ in how K9 is driven, not in autograd)."""
    a.fs.zero_()
    (a.net(x) ** 2).mean().backward()
    for b in others:
        b.fs.flat.copy_(a.fs.flat)


@pytest.mark.parametrize("event", [None, "lr", "scheduler", "betas"])
def test_fused_scheduled_stepping_equals_host_stepping(monkeypatch, event):
    """Two FusedClipAdam on identical nets, LinearLR live, an 8-entry window: one steps with step(), the other with
    ensure_window + launch_sched + host_step.  Parameters, gradients, moments and step_count are equal bit for bit after
    every update and no launch ran past its window.  event None: 20 updates, the table refilled exactly at updates 0, 8
    and 16.  Otherwise 12 updates and, before update 3 (mid-window), on both sides: the lr edited by hand, the scheduler
    replaced by a new LinearLR, or other betas — the next ensure_window refills (updates 0, 3, 11)."""
    from xuanpolicy_amd import flat
    monkeypatch.setattr(flat.FusedClipAdam, "SCHED_WINDOW", WINDOW)
    a = _Fused()
    b = _Fused(src=a.net, sched=True)
    gen = torch.Generator(device=DEV).manual_seed(3)
    lrs = []
    for u in range(20 if event is None else 12):
        if u == 3 and event is not None:
            for s in (a, b):
                if event == "lr":
                    s.opt.param_groups[0]["lr"] = 1e-4
                elif event == "scheduler":
                    s.scheduler = torch.optim.lr_scheduler.LinearLR(s.opt, start_factor=0.5, end_factor=0.1,
                                                                    total_iters=10)
                else:
                    s.opt.param_groups[0]["betas"] = (float(np.float32(0.8)), float(np.float32(0.99)))
        _grads_from(torch.randn(64, 17, device=DEV, generator=gen), a, [b])
        lrs.append(a.opt.param_groups[0]["lr"])
        assert b.opt.param_groups[0]["lr"] == lrs[-1], u
        a.step_host()
        b.step_sched()
        assert same_bits(a.buffers(), b.buffers()), (event, u)
        assert same_bits([a.fused.total_norm], [b.fused.total_norm]), (event, u)
        assert a.fused.step_count == b.fused.step_count == u + 1
        assert float(a.opt.state[a.fs.params[0]]["step"]) == float(b.opt.state[b.fs.params[0]]["step"]) == u + 1
        assert int(b.fused._cursor[0]) == b.fused.step_count - b.fused._sched_start, (event, u)
    assert not b.fused.sched_overflow()
    assert len(set(lrs)) == len(lrs)                 # the schedule is live: every update ran at its own lr
    assert float(a.fs.flat.abs().max()) > 0
    assert b.refills == ([0, 8, 16] if event is None else [0, 3, 11]), b.refills


def test_ensure_window_need(monkeypatch):
    """need above the window raises; need = k with fewer than k entries left refills, with k left it does not; the pair
    stays bit-identical through the early refill."""
    from xuanpolicy_amd import flat
    monkeypatch.setattr(flat.FusedClipAdam, "SCHED_WINDOW", WINDOW)
    a = _Fused()
    b = _Fused(src=a.net, sched=True)
    gen = torch.Generator(device=DEV).manual_seed(4)
    with pytest.raises(ValueError):
        b.fused.ensure_window(b.scheduler, need=WINDOW + 1)
    for u in range(10):
        _grads_from(torch.randn(64, 17, device=DEV, generator=gen), a, [b])
        a.step_host()
        if u == 6:   # entries 6 and 7 of the window [0, 8) are left
            b.fused.ensure_window(b.scheduler, need=2)
            assert b.fused._sched_start == 0
            with pytest.raises(ValueError):
                b.fused.ensure_window(b.scheduler, need=WINDOW + 1)
            b.step_sched(need=3)
            assert b.fused._sched_start == 6
        else:
            b.step_sched()
        assert same_bits(a.buffers(), b.buffers()), u
    assert b.refills == [0, 6] and not b.fused.sched_overflow()


@pytest.mark.parametrize("sched", [False, True], ids=["host-args", "scheduled-mid-window"])
def test_fused_adam_takes_a_loaded_optimizer_state(monkeypatch, sched):
    """A plain torch.optim.Adam twin (clip_grad_norm_ 0.5, LinearLR) runs five updates; its state_dict() is loaded into a
    FusedClipAdam's optimizer with optimizer.load_state_dict() — fresh, or scheduled and three updates into its own
    8-entry window.  The sixth update on both: the fused result is within the bound of the f64 sixth step from the
    twin's state (baseline: the twin's own f32 step).  The flat buffers keep their pointers, optimizer.state points at
    them again, step_count is 5, the window is refilled from step 5, and state_dict() describes what the kernel wrote.
    Before the load hook in flat.py the fused optimizer went on from its own moments and step."""
    from xuanpolicy_amd import flat
    monkeypatch.setattr(flat.FusedClipAdam, "SCHED_WINDOW", WINDOW)
    gen = torch.Generator(device=DEV).manual_seed(6)
    twin = _net(1)
    opt_t = torch.optim.Adam(twin.parameters(), LR, betas=(B1, B2), eps=EPS)
    sch_t = _linear_lr(opt_t)
    for _ in range(5):
        opt_t.zero_grad()
        (twin(torch.randn(64, 17, device=DEV, generator=gen)) ** 2).mean().backward()
        torch.nn.utils.clip_grad_norm_(twin.parameters(), 0.5)
        opt_t.step()
        sch_t.step()
    f = _Fused(sched=sched)
    if sched:
        for _ in range(3):
            for p in f.fs.params:
                p.grad.normal_(generator=gen)
            f.step_sched()
        assert f.fused.step_count == 3 and f.refills == [0]
    ptrs = [t.data_ptr() for t in f.buffers()]
    f.net.load_state_dict(twin.state_dict())
    f.opt.load_state_dict(opt_t.state_dict())
    f.scheduler.load_state_dict(sch_t.state_dict())
    assert [t.data_ptr() for t in f.buffers()] == ptrs
    loaded_step = f.fused.step_count
    repointed = all(f.opt.state[p]["step"] is f.fused._step_t
                    and f.opt.state[p]["exp_avg"].data_ptr() == f.fused.exp_avg[off:off + p.numel()].data_ptr()
                    and f.opt.state[p]["exp_avg_sq"].data_ptr() == f.fused.exp_avg_sq[off:off + p.numel()].data_ptr()
                    for p, off in zip(f.fs.params, f.fs.offsets))
    for p, q in zip(f.fs.params, twin.parameters()):
        assert torch.equal(p.detach(), q.detach()) and float(opt_t.state[q]["exp_avg"].abs().max()) > 0
    lr = opt_t.param_groups[0]["lr"]
    assert f.opt.param_groups[0]["lr"] == lr and lr < LR
    # the sixth update: one gradient (the twin's autograd), scaled so that the clip is active
    opt_t.zero_grad()
    (twin(torch.randn(64, 17, device=DEV, generator=gen)) ** 2).mean().backward()
    tp = list(twin.parameters())
    scale = 3.0 / float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in tp)))
    f.fs.zero_()
    for p, q in zip(f.fs.params, tp):
        q.grad.mul_(scale)
        p.grad.copy_(q.grad)
    p0 = [q.detach().clone() for q in tp]
    g0 = [q.grad.clone() for q in tp]
    m0 = [opt_t.state[q]["exp_avg"].clone() for q in tp]
    v0 = [opt_t.state[q]["exp_avg_sq"].clone() for q in tp]
    dbl = lambda ts: [t.double() for t in ts]   # noqa: E731
    P64, M64, V64, norm64 = sr.clip_adam_ref(dbl(p0), dbl(g0), dbl(m0), dbl(v0), 6, lr, 0.5, (B1, B2), EPS)
    torch.nn.utils.clip_grad_norm_(tp, 0.5)
    opt_t.step()
    if sched:
        f.step_sched()
    else:
        f.step_host()
    np.testing.assert_allclose(float(f.fused.total_norm), float(norm64), rtol=1e-5)
    flat_m = [f.fused.exp_avg[off:off + p.numel()].view_as(p) for p, off in zip(f.fs.params, f.fs.offsets)]
    flat_v = [f.fused.exp_avg_sq[off:off + p.numel()].view_as(p) for p, off in zip(f.fs.params, f.fs.offsets)]
    sets = {"step": ([p.detach().double() - b.double() for p, b in zip(f.fs.params, p0)],
                     [q.detach().double() - b.double() for q, b in zip(tp, p0)],
                     [a - b.double() for a, b in zip(P64, p0)]),
            "exp_avg": (flat_m, [opt_t.state[q]["exp_avg"] for q in tp], M64),          # the buffers the kernel wrote
            "exp_avg_sq": (flat_v, [opt_t.state[q]["exp_avg_sq"] for q in tp], V64),
            "grad": ([p.grad for p in f.fs.params], [q.grad for q in tp],
                     [clipped(g, norm64, 0.5) for g in dbl(g0)])}
    for name, (got, base, ref) in sets.items():
        res = sr.within_f32(got, base, ref)
        print("loaded state, sched %s, %s: worst |err| / E32 %.3g (E32 %.3g, scale %.3g)" %
              (sched, name, res.ratio, res.e32, res.scale))
        assert res.ok, (name, res)
    # the hook's bookkeeping: the loaded step, optimizer.state on the views, the window refilled from the loaded step
    assert loaded_step == 5 and f.fused.step_count == 6 and float(f.fused._step_t) == 6.0 and repointed
    if sched:
        assert f.refills == [0, 5] and not f.fused.sched_overflow()
    # state_dict() again describes the buffers the kernels write
    sd = f.opt.state_dict()["state"]
    for i, (p, off) in enumerate(zip(f.fs.params, f.fs.offsets)):
        k = p.numel()
        assert float(sd[i]["step"]) == 6.0
        assert torch.equal(sd[i]["exp_avg"].reshape(-1), f.fused.exp_avg[off:off + k])
        assert torch.equal(sd[i]["exp_avg_sq"].reshape(-1), f.fused.exp_avg_sq[off:off + k])
