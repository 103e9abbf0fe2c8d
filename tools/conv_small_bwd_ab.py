"""K28R-D (xpa_conv_dgrad_small) against the two routes a small-batch conv data gradient has without it, at C5's third
conv at batch 2048 and at a stride-2 shape K27 does not take (32 -> 32 channels).  Every leg ends with the previous
block's dz and bias gradient:

  library   the route planned below igemm_min_rows: aten.convolution_backward (input gradient only) on the
            channels-last views + K22 (xpa_act_bwd_bias) on the previous block + its finalize
  k28       xpa_conv_dgrad (the fp32-MFMA implicit GEMM, activation backward in its epilogue) + the finalize
  k28r_d    xpa_conv_dgrad_small from transposed planes split ahead + the finalize (the split's own cost is the
            `wsplit_t` line)

conv_small_ab.py's method: one process; every leg is captured as a graph of `--launches` back-to-back calls and the
graphs are replayed alternately, `--rounds` samples each.  Then, end to end and alternating in the same way, with the
config key conv_small_rows_bwd off and on: C5 learner steps (batch 2048) and A2C iterations whose update is one
2048-frame minibatch (64 envs x 32 steps).

    python tools/conv_small_bwd_ab.py [--launches 50] [--rounds 8] [--e2e 3] [--out profiles/conv_small_dgrad_ab.json]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from conv_small_ab import _median, _timed  # noqa: E402

# name -> (B, H, W, in_c, out_c, k, s, p): the conv whose INPUT gradient is formed
SHAPES = {"c5_conv3_2048": (2048, 10, 10, 64, 64, 3, 1, 1), "s2_32to32_2048": (2048, 21, 21, 32, 32, 4, 2, 1)}


def kernel_ab(name, launches, rounds):
    import torch
    from xuanpolicy_amd import _lib, graphs, ops
    L, dev, p = ops.lib(), torch.device("cuda:0"), ops._p
    B, H, W, cin, cout, k, s, pad = SHAPES[name]
    OH, OW = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    g = torch.Generator(device=dev).manual_seed(0)
    dz = torch.randn(B, OH, OW, cout, device=dev, generator=g)
    x = torch.rand(B, H, W, cin, device=dev, generator=g)
    y_prev = torch.relu(torch.randn(B, H, W, cin, device=dev, generator=g))
    w = torch.randn(cout, cin, k, k, device=dev, generator=g) / (cout * k * k) ** 0.5
    rows = B * H * W
    dx, db = torch.empty(B, H, W, cin, device=dev), torch.empty(cin, device=dev)
    planes = torch.empty(int(L.xpa_conv_wsplit_t_bytes(cin, cout, k)), dtype=torch.uint8, device=dev)
    parts = {r: torch.empty(int(n), cin, device=dev) for r, n in (
        ("library", L.xpa_act_bwd_bias_num_partials(rows, cin)), ("k28", L.xpa_conv_dgrad_num_partials(B, H, W)),
        ("k28r_d", L.xpa_conv_dgrad_small_num_partials(B, H, W, s)))}
    st = lambda: ops._stream(dev)   # read per launch: a capture runs on its own stream

    def finalize(route):
        _lib.call(L.xpa_colsum_finalize, p(parts[route]), parts[route].shape[0], cin, p(db), st())

    def wsplit_t():
        _lib.call(L.xpa_conv_wsplit_t, p(w), cin, cout, k, p(planes), st())

    def library():
        gx = torch.ops.aten.convolution_backward(dz.permute(0, 3, 1, 2), x.permute(0, 3, 1, 2), w, None, [s, s],
                                                 [pad, pad], [1, 1], False, [0, 0], 1, [True, False, False])[0]
        gx = gx.permute(0, 2, 3, 1)
        gx = gx if gx.is_contiguous() else gx.contiguous()
        _lib.call(L.xpa_act_bwd_bias, 1, p(gx), p(y_prev), rows, cin, 0.0, p(gx), p(parts["library"]), st())
        finalize("library")
        return gx

    def k28():
        _lib.call(L.xpa_conv_dgrad, p(dz), B, OH, OW, cout, p(w), cin, k, s, pad, H, W, 1, p(y_prev), 0.0, p(dx),
                  p(parts["k28"]), st())
        finalize("k28")

    def k28r_d():
        _lib.call(L.xpa_conv_dgrad_small, p(dz), B, OH, OW, cout, p(planes), cin, k, s, pad, H, W, 1, p(y_prev), 0.0,
                  p(dx), p(parts["k28r_d"]), st())
        finalize("k28r_d")

    wsplit_t()
    k28r_d()
    db_small = db.clone()
    ref = library()
    diff = float((dx - ref).abs().max())    # the routes compute the same thing before any is timed
    diff_db = float((db_small - db).abs().max() / db.abs().max())
    assert diff < 1e-4 and diff_db < 1e-4, (diff, diff_db)
    recorded = {}
    for route, fn in (("library", library), ("k28", k28), ("k28r_d", k28r_d), ("wsplit_t", wsplit_t)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        recorded[route], _ = graphs.capture(lambda fn=fn: [fn() for _ in range(launches)] and None)
        recorded[route].replay()
    torch.cuda.synchronize()
    res = {route: [] for route in recorded}
    for _ in range(rounds):
        for route, gr in recorded.items():
            res[route].append(round(_timed(gr.replay) * 1000 / launches, 2))
    return {"shape": dict(zip("B H W in_c out_c k s p".split(), SHAPES[name])), "rows": rows,
            "max_abs_diff_k28r_d_vs_library": diff, "max_rel_diff_bias_grad": diff_db, "samples": res,
            "median": {r: _median(v) for r, v in res.items()}}


def c5_e2e(iters, steps=20):
    import torch
    from xuanpolicy_amd.runner import build_perdqn
    dev = torch.device("cuda:0")
    learners = {key: build_perdqn(n_envs=8, n_size=4096, batch_size=2048, seed=1, conv_small_rows_bwd=key).learner
                for key in (False, True)}
    g = torch.Generator(device=dev).manual_seed(0)
    obs, nxt = (torch.randint(0, 256, (2048, 84, 84, 4), dtype=torch.uint8, device=dev, generator=g) for _ in range(2))
    act = torch.randint(0, 18, (2048,), device=dev, generator=g).float()
    rew, term = torch.randn(2048, device=dev, generator=g), torch.zeros(2048, device=dev)
    res = {"off": [], "on": []}
    for it in range(iters + 1):            # the first round warms up (plans, library algorithm choices): not kept
        for key, ln in learners.items():
            ms = _timed(lambda: [ln.update(obs, act, rew, nxt, term, sync_info=False) for _ in range(steps)])
            if it:
                res["on" if key else "off"].append(round(ms / steps, 3))
    forms = [c.dgrad for c in learners[True]._fused_q().eval_trunk.last_plan.convs]
    return {"unit": "ms per learner step (batch 2048: eval + target forward, backward, Adam)", "dgrad_forms_on": forms,
            "samples": res, "median": {k: _median(v) for k, v in res.items()}}


def a2c_e2e(iters):
    import torch
    from xuanpolicy_amd.runner import build_atari_a2c
    agents = {key: build_atari_a2c(n_envs=64, n_steps=32, seed=1, n_minibatch=1, n_epoch=1, conv_small_rows_bwd=key)
              for key in (False, True)}
    res = {"off": [], "on": []}
    for it in range(iters + 1):
        for key, agent in agents.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            agent.train(4 * 32)
            torch.cuda.synchronize()
            if it:
                res["on" if key else "off"].append(round((time.perf_counter() - t0) * 1000 / 4, 2))
    forms = [c.dgrad for c in agents[True].learner._fused_cnn().trunk_.plan(
        torch.empty((2048, 0), dtype=torch.uint8, device="cuda:0")).convs]
    return {"unit": "ms per iteration (64 envs x 32 steps + one 2048-frame update), 4 iterations per sample",
            "dgrad_forms_on": forms, "samples": res, "median": {k: _median(v) for k, v in res.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--e2e", type=int, default=3, help="kept end-to-end samples per side (0: kernels only)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {"unit": "us per launch", "launches_per_graph": a.launches,
           "kernels": {name: kernel_ab(name, a.launches, a.rounds) for name in SHAPES}}
    print(json.dumps(out["kernels"]), flush=True)
    if a.e2e:
        out["c5_learner_step"] = c5_e2e(a.e2e)
        print(json.dumps(out["c5_learner_step"]), flush=True)
        out["a2c_small_minibatch"] = a2c_e2e(a.e2e)
        print(json.dumps(out["a2c_small_minibatch"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
