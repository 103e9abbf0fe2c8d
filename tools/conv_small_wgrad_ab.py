"""K28R-W (xpa_conv_wgrad_small) against the two routes a small-batch conv weight gradient has without it, at C5's
third and second convs at batch 2048.  Every leg ends with weight.grad written:

  library   the route planned below igemm_min_rows: aten.convolution_backward (weight gradient only) on the
            channels-last views + the copy into weight.grad
  k29       xpa_conv_wgrad (the fp32-MFMA kernel, a fixed 512-block grid) + the finalize
  k28r_w    xpa_conv_wgrad_small + the finalize

conv_small_bwd_ab.py's method: one process; every leg is captured as a graph of `--launches` back-to-back calls and
the graphs are replayed alternately, `--rounds` samples each.  Then, end to end and alternating in the same way, with
the config key conv_small_rows_wgrad off and on (conv_small_rows and conv_small_rows_bwd on in both legs): C5 learner
steps (batch 2048) and A2C iterations whose update is one 2048-frame minibatch (64 envs x 32 steps).

    python tools/conv_small_wgrad_ab.py [--launches 50] [--rounds 8] [--e2e 3] [--out profiles/conv_small_wgrad_ab.json]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from conv_small_ab import _median, _timed  # noqa: E402

# name -> (B, H, W, in_c, out_c, k, s, p)
SHAPES = {"c5_conv3_2048": (2048, 10, 10, 64, 64, 3, 1, 1), "c5_conv2_2048": (2048, 21, 21, 32, 64, 4, 2, 1)}
KEYS = {"conv_small_rows": True, "conv_small_rows_bwd": True}


def kernel_ab(name, launches, rounds):
    import torch
    from xuanpolicy_amd import _lib, graphs, ops
    L, dev, p = ops.lib(), torch.device("cuda:0"), ops._p
    B, H, W, cin, cout, k, s, pad = SHAPES[name]
    OH, OW = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    g = torch.Generator(device=dev).manual_seed(0)
    dz = torch.randn(B, OH, OW, cout, device=dev, generator=g)
    x = torch.rand(B, H, W, cin, device=dev, generator=g)
    w = torch.randn(cout, cin, k, k, device=dev, generator=g)
    dw, cols = torch.empty_like(w), cout * cin * k * k
    G = {"k29": int(L.xpa_conv_wgrad_num_partials()),
         "k28r_w": int(L.xpa_conv_wgrad_small_num_partials(B, H, W, cin, cout, k, s, pad))}
    parts = {r: torch.empty(n, cols, device=dev) for r, n in G.items()}
    st = lambda: ops._stream(dev)   # read per launch: a capture runs on its own stream

    def finalize(route):
        _lib.call(L.xpa_colsum_finalize, p(parts[route]), G[route], cols, p(dw), st())

    def library():
        gw = torch.ops.aten.convolution_backward(dz.permute(0, 3, 1, 2), x.permute(0, 3, 1, 2), w, None, [s, s],
                                                 [pad, pad], [1, 1], False, [0, 0], 1, [False, True, False])[1]
        dw.copy_(gw)

    def k29():
        _lib.call(L.xpa_conv_wgrad, -1, p(dz), None, 0.0, p(x), B, H, W, cin, cout, k, s, pad, p(parts["k29"]), None,
                  st())
        finalize("k29")

    def k28r_w():
        _lib.call(L.xpa_conv_wgrad_small, p(dz), p(x), B, H, W, cin, cout, k, s, pad, OH, OW, p(parts["k28r_w"]), st())
        finalize("k28r_w")

    k28r_w()
    dw_small = dw.clone()
    library()
    diff = float((dw_small - dw).abs().max() / dw.abs().max())   # the routes compute the same thing before any is timed
    assert diff < 1e-4, diff
    recorded = {}
    for route, fn in (("library", library), ("k29", k29), ("k28r_w", k28r_w)):
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
    return {"shape": dict(zip("B H W in_c out_c k s p".split(), SHAPES[name])), "rows": B * OH * OW,
            "partials_k28r_w": G["k28r_w"], "max_rel_diff_k28r_w_vs_library": diff, "samples": res,
            "median": {r: _median(v) for r, v in res.items()}}


def c5_e2e(iters, steps=20):
    import torch
    from xuanpolicy_amd.runner import build_perdqn
    dev = torch.device("cuda:0")
    learners = {key: build_perdqn(n_envs=8, n_size=4096, batch_size=2048, seed=1, conv_small_rows_wgrad=key,
                                  **KEYS).learner for key in (False, True)}
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
    forms = [c.wgrad for c in learners[True]._fused_q().eval_trunk.last_plan.convs]
    return {"unit": "ms per learner step (batch 2048: eval + target forward, backward, Adam)", "wgrad_forms_on": forms,
            "samples": res, "median": {k: _median(v) for k, v in res.items()}}


def a2c_e2e(iters):
    import torch
    from xuanpolicy_amd.runner import build_atari_a2c
    agents = {key: build_atari_a2c(n_envs=64, n_steps=32, seed=1, n_minibatch=1, n_epoch=1, conv_small_rows_wgrad=key,
                                   **KEYS) for key in (False, True)}
    res = {"off": [], "on": []}
    for it in range(iters + 1):
        for key, agent in agents.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            agent.train(4 * 32)
            torch.cuda.synchronize()
            if it:
                res["on" if key else "off"].append(round((time.perf_counter() - t0) * 1000 / 4, 2))
    forms = [c.wgrad for c in agents[True].learner._fused_cnn().trunk_.plan(
        torch.empty((2048, 0), dtype=torch.uint8, device="cuda:0")).convs]
    return {"unit": "ms per iteration (64 envs x 32 steps + one 2048-frame update), 4 iterations per sample",
            "wgrad_forms_on": forms, "samples": res, "median": {k: _median(v) for k, v in res.items()}}


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
