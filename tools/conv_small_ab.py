"""K28R (xpa_conv_fwd_small) against the two routes a small-batch conv forward has without it, at the shapes that
motivated it: C3's conv2 and conv3 at the rollout's 1024 frames and C5's second conv at batch 2048.

  library   the route planned below igemm_min_rows: F.conv2d on the channels-last view + K21 (xpa_bias_act)
  k28       xpa_conv_fwd (the fp32-MFMA implicit GEMM)
  k28r      xpa_conv_fwd_small from planes split ahead (the split's own cost is the `wsplit` line)

One process; every route is captured as a graph of `--launches` back-to-back forwards and the graphs are replayed
alternately, `--rounds` samples each.  Then, end to end and alternating in the same way: C3 training iterations (A2C,
1024 envs x 128 steps) and C5 learner steps (batch 2048) with the config key conv_small_rows off and on.

    python tools/conv_small_ab.py [--launches 50] [--rounds 8] [--e2e 3] [--out profiles/conv_small_ab.json]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

# name -> (B, H, W, in_c, out_c, k, s, p)
SHAPES = {"c3_conv2_1024": (1024, 21, 21, 32, 64, 4, 2, 1), "c3_conv3_1024": (1024, 10, 10, 64, 64, 3, 1, 1),
          "c5_conv2_2048": (2048, 21, 21, 32, 64, 4, 2, 1)}


def _median(v):
    return sorted(v)[len(v) // 2]


def _timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def kernel_ab(name, launches, rounds):
    import torch
    import torch.nn.functional as F
    from xuanpolicy_amd import _lib, graphs, ops
    L, dev, p = ops.lib(), torch.device("cuda:0"), ops._p
    B, H, W, cin, cout, k, s, pad = SHAPES[name]
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(B, H, W, cin, device=dev, generator=g)
    w = torch.randn(cout, cin, k, k, device=dev, generator=g) / (cin * k * k) ** 0.5
    b = torch.randn(cout, device=dev, generator=g) * 0.1
    OH, OW = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    y = torch.empty(B, OH, OW, cout, device=dev)
    planes = torch.empty(int(L.xpa_conv_wsplit_bytes(cin, cout, k)), dtype=torch.uint8, device=dev)
    st = lambda: ops._stream(dev)   # read per launch: a capture runs on its own stream

    def wsplit():
        _lib.call(L.xpa_conv_wsplit, p(w), cin, cout, k, p(planes), st())

    def library():
        z = F.conv2d(x.permute(0, 3, 1, 2), w, None, s, pad).permute(0, 2, 3, 1)
        z = z if z.is_contiguous() else z.contiguous()
        _lib.call(L.xpa_bias_act, 1, p(z.view(-1, cout)), B * OH * OW, cout, p(b), 0.0, st())
        return z

    def k28():
        _lib.call(L.xpa_conv_fwd, 1, p(x), B, H, W, cin, p(w), p(b), cout, k, s, pad, 0.0, p(y), st())

    def k28r():
        _lib.call(L.xpa_conv_fwd_small, 1, p(x), B, H, W, cin, p(planes), p(b), cout, k, s, pad, 0.0, p(y), st())

    wsplit()
    k28r()
    diff = float((y - library()).abs().max())   # the routes compute the same thing before any is timed
    assert diff < 1e-4, diff
    recorded = {}
    for route, fn in (("library", library), ("k28", k28), ("k28r", k28r), ("wsplit", wsplit)):
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
            "max_abs_diff_k28r_vs_library": diff, "samples": res, "median": {r: _median(v) for r, v in res.items()}}


def c3_e2e(iters):
    import torch
    from xuanpolicy_amd.runner import build_atari_a2c
    agents = {key: build_atari_a2c(n_envs=1024, n_steps=128, seed=1, conv_small_rows=key) for key in (False, True)}
    res = {"off": [], "on": []}
    for it in range(iters + 1):            # the first round warms up (graph captures, plans): not kept
        for key, agent in agents.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            agent.train(128)
            torch.cuda.synchronize()
            if it:
                res["on" if key else "off"].append(round((time.perf_counter() - t0) * 1000, 2))
    fwd = [c.fwd for c in agents[True].learner._fused_cnn().trunk_.plan(
        torch.empty((1024, 0), dtype=torch.uint8, device="cuda:0")).convs]
    return {"unit": "ms per iteration (1024 envs x 128 steps + the update)", "rollout_forward_forms_on": fwd,
            "samples": res, "median": {k: _median(v) for k, v in res.items()}}


def c5_e2e(iters, steps=20):
    import torch
    from xuanpolicy_amd.runner import build_perdqn
    dev = torch.device("cuda:0")
    learners = {key: build_perdqn(n_envs=8, n_size=4096, batch_size=2048, seed=1, conv_small_rows=key).learner
                for key in (False, True)}
    g = torch.Generator(device=dev).manual_seed(0)
    obs, nxt = (torch.randint(0, 256, (2048, 84, 84, 4), dtype=torch.uint8, device=dev, generator=g) for _ in range(2))
    act = torch.randint(0, 18, (2048,), device=dev, generator=g).float()
    rew, term = torch.randn(2048, device=dev, generator=g), torch.zeros(2048, device=dev)
    res = {"off": [], "on": []}
    for it in range(iters + 1):
        for key, ln in learners.items():
            ms = _timed(lambda: [ln.update(obs, act, rew, nxt, term, sync_info=False) for _ in range(steps)])
            if it:
                res["on" if key else "off"].append(round(ms / steps, 3))
    fwd = [c.fwd for c in learners[True]._fused_q().eval_trunk.last_plan.convs]
    return {"unit": "ms per learner step (batch 2048: eval + target forward, backward, Adam)", "forward_forms_on": fwd,
            "samples": res, "median": {k: _median(v) for k, v in res.items()}}


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
        out["c3_end_to_end"] = c3_e2e(a.e2e)
        print(json.dumps(out["c3_end_to_end"]), flush=True)
        out["c5_learner_step"] = c5_e2e(a.e2e)
        print(json.dumps(out["c5_learner_step"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
