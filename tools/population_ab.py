"""A/B: Population.train against the Python loop over the same P agents ("Population training").

One process, two shapes — C1 (PPO-Clip CartPole-v1, 8 envs x 128 steps, [64] nets, 8 epochs x 8 minibatches) and the
committed CartPole-v1.yaml shape (10 envs x 256 steps, [128] nets) — and P in {1, 4, 16, 64}.  Per shape, two sets of
max(P) agents are built once (seeds 1 .. max(P)); a P uses the first P of each: one set as a Population, the other
trained by `for a in agents: a.train(...)`.  The legs alternate, after warm-up iterations that take every graph
capture out of the timed region, and every sample (host clock around work that ends in a device synchronise) goes to
the output file.  A further, separately timed iteration per leg records device events at the phase boundaries: the
split into rollout / closing (bootstrap critic pass + GAE) / epochs.

    python tools/population_ab.py --out profiles/population_ab.json

--small-close: the second leg is a Population of members built with small_close=True (the closing in ONE K33 launch,
xpa_small_close_batch) in place of the Python loop: the same shapes, P and protocol, the default population as the
other leg of the same process.  The figures of merit are the closing phase and ms per iteration of the two legs.

    python tools/population_ab.py --small-close --out profiles/population_close_ab.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"c1": dict(n_envs=8, n_steps=128, hidden=64), "yaml": dict(n_envs=10, n_steps=256, hidden=128)}


def _sync_time(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _split(events):
    """ms of rollout / closing / epochs from a list of (name, event) that starts with a "start" event; several
    agents' iterations in a row (the loop leg) are summed."""
    out = {"rollout": 0.0, "closing": 0.0, "epochs": 0.0}
    phase = {"rollout_end": "rollout", "close_end": "closing", "update_end": "epochs"}
    prev = events[0][1]
    for name, ev in events[1:]:
        if name in phase:
            out[phase[name]] += prev.elapsed_time(ev)
        prev = ev
    return {k: round(v, 4) for k, v in out.items()}


def _phase_pass(train, holders, n_steps):
    """One iteration of a leg with device events at the phase boundaries.  holders: the objects whose phase_events
    receive them, in the order they train."""
    import torch
    shared = []
    start = torch.cuda.Event(enable_timing=True)
    for h in holders:
        h.phase_events = shared
    torch.cuda.synchronize()
    start.record()
    shared.append(("start", start))
    train(n_steps)
    torch.cuda.synchronize()
    for h in holders:
        h.phase_events = None
    return _split(shared)


def measure(shape, ps, repeats, warmup, device, small_close=False):
    import torch
    from xuanpolicy_amd.population import Population
    from xuanpolicy_amd.runner import build_cartpole_ppo
    kw = SHAPES[shape]
    T, N = kw["n_steps"], kw["n_envs"]
    other = "population_small_close" if small_close else "loop"
    sets = [[build_cartpole_ppo(seed=s + 1, device=device, **dict(kw, **over)) for s in range(max(ps))]
            for over in ({}, dict(small_close=True) if small_close else {})]
    cfg = sets[0][0].config
    res = {"workload": "PPO-Clip CartPole-v1 num_envs=%d horizon=%d, n_epoch %d, n_minibatch %d, nets [%d]"
                       % (N, T, cfg.n_epoch, cfg.n_minibatch, kw["hidden"]), "P": {}}
    for P in ps:
        pop, loop = Population(sets[0][:P]), sets[1][:P]
        pop2 = Population(loop) if small_close else None
        assert not pop.plan().close_batch and (pop2 is None or pop2.plan().close_batch)
        iters = max(2, 32 // P)   # iterations per sample: a window of at least ~0.1 s at every P

        def pop_train(steps):
            pop.train(steps, log=False)

        def loop_train(steps):
            if small_close:
                return pop2.train(steps, log=False)
            for a in loop:
                a.train(steps, log=False)
        for _ in range(warmup):
            pop_train(T)
            loop_train(T)
        samples = {"population": [], other: []}
        for _ in range(repeats):
            for leg, fn in (("population", pop_train), (other, loop_train)):
                el = _sync_time(lambda: fn(T * iters))
                samples[leg].append({"ms_per_iteration": round(el / iters * 1e3, 4),
                                     "env_steps_per_s": round(P * N * T * iters / el, 1)})
        entry = {"iterations_per_sample": iters, "samples": samples}
        for leg in samples:
            ms = [s["ms_per_iteration"] for s in samples[leg]]
            entry[leg] = {"ms_per_iteration_median": round(statistics.median(ms), 4), "ms_per_iteration_min": min(ms),
                          "ms_per_iteration_max": max(ms),
                          "env_steps_per_s_median": round(statistics.median(s["env_steps_per_s"]
                                                                            for s in samples[leg]), 1)}
        entry["population"]["phase_ms"] = _phase_pass(pop_train, [pop], T)
        entry[other]["phase_ms"] = _phase_pass(loop_train, [pop2] if small_close else loop, T)
        entry[other + "_over_population"] = round(entry[other]["ms_per_iteration_median"]
                                                  / entry["population"]["ms_per_iteration_median"], 3)
        ph = entry["population"]["phase_ms"]
        for leg in ("population", other) if small_close else ("population",):
            lp = entry[leg]["phase_ms"]
            entry[leg]["closing_share"] = round(lp["closing"] / max(sum(lp.values()), 1e-9), 4)
        res["P"][str(P)] = entry
        print(shape, "P", P, {k: entry[k]["ms_per_iteration_median"] for k in ("population", other)},
              other, "/ population", entry[other + "_over_population"], "population phases", ph,
              *((other, "phases", entry[other]["phase_ms"]) if small_close else ()), flush=True)
    del sets
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/population_ab.json")
    ap.add_argument("--ps", default="1,4,16,64")
    ap.add_argument("--shapes", default="c1,yaml")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--small-close", action="store_true",
                    help="second leg: a population of small_close=True members (K33) instead of the Python loop")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "population_ab.py measures on a ROCm GPU"
    ps = [int(p) for p in args.ps.split(",")]
    out = {"what": ("Population.train of small_close=True members (population_small_close: the closing is one "
                    "xpa_small_close_batch launch) against Population.train of default members (population: each "
                    "member closes through its own _close_rollout), P agents each" if args.small_close else
                    "Population.train against `for a in agents: a.train(...)` over the same P agents") + ", one process, "
                   "legs alternating, %d warm-up iterations and %d samples per leg; ms per iteration of all P "
                   "agents, aggregate env-steps/s; phase_ms: one further iteration per leg with device events at "
                   "the phase boundaries (rollout | closing = bootstrap critic pass + GAE per member | epochs)"
                   % (args.warmup, args.repeats),
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for shape in args.shapes.split(","):
        out["shapes"][shape] = measure(shape, ps, args.repeats, args.warmup, args.device, args.small_close)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
