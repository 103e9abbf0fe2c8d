"""A/B: Population.test_device against the Python loop of the members' own test_device ("Population
evaluation (K32EB)").

One process, two shapes — C1's evaluation (PPO-Clip CartPole-v1, [64] nets, 8 test envs) and the same agents over 64
test envs — and P in {1, 4, 16, 64}.  Per shape, two sets of max(P) agents are built once (seeds 1 .. max(P)) and
trained for a few iterations as populations; a P uses the first P of each: one set through Population.test_device
(one xpa_small_eval_batch launch per chunk and one read of the P headers), the other through
`[a.test_device(e, n) for a, e in zip(agents, envs)]` (a K32E launch and a header read per member and chunk).  The test
envs are built once per member, outside the timed region (test_device resets them); test_episode and the episode
limit are the config's own.  The legs alternate, after warm-up calls; a sample is one whole call between two device
synchronisations, and every sample goes to the output file with the env steps its members ran (both legs draw the
same actions: twins on the same evaluation stream).

    python tools/population_eval_ab.py --out profiles/population_eval_ab.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"c1": dict(test_envs=8), "n64": dict(test_envs=64)}


def _sync_time(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def measure(shape, ps, repeats, warmup, train_iters, device):
    import copy
    import torch
    from xuanpolicy_amd.population import Population
    from xuanpolicy_amd.runner import build_cartpole_ppo, make_envs
    n_test = SHAPES[shape]["test_envs"]
    sets = [[build_cartpole_ppo(seed=s + 1, device=device) for s in range(max(ps))] for _ in range(2)]
    cfg = sets[0][0].config
    T, target = cfg.n_steps, int(cfg.test_episode)
    for members in sets:   # the same training for both sets: twins
        Population(members).train(train_iters * T, log=False)

    def envs_of(members):
        out = []
        for a in members:
            c = copy.deepcopy(a.config)
            c.parallels = n_test
            out.append(make_envs(c, device))
        return out
    envs = [envs_of(members) for members in sets]
    res = {"workload": "PPO-Clip CartPole-v1, nets [%d], %d test envs per member, test_episode %d, time limit %d, "
                       "members trained for %d iterations of %d x %d steps"
                       % (cfg.actor_hidden_size[0], n_test, target, envs[0][0].max_episode_steps, train_iters,
                          cfg.parallels, T), "P": {}}
    for P in ps:
        pop, pop_envs = Population(sets[0][:P]), envs[0][:P]
        loop, loop_envs = sets[1][:P], envs[1][:P]

        def batch_call():
            pop.test_device(pop_envs, target)

        def loop_call():
            for a, e in zip(loop, loop_envs):
                a.test_device(e, target)
        for _ in range(warmup):
            batch_call()
            loop_call()
        samples = {"population": [], "loop": []}
        for _ in range(repeats):
            for leg, fn, members in (("population", batch_call, pop.agents), ("loop", loop_call, loop)):
                el = _sync_time(fn)
                steps = [int(a.last_test_log["steps_run"]) for a in members]
                samples[leg].append({"ms_per_call": round(el * 1e3, 4), "env_steps_max": max(steps),
                                     "env_steps_sum": sum(steps)})
        entry = {"samples": samples}
        for leg in samples:
            ms = [s["ms_per_call"] for s in samples[leg]]
            entry[leg] = {"ms_per_call_median": round(statistics.median(ms), 4), "ms_per_call_min": min(ms),
                          "ms_per_call_max": max(ms)}
        entry["same_steps"] = [s["env_steps_sum"] for s in samples["population"]] == \
            [s["env_steps_sum"] for s in samples["loop"]]
        entry["loop_over_population"] = round(entry["loop"]["ms_per_call_median"]
                                              / entry["population"]["ms_per_call_median"], 3)
        res["P"][str(P)] = entry
        print(shape, "P", P, {k: entry[k]["ms_per_call_median"] for k in ("population", "loop")},
              "loop / population", entry["loop_over_population"], "same steps", entry["same_steps"], flush=True)
    del sets, envs
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/population_eval_ab.json")
    ap.add_argument("--ps", default="1,4,16,64")
    ap.add_argument("--shapes", default="c1,n64")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--train-iters", type=int, default=4)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "population_eval_ab.py measures on a ROCm GPU"
    ps = [int(p) for p in args.ps.split(",")]
    out = {"what": "Population.test_device (population: one xpa_small_eval_batch launch per chunk of 128 steps for all "
                   "P members, one read of the P log headers after it) against `[a.test_device(e, n) for a, e in "
                   "zip(agents, envs)]` over twins (loop: one K32E launch and one header read per member and chunk), "
                   "one process, legs alternating, %d warm-up calls and %d samples per leg; ms per call for all P "
                   "members between two device synchronisations (env reset, log upload, launches, header reads, log "
                   "download and decode); env_steps: the members' steps_run of that call" % (args.warmup, args.repeats),
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for shape in args.shapes.split(","):
        out["shapes"][shape] = measure(shape, ps, args.repeats, args.warmup, args.train_iters, args.device)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
