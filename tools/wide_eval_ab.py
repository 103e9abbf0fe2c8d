"""A/B of the 128-wide one-launch evaluation (K32WE / K32WEB, config.device_test_wide) and the batched test-env reset
(config.device_test_batch_reset) against the same process's flags-off legs ("128-wide evaluation
(K32WE / K32WEB) and the batched reset").

One process, legs alternating inside every repeat, warm-up calls first; a sample is one whole call between two device
synchronisations and goes to the output file with the env steps it ran.  The legs of a group do not draw the same
episodes (the tiers' forwards differ by rounding, and one set of agents serves all legs, so the evaluation stream and
the obs statistics move on from call to call): they are compared per env step.  There is no pass criterion.

  agent       the committed CartPole-v1.yaml's shape (10 envs, [128] nets, its test_episode and time limit), one agent:
              agent.test with device_test alone (the "steps" tier) and with device_test_wide (K32WE); 10 test envs
              built by env_fn inside the call, as Runner_DRL does.
  population  P in --ps members of that shape over 10 prebuilt test envs each: the per-member loop of test_device on
              the "steps" tier (what Population.test does without the flags), Population.test_device on K32WEB without
              and with batch_reset.
  c1_reset    the batch-reset A/B alone at C1's shape ([64] nets, 8 test envs, K32EB): tools/population_eval_ab.py's
              "c1" protocol, so the reset's effect reads against profiles/population_eval_ab.json.

    python tools/wide_eval_ab.py --out profiles/wide_eval_ab.json
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _sync_time(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _summary(samples):
    ms = [s["ms_per_call"] for s in samples]
    per = [s["ms_per_call"] * 1e3 / s["env_steps_sum"] for s in samples]
    return {"ms_per_call_median": round(statistics.median(ms), 4), "ms_per_call_min": min(ms), "ms_per_call_max": max(ms),
            "us_per_env_step_median": round(statistics.median(per), 3), "us_per_env_step_min": round(min(per), 3),
            "us_per_env_step_max": round(max(per), 3)}


def _alternate(legs, repeats, warmup):
    """legs: [(name, call, steps)]; call() runs one sample, steps() -> the env steps of its members.  Returns
    {name: {"samples": [...], summary...}}."""
    for _ in range(warmup):
        for _, call, _ in legs:
            call()
    samples = {name: [] for name, _, _ in legs}
    for _ in range(repeats):
        for name, call, steps in legs:
            ms = _sync_time(call)
            st = steps()
            samples[name].append({"ms_per_call": round(ms, 4), "env_steps_max": max(st), "env_steps_sum": sum(st)})
    return {name: dict(_summary(s), samples=s) for name, s in samples.items()}


def _set_flags(members, **flags):
    for a in members:
        for k, v in flags.items():
            setattr(a.config, k, v)


def _test_envs(members, n_test, device):
    from xuanpolicy_amd.runner import make_envs
    out = []
    for a in members:
        c = copy.deepcopy(a.config)
        c.parallels = n_test
        out.append(make_envs(c, device))
    return out


def measure_agent(args):
    from xuanpolicy_amd.runner import build_cartpole_ppo, make_envs
    agent = build_cartpole_ppo(n_envs=10, n_steps=256, hidden=128, seed=1, device=args.device, device_test=True)
    cfg = agent.config
    agent.train(args.train_iters * agent.n_steps, log=False)
    target = int(cfg.test_episode)

    def env_fn():
        return make_envs(copy.deepcopy(cfg), agent.device)

    def leg(wide):
        def call():
            cfg.device_test_wide = wide
            agent.test(env_fn, target)
        return call
    tiers = {}
    for name, wide in (("steps", False), ("K32WE", True)):
        cfg.device_test_wide = wide
        tiers[name] = agent.plan_test(env_fn())
    assert tiers == {"steps": "steps", "K32WE": "K32WE"}, tiers
    steps = lambda: [int(agent.last_test_log["steps_run"])]
    res = _alternate([("steps", leg(False), steps), ("K32WE", leg(True), steps)], args.repeats, args.warmup)
    res["workload"] = ("PPO-Clip CartPole-v1, nets [128], %d test envs, test_episode %d, time limit %d, trained for %d "
                       "iterations of %d x %d steps" % (cfg.parallels, target, cfg.max_episode_steps, args.train_iters,
                                                        cfg.parallels, cfg.n_steps))
    res["steps_over_K32WE_per_env_step"] = round(res["steps"]["us_per_env_step_median"]
                                                 / res["K32WE"]["us_per_env_step_median"], 2)
    print("agent", {k: (res[k]["ms_per_call_median"], res[k]["us_per_env_step_median"]) for k in ("steps", "K32WE")},
          flush=True)
    return res


def measure_population(args, hidden, n_envs, n_steps, n_test, wide_legs):
    import torch
    from xuanpolicy_amd.population import Population
    from xuanpolicy_amd.runner import build_cartpole_ppo
    ps = [int(p) for p in args.ps.split(",")]
    members = [build_cartpole_ppo(n_envs=n_envs, n_steps=n_steps, hidden=hidden, seed=s + 1, device=args.device)
               for s in range(max(ps))]
    cfg = members[0].config
    target = int(cfg.test_episode)
    Population(members).train(args.train_iters * n_steps, log=False)
    envs = _test_envs(members, n_test, args.device)
    res = {"workload": "PPO-Clip CartPole-v1, nets [%d], %d test envs per member, test_episode %d, time limit %d, members "
                       "trained for %d iterations of %d x %d steps"
                       % (hidden, n_test, target, envs[0].max_episode_steps, args.train_iters, n_envs, n_steps), "P": {}}
    for P in ps:
        sub, sub_envs = members[:P], envs[:P]
        pop = Population(sub)

        def loop_call():
            _set_flags(sub, device_test_wide=False)
            for a, e in zip(sub, sub_envs):
                a.test_device(e, target)

        def batch_call(batch_reset):
            def call():
                _set_flags(sub, device_test_wide=True)
                pop.test_device(sub_envs, target, batch_reset=batch_reset)
            return call
        steps = lambda: [int(a.last_test_log["steps_run"]) for a in sub]
        legs = [("batch", batch_call(False), steps), ("batch_reset", batch_call(True), steps)]
        if wide_legs:
            _set_flags(sub, device_test_wide=False)
            assert {a.plan_test(e) for a, e in zip(sub, sub_envs)} == {"steps"}
            legs.insert(0, ("loop_steps_tier", loop_call, steps))
        _set_flags(sub, device_test_wide=True)
        assert pop.plan_test(sub_envs).wide == wide_legs
        entry = _alternate(legs, args.repeats, args.warmup)
        entry["batch_over_batch_reset"] = round(entry["batch"]["ms_per_call_median"]
                                                / entry["batch_reset"]["ms_per_call_median"], 3)
        if wide_legs:
            entry["loop_over_batch_reset_per_env_step"] = round(entry["loop_steps_tier"]["us_per_env_step_median"]
                                                                / entry["batch_reset"]["us_per_env_step_median"], 2)
        res["P"][str(P)] = entry
        print("[%d]" % hidden, "P", P, {n: (entry[n]["ms_per_call_median"], entry[n]["us_per_env_step_median"])
                                       for n, _, _ in legs}, flush=True)
    del members, envs
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/wide_eval_ab.json")
    ap.add_argument("--ps", default="1,4,16,64")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--train-iters", type=int, default=4)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "wide_eval_ab.py measures on a ROCm GPU"
    out = {"what": "one process, legs alternating inside every repeat, %d warm-up calls and %d samples per leg; "
                   "ms_per_call: one whole call for all members between two device synchronisations (agent: env "
                   "construction, reset, launches, header reads, score statistics; population / c1_reset: test_device "
                   "over prebuilt envs: reset, log upload, launches, header reads, log download and decode); "
                   "env_steps_sum / _max: the members' steps_run of that call; us_per_env_step: ms_per_call / "
                   "env_steps_sum.  The legs of a group draw different episodes: compare them per env step"
                   % (args.warmup, args.repeats),
           "device": torch.cuda.get_device_name(0)}
    out["agent"] = measure_agent(args)
    out["population"] = measure_population(args, 128, 10, 256, 10, True)
    out["c1_reset"] = measure_population(args, 64, 8, 128, 8, False)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
