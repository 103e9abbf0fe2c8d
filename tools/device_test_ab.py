"""A/B of agent.test() with config.device_test off (the reference's host loop: one host round trip per env step) and on
(agent.test_device) in ONE process, on the two tiers:
    C1   PPO-Clip, CartPole-v1, 8 envs x 128 steps, [64] nets; test_episode = 3 test envs as Runner_DRL.benchmark()
         builds them                                                            -> tier K32E (xpa_small_eval_cartpole)
    C2   PPO-Clip, SynthBox 17/6, [256] nets; 64 test envs, test_episode = 64    -> tier steps (+ xpa_eval_post)
Each repeat times one whole agent.test(env_fn, test_episode) call — env construction, reset, the loop, the score
statistics — between two device synchronisations; the legs alternate (host, device, host, ...) so that clock drift falls
on both alike.  The two paths draw their actions from different generators, so their episodes differ: the env steps of
every call are recorded beside its time.  Acceptance (per leg pair): the device path's maximum below the host path's
minimum.

    python tools/device_test_ab.py [--repeats 7] [--train-iters 4] [--out profiles/device_test_ab.json]"""
import argparse
import json
import os
import statistics
import sys
import time
from copy import deepcopy

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--train-iters", type=int, default=4, help="training iterations before the measurement")
    ap.add_argument("--out", default=os.path.join("profiles", "device_test_ab.json"))
    args = ap.parse_args()
    import torch
    from xuanpolicy_amd.runner import build_cartpole_ppo, build_synthbox_ppo, make_envs

    def setup(name):
        if name == "C1":
            agent, n_test = build_cartpole_ppo(n_envs=8, n_steps=128, hidden=64, seed=1, device="cuda:0"), 3
        else:
            agent, n_test = build_synthbox_ppo(seed=1, device="cuda:0"), 64
        agent.train(args.train_iters * agent.n_steps, log=False)
        steps = []

        def env_fn():   # Runner_DRL._test_env_fn
            cfg = deepcopy(agent.config)
            cfg.parallels = n_test
            env = make_envs(cfg, agent.device)
            host_step = env.step

            def counted(actions):
                steps[-1] += 1
                return host_step(actions)
            env.step = counted
            steps.append(0)
            return env
        return agent, n_test, env_fn, steps

    def run(agent, n_test, env_fn, steps, device):
        agent.config.device_test = device
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scores = agent.test(env_fn, n_test)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        return ms, (agent.last_test_log["steps_run"] if device else steps[-1]), len(scores)

    out = {"config": {"repeats": args.repeats, "warmup": args.warmup, "train_iters": args.train_iters,
                      "device": torch.cuda.get_device_name(0)}, "legs": {}}
    for name in ("C1", "C2"):
        agent, n_test, env_fn, steps = setup(name)
        tier = agent.plan_test(env_fn())
        res = {False: [], True: []}
        for _ in range(args.warmup):
            for device in (False, True):
                run(agent, n_test, env_fn, steps, device)
        for _ in range(args.repeats):
            for device in (False, True):
                res[device].append(run(agent, n_test, env_fn, steps, device))
        leg = {"tier": tier, "test_envs": n_test, "test_episode": n_test,
               "train_envs": agent.n_envs, "hidden": list(agent.config.representation_hidden_size)}
        for device, key in ((False, "host"), (True, "device")):
            ms = [r[0] for r in res[device]]
            st = [r[1] for r in res[device]]
            leg[key] = {"ms": [round(x, 3) for x in ms], "median_ms": round(statistics.median(ms), 3),
                        "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "env_steps": st,
                        "episodes": [r[2] for r in res[device]],
                        "median_us_per_step": round(statistics.median(m / s * 1e3 for m, s in zip(ms, st)), 2)}
        leg["speedup_median"] = round(leg["host"]["median_ms"] / leg["device"]["median_ms"], 2)
        leg["speedup_per_step_median"] = round(leg["host"]["median_us_per_step"]
                                               / leg["device"]["median_us_per_step"], 2)
        leg["device_max_below_host_min"] = leg["device"]["max_ms"] < leg["host"]["min_ms"]
        out["legs"][name] = leg
        print("%s %-5s host median %.2f ms (min %.2f, max %.2f; %.1f us/step)  device median %.2f ms (min %.2f, max %.2f;"
              " %.1f us/step)  x%.2f  accepted %s" % (
                  name, tier, leg["host"]["median_ms"], leg["host"]["min_ms"], leg["host"]["max_ms"],
                  leg["host"]["median_us_per_step"], leg["device"]["median_ms"], leg["device"]["min_ms"],
                  leg["device"]["max_ms"], leg["device"]["median_us_per_step"], leg["speedup_median"],
                  leg["device_max_below_host_min"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
