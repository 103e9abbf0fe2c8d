"""A/B of the one-launch small path on the device classic-control envs (by default Acrobot-v1 and MountainCar-v0, 8
envs x 128 steps, [64] nets, PPO-Clip) in ONE process: per env, two legs alternate on one agent by flipping its switches (the
plan is re-made when a switch changes) —
    small    K32 / K32W rollout (xpa_small_rollout_<env>) + K30 updates (xpa_small_mlp_update[_gauss])
    multi    the multi-kernel path: graph-replayed rollout steps (fused_rollout = False) and multi-kernel updates
             (learner.small_updates = False)
Each repeat times `--iters` whole iterations (rollout + GAE + the updates) between two device synchronisations; the legs
are interleaved (small, multi, small, ...) so that clock drift falls on both alike, and every sample is recorded.
--hidden 128 --n-envs 10 --n-steps 256 is the reference's classic-control shape (K32W, K30's one-image form).

    python tools/classic_ab.py [--repeats 7] [--iters 20] [--hidden 64] [--n-envs 8] [--n-steps 128]
                               [--envs Acrobot-v1,MountainCar-v0] [--out profiles/classic_small_ab.json]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEGS = {"small": (True, True), "multi": (False, False)}
ENV_IDS = ("Acrobot-v1", "MountainCar-v0")


def measure(env_id, args):
    import torch
    from xuanpolicy_amd.rollout_plan import K32_DRIVERS
    from xuanpolicy_amd.runner import build_classic_control
    N, T = args.n_envs, args.n_steps
    agent = build_classic_control(env_id, n_envs=N, n_steps=T, hidden=args.hidden, seed=1, device="cuda:0")

    def select(leg):
        agent.fused_rollout, agent.learner.small_updates = LEGS[leg]
        plan = agent.plan()
        assert (plan.driver in K32_DRIVERS) == LEGS[leg][0] and (plan.feed == "small") == LEGS[leg][1], (leg, plan)
        return plan

    def run(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        agent.train(iters * T, log=False)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / iters

    plans = {}
    for leg in LEGS:   # warm-up: every leg's graphs captured, its plan recorded
        plans[leg] = select(leg)
        run(args.warmup)
    ms = {leg: [] for leg in LEGS}
    for _ in range(args.repeats):
        for leg in LEGS:
            select(leg)
            ms[leg].append(run(args.iters))
    out = {"config": {"env": env_id, "agent": "PPO_Clip", "n_envs": N, "n_steps": T, "hidden": [args.hidden],
                      "n_epoch": agent.config.n_epoch, "n_minibatch": agent.config.n_minibatch},
           "legs": {}}
    for leg, v in ms.items():
        med = statistics.median(v)
        out["legs"][leg] = {"fused_rollout": LEGS[leg][0], "small_updates": LEGS[leg][1],
                            "driver": plans[leg].driver, "feed": plans[leg].feed,
                            "step_launches": plans[leg].step_launches(),
                            "ms_per_iter": [round(x, 4) for x in v], "median_ms": round(med, 4),
                            "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                            "env_steps_per_s": round(N * T / med * 1e3, 1)}
    out["small_max_below_multi_min"] = out["legs"]["small"]["max_ms"] < out["legs"]["multi"]["min_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--hidden", type=int, default=64, help="width of the representation, actor and critic layers")
    ap.add_argument("--n-envs", type=int, default=8)
    ap.add_argument("--n-steps", type=int, default=128)
    ap.add_argument("--envs", default=",".join(ENV_IDS), help="comma-separated env ids (classic_control PPO configs)")
    ap.add_argument("--out", default=os.path.join("profiles", "classic_small_ab.json"))
    args = ap.parse_args()
    import torch
    out = {"repeats": args.repeats, "iters_per_repeat": args.iters, "warmup_iters": args.warmup,
           "device": torch.cuda.get_device_name(0), "envs": {e: measure(e, args) for e in args.envs.split(",")}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for env_id, res in out["envs"].items():
        for leg, r in res["legs"].items():
            print("%-15s %-6s %-11s %-6s median %.3f ms/iter (min %.3f, max %.3f), %.0f env-steps/s" % (
                env_id, leg, r["driver"], r["feed"], r["median_ms"], r["min_ms"], r["max_ms"], r["env_steps_per_s"]))


if __name__ == "__main__":
    main()
