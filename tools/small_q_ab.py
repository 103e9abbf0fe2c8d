"""A/B of K34 (small_q) against the eager PER-DQN learner step, in one process, the two alternating.

  learner: PerDQN_Learner.update at the reference's classic-control shape (D 4, 128 / 128, A 2, batch 128), device
           events around STEPS updates, us per update;
  agent:   PerDQN_Agent.train of runner.build_perdqn_classic("CartPole-v1"), host clock around train() ending in a
           device synchronise, ms per 1000 env steps.
Warm-up first, then SAMPLES samples of each arm, off / on alternating; every sample goes to profiles/small_q_ab.json.

    python tools/small_q_ab.py [--out profiles/small_q_ab.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEPS, SAMPLES, AGENT_STEPS = 400, 8, 1000
DEV = torch.device("cuda:0")


def _learner(small_q):
    from xuanpolicy_amd.learners import PerDQN_Learner
    from xuanpolicy_amd.policies import BasicQnetwork, Basic_MLP

    class Disc:
        n, shape = 2, ()
    torch.manual_seed(1)
    act = torch.nn.ReLU
    rep = Basic_MLP((4,), [128], None, torch.nn.init.orthogonal_, act, DEV)
    pol = BasicQnetwork(Disc(), rep, [128], None, torch.nn.init.orthogonal_, act, DEV)
    opt = torch.optim.Adam(pol.parameters(), 1e-3, eps=1e-5)
    sch = torch.optim.lr_scheduler.LinearLR(opt, start_factor=1.0, end_factor=0.0, total_iters=200000)
    lrn = PerDQN_Learner(pol, opt, sch, DEV, "./", 0.99, 100)
    lrn.small_q = small_q
    return lrn


def _learner_sample(lrn, batch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(STEPS):
        lrn.update(*batch, sync_info=False)
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / STEPS   # us per update


def _agent_sample(agent):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    agent.train(AGENT_STEPS // agent.n_envs)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) * 1000.0 / AGENT_STEPS   # ms per 1000 env steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "small_q_ab.json"))
    out = ap.parse_args().out
    if not torch.cuda.is_available():
        raise SystemExit("small_q_ab.py measures on the GPU; none found")
    from xuanpolicy_amd.runner import build_perdqn_classic
    g = torch.Generator().manual_seed(0)
    batch = (torch.randn(128, 4, generator=g).to(DEV), torch.randint(0, 2, (128,), generator=g).float().to(DEV),
             torch.randn(128, generator=g).to(DEV), torch.randn(128, 4, generator=g).to(DEV),
             (torch.rand(128, generator=g) < 0.1).float().to(DEV))
    learners = {"off": _learner(False), "on": _learner(True)}
    agents = {"off": build_perdqn_classic("CartPole-v1", small_q=False), "on": build_perdqn_classic("CartPole-v1", small_q=True)}
    assert learners["on"].small_q_ok(batch[0], 128)
    res = {"shape": {"d_in": 4, "h0": 128, "h1": 128, "actions": 2, "batch": 128}, "steps_per_sample": STEPS,
           "agent_env_steps_per_sample": AGENT_STEPS, "learner_us_per_update": {"off": [], "on": []},
           "agent_ms_per_1000_env_steps": {"off": [], "on": []}}
    for arm in ("off", "on"):   # warm-up: code objects, GEMM algorithms, the replay past start_training
        _learner_sample(learners[arm], batch)
        agents[arm].train(300)
    for _ in range(SAMPLES):
        for arm in ("off", "on"):
            res["learner_us_per_update"][arm].append(_learner_sample(learners[arm], batch))
    for _ in range(SAMPLES):
        for arm in ("off", "on"):
            res["agent_ms_per_1000_env_steps"][arm].append(_agent_sample(agents[arm]))
    for key in ("learner_us_per_update", "agent_ms_per_1000_env_steps"):
        res[key + "_median"] = {arm: statistics.median(v) for arm, v in res[key].items()}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k.endswith("_median")}))


if __name__ == "__main__":
    main()
