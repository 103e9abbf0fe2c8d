"""K32 phase timing (s_memtime cycles per phase, averaged over the steps of one 128-step launch) on the C1 agent:
python tools/k32_stamps.py [--hidden 64]     (--hidden 128: K32W)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, default=64)
    args = ap.parse_args()
    import torch
    from xuanpolicy_amd.rollout_plan import K32_DRIVERS
    from xuanpolicy_amd.runner import build_cartpole_ppo
    agent = build_cartpole_ppo(n_envs=8, n_steps=128, hidden=args.hidden, seed=1, device="cuda:0")
    st = torch.zeros(16, dtype=torch.int64, device="cuda:0")
    names = ["rms", "normalise", "-", "-", "forward", "sample+env+post", "ret_rms", "loop barrier"]
    for it in range(4):
        assert agent.plan().driver in K32_DRIVERS   # plan() also builds the argument block
        a = agent._k32
        a.stamps = st.data_ptr()
        agent.train(128, log=False)
        torch.cuda.synchronize()
        v = st.cpu().tolist()
        print(" ".join("%s %.0f" % (n, v[i] / 128) for i, n in enumerate(names)),
              "| per step %.0f cycles, launch %.0f" % (v[8] / 128, v[8]))
