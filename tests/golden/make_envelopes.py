"""Precision envelopes of the production-net fixtures (test infrastructure; imports the oracle, never the reference).

A few Adam steps of an f32 network are chaotic in the last bits: Adam normalises every gradient element, so an
element whose f32 value is dominated by rounding (a near-zero sum, a max-pool argmax or ReLU kink decided by an ulp)
moves its weight by ~lr in a direction the rounding picks.  Two correct f32 implementations therefore drift apart
update by update (measured: the exact f64 replay of G9P leaves the f32 reference by 2.5e-7 in |TD| at update 0,
8e-6 at update 1, 7e-4 at update 2).  This script replays each fixture with the CPU oracle in float64 from the same
start and records, per checked quantity, how far the reference's own f32 result is from that exact replay.  The GPU
replay tests accept a deviation of max(base tolerance, 3 x this envelope): the device path must stay as close to the
reference as the reference itself is to exact arithmetic.

    python tests/golden/make_envelopes.py      (writes <fixture>_env.npz next to each fixture)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from oracle import cpu_ref  # noqa: E402
from oracle.synth_env import SynthAtariEnv  # noqa: E402
from tests.golden.fixture_init import uniform_state  # noqa: E402
from tests.golden.parts import load_npz  # noqa: E402


def _load(name):
    return load_npz(os.path.join(HERE, name))


def _perdqn_batch(seed, k, B, A):   # make_golden.perdqn_batch
    rng = np.random.default_rng(seed * 1000 + k)
    obs = rng.integers(0, 256, (B, 84, 84, 4), dtype=np.uint8)
    nxt = rng.integers(0, 256, (B, 84, 84, 4), dtype=np.uint8)
    act = rng.integers(0, A, B).astype(np.float32)
    rew = rng.normal(0, 1, B).astype(np.float32)
    term = (rng.random(B) < 0.2).astype(np.float32)
    return obs, act, rew, nxt, term


def envelope_perdqn(name="perdqn_prod.npz"):
    g = _load(name)
    B, A, n_up, seed, sync = (int(x) for x in g["config"])
    net = [int(x) for x in g["net"]]
    nl = (len(net) - 1) // 3
    pol = cpu_ref.build_qnetwork_ref(A, net[:nl], net[nl:2 * nl], net[2 * nl:3 * nl], net[3 * nl:])
    pol.load_state_dict({k[4:]: torch.as_tensor(v) for k, v in g.items() if k.startswith("sd0/")})
    pol.double()
    opt = torch.optim.Adam(pol.parameters(), 1e-3, eps=1e-5)
    sch = torch.optim.lr_scheduler.LinearLR(opt, start_factor=1.0, end_factor=0.5, total_iters=10)
    lrn = cpu_ref.PerDQNLearnerRef(pol, opt, sch, float(g["gamma"]), sync)
    out = {"td": [], "info": []}
    for k in range(n_up):
        obs, act, rew, nxt, term = _perdqn_batch(seed, k, B, A)
        td, info = lrn.update(obs, act, rew, nxt, term)
        out["td"].append(np.abs(td - g["td_abs"][k]).max())
        out["info"].append(np.abs(np.asarray([info["Qloss"], info["learning_rate"], info["predictQ"]]) -
                                  g["infos"][k]))
    res = {"td": np.asarray(out["td"]), "info": np.stack(out["info"])}
    for key, v in pol.state_dict().items():
        res["sd/" + key] = np.asarray(np.abs(v.numpy() - g["sd%d/%s" % (n_up, key)]).max())
    np.savez_compressed(os.path.join(HERE, name.replace(".npz", "_env.npz")), **res)
    print(name, "td", res["td"], "info", res["info"].max(0))


def _replay_atari(g, dtype, jitter_seed=None, threads=None):
    """One replay of a G8 / G12 fixture by the CPU oracle from the fixture's starting weights, in `dtype`.  jitter_seed:
    after every update, each weight moves by one ulp of f32 up or down (or stays) at random — a stand-in for another
    correct f32 implementation, whose every update rounds differently.  threads: torch intra-op threads (another
    summation order in the CPU convolutions / GEMMs).  Returns (per-update info rows, {reference key: weights})."""
    N, T, K, n_epoch, n_mb, max_ep, seed = (int(x) for x in g["config"])
    net = [int(x) for x in g["net"]]
    nl = (len(net) - 1) // 3
    filters, kernels, strides, fc = net[:nl], net[nl:2 * nl], net[2 * nl:3 * nl], net[3 * nl:]
    pol = cpu_ref.build_atari_ac_ref(K, filters, kernels, strides, fc)
    small = "init_seed" not in g   # the small-net fixtures store their starting weights (sd0/)
    pre = "sd0/" if small else "sd0sum/"
    ref_keys = [k[len(pre):] for k in g if k.startswith(pre)]
    mine = list(pol.state_dict().keys())
    assert len(mine) == len(ref_keys)
    # the reference's state_dict order (representation, actor, critic) == the oracle's (critic_head last)
    order = [k for k in ref_keys if k.startswith("representation")] + [k for k in ref_keys if k.startswith("actor")] \
        + [k for k in ref_keys if k.startswith("critic")]
    shapes = [(k, pol.state_dict()[m].shape) for k, m in zip(order, mine)]
    vals = {k: g["sd0/" + k] for k, _ in shapes} if small else uniform_state(shapes, int(g["init_seed"]))
    pol.load_state_dict({m: torch.as_tensor(vals[k]) for k, m in zip(order, mine)})
    pol.to(dtype)
    ppo = int(g.get("algo", 0)) == 1   # G12P: PPOCLIP_Agent (ppo/atari.yaml coefficients, make_golden.capture_atari)
    if ppo:
        lr, vf, ent, clip, gn = (float(x) for x in g["hyper"])
    else:
        lr, vf, ent, clip, gn = 7e-4, 0.25, 0.01, 0.0, 0.2
    opt = torch.optim.Adam(pol.parameters(), lr, eps=1e-5)
    sch = torch.optim.lr_scheduler.LinearLR(opt, start_factor=1.0, end_factor=0.0, total_iters=10000)
    lrn = cpu_ref.LearnerRef(pol, opt, sch, "ppo" if ppo else "a2c", vf, ent, clip, gn, True)
    rng = torch.Generator().manual_seed(jitter_seed) if jitter_seed is not None else None
    nthreads = torch.get_num_threads()
    if threads:
        torch.set_num_threads(threads)
    envs = [SynthAtariEnv(i, seed=seed, n_actions=K, max_episode_steps=max_ep) for i in range(N)]
    obs = np.stack([e.reset()[0] for e in envs])
    B = N * T // n_mb
    k = 0
    infos = []
    for it in range(g["act"].shape[0]):
        frames = np.zeros((N, T, 84, 84, 4), np.uint8)
        for t in range(T):
            acts = g["env_actions"][k]
            k += 1
            nxt, raw = obs.copy(), obs.copy()
            for i, e in enumerate(envs):
                o, r, te, tr, info = e.step(acts[i])
                if te or tr:
                    info["reset_obs"] = e.reset()[0]
                raw[i] = o
                nxt[i] = info["reset_obs"] if tr else o
            frames[:, t] = raw if (it, t) == (0, 0) else obs
            obs = nxt
        fl = frames.reshape(N * T, 84, 84, 4)
        act, ret, adv = g["act"][it].reshape(-1), g["ret"][it].reshape(-1), g["adv"][it].reshape(-1)
        for e in range(n_epoch):
            perm = g["perms"][it * n_epoch + e]
            for s in range(0, N * T, B):
                idx = perm[s:s + B]
                a = adv[idx]
                a = (a - a.mean()) / (a.std() + 1e-8)    # memory_tools.py:241-242 (sample's adv-norm)
                info = lrn.update(fl[idx], act[idx].astype(np.int64), ret[idx], a.astype(np.float32),
                                  old_logp=g["old_logp"][it].reshape(-1)[idx] if ppo else None)
                infos.append([info["actor-loss"], info["critic-loss"], info["entropy"], info["learning_rate"],
                              info["predict_value"]] + ([info["clip_ratio"]] if ppo else []))
                if rng is not None:
                    with torch.no_grad():
                        for p in pol.parameters():
                            step = torch.randint(-1, 2, p.shape, generator=rng).to(p.dtype)
                            p.add_(step * p.abs().clamp_min(1e-30) * 2.0 ** -23)
    torch.set_num_threads(nthreads)
    sd = pol.state_dict()
    return np.asarray(infos, np.float64), {key: sd[m].double().numpy() for key, m in zip(order, mine)}


def envelope_atari(name="atari_a2c_prod.npz"):
    """The per-update, per-quantity distance from the reference's recorded f32 run of an ENSEMBLE of replays (running
    maximum over the updates): the exact
    f64 replay (r03's envelope), f32 replays on 1 and 8 threads, and f32 replays jittered by one ulp after every update
    (3 seeds).  r06: the single f64 sample underestimated how far a correct f32 implementation lands — on G8P's update 6
    the device's predict_value sat at 6.8-8.4x the f64 distance on BOTH conv paths (the library MIOpen / hipBLASLt path
    as well as K28 + K40G), while the f32 ensemble members reach it too; info_f64 keeps the old envelope beside it."""
    g = _load(name)
    runs = {"f64": _replay_atari(g, torch.float64), "f32_t1": _replay_atari(g, torch.float32, threads=1),
            "f32_t8": _replay_atari(g, torch.float32, threads=8)}
    for sd_ in (1, 2, 3):
        runs["f32_jitter%d" % sd_] = _replay_atari(g, torch.float32, jitter_seed=sd_)
    ref_info = g["infos"]
    res = {}
    for tag, (info, _) in runs.items():
        res["info_" + tag] = np.abs(info - ref_info)
    # the ensemble's largest distance, then its running maximum over the updates: one trajectory's distance dips by
    # chance (G12P's f64 replay: 4.4e-4 at update 23 between 5.2e-3 and 6.8e-3 in predict_value), while the spread of
    # correct f32 runs does not shrink as the updates go on
    res["info_point"] = np.max(np.stack([res["info_" + t] for t in runs]), axis=0)
    res["info"] = np.maximum.accumulate(res["info_point"], axis=0)
    for tag, (_, w) in runs.items():
        for key, a in w.items():
            if "sd1/" + key in g:
                d = {"sd/" + key: np.abs(a - g["sd1/" + key]).max()}
            else:
                d = {"sd/" + key + "::rows16": np.abs(a[::16] - g["sd1/" + key + "::rows16"]).max(),
                     "sd/" + key + "::rowsum": np.abs(a.reshape(a.shape[0], -1).sum(1) -
                                                      g["sd1/" + key + "::rowsum"]).max()}
            for kk, v in d.items():
                res[kk] = np.asarray(max(float(res.get(kk, 0.0)), float(v)))
    np.savez_compressed(os.path.join(HERE, name.replace(".npz", "_env.npz")), **res)
    print(name, "info f64", res["info_f64"].max(0), "ensemble", res["info"].max(0))


if __name__ == "__main__":
    torch.set_num_threads(8)
    envelope_perdqn()
    for fixture in ("atari_a2c_prod.npz", "atari_ppo_prod.npz", "atari_ppo.npz"):
        envelope_atari(fixture)
