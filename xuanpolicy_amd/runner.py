"""Config surface and runner for the on-policy path.

Mirrors (reference paths):
  get_arguments / recursive_dict_update   xuance/common/common_tools.py:13-83 (basic.yaml -> algo/env yaml ->
                                          user yaml -> parser args, as a SimpleNamespace)
  Runner_DRL.__init__ / run               xuance/torch/runners/runner_drl.py:15-98 (representation, policy,
                                          Adam(eps=1e-5), LinearLR(end_factor=0, total_iters=running_steps),
                                          REGISTRY_Agent[...](args, envs, policy, optimizer, scheduler, device))
The YAML files under xuanpolicy_amd/configs/ carry the reference's key names; env_name "SynthBox"
selects the device-resident SynthBox env (BASELINE.json configs).
"""
import os
from copy import deepcopy
from types import SimpleNamespace

import torch
import yaml

from . import agents
from .envs import (AcrobotVecEnv, CartPoleVecEnv, MountainCarVecEnv, PendulumVecEnv, SynthAtariVecEnv,
                   SynthBoxVecEnv)
from .policies import (AC_CNN_Atari, ActivationFunctions, Basic_MLP, REGISTRY as REGISTRY_Policy,
                       REGISTRY_Representation)

CONFIG_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs")


def recursive_dict_update(basic, target):
    out = deepcopy(basic)
    for k, v in target.items():
        out[k] = recursive_dict_update(out.get(k, {}), v) if isinstance(v, dict) else v
    return out


def get_config(path):
    with open(path) as f:
        return yaml.safe_load(f)


FLAT_ENVS = ("atari", "mujoco", "Platform", "synthbox")  # perdqn/atari.yaml too   # <method>/<env>.yaml; others <method>/<env>/<env_id>.yaml


def get_arguments(method, env, env_id, config_path=None, parser_args=None):
    """common_tools.py:32-83 for a single method: basic.yaml, then the method's <env>.yaml (or
    <env>/<env_id>.yaml) when it exists, then the user YAML (relative to the working directory), then the
    parser args (their names override)."""
    cfg = get_config(os.path.join(CONFIG_DIR, "basic.yaml"))
    file_name = env + ".yaml" if env in FLAT_ENVS else os.path.join(env, env_id + ".yaml")
    algo = os.path.join(CONFIG_DIR, method, file_name)
    if os.path.exists(algo):
        cfg = recursive_dict_update(cfg, get_config(algo))
    if config_path is not None:
        cfg = recursive_dict_update(cfg, get_config(os.path.join(os.getcwd(), config_path)))
    if parser_args is not None:
        cfg = recursive_dict_update(cfg, dict(vars(parser_args)))
    args = SimpleNamespace(**cfg)
    if env in FLAT_ENVS or not hasattr(args, "env_id"):
        args.env_id = env_id
    return args


def set_seed(seed):
    """xuance/torch/utils/operations.py:17-22."""
    import random

    import numpy as np
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(seed)
        torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    random.seed(seed)


def make_envs(config, device=None, shard=0):
    """xuance/environment/__init__.py:36-99 for the envs built in here: the device-resident SynthBox /
    SynthAtari vector envs (config.parallels envs on config.device)."""
    if device is None:
        device = getattr(config, "device", None)
    if config.env_name == "SynthBox":
        return SynthBoxVecEnv(config.parallels, config.obs_dim, config.act_dim, seed=config.seed,
                              discrete=bool(getattr(config, "discrete", False)),
                              max_episode_steps=getattr(config, "max_episode_steps", 1000), device=device, shard=shard)
    if config.env_name == "Classic Control" and str(getattr(config, "env_id", "")) == "CartPole-v1":
        return CartPoleVecEnv(config.parallels, seed=config.seed, max_episode_steps=getattr(config, "max_episode_steps",
                                                                                            500),
                              device=device, shard=shard)
    if config.env_name == "Classic Control" and str(getattr(config, "env_id", "")) == "Pendulum-v1":
        return PendulumVecEnv(config.parallels, seed=config.seed,
                              max_episode_steps=getattr(config, "max_episode_steps", 200), device=device, shard=shard)
    if config.env_name == "Classic Control" and str(getattr(config, "env_id", "")) == "Acrobot-v1":
        return AcrobotVecEnv(config.parallels, seed=config.seed,
                             max_episode_steps=getattr(config, "max_episode_steps", 500), device=device, shard=shard)
    if config.env_name == "Classic Control" and str(getattr(config, "env_id", "")) == "MountainCar-v0":
        return MountainCarVecEnv(config.parallels, seed=config.seed,
                                 max_episode_steps=getattr(config, "max_episode_steps", 200), device=device,
                                 shard=shard)
    if config.env_name == "Atari" and str(getattr(config, "env_id", "")).startswith("SynthAtari"):
        return SynthAtariVecEnv(config.parallels, getattr(config, "n_actions", 6), seed=config.seed,
                                max_episode_steps=getattr(config, "max_episode_steps", 27000), device=device,
                                shard=shard)
    raise NotImplementedError("env_name %r: only the device-resident SynthBox / SynthAtari / CartPole-v1 / "
                              "Pendulum-v1 / Acrobot-v1 / MountainCar-v0 envs are built in; pass "
                              "any VecEnv with the reference's step contract to the agent directly" % config.env_name)


TUNED_GEMMS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuning", "tunableop_results0.csv")


def enable_tuned_gemms(path=TUNED_GEMMS):
    """Use the committed TunableOp table (tools/tune_gemms.py: hipBLASLt/rocBLAS solutions measured on
    MI355X for the update's GEMM shapes).  Lookup only (no tuning at run time); shapes not in the table
    fall back to the default heuristics.  Returns True when the table was loaded."""
    if not os.path.exists(path) or not torch.cuda.is_available():
        return False
    tun = torch.cuda.tunable
    tun.enable(True)
    tun.tuning_enable(False)
    tun.read_file(path)
    return True


def build_agent(config, device=None, envs=None, shard=0):
    """runner_drl.py:15-75 for PPO_Clip / A2C."""
    device = torch.device(device if device is not None else config.device)
    # The committed table (tools/tune_gemms.py, the paired-layer shapes) gives 1.2 % end to end
    # (81.3 -> 80.3 ms/iteration at C2, `tune_gemms.py check`); shapes outside it keep the heuristics.
    if getattr(config, "tunableop", True) and device.type == "cuda":
        enable_tuned_gemms()
    shard = getattr(config, "shard", shard)
    envs = envs if envs is not None else make_envs(config, device, shard)
    config.observation_space, config.action_space = envs.observation_space, envs.action_space
    act = ActivationFunctions[config.activation]
    init = torch.nn.init.orthogonal_
    if config.representation == "Basic_MLP":
        rep = Basic_MLP(envs.observation_space.shape, config.representation_hidden_size, None, init, act, device)
    elif config.representation == "AC_CNN_Atari":   # input_reformat.py:20-35 argument set
        rep = AC_CNN_Atari(envs.observation_space.shape, config.kernels, config.strides, config.filters, None, init,
                           act, device, config.fc_hidden_sizes)
    else:
        rep = REGISTRY_Representation[config.representation](envs.observation_space.shape, device)
    policy = REGISTRY_Policy[config.policy](envs.action_space, rep, config.actor_hidden_size, config.critic_hidden_size,
                                            None, init, act, device)
    opt_kw = {"fused": True} if getattr(config, "fused_adam", True) and device.type == "cuda" else {}
    optimizer = torch.optim.Adam(policy.parameters(), config.learning_rate, eps=1e-5, **opt_kw)
    scheduler = torch.optim.lr_scheduler.LinearLR(optimizer, start_factor=1.0, end_factor=0.0,
                                                  total_iters=config.running_steps)
    agent = agents.REGISTRY[config.agent](config, envs, policy, optimizer, scheduler, device)
    if getattr(config, "fast_path", True) and device.type == "cuda":
        agent.learner.enable_fast_path(fused_optimizer=getattr(config, "fused_adam", True))
    return agent


def build_synthbox_ppo(n_envs=4096, n_steps=128, obs_dim=17, act_dim=6, hidden=256, n_epoch=16, n_minibatch=8,
                       seed=1, device="cuda:0", agent="PPO_Clip", discrete=False, **overrides):
    """The BASELINE.json C2 configuration (ppo/mujoco.yaml hyper-parameters on SynthBox(17, 6))."""
    method = "ppo" if agent == "PPO_Clip" else "a2c"
    cfg = get_arguments(method, "synthbox", "SynthBox-v0")
    cfg.agent = agent
    cfg.parallels, cfg.n_steps, cfg.obs_dim, cfg.act_dim = n_envs, n_steps, obs_dim, act_dim
    cfg.n_epoch, cfg.n_minibatch, cfg.seed, cfg.discrete = n_epoch, n_minibatch, seed, discrete
    cfg.policy = "Categorical_AC" if discrete else "Gaussian_AC"
    cfg.representation_hidden_size = cfg.actor_hidden_size = cfg.critic_hidden_size = [hidden]
    for k, v in overrides.items():
        setattr(cfg, k, v)
    torch.manual_seed(seed)
    return build_agent(cfg, device)


def build_cartpole_ppo(n_envs=8, n_steps=128, hidden=64, seed=1, device="cuda:0", **overrides):
    """The BASELINE.json C1 configuration: PPO-Clip on CartPole-v1 (ppo/classic_control/CartPole-v1.yaml keys),
    8 envs x 128 steps, [64] hidden layers for the representation, actor and critic (SURVEY.md §8(d) reading of
    "MLP[64,64]")."""
    cfg = get_arguments("ppo", "classic_control", "CartPole-v1")
    cfg.parallels, cfg.n_steps, cfg.seed = n_envs, n_steps, seed
    cfg.representation_hidden_size = cfg.actor_hidden_size = cfg.critic_hidden_size = [hidden]
    for k, v in overrides.items():
        setattr(cfg, k, v)
    torch.manual_seed(seed)
    return build_agent(cfg, device)


def build_pendulum_ppo(n_envs=8, n_steps=128, hidden=64, seed=1, device="cuda:0", agent="PPO_Clip", **overrides):
    """PPO-Clip (or agent="A2C") on the device Pendulum-v1 (<method>/classic_control/Pendulum-v1.yaml keys) at C1's
    shape: 8 envs x 128 steps, [64] hidden layers for the representation, actor and critic, Gaussian heads."""
    cfg = get_arguments("ppo" if agent == "PPO_Clip" else "a2c", "classic_control", "Pendulum-v1")
    cfg.agent = agent
    cfg.parallels, cfg.n_steps, cfg.seed = n_envs, n_steps, seed
    cfg.representation_hidden_size = cfg.actor_hidden_size = cfg.critic_hidden_size = [hidden]
    for k, v in overrides.items():
        setattr(cfg, k, v)
    torch.manual_seed(seed)
    return build_agent(cfg, device)


def build_classic_control(env_id, agent="PPO_Clip", n_envs=8, n_steps=128, hidden=64, seed=1, device="cuda:0",
                          **overrides):
    """PPO-Clip (or agent="A2C") on a device classic-control env by its id (<method>/classic_control/<env_id>.yaml
    keys: CartPole-v1 for PPO, Pendulum-v1, Acrobot-v1, MountainCar-v0) at C1's shape: 8 envs x 128 steps, [hidden]
    layers for the representation, actor and critic — the shape the one-launch small path takes."""
    cfg = get_arguments("ppo" if agent == "PPO_Clip" else "a2c", "classic_control", env_id)
    if getattr(cfg, "env_name", None) != "Classic Control" or getattr(cfg, "env_id", None) != env_id:
        raise ValueError("no %s config for the classic-control env %r" % (agent, env_id))
    cfg.agent = agent
    cfg.parallels, cfg.n_steps, cfg.seed = n_envs, n_steps, seed
    cfg.representation_hidden_size = cfg.actor_hidden_size = cfg.critic_hidden_size = [hidden]
    for k, v in overrides.items():
        setattr(cfg, k, v)
    torch.manual_seed(seed)
    return build_agent(cfg, device)


def build_classic_population(env_id, seeds, agent="PPO_Clip", **kw):
    """One member per seed of `seeds`, each built as it would be alone (build_cartpole_ppo for CartPole-v1,
    build_pendulum_ppo for Pendulum-v1, build_classic_control for the rest; kw goes to the builder), as a
    population.Population: train() runs the members side by side, one launch per stage for all of them, each
    computing what it would compute alone.  Raises ValueError when the members are not one small-path shape."""
    from .population import Population
    build = {"CartPole-v1": build_cartpole_ppo, "Pendulum-v1": build_pendulum_ppo}.get(env_id)
    members = []
    for seed in seeds:
        if build is None:
            members.append(build_classic_control(env_id, agent=agent, seed=seed, **kw))
        else:
            members.append(build(agent=agent, seed=seed, **kw))
    return Population(members)


def build_perdqn(n_envs=8, n_size=131072, batch_size=2048, seed=1, device="cuda:0", **overrides):
    """The BASELINE.json C5 configuration: PER-DQN (perdqn/atari.yaml keys) on SynthAtari frames with 18 actions,
    replay n_envs x n_size (8 x 131 072 = 1 M transitions), batch 2048, BasicQnetwork over Basic_CNN; Adam(eps=1e-5)
    + LinearLR as runner_drl.py:71-76 builds them."""
    from .agents import PerDQN_Agent
    from .policies import BasicQnetwork, Basic_CNN
    cfg = get_arguments("perdqn", "atari", "SynthAtari-v0")
    cfg.parallels, cfg.n_size, cfg.batch_size, cfg.seed = n_envs, n_size, batch_size, seed
    for k, v in overrides.items():
        setattr(cfg, k, v)
    cfg.device = str(device)
    torch.manual_seed(seed)
    envs = make_envs(cfg, device=device)
    act = ActivationFunctions[cfg.activation]
    rep = Basic_CNN(envs.observation_space.shape, cfg.kernels, cfg.strides, cfg.filters, None,
                    torch.nn.init.orthogonal_, act, device)
    policy = BasicQnetwork(envs.action_space, rep, cfg.q_hidden_size, None, torch.nn.init.orthogonal_, act, device)
    opt = torch.optim.Adam(policy.parameters(), cfg.learning_rate, eps=1e-5)
    sch = torch.optim.lr_scheduler.LinearLR(opt, start_factor=1.0, end_factor=0.0, total_iters=cfg.running_steps)
    return PerDQN_Agent(cfg, envs, policy, opt, sch, device)


def build_atari_a2c(n_envs=1024, n_steps=128, seed=1, device="cuda:0", **overrides):
    """The BASELINE.json C3 configuration: A2C, AC_CNN_Atari, SynthAtari 4x84x84 uint8 frames, 6 actions."""
    cfg = get_arguments("a2c", "atari", "SynthAtari-v0")
    cfg.parallels, cfg.n_steps, cfg.seed = n_envs, n_steps, seed
    for k, v in overrides.items():
        setattr(cfg, k, v)
    torch.manual_seed(seed)
    return build_agent(cfg, device)


class Runner_DRL:
    """runner_drl.py:15-134 (with runner_basic.py:5-13) for PPO_Clip / A2C: seed, envs, representation,
    policy, Adam(eps=1e-5) + LinearLR, the agent; run() trains (or tests a saved model in test_mode) and
    benchmark() alternates training and test episodes, keeping the best model."""

    def __init__(self, args):
        self.args = args
        self.agent_name = args.agent
        self.env_id = args.env_id
        set_seed(args.seed)
        self.envs = make_envs(args)
        self.envs.reset()
        self.n_envs = self.envs.num_envs
        self.agent = build_agent(args, envs=self.envs)

    def _test_env_fn(self, parallels):
        def env_fn():
            args_test = deepcopy(self.args)
            args_test.parallels = parallels
            return make_envs(args_test)
        return env_fn

    def run(self):
        import numpy as np
        if getattr(self.args, "test_mode", False):
            self.agent.render = True
            self.agent.load_model(self.agent.model_dir_load, self.args.seed)
            scores = self.agent.test(self._test_env_fn(1), self.args.test_episode)
            print(f"Mean Score: {np.mean(scores)}, Std: {np.std(scores)}")
            print("Finish testing.")
        else:
            self.agent.train(self.args.running_steps // self.n_envs)
            print("Finish training.")
            self.agent.save_model("final_train_model.pth")
        self.envs.close()
        self.agent.finish()

    def benchmark(self):
        import numpy as np
        env_fn = self._test_env_fn(self.args.test_episode)
        train_steps = self.args.running_steps // self.n_envs
        eval_interval = self.args.eval_interval // self.n_envs
        test_episode = self.args.test_episode
        num_epoch = int(train_steps / eval_interval)
        test_scores = self.agent.test(env_fn, test_episode)
        best = {"mean": np.mean(test_scores), "std": np.std(test_scores), "step": self.agent.current_step}
        for i_epoch in range(num_epoch):
            print("Epoch: %d/%d:" % (i_epoch, num_epoch))
            self.agent.train(eval_interval)
            test_scores = self.agent.test(env_fn, test_episode)
            if np.mean(test_scores) > best["mean"]:
                best = {"mean": np.mean(test_scores), "std": np.std(test_scores), "step": self.agent.current_step}
                self.agent.save_model(model_name="best_model.pth")
        print("Best Model Score: %.2f, std=%.2f" % (best["mean"], best["std"]))
        self.envs.close()
        self.agent.finish()
        return best


REGISTRY = {"DRL": Runner_DRL}


def get_runner(method, env, env_id, config_path=None, parser_args=None, is_test=False):
    """common_tools.py:86-167 for a single method."""
    args = get_arguments(method, env, env_id, config_path, parser_args)
    args.agent_name = method
    args.model_dir = os.path.join(os.getcwd(), args.model_dir, args.dl_toolbox, args.env_id)
    args.log_dir = os.path.join(args.log_dir, args.dl_toolbox + "/", args.env_id)
    if is_test:
        args.test_mode = int(is_test)
        args.parallels = 1
    print("Algorithm:", args.agent)
    print("Environment:", args.env_name)
    print("Scenario:", args.env_id)
    return REGISTRY[args.runner](args)
