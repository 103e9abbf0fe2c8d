"""Record the parts of the reference's surface that tests/test_dropin_surface_cpu.py checks, as data
(tests/golden/ref_surface.json), so those tests run without the reference:

  example_imports  every `from xuance... import names` of examples/ppo/ppo_mujoco.py and ppo_atari.py
  agents_module    the REGISTRY keys of xuance.torch.agents and which of the names INTEGRATION.md's patch rebinds exist
  policies         for Gaussian_AC_Policy / Categorical_AC_Policy over Basic_MLP at the C2 sizes ((17,) -> [256],
                   heads [256], LeakyReLU): the module tree (name, class, the Linear / LeakyReLU constructor
                   arguments), the parameter names and shapes in state_dict order, and whether the object has a
                   `discrete` attribute

Run where the reference is importable (tests/golden/ref_loader.py):  python tests/golden/make_ref_surface.py
"""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden.ref_loader import REF_ROOT, import_reference  # noqa: E402


def example_imports(path):
    out = []
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.ImportFrom) and node.module and node.module.split(".")[0] == "xuance":
            out.append([node.module, [a.name for a in node.names]])
    return out


def module_tree(policy):
    import torch.nn as nn
    mods = []
    for name, m in policy.named_modules():
        if not name:
            continue
        args = {}
        if isinstance(m, nn.Linear):
            args = {"in_features": m.in_features, "out_features": m.out_features, "bias": m.bias is not None}
        elif isinstance(m, nn.LeakyReLU):
            args = {"negative_slope": m.negative_slope}
        kind = next((k for k in ("Linear", "LeakyReLU", "Sequential") if isinstance(m, getattr(nn, k))), "Module")
        mods.append([name, kind, args])
    return {"has_discrete": hasattr(policy, "discrete"), "modules": mods,
            "state_dict": [[k, list(v.shape)] for k, v in policy.state_dict().items()]}


def main():
    import_reference()
    import gym
    import torch
    import xuance.torch.agents as ref_agents
    from xuance.torch.policies import Categorical_AC_Policy, Gaussian_AC_Policy
    from xuance.torch.representations import Basic_MLP
    from xuance.torch.utils import ActivationFunctions
    res = {"example_imports": {f: example_imports(os.path.join(REF_ROOT, "examples", "ppo", f))
                               for f in ("ppo_mujoco.py", "ppo_atari.py")},
           "agents_module": {"registry_keys": sorted(ref_agents.REGISTRY),
                             "names": [n for n in ("PPOCLIP_Agent", "A2C_Agent", "get_total_iters")
                                       if hasattr(ref_agents, n)]},
           "policies": {}}
    init = torch.nn.init.orthogonal_
    for tag, cls, space in (("gaussian", Gaussian_AC_Policy, gym.spaces.Box(-1, 1, (6,))),
                            ("categorical", Categorical_AC_Policy, gym.spaces.Discrete(4))):
        rep = Basic_MLP(input_shape=(17,), hidden_sizes=[256], normalize=None, initialize=init,
                        activation=ActivationFunctions["LeakyReLU"], device="cpu")
        pol = cls(action_space=space, representation=rep, actor_hidden_size=[256], critic_hidden_size=[256],
                  normalize=None, initialize=init, activation=ActivationFunctions["LeakyReLU"], device="cpu")
        res["policies"][tag] = module_tree(pol)
    with open(os.path.join(HERE, "ref_surface.json"), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
