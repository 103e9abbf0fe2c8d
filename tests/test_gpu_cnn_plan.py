"""The convolutional trunk runs what its plan says: one FusedCNNActorCritic / FusedQNetwork forward + backward with
every library call recorded; the trunk's ordered entry points must equal CnnPlan.launches("forward") +
CnnPlan.launches("backward"), which are built from the plan's fields alone, and the plan must be the named one.  A
first, unrecorded forward leaves the first fc weight's split planes fresh (their re-split after an optimizer step is
state, not plan)."""
import pytest
import torch

from xuanpolicy_amd.cnn_plan import ConvForm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

K25 = ConvForm("K25", "K26", "K26", "none")
CASES = [
    # (name, net, B, class switches, (convs, frames, slack, fc0_fwd, fc0_dw, fc0_dx))
    ("c3", ("ac", 84), 96, {"igemm_min_rows": 0, "fc_split_min_rows": 0},
     ((K25, ConvForm("K28", "K28-dgrad", "K29", "K27"), ConvForm("K28", "K40G-act", "K29", "K28")),
      "none", 0, "K40G", "K41V", "K40G-act")),
    ("c3_no_fuse", ("ac", 84), 96, {"igemm_min_rows": 0, "fc_split_min_rows": 0, "fc_fuse_act": False},
     ((K25, ConvForm("K28", "K28-dgrad", "K29", "K27"), ConvForm("K28", "K22", "K29", "K28")),
      "none", 0, "K40G", "K41V", "K40G")),
    ("c3_library", ("ac", 84), 96, {},
     ((K25, ConvForm("miopen", "K22", "miopen", "K27"), ConvForm("miopen", "K22", "miopen", "miopen")),
      "none", 0, "linear", "mm", "mm")),
    ("ragged_padded", ("ac", 76), 96, {"igemm_min_rows": 0, "fc_split_min_rows": 0},
     ((K25, ConvForm("K28", "K28-dgrad", "K29", "K27"), ConvForm("K28", "K22", "K29", "K28")),
      "none", 5248 - 5184, "K40G", "K41V-padded", "K40G")),
    ("c5_32_64", ("q", [32, 64]), 64, {"igemm_min_rows": 0, "fc_split_min_rows": 0},
     ((K25, ConvForm("K28", "K24", "K29", "K27")), "none", 0, None, "mm", "mm")),
    ("q_8_8", ("q", [8, 8]), 64, {"igemm_min_rows": 0, "fc_split_min_rows": 0},
     ((ConvForm("K28", "K28-dgrad", "K29", "none"), ConvForm("K28", "K24", "K29", "K28")),
      "forward", 0, None, "mm", "mm")),
]


class _Disc:
    n, shape = 6, ()


def _net(kind, arg):
    """(policy, the fused network, its trunk, the frame size, the per-row shapes of backward's gradient arguments)."""
    from xuanpolicy_amd.fused_cnn import FusedCNNActorCritic, FusedQNetwork
    from xuanpolicy_amd.policies import AC_CNN_Atari, Basic_CNN, BasicQnetwork, Categorical_AC_Policy
    init, relu = torch.nn.init.orthogonal_, torch.nn.ReLU
    torch.manual_seed(0)
    if kind == "ac":
        rep = AC_CNN_Atari((arg, arg, 4), [8, 4, 3], [4, 2, 1], [32, 64, 64], None, init, relu, DEV, [512])
        pol = Categorical_AC_Policy(_Disc(), rep, [], [], None, init, relu, DEV)
        net = FusedCNNActorCritic(pol)
        trunk, hw = net.trunk_, arg
        d_shapes = [(6,), ()]   # d logits, d v
    else:
        rep = Basic_CNN((84, 84, 4), [8, 4], [4, 2], arg, None, init, relu, DEV)
        pol = BasicQnetwork(_Disc(), rep, [32], None, init, relu, DEV)
        net = FusedQNetwork(pol)
        trunk, hw = net.eval_trunk, 84
        d_shapes = [(6,)]       # d evalQ
    for p in pol.parameters():
        p.grad = torch.full_like(p, float("nan"))
    return pol, net, trunk, hw, d_shapes


@pytest.mark.parametrize("name,net,B,switches,want", CASES, ids=[c[0] for c in CASES])
def test_trunk_launches_what_its_plan_declares(name, net, B, switches, want, monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from xuanpolicy_amd import _lib, fused_cnn
    for k, v in switches.items():
        monkeypatch.setattr(fused_cnn._Trunk, k, v)
    pol, fnet, trunk, hw, d_shapes = _net(*net)
    g = torch.Generator(device="cpu").manual_seed(3)
    x = torch.randint(0, 256, (B, hw, hw, 4), generator=g, dtype=torch.int32).to(torch.uint8).to(DEV)
    d_out = [(torch.randn((B,) + s, generator=g) / B).to(DEV) for s in d_shapes]
    fnet.forward(x)   # the fc planes' split happens here

    log = []
    real_call, real_fwd, real_bwd = _lib.call, trunk.forward, trunk.backward
    monkeypatch.setattr(_lib, "call", lambda fn, *a: (log.append(fn.__name__), real_call(fn, *a))[1])
    monkeypatch.setattr(trunk, "forward", lambda *a: (real_fwd(*a), log.append("HEADS"))[0])
    monkeypatch.setattr(trunk, "backward", lambda *a: (log.append("TRUNK"), real_bwd(*a))[1])
    ctx = fnet.forward(x)[-1]
    fnet.backward(ctx, *d_out)
    torch.cuda.synchronize()
    trunk_params = {id(p) for p in trunk.params()}
    for n, p in pol.named_parameters():
        if id(p) in trunk_params:
            assert torch.isfinite(p.grad).all(), n
    plan = trunk.last_plan
    assert plan is ctx[0].plan and plan == trunk.plan(x)
    assert (plan.convs, plan.frames, plan.slack, plan.fc0_fwd, plan.fc0_dw, plan.fc0_dx) == want
    assert log[:log.index("HEADS")] == plan.launches("forward")
    assert log[log.index("TRUNK") + 1:] == plan.launches("backward")
    assert log.count("HEADS") == log.count("TRUNK") == 1
