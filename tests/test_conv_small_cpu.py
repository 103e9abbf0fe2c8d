"""CPU checks of where K28R (xpa_conv_fwd_small) is planned: cnn_plan.plan_cnn over facts gathered from CPU trunks, no
GPU and no kernel launch.  With small_conv on, exactly the forwards the library route would have taken become K28R;
with it off (or the field absent) every plan is what it was."""
import pytest
import torch

from xuanpolicy_amd import fused_cnn, ops
from xuanpolicy_amd.cnn_plan import conv_facts, plan_cnn
from xuanpolicy_amd.policies import AC_CNN_Atari, Basic_CNN


def _c3(filters=(32, 64, 64)):
    rep = AC_CNN_Atari((84, 84, 4), [8, 4, 3], [4, 2, 1], list(filters), None, torch.nn.init.orthogonal_,
                       torch.nn.ReLU, "cpu", [512])
    return fused_cnn._Trunk(rep, fused_cnn._Part())


def _c5(filters=(32, 64, 64)):
    rep = Basic_CNN((84, 84, 4), [8, 4, 3], [4, 2, 1], list(filters), None, None, torch.nn.ReLU, "cpu")
    return fused_cnn._Trunk(rep, fused_cnn._Part())


def _fwd(plan):
    return tuple(c.fwd for c in plan.convs)


def test_c3_rollout_plans_k28r_and_the_update_does_not():
    t = _c3()
    off = {B: plan_cnn(t.facts(B)) for B in (1024, 16384)}
    t.small_conv = True
    p = plan_cnn(t.facts(1024))
    assert _fwd(p) == ("K25", "K28R", "K28R")
    assert p.launches("forward").count("xpa_conv_fwd_small") == 2 and "xpa_bias_act" not in p.launches("forward")[:3]
    # forward only: every backward form, and everything but the forwards, is the switch-off plan's
    assert [c[1:] for c in p.convs] == [c[1:] for c in off[1024].convs]
    assert p._replace(convs=off[1024].convs) == off[1024]
    assert p.launches("backward") == off[1024].launches("backward")
    assert _fwd(off[16384]) == ("K25", "K28", "K28") and plan_cnn(t.facts(16384)) == off[16384]
    assert type(t).small_conv is False          # the switch was set on this trunk, not on the class


@pytest.mark.parametrize("B", [1024, 2048, 16384])
def test_switch_off_plans_are_the_parents(B):
    for t in (_c3(), _c5()):
        f = t.facts(B)
        assert f.small_conv is False and all(c.small for c in f.convs[1:]) and not f.convs[0].small
        bare = f._replace(convs=tuple(c._replace(small=False) for c in f.convs))   # as gathered before the field existed
        assert type(f)(*f[:-1]) == f and plan_cnn(f) == plan_cnn(bare)
        assert "K28R" not in _fwd(plan_cnn(f))
        assert plan_cnn(bare._replace(small_conv=True)) == plan_cnn(f)             # the library did not admit: no K28R


def test_c5_and_the_envelope():
    t = _c5()
    t.small_conv = True
    assert _fwd(plan_cnn(t.facts(2048))) == ("K25", "K28R", "K28R")
    assert _fwd(t.plan(torch.empty((2048, 0), dtype=torch.uint8))) == ("K28", "K28R", "K28R")   # host frames: no K25
    # 12 input channels: outside K28R's envelope, the block keeps the form it had
    L = ops.lib()
    odd = conv_facts(12, 64, (3, 3), (1, 1), (1, 1), True, True, 1, L.xpa_conv_igemm_ok, L.xpa_conv_wgrad_ok,
                     L.xpa_conv_small_ok)
    f = t.facts(2048)
    f = f._replace(convs=f.convs[:2] + (odd,))
    assert not odd.small and plan_cnn(f).convs[2] == plan_cnn(f._replace(small_conv=False)).convs[2]
    assert _fwd(plan_cnn(f)) == ("K25", "K28R", "K28")
    # an operand of 2 GiB (32 channels x 21 x 21 x 4 B x 38044 frames > 2^31) stays with the library
    assert 38044 * 21 * 21 * 32 * 4 > 2 ** 31 > 38043 * 21 * 21 * 32 * 4
    assert _fwd(plan_cnn(t.facts(38044))) == ("K25", "miopen", "K28") and plan_cnn(t.facts(38043)).convs[1].fwd == "K28"
