"""CPU: where K28R-D (xpa_conv_dgrad_small) is planned, from CPU trunks' facts.  With small_conv_bwd on, the data
gradients the library route would take become K28R and the block upstream drops its K22; off, no plan changes."""
import pytest
import torch

from xuanpolicy_amd import fused_cnn
from xuanpolicy_amd.cnn_plan import plan_cnn
from xuanpolicy_amd.policies import AC_CNN_Atari, Basic_CNN


def _trunks():
    c3 = AC_CNN_Atari((84, 84, 4), [8, 4, 3], [4, 2, 1], [32, 64, 64], None, torch.nn.init.orthogonal_, torch.nn.ReLU,
                      "cpu", [512])
    c5 = Basic_CNN((84, 84, 4), [8, 4, 3], [4, 2, 1], [32, 64, 64], None, None, torch.nn.ReLU, "cpu")
    return [fused_cnn._Trunk(rep, fused_cnn._Part()) for rep in (c3, c5)]


def test_c5_learner_step_plans_k28r_dgrad():
    t = _trunks()[1]
    off = plan_cnn(t.facts(2048))
    t.small_conv_bwd = True
    p = plan_cnn(t.facts(2048))
    assert [c.dgrad for c in p.convs] == ["none", "K27", "K28R"] and off.convs[2].dgrad == "miopen"
    assert p.convs[1].act_bwd == "K28R-dgrad" and off.convs[1].act_bwd == "K22"
    assert p.convs[0] == off.convs[0] and p._replace(convs=off.convs) == off
    assert [c.fwd for c in p.convs] == [c.fwd for c in off.convs]          # independent of the forward's switch
    bwd, bwd_off = p.launches("backward"), off.launches("backward")
    i = bwd.index("xpa_conv_dgrad_small")
    assert bwd[i + 1] == "xpa_colsum_finalize" and "xpa_conv_dgrad_small" not in bwd_off
    assert bwd.count("xpa_act_bwd_bias") == bwd_off.count("xpa_act_bwd_bias") - 1 and len(bwd) == len(bwd_off)
    assert type(t).small_conv_bwd is False


@pytest.mark.parametrize("B", [64, 2048, 16384])
def test_switch_off_plans_are_the_parents_and_large_rows_ignore_it(B):
    for t in _trunks():
        f = t.facts(B)
        assert f.small_conv_bwd is False and all(c.small_dgrad for c in f.convs[1:]) and not f.convs[0].small_dgrad
        bare = f._replace(convs=tuple(c._replace(small_dgrad=False) for c in f.convs))   # before the field existed
        assert type(f)(*f[:-1]) == f and plan_cnn(f) == plan_cnn(bare) == plan_cnn(bare._replace(small_conv_bwd=True))
        on = plan_cnn(f._replace(small_conv_bwd=True))
        if B * 10 * 10 >= f.igemm_min_rows:        # K28 keeps every block at or above igemm_min_rows
            assert on == plan_cnn(f) and on.convs[2].dgrad == "K28"
        else:
            assert [c.dgrad for c in on.convs] == ["none", "K27", "K28R"]


def test_config_key_reaches_the_trunk():
    """The learner sets its key on the trunks it builds, the target's excepted (the GPU test starts from a config)."""
    from xuanpolicy_amd import learners
    ln = learners.Learner(None, None)
    assert ln.conv_small_rows_bwd is False
    ln.conv_small_rows_bwd = True
    ev, tg = _trunks()
    ln._trunk_switches(ev)
    ln._trunk_switches(tg, backward=False)
    assert (ev.small_conv, ev.small_conv_bwd, tg.small_conv, tg.small_conv_bwd) == (False, True, False, False)
    assert ev.plan(torch.empty((2048, 0), dtype=torch.uint8)).convs[2].dgrad == "K28R"
