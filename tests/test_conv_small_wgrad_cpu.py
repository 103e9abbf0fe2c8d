"""CPU: where K28R-W (xpa_conv_wgrad_small) is planned, from CPU trunks' facts.  With small_conv_wgrad on, the weight
gradients the library route would take become K28R; off, no plan changes."""
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


def test_c5_learner_step_plans_k28r_wgrad():
    t = _trunks()[1]
    off = plan_cnn(t.facts(2048))
    t.small_conv_wgrad = True
    p = plan_cnn(t.facts(2048))
    assert [c.wgrad for c in p.convs] == ["K26", "K28R", "K28R"] and [c.wgrad for c in off.convs][1:] == ["miopen"] * 2
    for field in ("act_bwd", "dgrad", "fwd"):
        assert [getattr(c, field) for c in p.convs] == [getattr(c, field) for c in off.convs]
    assert p._replace(convs=off.convs) == off
    bwd, bwd_off = p.launches("backward"), off.launches("backward")
    at = [i for i, name in enumerate(bwd) if name == "xpa_conv_wgrad_small"]
    assert len(at) == 2 and all(bwd[i + 1] == "xpa_colsum_finalize" for i in at)
    assert "xpa_conv_wgrad_small" not in bwd_off and len(bwd) == len(bwd_off) + 4
    assert type(t).small_conv_wgrad is False


@pytest.mark.parametrize("B", [64, 2048, 16384])
def test_switch_off_plans_are_the_parents_and_large_rows_ignore_it(B):
    for t in _trunks():
        f = t.facts(B)
        assert f.small_conv_wgrad is False and all(c.small_wgrad for c in f.convs[1:]) and not f.convs[0].small_wgrad
        bare = f._replace(convs=tuple(c._replace(small_wgrad=False) for c in f.convs))   # before the field existed
        assert type(f)(*f[:-1]) == f and all(type(c)(*c[:-1]) == c._replace(small_wgrad=False) for c in f.convs)
        assert plan_cnn(f) == plan_cnn(bare) == plan_cnn(bare._replace(small_conv_wgrad=True))
        on = plan_cnn(f._replace(small_conv_wgrad=True))
        if B * 10 * 10 >= f.igemm_min_rows:        # K29 keeps every block at or above igemm_min_rows
            assert on == plan_cnn(f) and on.convs[2].wgrad == "K29"
        else:
            assert [c.wgrad for c in on.convs][1:] == ["K28R", "K28R"]


def test_config_key_reaches_the_trunk():
    """The learner sets its key on the trunks it builds, the target's excepted (the GPU test starts from a config)."""
    from xuanpolicy_amd import learners
    ln = learners.Learner(None, None)
    assert ln.conv_small_rows_wgrad is False
    ln.conv_small_rows_wgrad = True
    ev, tg = _trunks()
    ln._trunk_switches(ev)
    ln._trunk_switches(tg, backward=False)
    assert (ev.small_conv_wgrad, ev.small_conv_bwd, tg.small_conv_wgrad) == (True, False, False)
    assert ev.plan(torch.empty((2048, 0), dtype=torch.uint8)).convs[2].wgrad == "K28R"


def test_a_map_too_wide_for_one_slab_row_keeps_the_library():
    """xpa_conv_wgrad_small_fits (the launch's own rule) is part of the fact: on a 324 x 324 input conv 2 sees an 81-wide
    map (32 -> 64 4 x 4 stride 2 fits up to 53) and conv 3 a 40-wide one (64 -> 64 3 x 3 fits up to 32), so with the
    switch on both still plan the library and no backward can meet a launch that rejects its map."""
    from xuanpolicy_amd import ops
    L = ops.lib()
    assert L.xpa_conv_wgrad_small_fits(32, 32, 64, 64, 3, 1, 1) and not L.xpa_conv_wgrad_small_fits(33, 33, 64, 64, 3, 1, 1)
    assert L.xpa_conv_wgrad_small_fits(53, 53, 32, 64, 4, 2, 1) and not L.xpa_conv_wgrad_small_fits(54, 54, 32, 64, 4, 2, 1)
    assert not L.xpa_conv_wgrad_small_fits(10, 10, 48, 64, 3, 1, 1)      # outside the envelope
    wide = Basic_CNN((324, 324, 4), [8, 4, 3], [4, 2, 1], [32, 64, 64], None, None, torch.nn.ReLU, "cpu")
    t = fused_cnn._Trunk(wide, fused_cnn._Part())
    t.small_conv_wgrad = True
    f = t.facts(8)
    assert [c.small_wgrad for c in f.convs] == [False, False, False]
    assert all(L.xpa_conv_small_wgrad_ok(c.cin, c.cout, c.k, c.s) for c in f.convs[1:])   # the envelope alone admits them
    assert [c.wgrad for c in plan_cnn(f).convs][1:] == ["miopen", "miopen"]
