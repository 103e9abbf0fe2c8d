"""CPU checks of the CNN host plans (cnn_plan.plan_cnn over facts gathered from CPU trunks; no GPU, no kernel launches):
  * C3's trunk (AC_CNN_Atari 4x84x84, [32, 64, 64], fc 512) takes the split fc path for the update's minibatches and
    not for the rollout's 1024 frames, with the last conv's activation backward fused (6400 = 25 x 256 columns);
  * a trunk whose flattened width is not a multiple of 256 keeps the split but not the fused epilogue, and its last
    data-gradient column block is aligned to the row's end (overlapping its neighbour, never padded);
  * the named production plans (C3 at the update's and the rollout's batch, C5, the 8-channel test net, the padded
    K41V) and the plan's invariants over every switch;
  * a conv whose output reaches 2 GiB while its input does not is not planned K28;
  * the grouped split GEMM entries refuse host tensors (no CPU path);
  * the conv forms' defaults: K25B / K26B / K27B on, K28B off."""
import itertools

import pytest
import torch

from xuanpolicy_amd import _lib, fused_cnn, ops
from xuanpolicy_amd.cnn_plan import ConvForm, plan_cnn
from xuanpolicy_amd.policies import AC_CNN_Atari, Basic_CNN


def _trunk(hw):
    rep = AC_CNN_Atari((hw, hw, 4), [8, 4, 3], [4, 2, 1], [32, 64, 64], None, torch.nn.init.orthogonal_,
                       torch.nn.ReLU, "cpu", [512])
    return fused_cnn._Trunk(rep, fused_cnn._Part())


def _basic(filters):
    rep = Basic_CNN((84, 84, 4), [8, 4], [4, 2], filters, None, None, torch.nn.ReLU, "cpu")
    return fused_cnn._Trunk(rep, fused_cnn._Part())


def _basic_ks(kernels, strides, filters):
    rep = Basic_CNN((84, 84, 4), kernels, strides, filters, None, None, torch.nn.ReLU, "cpu")
    return fused_cnn._Trunk(rep, fused_cnn._Part())


def _plan(t, B):
    """The plan of a pass over B contiguous uint8 device frames (what the agents feed), at the current switches."""
    return plan_cnn(t.facts(B))


def test_c3_trunk_plans_the_split_fc_and_the_fused_act():
    t = _trunk(84)
    assert t.tail == "flatten" and t.fc[0][0].in_features == 6400
    p = _plan(t, 16384)
    assert ops.S3_GEMMS and p.fc0_fwd == "K40G" and p.fc0_dx == "K40G-act"
    p = _plan(t, 1024)
    assert p.fc0_fwd == "linear" and p.fc0_dx == "mm"        # the rollout's forwards stay on hipBLASLt
    c0s = [min(c, 6400 - 256) for c in range(0, 6400, 256)]
    assert len(c0s) == 25 and c0s[-1] == 6144 and all(c % 64 == 0 for c in c0s)


def test_ragged_fc_width_keeps_split_without_fused_act():
    t = _trunk(76)   # 19 -> 9 -> 9: 9 x 9 x 64 = 5184 columns
    in_f = t.fc[0][0].in_features
    assert in_f == 5184 and in_f % 256 == 64
    p = _plan(t, 16384)
    assert p.fc0_fwd == "K40G" and p.fc0_dx == "K40G"
    c0s = [min(c, in_f - 256) for c in range(0, in_f, 256)]
    assert c0s[-1] == in_f - 256 and c0s[-2] + 256 > c0s[-1]   # the overlap, no padded block


def test_fc_split_switches():
    t = _trunk(84)
    old = fused_cnn._Trunk.fc_split, fused_cnn._Trunk.fc_fuse_act
    x = torch.empty((16384, 0), dtype=torch.uint8)   # _Trunk.plan reads the rows, the dtype, the layout and the device
    try:
        p = t.plan(x)
        assert p.fc0_fwd == "K40G" and p.fc0_dx == "K40G-act" and t.plan(x) is p
        fused_cnn._Trunk.fc_fuse_act = False     # a switch flipped after the first plan takes effect
        p = t.plan(x)
        assert p.fc0_fwd == "K40G" and p.fc0_dx == "K40G" and _plan(t, 16384).fc0_dx == "K40G"
        fused_cnn._Trunk.fc_split = False
        p = t.plan(x)
        assert p.fc0_fwd == "linear" and p.fc0_dx == "mm" and _plan(t, 16384).fc0_fwd == "linear"
    finally:
        fused_cnn._Trunk.fc_split, fused_cnn._Trunk.fc_fuse_act = old


# ---- named production cases ------------------------------------------------------------------------------------------
def test_c3_update_plan():
    p = _plan(_trunk(84), 16384)
    assert p.convs == (ConvForm("K25", "K26", "K26", "none"), ConvForm("K28", "K28-dgrad", "K29", "K27"),
                       ConvForm("K28", "K40G-act", "K29", "K28"))
    assert (p.frames, p.slack, p.fc0_fwd, p.fc0_dw, p.fc0_dx) == ("none", 0, "K40G", "K41V", "K40G-act")
    assert p.launches("forward") == ["xpa_conv1_u8_fwd", "xpa_conv_fwd", "xpa_conv_fwd", "xpa_s3_gemm_group",
                                     "xpa_bias_act"]
    assert p.launches("backward") == [
        "xpa_act_bwd_bias", "xpa_colsum_finalize", "xpa_s3_wgrad", "xpa_s3_wgrad", "xpa_colsum_finalize_batch_map",
        "xpa_s3_gemm_group_act", "xpa_colsum_finalize",
        "xpa_conv_wgrad", "xpa_colsum_finalize", "xpa_conv_dgrad", "xpa_colsum_finalize",
        "xpa_conv_wgrad", "xpa_colsum_finalize", "xpa_conv_dgrad_s2k",
        "xpa_conv1_u8_wgrad_act", "xpa_colsum_finalize", "xpa_colsum_finalize"]


def test_c3_rollout_plan_is_the_library_plan():
    p = _plan(_trunk(84), 1024)
    assert p.convs == (ConvForm("K25", "K26", "K26", "none"), ConvForm("miopen", "K22", "miopen", "K27"),
                       ConvForm("miopen", "K22", "miopen", "miopen"))
    assert (p.frames, p.slack, p.fc0_fwd, p.fc0_dw, p.fc0_dx) == ("none", 0, "linear", "mm", "mm")


def test_c5_plan():
    p = _plan(_basic([32, 64]), 2048)
    assert p.convs == (ConvForm("K25", "K26", "K26", "none"), ConvForm("miopen", "K24", "miopen", "K27"))
    assert (p.frames, p.slack, p.fc0_fwd, p.fc0_dw, p.fc0_dx) == ("none", 0, None, "mm", "mm")
    assert p.launches("forward") == ["xpa_conv1_u8_fwd", "xpa_bias_act", "xpa_global_maxpool"]


def test_small_channel_net_is_k28_everywhere():
    for B in (64, 2048):
        p = _plan(_basic([8, 8]), B)
        assert p.convs == (ConvForm("K28", "K28-dgrad", "K29", "none"), ConvForm("K28", "K24", "K29", "K28"))
        assert p.frames == "forward" and p.launches("forward")[0] == "xpa_frames_to_f32"


def test_fc_split_over_a_library_last_block():
    """B = 8192: the fc split's rows, but 819200 output pixels of the last block (below igemm_min_rows).  No K28 output,
    so no slack; K41V all the same, only because 6400 is a multiple of 128."""
    p = _plan(_trunk(84), 8192)
    assert p.convs[-1] == ConvForm("miopen", "K40G-act", "miopen", "miopen")
    assert p.slack == 0 and p.fc0_dw == "K41V" and p.fc0_fwd == "K40G"
    q = _plan(_trunk(76), 8192)   # the ragged width there: no slack to read, the library GEMM
    assert q.convs[-1].fwd == "miopen" and q.slack == 0 and q.fc0_dw == "mm" and q.fc0_fwd == "K40G"


def test_ragged_width_takes_the_padded_weight_gradient():
    p = _plan(_trunk(76), 16384)
    assert p.convs[-1].fwd == "K28" and p.fc0_dw == "K41V-padded" and p.slack == 5248 - 5184
    assert p.launches("backward")[2:5] == ["xpa_s3_wgrad_padded", "xpa_s3_wgrad_padded",
                                           "xpa_colsum_finalize_batch_map"]


def test_strided_conv0_gradients_move_the_frame_copy_into_the_backward():
    f = _trunk(84).facts(16384)._replace(grads0_contig=False)
    p = plan_cnn(f)
    assert p.convs[0] == ConvForm("K25", "K29", "K29", "none") and p.frames == "backward"
    assert p.launches("backward")[-4:] == ["xpa_frames_to_f32", "xpa_conv_wgrad", "xpa_colsum_finalize",
                                           "xpa_colsum_finalize"]


def test_conv_output_of_2_gib_is_not_planned_k28():
    """K28 stores through a 32-bit buffer record as it loads through one: a stride-1 conv with more output than input
    channels (32 -> 64, 21 x 21) whose output reaches 2 GiB while its input stays at half that is the library's in the
    forward too.  Facts only: no tensor of that size exists."""
    t = _basic_ks([8, 3], [4, 1], [32, 64])
    c = t.conv_facts[1]
    assert c.igemm and c.igemm_dgrad and (c.cin, c.cout, c.k, c.s, c.p) == (32, 64, 3, 1, 1)
    for B, over in ((19000, False), (19021, False), (19022, True), (20000, True)):
        x_bytes, y_bytes = B * 21 * 21 * 32 * 4, B * 21 * 21 * 64 * 4
        assert x_bytes < 2 ** 31 and (y_bytes >= 2 ** 31) == over, B
        form = _plan(t, B).convs[1]
        assert form == (ConvForm("miopen", "K24", "miopen", "miopen") if over else
                        ConvForm("K28", "K24", "K29", "K28")), (B, form)


# ---- invariants over every switch ------------------------------------------------------------------------------------
SWITCHES = {"use_igemm": (True, False), "igemm_min_rows": (0, 1 << 20), "fc_split": (True, False),
            "fc_split_min_rows": (0, 8192), "fc_fuse_act": (True, False), "fc_wsplit": (True, False),
            "s3_gemms": (True, False)}


@pytest.mark.parametrize("name", ["c3", "ragged", "c5", "small"])
def test_plan_invariants_over_every_switch(name):
    t = {"c3": lambda: _trunk(84), "ragged": lambda: _trunk(76), "c5": lambda: _basic([32, 64]),
         "small": lambda: _basic([8, 8])}[name]()
    small = [min(c.cin, c.cout) < 16 for c in t.conv_facts]
    seen = raised = 0
    for B in (96, 8192, 16384):
        base = t.facts(B)
        for values in itertools.product(*SWITCHES.values()):
            f = base._replace(**dict(zip(SWITCHES, values)))
            try:
                p = plan_cnn(f)
            except RuntimeError as e:   # the small-channel refusal: only with use_igemm off, only on such a net
                assert "small-channel MIOpen route is refused" in str(e) and not f.use_igemm, f
                assert any(s and not (i == 0 and f.u8_conv1) for i, s in enumerate(small)), f
                raised += 1
                continue
            seen += 1
            n = len(p.convs)
            assert n == len(f.convs)
            for i, c in enumerate(p.convs):
                assert c.fwd in ("K25", "K28", "miopen") and c.wgrad in ("K26", "K29", "miopen"), (f, p)
                # exactly one stage forms each block's dz and bias gradient
                assert c.act_bwd in ("K22", "K24", "K26", "K29", "K40G-act", "K28-dgrad"), (f, p)
                assert (c.act_bwd == "K28-dgrad") == (i + 1 < n and p.convs[i + 1].dgrad == "K28"), (f, p)
                assert (c.act_bwd == "K24") == (i == n - 1 and f.tail == "maxpool"), (f, p)
                if c.act_bwd == "K40G-act":
                    assert i == n - 1 and p.fc0_dx == "K40G-act", (f, p)
                if c.act_bwd in ("K26", "K29"):   # folded into the weight gradient that runs
                    assert c.wgrad == c.act_bwd and i == 0, (f, p)
                assert (c.dgrad == "none") == (i == 0) and c.dgrad in ("none", "K27", "K28", "miopen"), (f, p)
                if small[i]:
                    assert "miopen" not in c, (f, p)
                if c.fwd == "K25" or c.wgrad == "K26":
                    assert i == 0 and f.u8_conv1, (f, p)
            assert (p.fc0_dx == "K40G-act") == (p.convs[-1].act_bwd == "K40G-act"), (f, p)
            if p.fc0_dw == "K41V-padded":
                assert p.slack > 0 and p.convs[-1].fwd == "K28" and (f.fc0[0] + p.slack) % 128 == 0, (f, p)
            else:
                assert p.slack == 0, (f, p)
            assert p.frames == ("forward" if p.convs[0].fwd != "K25" else
                                "backward" if p.convs[0].wgrad != "K26" else "none"), (f, p)
            assert (p.fc0_fwd is None) == (f.tail == "maxpool"), (f, p)
            if p.fc0_fwd != "K40G":
                assert p.fc0_dx == "mm", (f, p)
            for d in ("forward", "backward"):
                assert all(s in _lib.SIGNATURES for s in p.launches(d)), (f, p)
    assert seen and (raised > 0) == (name == "small")
    with pytest.raises(ValueError):
        p.launches("sideways")


def test_grouped_split_gemm_refuses_host_tensors():
    a = torch.zeros(512, 64)
    b = torch.zeros(16, dtype=torch.uint8)
    c = torch.zeros(512, 256)
    with pytest.raises(ValueError):
        ops.s3_gemm_group([(a, b, c)], 64)
    with pytest.raises(ValueError):
        ops.s3_gemm_group_act([(a, b, c)], 64, [c], 1, 0.0, 64, torch.zeros(2, 64))


def test_conv_form_defaults():
    L = ops.lib()
    assert L.xpa_conv1_form(-1) == 7
    assert L.xpa_conv_igemm_form(-1) == 0
