"""Explicit (autograd-free) forward / backward of the convolutional policies: the AC_CNN_Atari actor-critic (C3) and
the Basic_CNN Q-network of PER-DQN (C5).

Reference: AC_CNN_Atari xuance/torch/representations/cnn.py:45-93 (conv blocks with padding (k - s) // 2 + ReLU,
Flatten, fc blocks), Basic_CNN cnn.py:5-40 (conv blocks, AdaptiveMaxPool2d((1, 1)), Flatten), cnn_block / mlp_block
xuance/torch/utils/layers.py:8-57, Categorical_AC_Policy xuance/torch/policies/categorical.py:61-85, BasicQnetwork
deterministic.py:148-182; the learners' loss.backward() (a2c_learner.py:31-33, perdqn_learner.py:37-40).

Every activation stays NHWC ([rows = B*H*W, C] row-major), the layout the uint8 frames arrive in.  A trunk's forward
and backward run from a CnnPlan (cnn_plan.py): _Trunk.plan is the only reader of the switches and the only place a
capability is tested, the stages dispatch on the plan's fields ("Where the CNN trunk's forms are
decided"):
  frames    "forward": K20 xpa_frames_to_f32 ahead of the first conv; "backward": K25 read the uint8 frames and only
            the first conv's library weight gradient needs the f32 copy; "none": K25 + K26, no f32 frames anywhere
  fwd       per conv block: "K25" xpa_conv1_u8_fwd (the 4 x 8 x 8 -> 32 conv on fp32 MFMA straight from the uint8
            frames as sum x (w / 255) — one f32 rounding per term like the reference's sum float(x / 255) w —, bias +
            activation in its epilogue), "K28" xpa_conv_fwd (the same epilogue; the last block's output with `slack`
            floats after it), "miopen" (conv2d without bias on the channels-last view + K21 xpa_bias_act in place)
  tail      AC_CNN_Atari: Flatten in NHWC order — the first fc layer uses its weight with the columns permuted from
            the reference's (C, H, W) order to (H, W, C) (one 13 MB copy per parameter update, instead of an
            NHWC -> NCHW copy of the [B, 6400] activations every forward); Basic_CNN: K23 xpa_global_maxpool (max +
            argmax per (b, c), torch's tie rule)
  fc0_fwd   "K40G" (the three-way split on the bf16 matrix cores + K21) or "linear" (hipBLASLt + K21)
  fc0_dw    "K41V" / "K41V-padded" (split weight-gradient slices + the batched f64 finalize) or "mm"; permuted back into
            the reference layout either way
  fc0_dx    "K40G-act" (the last conv block's activation backward + bias partials in its epilogue), "K40G" or "mm"
  act_bwd   who forms a conv block's dz and bias gradient: "K22" xpa_act_bwd_bias, "K24" (the pooled gradient routed
            to the argmax), "K26" / "K29" (folded into the weight gradient), "K40G-act", "K28-dgrad" (the epilogue of
            the following block's data gradient)
  wgrad     "K26" xpa_conv1_u8_wgrad_act (from the uint8 frames), "K29" xpa_conv_wgrad, "miopen"
  dgrad     "K27" xpa_conv_dgrad_s2k (the 4 x 4 stride-2 32 -> 64 conv), "K28" xpa_conv_dgrad, "miopen", "none"
The heads / Q head are GEMMs + K21 forward, GEMMs + K10 / K22 bias column sums backward.
Parameter gradients are written into the parameters' .grad views (allocated when missing).
"""
from typing import NamedTuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops
from .cnn_plan import CnnFacts, CnnPlan, conv_facts, k22_width, out_hw, plan_cnn
from .fused_mlp import _act_code, _no_form, _parse
from .policies import AC_CNN_Atari, Basic_CNN, policy_discrete


def _out_hw(conv, H, W):
    return out_hw(H, W, conv.kernel_size[0], conv.stride[0], conv.padding[0])


def _conv_facts(conv, code, igemm_ok=None, wgrad_ok=None):
    return conv_facts(conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.padding,
                      conv.padding_mode == "zeros", conv.weight.is_contiguous(), code, igemm_ok, wgrad_ok)


class _Ctx(NamedTuple):
    """What a trunk forward leaves for its backward."""
    hs: list          # the uint8 frames (K25) or their f32 copy, then every conv block's output (NHWC)
    am: object        # the max pool's argmax, or None
    flat: object      # the first fc layer's input, or None
    fouts: list       # the fc layers' outputs
    plan: CnnPlan


def _conv_layers(model):
    """(conv blocks [(conv, act code, slope)], tail, fc layers): tail "flatten" (AC_CNN_Atari) or "maxpool"
    (Basic_CNN)."""
    convs, i = [], 0
    mods = list(model)
    while i < len(mods) and isinstance(mods[i], nn.Conv2d):
        conv = mods[i]
        nxt = mods[i + 1] if i + 1 < len(mods) else None
        act = nxt if isinstance(nxt, (nn.ReLU, nn.LeakyReLU, nn.Tanh)) else None
        if conv.bias is None or conv.groups != 1 or tuple(conv.dilation) != (1, 1):
            raise ValueError("expected Conv2d with bias, groups 1, dilation 1")
        convs.append((conv,) + _act_code(act))
        i += 2 if act is not None else 1
    if not convs:
        raise ValueError("no conv blocks")
    if i < len(mods) and isinstance(mods[i], nn.AdaptiveMaxPool2d):
        if tuple(nn.modules.utils._pair(mods[i].output_size)) != (1, 1) or i + 1 >= len(mods) \
                or not isinstance(mods[i + 1], nn.Flatten) or i + 2 != len(mods):
            raise ValueError("expected AdaptiveMaxPool2d((1, 1)) + Flatten as the tail")
        return convs, "maxpool", []
    if i >= len(mods) or not isinstance(mods[i], nn.Flatten):
        raise ValueError("expected Flatten (or a global max pool) after the conv blocks")
    fc = _parse(mods[i + 1:])
    if not fc:
        raise ValueError("Flatten without fc layers")
    return convs, "flatten", fc


class _Part:
    """Per-block partial buffers of the bias-gradient reductions, by shape."""

    def __init__(self):
        self.bufs = {}

    def buf(self, key, shape, device):
        """A cached float32 buffer by key (K28 / K29 partials)."""
        p = self.bufs.get(key)
        if p is None:
            p = torch.empty(shape, dtype=torch.float32, device=device)
            self.bufs[key] = p
        return p

    def get(self, rows, cols, device, k22):
        key = (rows, cols, k22)
        p = self.bufs.get(key)
        if p is None:
            L = ops.lib()
            G = int(L.xpa_act_bwd_bias_num_partials(rows, cols)) if k22 else int(L.xpa_act_bwd_num_partials(rows))
            p = torch.empty((G, cols), dtype=torch.float32, device=device)
            self.bufs[key] = p
        return p


def _bias_act(code, y2d, bias, slope):
    _lib.call(ops.lib().xpa_bias_act, code, ops._p(y2d), y2d.shape[0], y2d.shape[1],
              ops._p(bias) if bias is not None else None, float(slope), ops._stream(y2d.device))


def _act_bwd_bias(parts, code, g2d, h2d, slope, bias_grad):
    """g2d <- g2d * act'(h2d) in place; bias_grad <- column sums (K22, or K10 for widths K22 does not take)."""
    rows, cols = g2d.shape
    L, s = ops.lib(), ops._stream(g2d.device)
    if not g2d.is_contiguous():
        raise ValueError("gradient rows must be contiguous")
    k22 = k22_width(cols)
    part = parts.get(rows, cols, g2d.device, k22)
    hp = ops._p(h2d) if code else None
    gp = ops._p(g2d) if code else None
    if k22:
        _lib.call(L.xpa_act_bwd_bias, code, ops._p(g2d), hp, rows, cols, float(slope), gp, ops._p(part), s)
    else:
        _lib.call(L.xpa_act_bwd_colsum, code, ops._p(g2d), hp, rows, cols, float(slope), gp, ops._p(part), s)
    _lib.call(L.xpa_colsum_finalize, ops._p(part), part.shape[0], cols, ops._p(bias_grad), s)


def _chain(layers, x):
    outs, h = [], x
    for lin, code, slope in layers:
        h = F.linear(h, lin.weight, lin.bias)
        if code and k22_width(h.shape[1]):
            _bias_act(code, h, None, slope)   # K21 in place
        elif code == 1:
            F.leaky_relu(h, slope, inplace=True)
        elif code == 2:
            h.tanh_()
        outs.append(h)
    return outs


def _chain_backward(parts, layers, inputs, outs, g, acc=None, need_dx=True):
    """Linear(+act) chain backward; returns d(input) (added into acc when given)."""
    for j in range(len(layers) - 1, -1, -1):
        lin, code, slope = layers[j]
        g = g.contiguous()
        _act_bwd_bias(parts, code, g, outs[j], slope, lin.bias.grad)
        torch.mm(g.t(), inputs[j], out=lin.weight.grad)
        if j == 0 and not need_dx:
            return None
        if j == 0 and acc is not None:
            g = acc.addmm_(g, lin.weight)
        else:
            g = torch.mm(g, lin.weight)
    return g


def _ensure_grads(params):
    for p in params:
        if p.grad is None:
            p.grad = torch.zeros_like(p)


class _Trunk:
    """The explicit forward / backward of one AC_CNN_Atari or Basic_CNN representation."""

    def __init__(self, rep, parts):
        # structural, not nominal: the reference's own AC_CNN_Atari / Basic_CNN (cnn.py:5-93: a `.model` nn.Sequential
        # of conv blocks [+ max pool] + Flatten [+ fc blocks], input_shape (C, H, W), observations / 255 in forward)
        # take this path as ours do; _conv_layers raises ValueError on anything else
        if not (isinstance(rep, (AC_CNN_Atari, Basic_CNN)) or (isinstance(getattr(rep, "model", None), nn.Sequential)
                                                                and len(getattr(rep, "input_shape", ())) == 3)):
            raise ValueError("representation %r has no explicit CNN path" % type(rep).__name__)
        self.rep = rep
        self.convs, self.tail, self.fc = _conv_layers(rep.model)
        for conv, _, _ in self.convs:
            if not k22_width(conv.out_channels):
                raise ValueError("conv channels must be a multiple of 4 dividing 1024")
        C, H, W = rep.input_shape
        self.in_hwc = (H, W, C)
        shape = (C, H, W)
        for conv, _, _ in self.convs:
            shape = (conv.out_channels,) + _out_hw(conv, shape[1], shape[2])
        self._chw = shape
        if self.tail == "flatten" and self.fc[0][0].in_features != shape[0] * shape[1] * shape[2]:
            raise ValueError("fc input width does not match the conv output")
        self._w_hwc = None      # the first fc weight with (H, W, C)-ordered columns, refreshed after each update
        self._w_ver = 0         # bumped whenever _w_hwc is re-derived (the fc split planes follow it)
        self._fcs = None        # K40G planes of _w_hwc (forward k halves, data-gradient column blocks) + their version
        self.stale = True
        self._dw_tmp = None
        self._fcq = ops.ColsumQueue()   # K41V's batched finalize
        self.err = None         # K24's device error word (argmax outside [0, HW)), made by the first backward
        self._plans = {}        # (switches, B, the input's kind, conv 0's gradient layout) -> CnnPlan
        self.last_plan = None   # the plan of the latest forward
        self.parts = parts
        self.n_params = 2 * (len(self.convs) + len(self.fc))
        # the static shape rules of K27 / K28 / K29, asked once (the library's xpa_conv_igemm_ok and xpa_conv_wgrad_ok
        # included)
        igemm_ok, wgrad_ok = ops.lib().xpa_conv_igemm_ok, ops.lib().xpa_conv_wgrad_ok
        self.conv_facts = tuple(_conv_facts(conv, code, igemm_ok, wgrad_ok) for conv, code, _ in self.convs)
        # K25: the first conv block straight from the uint8 frames (4 channels, 8 x 8 kernel, 32 outputs: the Nature
        # CNN's first layer); the f32 frame copy (K20) is then only made in the backward, for MIOpen's weight gradient
        c0 = self.conv_facts[0]
        self.u8_conv1 = C == 4 and c0.cin == 4 and c0.cout == 32 and c0.k == 8 and c0.square and c0.zeros
        # a small-channel conv (< 16 in or out) must run on K28 / K29 (forward, weight gradient and, past the first
        # block, the data gradient): the planner refuses MIOpen's small-channel route.  A net with such a conv that
        # K28 / K29 cannot take (e.g. a 3-channel RGB first conv, in_channels % 4 != 0) gets no explicit path:
        # ValueError here sends the learner to the generic autograd path instead of failing mid-update.
        for i, c in enumerate(self.conv_facts):
            if min(c.cin, c.cout) >= 16 or (i == 0 and self.u8_conv1):
                continue
            if not c.igemm or (i > 0 and not c.k27 and not c.igemm_dgrad):
                raise ValueError("conv %d -> %d channels (kernel %s): no K28 / K29 form and the small-channel "
                                 "library route is refused" % (c.cin, c.cout, tuple(self.convs[i][0].kernel_size)))

    # The switches (read by plan() alone).
    # use_igemm: K28 / K29 for the convs they take (False: MIOpen for every conv, the r02 path).  They hold one weight
    # image per CU and tile the output rows 32 at a time per wave, so below ~1 M output rows (igemm_min_rows) a launch
    # has too few tiles per CU to balance (C5's batch 2048 = 800 rows per CU = 25 tiles over 16 waves) and MIOpen's
    # kernels measure faster there (tools/c5_ab.py: 2.26 vs 2.65 ms per C5 learner step; C3's rollout forwards at 1024
    # frames 71 vs 84-94 us).  Small-channel convs (< 16 in or out: the test nets, r02's fault suspect) always take
    # K28 / K29.
    use_igemm = True
    igemm_min_rows = 1 << 20
    # r05, fc_split: the first fc layer of the update's minibatches (C3: [16384, 6400] x [6400, 512]) on the bf16 matrix
    # cores by the three-way split (K40G: one launch per GEMM; forward in 2 k halves x 256-column blocks, summed in a
    # fixed order; the data gradient in 256-column blocks, the last one aligned to the end so no block is padded — the
    # columns it shares with its neighbour come out bit-identical from both).  The rollout's 1024-frame forwards stay
    # on hipBLASLt (fc_split_min_rows).
    fc_split = True
    fc_split_min_rows = 8192
    # r05, fc_fuse_act: with the fc split, the data gradient's epilogue also applies the last conv block's activation
    # backward and writes its bias-gradient partials (xpa_s3_gemm_group_act): that block's K22 pass over
    # [B x H x W, C] is gone
    fc_fuse_act = True
    # r06, fc_wsplit: the first fc layer's weight gradient on the split too (was hipBLASLt's f32 GEMM: 822 us per C3
    # minibatch, profiles/r05/r05k28b): dW^T = flat^T g as K41V slices per 256-column half of g (AC_CNN_Atari: flat
    # [B, 6400] = 50 row tiles of 128; a width that is not a multiple of 128 takes the padded form, the columns past a
    # row reading the next row or the slack the forward leaves after the last row, into output rows the finalize map
    # drops); the batched f64 finalize writes the kept rows transposed into dW.  Same row rule as the forward's split.
    fc_wsplit = True

    def _grads0_contig(self):
        """Conv 0's weight and bias gradients are contiguous, as K26 writes them (a missing one is allocated so)."""
        c0 = self.convs[0][0]
        return all(p.grad is None or p.grad.is_contiguous() for p in (c0.weight, c0.bias))

    def _pass_facts(self, B, x_u8):
        """What can differ between two passes of this trunk (CnnFacts' last fields, and the plan cache's key): the only
        reader of the switches above and of ops.S3_GEMMS."""
        return (B, x_u8, self._grads0_contig(), self.use_igemm, self.igemm_min_rows, self.fc_split,
                self.fc_split_min_rows, self.fc_fuse_act, self.fc_wsplit, ops.S3_GEMMS)

    def facts(self, B, x_u8=True):
        """The CnnFacts of a pass over B frames (x_u8: a contiguous uint8 device tensor, what the agents feed)."""
        lin = self.fc[0][0] if self.fc else None
        return CnnFacts(self.conv_facts, self.in_hwc, self.tail,
                        (lin.in_features, lin.out_features) if lin is not None else None,
                        tuple((lin.out_features, code) for lin, code, _ in self.fc), self.u8_conv1,
                        *self._pass_facts(B, x_u8))

    def plan(self, x):
        """The CnnPlan of one forward + backward over the frames x (of which only the rows, the dtype, the contiguity
        and the device type are read).  Host logic alone (cnn_plan.plan_cnn), cached under every switch's value, B, the
        input's kind and conv 0's gradient layout: a switch flipped later takes effect, a steady pass pays one
        lookup."""
        x_u8 = x.dtype == torch.uint8 and x.is_contiguous() and x.device.type == "cuda"
        key = self._pass_facts(x.shape[0], x_u8)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = plan_cnn(self.facts(x.shape[0], x_u8))
        return plan

    def params(self):
        out = []
        for conv, _, _ in self.convs:
            out += [conv.weight, conv.bias]
        for lin, _, _ in self.fc:
            out += [lin.weight, lin.bias]
        return out

    def refresh(self):
        self.stale = True
        if self.tail == "flatten":
            self._fc0_weight()

    def _fc0_weight(self):
        if self.stale or self._w_hwc is None:
            w = self.fc[0][0].weight
            Cl, Hl, Wl = self._chw
            if self._w_hwc is None:
                self._w_hwc = torch.empty_like(w)
            self._w_hwc.view(w.shape[0], Hl, Wl, Cl).copy_(w.view(w.shape[0], Cl, Hl, Wl).permute(0, 2, 3, 1))
            self.stale = False
            self._w_ver += 1
        return self._w_hwc

    def _fc_planes(self):
        """The split planes of the current _w_hwc: forward (column block j, k half p) and data-gradient column
        blocks, re-split (4 matrices per launch) whenever _w_hwc was re-derived."""
        w = self._fc0_weight()
        if self._fcs is not None and self._fcs[0] == self._w_ver:
            return self._fcs
        out_f, in_f = w.shape
        kh = in_f // 2
        fwd = [w[j * 256:(j + 1) * 256, p * kh:(p + 1) * kh].t() for j in range(out_f // 256) for p in range(2)]
        c0s = [min(c, in_f - 256) for c in range(0, in_f, 256)]
        dgr = [w[:, c0:c0 + 256] for c0 in c0s]
        old = self._fcs
        if old is None:
            nb_f, nb_d = int(ops.lib().xpa_s3_split_bytes(kh, 256)), int(ops.lib().xpa_s3_split_bytes(out_f, 256))
            bufs_f = [torch.empty(nb_f, dtype=torch.uint8, device=w.device) for _ in fwd]
            bufs_d = [torch.empty(nb_d, dtype=torch.uint8, device=w.device) for _ in dgr]
        else:
            bufs_f, bufs_d = old[1], old[2]
        pairs = list(zip(fwd, bufs_f)) + list(zip(dgr, bufs_d))
        for i in range(0, len(pairs), 4):
            ops.s3_split_batch(pairs[i:i + 4])
        self._fcs = (self._w_ver, bufs_f, bufs_d, c0s)
        return self._fcs

    def _fc0_forward_split(self, flat, lin, code, slope):
        rows, in_f = flat.shape
        out_f, kh = lin.out_features, in_f // 2
        _, bf, _, _ = self._fc_planes()
        part = self.parts.buf(("fcs", rows, out_f), (2, rows, out_f), flat.device)
        probs = [(flat[:, p * kh:(p + 1) * kh], bf[j * 2 + p], part[p, :, j * 256:(j + 1) * 256])
                 for j in range(out_f // 256) for p in range(2)]
        ops.s3_gemm_group(probs, kh)
        s = torch.add(part[0], part[1])
        _bias_act(code, s, lin.bias, slope)
        return s

    def _fc0_dgrad_split_act(self, g, y_flat):
        """dz of the last conv block (its output gradient x act'(its output)) from the fc's K40G data gradient, and
        that block's bias gradient (f64 finalize of the per-block partials)."""
        rows = g.shape[0]
        _, _, bd, c0s = self._fc_planes()
        conv, code, slope = self.convs[-1]
        C = conv.out_channels
        dz = torch.empty((rows, self.fc[0][0].in_features), dtype=torch.float32, device=g.device)
        G = int(ops.lib().xpa_s3_gemm_group_act_num_partials(len(c0s), rows))
        part = self.parts.buf(("fcab", rows, C), (G, C), g.device)
        ops.s3_gemm_group_act([(g, b, dz[:, c0:c0 + 256]) for b, c0 in zip(bd, c0s)], g.shape[1],
                              [y_flat[:, c0:c0 + 256] for c0 in c0s], code, slope, C, part)
        _lib.call(ops.lib().xpa_colsum_finalize, ops._p(part), G, C, ops._p(conv.bias.grad), ops._stream(g.device))
        return dz

    def _fc0_wgrad_split(self, g, flat):
        """K41V / K41V-padded (by flat's width): self._dw_tmp = g^T flat ([out, in], the forward's (H, W, C) column
        order).  Returns True; raises where the buffers do not meet the form (rows not contiguous, or a ragged width
        without the forward's slack after the last row)."""
        rows, in_f = flat.shape
        m = (in_f + 127) // 128 * 128
        if not (g.is_contiguous() and flat.stride(1) == 1 and flat.stride(0) == in_f
                and flat.untyped_storage().nbytes() // 4 >= flat.storage_offset() + (rows - 1) * in_f + m):
            _no_form("the fc weight gradient on these buffers", "K41V" if m == in_f else "K41V-padded")
        out_f = g.shape[1]
        S = ops.s3_wgrad_slices(rows, m)
        for h in range(out_f // 256):
            part = self.parts.buf(("fcw", h, S, m), (S, m, 256), g.device)
            ops.s3_wgrad(flat, g[:, 256 * h:256 * (h + 1)], out=part, slices=S, m=m if m != in_f else None)
            self._fcq.add(part.view(S, -1), self._dw_tmp[256 * h:256 * (h + 1)], tmap=(256, in_f, in_f))
        self._fcq.flush(g.device)
        return True

    def _fc0_dgrad_split(self, g):
        rows = g.shape[0]
        _, _, bd, c0s = self._fc_planes()
        in_f = self.fc[0][0].in_features
        dx = torch.empty((rows, in_f), dtype=torch.float32, device=g.device)
        ops.s3_gemm_group([(g, b, dx[:, c0:c0 + 256]) for b, c0 in zip(bd, c0s)], g.shape[1])
        return dx

    @staticmethod
    def frames(x):
        """uint8 [B, H, W, C] -> float32 / 255 [B, H, W, C] (K20)."""
        if x.dtype != torch.uint8 or x.device.type != "cuda" or not x.is_contiguous():
            raise ValueError("frames must be a contiguous uint8 ROCm tensor [B, H, W, C]")
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        _lib.call(ops.lib().xpa_frames_to_f32, ops._p(x), x.numel(), ops._p(out), ops._stream(x.device))
        return out

    def _conv1_u8(self, xu):
        """K25: act(conv1(x / 255) + b) from the uint8 frames xu [B, H, W, 4] -> NHWC f32."""
        conv, code, slope = self.convs[0]
        B, H, W, C = xu.shape
        k, st, pd = 8, conv.stride[0], conv.padding[0]
        OH, OW = _out_hw(conv, H, W)
        w = conv.weight if conv.weight.is_contiguous() else conv.weight.contiguous()
        y = torch.empty((B, OH, OW, 32), dtype=torch.float32, device=xu.device)
        _lib.call(ops.lib().xpa_conv1_u8_fwd, code, ops._p(xu), B, H, W, C, k, st, pd, ops._p(w), ops._p(conv.bias), 32,
                  float(slope), ops._p(y), ops._stream(xu.device))
        return y

    @torch.no_grad()
    def forward(self, x):
        """x uint8 [B, H, W, C] -> (state [B, d], context for backward).  With K25 the context keeps the uint8 frames
        as its first entry (backward converts them for the first conv's weight gradient)."""
        B = x.shape[0]
        xu = x.reshape((B,) + self.in_hwc)
        plan = self.last_plan = self.plan(xu)
        h = self.frames(xu) if plan.frames == "forward" else xu
        hs = [h]
        last = len(self.convs) - 1
        for i, (conv, code, slope) in enumerate(self.convs):
            fwd = plan.convs[i].fwd
            if fwd == "K25" and i == 0:
                y = self._conv1_u8(h)
            elif fwd == "K28":   # bias + activation fused; the last block's output (the fc layer's flat input) with
                # the plan's slack after it, where the padded K41V reads it as 128-row tiles
                y = self._conv_fwd(conv, code, slope, h, slack=plan.slack if i == last else 0)
            elif fwd == "miopen":
                z = F.conv2d(h.permute(0, 3, 1, 2), conv.weight, None, conv.stride, conv.padding)
                y = z.permute(0, 2, 3, 1)
                if not y.is_contiguous():
                    y = y.contiguous()
                _bias_act(code, y.view(-1, y.shape[3]), conv.bias, slope)
            else:
                _no_form("conv block %d's forward" % i, fwd)
            hs.append(y)
            h = y
        if self.tail == "maxpool":
            Cl = h.shape[3]
            s = torch.empty((B, Cl), dtype=torch.float32, device=x.device)
            am = torch.empty((B, Cl), dtype=torch.int32, device=x.device)
            _lib.call(ops.lib().xpa_global_maxpool, ops._p(h), B, h.shape[1] * h.shape[2], Cl, ops._p(s), ops._p(am),
                      ops._stream(x.device))
            return s, _Ctx(hs, am, None, [], plan)
        flat = h.reshape(B, -1)                  # (H, W, C) order: no copy
        fouts = []
        s = flat
        for j, (lin, code, slope) in enumerate(self.fc):
            if j == 0 and plan.fc0_fwd == "K40G":
                if not flat.is_contiguous():
                    _no_form("the first fc layer on a strided input", "K40G")
                s = self._fc0_forward_split(flat, lin, code, slope)
            elif j == 0 and plan.fc0_fwd != "linear":
                _no_form("the first fc layer's forward", plan.fc0_fwd)
            else:
                w = self._fc0_weight() if j == 0 else lin.weight
                s = F.linear(s, w, lin.bias)
                if code:
                    _bias_act(code, s, None, slope)
            fouts.append(s)
        return s, _Ctx(hs, None, flat, fouts, plan)

    @staticmethod
    def _conv_fwd(conv, code, slope, h, slack=0):
        """K28 forward: act(conv(h) + b), h NHWC f32 [B, H, W, C] -> NHWC [B, OH, OW, out].  slack: floats of the same
        allocation after the output (readable, never written: the padded K41 reads them into output rows it drops)."""
        B, H, W, C = h.shape
        k, st, pd = conv.kernel_size[0], conv.stride[0], conv.padding[0]
        OH, OW = _out_hw(conv, H, W)
        h = h if h.is_contiguous() else h.contiguous()
        n = B * OH * OW * conv.out_channels
        y = torch.empty((n + slack,), dtype=torch.float32, device=h.device)[:n].view(B, OH, OW, conv.out_channels)
        _lib.call(ops.lib().xpa_conv_fwd, code, ops._p(h), B, H, W, C, ops._p(conv.weight), ops._p(conv.bias),
                  conv.out_channels, k, st, pd, float(slope), ops._p(y), ops._stream(h.device))
        return y

    def _conv_wgrad(self, conv, g, act, slope, y, x):
        """K29: conv.weight.grad (and with act >= 0: g * act'(y) is the operand and conv.bias.grad is written too) from
        g NHWC [B, OH, OW, out] and the block's input x NHWC f32 [B, H, W, in]."""
        L, st = ops.lib(), ops._stream(g.device)
        B, H, W, C = x.shape
        k = conv.kernel_size[0]
        cout, cols = conv.out_channels, k * k * C
        G = int(L.xpa_conv_wgrad_num_partials())
        part = self.parts.buf(("wg", cout, cols), (G, cout * cols), g.device)
        bpart = self.parts.buf(("wgb", cout), (G, cout), g.device) if act >= 0 else None
        g = g if g.is_contiguous() else g.contiguous()
        _lib.call(L.xpa_conv_wgrad, act, ops._p(g), ops._p(y) if act >= 0 else None, float(slope), ops._p(x), B, H, W,
                  C, cout, k, conv.stride[0], conv.padding[0], ops._p(part), ops._p(bpart), st)
        _lib.call(L.xpa_colsum_finalize, ops._p(part), G, cout * cols, ops._p(conv.weight.grad), st)
        if act >= 0:
            _lib.call(L.xpa_colsum_finalize, ops._p(bpart), G, cout, ops._p(conv.bias.grad), st)

    def _conv_dgrad(self, conv, dz, x_shape, prev):
        """K28 data gradient from dz (the block's pre-activation gradient, NHWC) into the block's input; prev = (code,
        slope, y_prev, bias_grad_prev) of the previous block: its activation backward and bias gradient fused in (the
        result is then that block's dz)."""
        L, st = ops.lib(), ops._stream(dz.device)
        B, H, W, Cin = x_shape
        k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
        OH, OW = dz.shape[1], dz.shape[2]
        dx = torch.empty((B, H, W, Cin), dtype=torch.float32, device=dz.device)
        code, slope, y_prev, bgrad = prev
        G = int(L.xpa_conv_dgrad_num_partials(B, H, W))
        bpart = self.parts.buf(("dgb", B * H * W, Cin), (G, Cin), dz.device)
        dz = dz if dz.is_contiguous() else dz.contiguous()
        _lib.call(L.xpa_conv_dgrad, ops._p(dz), B, OH, OW, conv.out_channels, ops._p(conv.weight), Cin, k, s, p, H, W,
                  code, ops._p(y_prev), float(slope), ops._p(dx), ops._p(bpart), st)
        _lib.call(L.xpa_colsum_finalize, ops._p(bpart), G, Cin, ops._p(bgrad), st)
        return dx

    def _conv1_wgrad(self, conv, g, xu, act=None):
        """K26 partials + the f64 column-sum finalize -> conv.weight.grad.  act None: g is d output after the
        activation backward (K22 / K24 ran); act = (code, slope, y): g is d loss / d y and K26 also forms the
        activation backward and the bias-gradient partials (-> conv.bias.grad)."""
        if xu.dtype != torch.uint8 or not (conv.weight.grad.is_contiguous() and conv.bias.grad.is_contiguous()):
            _no_form("the first conv's weight gradient without uint8 frames or contiguous gradients", "K26")
        L, st = ops.lib(), ops._stream(g.device)
        G = int(L.xpa_conv1_u8_wgrad_num_partials())
        wg_part = self.parts.buf(("k26w", G), (G, 8192), g.device)
        wb_part = self.parts.buf(("k26b", G), (G, 32), g.device)
        g = g if g.is_contiguous() else g.contiguous()
        B, H, W, C = xu.shape
        code, slope, y = act if act is not None else (-1, 0.0, None)
        _lib.call(L.xpa_conv1_u8_wgrad_act, code, ops._p(g), ops._p(y) if y is not None else None, float(slope),
                  ops._p(xu), B, H, W, C, 8, conv.stride[0], conv.padding[0], 32, ops._p(wg_part),
                  ops._p(wb_part) if y is not None else None, st)
        _lib.call(L.xpa_colsum_finalize, ops._p(wg_part), G, 8192, ops._p(conv.weight.grad), st)
        if y is not None:
            _lib.call(L.xpa_colsum_finalize, ops._p(wb_part), G, 32, ops._p(conv.bias.grad), st)

    @staticmethod
    def _dgrad_ok(conv):
        """K27 takes conv's data gradient (ConvFacts.k27: the shape rule alone, what the planner reads)."""
        return _conv_facts(conv, 0).k27

    @staticmethod
    def _dgrad(conv, g, in_shape):
        """K27: d input (NHWC [B, H, W, 32]) from g = d output (NHWC [B, OH, OW, 64], contiguous)."""
        B, H, W = in_shape[0], in_shape[1], in_shape[2]
        dx = torch.empty((B, H, W, 32), dtype=torch.float32, device=g.device)
        _lib.call(ops.lib().xpa_conv_dgrad_s2k, ops._p(g), B, g.shape[1], g.shape[2], 64, ops._p(conv.weight), 32,
                  conv.kernel_size[0], conv.stride[0], conv.padding[0], H, W, ops._p(dx), ops._stream(g.device))
        return dx

    @torch.no_grad()
    def backward(self, ctx, ds):
        """ds: d loss / d state [B, d]; writes every trunk parameter's gradient."""
        hs, am, flat, fouts, plan = ctx
        g = ds
        for j in range(len(self.fc) - 1, -1, -1):
            lin, code, slope = self.fc[j]
            g = g.contiguous()
            _act_bwd_bias(self.parts, code, g, fouts[j], slope, lin.bias.grad)
            if j > 0:
                torch.mm(g.t(), fouts[j - 1], out=lin.weight.grad)
                g = torch.mm(g, lin.weight)
            else:
                g = self._fc0_backward(plan, g, flat)
        # conv blocks, last to first.  g is the NHWC gradient of the block's output (after its activation), or — where
        # act_bwd names a stage upstream of the block (K40G-act, K24, K28-dgrad) — its pre-activation gradient dz, with
        # the block's bias gradient already written.
        for i in range(len(self.convs) - 1, -1, -1):
            conv, code, slope = self.convs[i]
            act_bwd, wgrad, dgrad = plan.convs[i][1:]
            y = hs[i + 1]
            Cy = y.shape[3]
            if act_bwd == "K24":
                g = self._maxpool_backward(ds, am, y, i)
            else:
                g = g.reshape(y.shape)
                if not g.is_contiguous():
                    g = g.contiguous()
            x_in = self.frames(hs[0]) if i == 0 and plan.frames == "backward" else hs[i]
            if act_bwd == "K22":   # the data gradient and the library weight gradient read dz: in place, + the bias
                _act_bwd_bias(self.parts, code, g.view(-1, Cy), y.view(-1, Cy), slope, conv.bias.grad)
            elif act_bwd not in ("K24", "K40G-act", "K28-dgrad") and act_bwd != wgrad:   # upstream, or K26 / K29's own
                _no_form("conv block %d's activation backward" % i, act_bwd)
            # the weight gradient, with the activation backward + bias gradient folded in where act_bwd names it
            if wgrad == "K26":
                self._conv1_wgrad(conv, g, x_in, act=(code, slope, y) if act_bwd == "K26" else None)
            elif wgrad == "K29":
                self._conv_wgrad(conv, g, code if act_bwd == "K29" else -1, slope, y, x_in)
            elif wgrad != "miopen":
                _no_form("conv block %d's weight gradient" % i, wgrad)
            if "miopen" in (wgrad, dgrad):
                gx, gw, _ = torch.ops.aten.convolution_backward(
                    g.permute(0, 3, 1, 2), x_in.permute(0, 3, 1, 2), conv.weight, None, list(conv.stride),
                    list(conv.padding), [1, 1], False, [0, 0], 1, [dgrad == "miopen", wgrad == "miopen", False])
                if wgrad == "miopen":
                    conv.weight.grad.copy_(gw)
            if dgrad == "miopen":
                g = gx.permute(0, 2, 3, 1)
            elif dgrad == "K27":   # (the stride-2 32 -> 64 conv): the previous block's g, not dz
                g = self._dgrad(conv, g, x_in.shape)
            elif dgrad == "K28":   # with the previous block's activation backward + bias gradient
                pconv, pcode, pslope = self.convs[i - 1]
                g = self._conv_dgrad(conv, g, tuple(x_in.shape), (pcode, pslope, hs[i], pconv.bias.grad))
            elif dgrad != "none" or i > 0:
                _no_form("conv block %d's data gradient" % i, dgrad)
        self.stale = True   # the optimizer step that follows changes the fc weight

    def _fc0_backward(self, plan, g, flat):
        """The first fc layer's weight gradient (permuted back into the reference's (C, H, W) column order) and its
        data gradient, which plan.fc0_dx "K40G-act" returns as the last conv block's dz."""
        lin = self.fc[0][0]
        if self._dw_tmp is None:
            self._dw_tmp = torch.empty_like(lin.weight)
        if plan.fc0_dw in ("K41V", "K41V-padded"):
            self._fc0_wgrad_split(g, flat)
        elif plan.fc0_dw == "mm":
            torch.mm(g.t(), flat, out=self._dw_tmp)
        else:
            _no_form("the first fc layer's weight gradient", plan.fc0_dw)
        Cl, Hl, Wl = self._chw
        lin.weight.grad.view(lin.out_features, Cl, Hl, Wl).copy_(
            self._dw_tmp.view(lin.out_features, Hl, Wl, Cl).permute(0, 3, 1, 2))
        if plan.fc0_dx == "K40G-act":
            if not flat.is_contiguous():
                _no_form("the first fc layer's data gradient on a strided input", "K40G-act")
            return self._fc0_dgrad_split_act(g, flat)
        if plan.fc0_dx == "K40G":
            return self._fc0_dgrad_split(g)
        if plan.fc0_dx != "mm":
            _no_form("the first fc layer's data gradient", plan.fc0_dx)
        return torch.mm(g, self._fc0_weight())

    def _maxpool_backward(self, ds, am, y, i):
        """K24: the last block's dz (the pooled gradient routed to the argmax, times act'(y)) and its bias gradient."""
        conv, code, slope = self.convs[i]
        B, HW, Cy = y.shape[0], y.shape[1] * y.shape[2], y.shape[3]
        dz = torch.empty_like(y)
        part = self.parts.get(B * HW, Cy, y.device, True)
        L, st = ops.lib(), ops._stream(y.device)
        if self.err is None:
            self.err = torch.zeros((1,), dtype=torch.int32, device=y.device)   # argmax outside [0, HW)
        _lib.call(L.xpa_maxpool_act_bwd_bias, code, ops._p(ds.contiguous()), ops._p(am), ops._p(y), B, HW, Cy,
                  float(slope), ops._p(dz), ops._p(part), ops._p(self.err), st)
        _lib.call(L.xpa_colsum_finalize, ops._p(part), part.shape[0], Cy, ops._p(conv.bias.grad), st)
        return dz


class FusedCNNActorCritic:
    """Built from a Categorical/Gaussian actor-critic policy with an AC_CNN_Atari representation."""

    def __init__(self, policy):
        self.parts = _Part()
        self.trunk_ = _Trunk(policy.representation, self.parts)
        if self.trunk_.tail != "flatten":
            raise ValueError("the actor-critic path expects AC_CNN_Atari")
        self.discrete = policy_discrete(policy)
        self.actor = _parse(policy.actor.model if self.discrete else policy.actor.mu)
        self.critic = _parse(policy.critic.model)
        self.logstd = None if self.discrete else policy.actor.logstd
        n_params = sum(1 for _ in policy.parameters())
        n_cov = self.trunk_.n_params + 2 * (len(self.actor) + len(self.critic)) + (0 if self.discrete else 1)
        if n_params != n_cov:
            raise ValueError("policy has parameters outside the conv / Linear chains")

    @property
    def stale(self):
        return self.trunk_.stale

    @stale.setter
    def stale(self, v):
        self.trunk_.stale = v

    def refresh(self):
        """Re-derive the (H, W, C)-ordered first fc weight now (the agent calls it before a captured rollout, whose
        graph must not contain the copy)."""
        self.trunk_.refresh()

    def frames(self, x):
        return self.trunk_.frames(x)

    @torch.no_grad()
    def trunk(self, x):
        return self.trunk_.forward(x)

    @torch.no_grad()
    def forward(self, x):
        """(logits or mu, logstd or None, v, ctx)."""
        s, tctx = self.trunk_.forward(x)
        a_outs = _chain(self.actor, s)
        c_outs = _chain(self.critic, s)
        return a_outs[-1], self.logstd, c_outs[-1][:, 0], (tctx, s, a_outs, c_outs)

    @torch.no_grad()
    def heads(self, x):
        head, logstd, v, _ = self.forward(x)
        return head, logstd, v

    @torch.no_grad()
    def backward(self, ctx, d_head, d_v):
        """Writes every parameter gradient (d_head [B, K], d_v [B]: the loss kernel's outputs)."""
        tctx, s, a_outs, c_outs = ctx
        ds = _chain_backward(self.parts, self.actor, [s] + a_outs[:-1], a_outs, d_head)
        ds = _chain_backward(self.parts, self.critic, [s] + c_outs[:-1], c_outs, d_v.view(-1, 1), acc=ds)
        self.trunk_.backward(tctx, ds)


class FusedQNetwork:
    """BasicQnetwork over a Basic_CNN (or AC_CNN_Atari) representation: explicit eval forward / backward and the
    target forward (deterministic.py:148-182)."""

    def __init__(self, policy):
        self.parts = _Part()
        self.eval_trunk = _Trunk(policy.representation, self.parts)
        self.target_trunk = _Trunk(policy.target_representation, self.parts)
        self.eval_head = _parse(policy.eval_Qhead.model)
        self.target_head = _parse(policy.target_Qhead.model)
        n_params = sum(1 for _ in policy.parameters())
        n_cov = 2 * self.eval_trunk.n_params + 4 * len(self.eval_head)
        if n_params != n_cov:
            raise ValueError("Q-network has parameters outside the conv / Linear chains")
        self.eval_params = self.eval_trunk.params() + [t for lin, _, _ in self.eval_head for t in (lin.weight, lin.bias)]

    @torch.no_grad()
    def forward(self, x):
        """evalQ [B, A] and the backward context."""
        s, tctx = self.eval_trunk.forward(x)
        outs = _chain(self.eval_head, s)
        return outs[-1], (tctx, s, outs)

    @torch.no_grad()
    def target(self, x):
        if self.target_trunk.tail == "flatten":
            self.target_trunk.stale = True   # copy_target() may have changed it since the last call
        s, _ = self.target_trunk.forward(x)
        return _chain(self.target_head, s)[-1]

    @torch.no_grad()
    def backward(self, ctx, dq):
        """dq = d loss / d evalQ [B, A] (K19); writes every eval parameter's gradient."""
        _ensure_grads(self.eval_params)
        tctx, s, outs = ctx
        ds = _chain_backward(self.parts, self.eval_head, [s] + outs[:-1], outs, dq.contiguous())
        self.eval_trunk.backward(tctx, ds)

    def refresh(self):
        self.eval_trunk.refresh()
        self.target_trunk.refresh()
