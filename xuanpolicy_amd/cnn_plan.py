"""The kernel form of every stage of one convolutional trunk's forward and backward (fused_cnn._Trunk): chosen once by
plan_cnn from a facts record (host logic alone: no tensor, no device, no library call), run by the trunk's stages, which
dispatch on the plan's fields and test no capability of their own ("Where the CNN trunk's forms are
decided")."""
from typing import NamedTuple


def out_hw(H, W, k, s, p):
    """A conv's output height and width."""
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def k22_width(cols):
    """The widths K21 / K22 take: 4 columns per thread, a whole number of rows per 256-thread block."""
    return cols % 4 == 0 and 256 % (cols // 4) == 0


class ConvFacts(NamedTuple):
    """One conv block, gathered once by _Trunk.__init__ (conv_facts)."""
    cin: int
    cout: int
    k: int
    s: int
    p: int
    square: bool        # kernel, stride and padding the same in both directions
    zeros: bool         # padding_mode "zeros"
    w_contig: bool      # the weight is contiguous
    act: int            # the activation code
    igemm: bool         # K28 forward and K29 both take the shape (xpa_conv_igemm_ok and xpa_conv_wgrad_ok included)
    igemm_dgrad: bool   # K28's data gradient takes it
    k27: bool           # K27 takes the data gradient: 2s x 2s, stride s (1, 2), 32 -> 64 channels


def conv_facts(cin, cout, kernel, stride, padding, zeros, w_contig, act, igemm_ok=None, wgrad_ok=None):
    """The ConvFacts of one Conv2d: the static shape rules of K27 / K28 / K29.  igemm_ok(in, out, k) and
    wgrad_ok(in, out, k) are the library's xpa_conv_igemm_ok (K28's weight image) and xpa_conv_wgrad_ok (K29's tiling),
    asked by the caller's hand (the planner never asks; None: not asked, no K28 / K29).  A block is on the K28 / K29
    path only when both take it: one that K29 cannot take plans the library route in all three directions."""
    k, s, p = kernel[0], stride[0], padding[0]
    square = kernel[0] == kernel[1] and stride[0] == stride[1] and padding[0] == padding[1]
    plain = square and zeros and w_contig
    igemm = bool(plain and cin % 4 == 0 and igemm_ok is not None and wgrad_ok is not None
                 and igemm_ok(cin, cout, k) and wgrad_ok(cin, cout, k))
    dgrad = bool(igemm and s <= 2 and cout % 4 == 0 and igemm_ok(cout, cin, k))
    k27 = plain and cin == 32 and cout == 64 and s in (1, 2) and k == 2 * s and p < k
    return ConvFacts(cin, cout, k, s, p, square, zeros, w_contig, act, igemm, dgrad, k27)


class CnnFacts(NamedTuple):
    """What plan_cnn decides from.  _Trunk.facts gathers it."""
    convs: tuple              # of ConvFacts
    in_hwc: tuple             # the input's (H, W, C)
    tail: str                 # "flatten" | "maxpool"
    fc0: object               # the first fc layer's (in_features, out_features), or None
    fcs: tuple                # per fc layer (out_features, activation code): what launches() lists for them
    u8_conv1: bool            # K25's shape: 4 channels, 8 x 8 kernel, 32 outputs
    # the pass
    B: int
    x_u8: bool                # the input is a contiguous uint8 device tensor (what K25 / K26 read)
    grads0_contig: bool       # conv 0's weight and bias gradients are contiguous (K26 writes them)
    # the switches
    use_igemm: bool
    igemm_min_rows: int
    fc_split: bool
    fc_split_min_rows: int
    fc_fuse_act: bool
    fc_wsplit: bool
    s3_gemms: bool            # ops.S3_GEMMS


class ConvForm(NamedTuple):
    fwd: str       # "K25" | "K28" | "miopen" (+ K21)
    act_bwd: str   # who forms this block's dz and bias gradient: "K22" | "K24" (the max pool's) | "K26" | "K29" |
                   # "K40G-act" (the fc data gradient's epilogue) | "K28-dgrad" (the next block's data gradient's)
    wgrad: str     # "K26" | "K29" | "miopen"
    dgrad: str     # "none" (the first block) | "K27" | "K28" | "miopen"


_FWD = {"K25": ("xpa_conv1_u8_fwd",), "K28": ("xpa_conv_fwd",), "miopen": ("xpa_bias_act",)}
_ACT_BWD = {"K22": ("xpa_act_bwd_bias", "xpa_colsum_finalize"), "K10": ("xpa_act_bwd_colsum", "xpa_colsum_finalize"),
            "K24": ("xpa_maxpool_act_bwd_bias", "xpa_colsum_finalize")}
# (the weight gradient's finalize, + the bias gradient's where the kernel also forms the activation backward)
_WGRAD = {"K26": ("xpa_conv1_u8_wgrad_act", "xpa_colsum_finalize"), "K29": ("xpa_conv_wgrad", "xpa_colsum_finalize"),
          "miopen": ()}
_DGRAD = {"none": (), "K27": ("xpa_conv_dgrad_s2k",), "K28": ("xpa_conv_dgrad", "xpa_colsum_finalize"), "miopen": ()}
_FC0_FWD = {"K40G": ("xpa_s3_gemm_group",), "linear": ()}
_FC0_DW = {"K41V": "xpa_s3_wgrad", "K41V-padded": "xpa_s3_wgrad_padded"}
_FC0_DX = {"K40G-act": ("xpa_s3_gemm_group_act", "xpa_colsum_finalize"), "K40G": ("xpa_s3_gemm_group",), "mm": ()}


class CnnPlan(NamedTuple):
    """One trunk forward + backward's forms."""
    convs: tuple       # of ConvForm
    frames: str        # where K20 makes the f32 frames: "forward" (conv 0 is not K25) | "backward" (K25, but conv 0's
                       # weight gradient is not K26) | "none"
    slack: int         # floats allocated after the last block's output (the padded K41V reads them)
    fc0_fwd: object    # "K40G" | "linear" | None (no fc layers: the max-pool tail)
    fc0_dw: str        # "K41V" | "K41V-padded" | "mm"
    fc0_dx: str        # "K40G-act" | "K40G" | "mm"
    fc0_halves: int    # 256-column halves of the first fc layer's output gradient: one K41V launch each
    fcs: tuple         # per fc layer (its forward's activation pass: "K21" | None, its backward's: "K22" | "K10")

    def launches(self, direction):
        """The library entry points of one trunk "forward" or "backward", in order.  MIOpen's, hipBLASLt's and torch's
        launches are not counted, nor is the re-split of the first fc weight's planes after an optimizer step
        (xpa_s3_split_batch: state, not plan)."""
        out = []
        if direction == "forward":
            if self.frames == "forward":
                out.append("xpa_frames_to_f32")
            for c in self.convs:
                out += _FWD[c.fwd]
            if self.fc0_fwd is None:
                return out + ["xpa_global_maxpool"]
            out += _FC0_FWD[self.fc0_fwd]
            for fwd, _ in self.fcs:
                out += ["xpa_bias_act"] if fwd else []
            return out
        if direction != "backward":
            raise ValueError("direction: forward | backward")
        for j in range(len(self.fcs) - 1, -1, -1):
            out += _ACT_BWD[self.fcs[j][1]]
            if j == 0:
                if self.fc0_dw != "mm":   # the batched finalize takes 16 segments per launch
                    out += [_FC0_DW[self.fc0_dw]] * self.fc0_halves
                    out += ["xpa_colsum_finalize_batch_map"] * ((self.fc0_halves + 15) // 16)
                out += _FC0_DX[self.fc0_dx]
        for i in range(len(self.convs) - 1, -1, -1):
            c = self.convs[i]
            frames = ["xpa_frames_to_f32"] if i == 0 and self.frames == "backward" else []
            if c.act_bwd == "K24":
                out += _ACT_BWD["K24"]
            out += frames
            if c.act_bwd == "K22":
                out += _ACT_BWD["K22"]
            out += _WGRAD[c.wgrad]
            if c.act_bwd == c.wgrad:   # K26 / K29 with the activation backward folded in: the bias gradient's finalize
                out.append("xpa_colsum_finalize")
            out += _DGRAD[c.dgrad]
        return out


def plan_cnn(f):
    """The CnnPlan of facts f: the only place a CNN-side switch is read or a capability tested.  Raises the
    small-channel refusal (RuntimeError) for any block and direction that would go to MIOpen with fewer than 16 input
    or output channels."""
    n = len(f.convs)
    H, W, C = f.in_hwc
    shapes = [(H, W, C)]
    for c in f.convs:
        shapes.append(out_hw(shapes[-1][0], shapes[-1][1], c.k, c.s, c.p) + (c.cout,))
    numel = [f.B * h * w * ch for h, w, ch in shapes]

    def igemm(i, operand):
        """K28 / K29 for block i: operand is the largest tensor they load or store (32-bit buffer offsets: under
        2 GiB); the row preference is waived for small-channel blocks, which MIOpen must not take."""
        c = f.convs[i]
        rows = f.B * shapes[i + 1][0] * shapes[i + 1][1]
        return (f.use_igemm and operand * 4 < 2 ** 31 and (min(c.cin, c.cout) < 16 or rows >= f.igemm_min_rows)
                and c.igemm)

    # forward: the operand is the larger of the block's input and its output (K28 stores through a buffer record too)
    fwd = ["K25" if i == 0 and f.u8_conv1 and f.x_u8 else "K28" if igemm(i, max(numel[i], numel[i + 1])) else "miopen"
           for i in range(n)]
    # the first fc layer
    fc0_fwd, fc0_dw, fc0_dx, slack, halves, fcs = None, "mm", "mm", 0, 0, ()
    if f.tail == "flatten":
        in_f, out_f = f.fc0
        rows_ok = f.s3_gemms and f.B >= f.fc_split_min_rows
        split = (f.fc_split and rows_ok and out_f % 256 == 0 and in_f % 32 == 0 and in_f >= 512
                 and out_f // 256 * 2 <= 32 and (in_f + 255) // 256 <= 32)
        fuse = (f.fc_fuse_act and split and in_f % 256 == 0 and f.convs[-1].cout in (32, 64)
                and f.convs[-1].act in (0, 1, 2))
        fc0_fwd = "K40G" if split else "linear"
        fc0_dx = "K40G-act" if fuse else "K40G" if split else "mm"
        # K41V reads the flat input as 128-row tiles: a ragged width needs slack after the last row, which only K28's
        # output can carry
        pad = -in_f % 128
        if f.fc_wsplit and rows_ok and out_f % 256 == 0 and in_f % 4 == 0:
            slack = pad if fwd[-1] == "K28" else 0
            fc0_dw = "K41V" if not pad else "K41V-padded" if slack else "mm"
            halves = out_f // 256 if fc0_dw != "mm" else 0
        fcs = tuple(("K21" if code or (j == 0 and split) else None, "K22" if k22_width(width) else "K10")
                    for j, (width, code) in enumerate(f.fcs))
    # backward, last block to first: the operand is the larger of the block's input and its output gradient.  `up` is
    # the stage upstream of the block that has already applied its activation backward, if one has
    forms = [None] * n
    up = "K40G-act" if fc0_dx == "K40G-act" else "K24" if f.tail == "maxpool" else None
    for i in range(n - 1, -1, -1):
        c = f.convs[i]
        if i == 0 and fwd[0] == "K25" and f.grads0_contig:   # K26 from the uint8 frames
            forms[0] = ConvForm(fwd[0], up or "K26", "K26", "none")
            continue
        ig = igemm(i, max(numel[i], numel[i + 1]))
        dgrad = "none" if i == 0 else "K27" if c.k27 else "K28" if ig and c.igemm_dgrad else "miopen"
        # the data gradient and the library's weight gradient read dz (K22); K29 alone folds the activation in
        forms[i] = ConvForm(fwd[i], up or ("K22" if i > 0 or not ig else "K29"), "K29" if ig else "miopen", dgrad)
        up = "K28-dgrad" if dgrad == "K28" else None
    # MIOpen is refused for convs with fewer than 16 input or output channels.  The r02 intermittent
    # hipErrorIllegalAddress of the PER-DQN agent loop (2 of 9 runs, 8-channel test net) surfaced at the
    # first host sync after one agent step whose only library convolutions were MIOpen's NHWC kernels for 4 / 8-channel
    # shapes; every hand-written kernel of that step carries a device error word since r03 and reported 0 in every
    # later run.  K28 / K29 take every such conv, so planning MIOpen here means use_igemm was turned off (or an operand
    # of 2 GiB): an error before the pass's first launch instead of the unproven route.
    for c, form in zip(f.convs, forms):
        if min(c.cin, c.cout) < 16 and "miopen" in (form.fwd, form.wgrad, form.dgrad):
            raise RuntimeError("conv %d -> %d channels: the small-channel MIOpen route is refused (r02 fault suspect); "
                               "keep use_igemm on (K28 / K29 take convs with in_channels %% 4 == 0, <= 64 channels)"
                               % (c.cin, c.cout))
    frames = "forward" if fwd[0] != "K25" else "backward" if forms[0].wgrad != "K26" else "none"
    return CnnPlan(tuple(forms), frames, slack, fc0_fwd, fc0_dw, fc0_dx, halves, fcs)
