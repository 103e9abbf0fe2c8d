"""CPU tests of the drop-in boundary: the C-ABI library builds, loads and exports every symbol that
include/xuanpolicy_amd.h declares; the Python bindings cover them; no compute call without a GPU."""
import os
import re
import subprocess

import pytest
import torch

from xuanpolicy_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_functions():
    src = open(os.path.join(REPO, "include", "xuanpolicy_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(xpa_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def test_header_symbols_exported(lib):
    names = _header_functions()
    assert len(names) >= 15
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (xpa_\w+)", out))
    assert set(names) == exported, (set(names) ^ exported)
    for n in names:
        assert hasattr(lib, n)


def test_bindings_cover_header():
    assert set(_header_functions()) == set(_lib.SIGNATURES)


def test_abi_version_and_size_helpers(lib):
    assert lib.xpa_abi_version() == _lib.ABI_VERSION
    assert lib.xpa_loss_num_partials(65536) == 256 and lib.xpa_loss_num_partials(1 << 22) == 2048
    assert lib.xpa_loss_partial_width(6) == 11
    assert lib.xpa_gather_num_partials(65537) == 1025
    assert lib.xpa_rms_num_partials(4096) == 16


def test_invalid_arguments_rejected_before_launch(lib):
    # null pointers / bad shapes return hipErrorInvalidValue (1) without touching a device
    assert lib.xpa_gae_scan(None, None, None, None, None, 4, 4, 0.99, 0.95, 1, None, None, None) == 1
    assert lib.xpa_gae_scan(None, None, None, None, None, -1, 4, 0.99, 0.95, 1, None, None, None) == 1
    assert lib.xpa_policy_loss_fwd_bwd(0, 0, 0, 6, *([None] * 4), 1, *([None] * 5), 0, 0.2, 0.25, 0.0,
                                       None, None, None, None) == 1
    assert lib.xpa_policy_loss_fwd_bwd(0, 1, 8, 1, *([None] * 4), 8, *([None] * 5), 0, 0.2, 0.25, 0.0,
                                       None, None, None, None) == 1
    assert lib.xpa_gather_minibatch(None, 8, 8, None, 4, None, None, None, None, None) == 1
    assert lib.xpa_rms_merge(None, 3, 100, 4, None, None, None, None) == 1
    # K16X: the trunk width (d_in <= 20), the head width (<= 8) and h_out's alignment are checked before any launch
    # (fake, 16-B aligned non-null pointers elsewhere, so only the checked argument can fail)
    import ctypes
    P = ctypes.c_void_p(256)

    def trunk_actor(act_dim=6, d_in=17, h_out=P):
        return lib.xpa_head_gemm_trunk_actor(0, 0, 1, 64, act_dim, 256, P, d_in, d_in, P, P, 0.01, h_out, 256, P, P,
                                             512, P, P, 0.01, P, P, 100, P, P, P, P, 1, 0.2, 0.0, P, P, P, P, P, 16, None)
    assert trunk_actor(d_in=21) == 1
    assert trunk_actor(act_dim=9) == 1
    assert trunk_actor(h_out=ctypes.c_void_p(260)) == 1
    assert lib.xpa_head_gemm_trunk_critic(1, 64, 256, P, 21, 21, P, P, 0.01, None, 256, P, P, 512, P, P, 0.01, P, 100,
                                          P, 0.25, P, P, P, P, P, 16, None) == 1
    # K28 / K29: every operand AND every output under 2 GiB (32-bit buffer byte offsets), checked in bytes before any
    # launch; the sizes sit just either side of the bound, and the same call just under it fails only on what is
    # checked later (K29's tiling), never on the size
    def conv_fwd(batch, hw, in_c=4, out_c=64, x=P):
        return lib.xpa_conv_fwd(1, x, batch, hw, hw, in_c, P, P, out_c, 1, 1, 0, 0.0, P, None)
    assert 8 * 1024 * 1024 * 64 * 4 == 1 << 31 and 8 * 1024 * 1024 * 4 * 4 < 1 << 31
    assert conv_fwd(8, 1024) == 1                          # x 128 MiB, y exactly 2 GiB
    assert conv_fwd(8, 1024, in_c=64, out_c=4) == 1        # the input bound, as before
    assert conv_fwd(1, 4, x=ctypes.c_void_p(260)) == 1     # x's alignment

    def conv_dgrad(batch, hw, in_c, out_c):
        return lib.xpa_conv_dgrad(P, batch, hw, hw, out_c, P, in_c, 1, 1, 0, hw, hw, -1, None, 0.0, P, None, None)
    assert conv_dgrad(8, 1024, 64, 4) == 1                 # dx exactly 2 GiB (2^29 elements), dy 128 MiB
    assert conv_dgrad(8, 1024, 4, 64) == 1                 # dy exactly 2 GiB

    def conv_wgrad(in_c, out_c, k, batch=1, hw=16):
        return lib.xpa_conv_wgrad(-1, P, None, 0.0, P, batch, hw, hw, in_c, out_c, k, 1, 0, P, None, None)
    assert conv_wgrad(32, 32, 5) == 1 and not lib.xpa_conv_wgrad_ok(32, 32, 5)     # 800 columns: 50 tiles
    assert conv_wgrad(16, 16, 8) == 1 and not lib.xpa_conv_wgrad_ok(16, 16, 8)
    assert conv_wgrad(64, 65, 3) == 1 and not lib.xpa_conv_wgrad_ok(64, 65, 3)
    assert lib.xpa_conv_wgrad_ok(64, 64, 3) and lib.xpa_conv_wgrad_ok(36, 64, 4) and not lib.xpa_conv_wgrad_ok(40, 64, 4)
    assert conv_wgrad(64, 4, 1, batch=8, hw=1024) == 1     # x exactly 2 GiB
    assert conv_wgrad(4, 64, 1, batch=8, hw=1024) == 1     # g exactly 2 GiB
    # the gather-only K13 form needs the rows output when h is NULL
    assert lib.xpa_thin_linear_act_fwd_gather(1, P, 17, 100, P, 64, 17, 256, P, P, 0.01, None, 256, P, P, None,
                                              None) == 1


def test_bindings_literal_pins():
    """The header-derived bindings of entry points that between them use every type spelling and declaration shape
    the parser handles, written out (as the hand-kept table had them)."""
    from ctypes import c_double, c_float as f32, c_int, c_int32 as i32, c_int64 as i64, c_uint32 as u32, c_void_p as p
    pins = {
        "xpa_abi_version": (c_int, []),                                                     # (void)
        "xpa_gae_scan": (c_int, [p, p, p, p, p, i64, i64, f32, f32, c_int, p, p, p]),       # multi-line, const T *, stream
        "xpa_gather_num_partials": (i64, [i64]),                                            # int64_t return
        "xpa_adam_sched_entry": (None, [f32, f32, f32, i64, p]),                            # void return
        "xpa_conv_wgrad_force_stream": (None, [c_int]),
        "xpa_per_store": (c_int, [p, p, p, i64, i64, i64, c_double, p]),                    # double
        "xpa_synthbox_step": (c_int, [i64, i64, p, u32, i32, f32, f32, f32, p, i64] + [p] * 10),   # uint32_t, int32_t
        "xpa_small_mlp_update": (c_int, [p, p]),                                            # struct pointer
        "xpa_rollout_step_workspace": (i64, [i64, i64, c_int, p]),                          # int64_t * out-parameter
        "xpa_colsum_finalize_batch": (c_int, [c_int, p, p, p, p, p]),                       # T *const *
    }
    for name, want in pins.items():
        assert _lib.SIGNATURES[name] == want, name
    assert len(_lib.SIGNATURES) == len(_header_functions())


def _bundled_clang():
    """The clang beside the hipcc build_library uses (host compiles only here)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = subprocess.run([hipcc, "--version"], capture_output=True, text=True, check=True).stdout
    return os.path.join(re.search(r"InstalledDir:\s*(\S+)", out).group(1), "clang")


def test_struct_layout_matches_compiler(lib, tmp_path):
    """sizeof and every offsetof of the two argument structs, as the C compiler lays the header out, against the
    ctypes classes derived from the same header."""
    import ctypes
    classes = (_lib.XpaSmallMlpArgs, _lib.XpaSmallRolloutArgs)
    assert [len(c._fields_) for c in classes] == [59, 69]
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "xuanpolicy_amd.h"', "int main(void) {"]
    for c in classes:
        lines.append('    printf("%%zu\\n", sizeof(%s));' % c.__name__)
        lines += ['    printf("%%zu\\n", offsetof(%s, %s));' % (c.__name__, n) for n, _ in c._fields_]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    exe = str(tmp_path / "layout")
    subprocess.run([_bundled_clang(), "-I", os.path.dirname(_lib.HEADER), "-o", exe, str(src)], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for c in classes:
        want += [ctypes.sizeof(c)] + [getattr(c, n).offset for n, _ in c._fields_]
    assert got == want
    assert (got[0], got[60]) == (400, 472)


def test_parser_refuses_what_it_does_not_know():
    with pytest.raises(_lib.XpaError, match="xpa_x"):
        _lib.parse_header("int xpa_x(long double y);")
    with pytest.raises(_lib.XpaError, match="xpa_y"):
        _lib.parse_header("int xpa_y(int (*callback)(int));")
    with pytest.raises(_lib.XpaError, match="xpa_z"):
        _lib.parse_header("size_t xpa_z(void);")
    with pytest.raises(_lib.XpaError, match="XpaThing"):
        _lib.parse_header("typedef struct XpaThing { int a, b; size_t n; } XpaThing;")
    sig, structs, consts = _lib.parse_header("#define XPA_N 7\ntypedef struct XpaOk { int a, b; const float *p, *q; } XpaOk;\n"
                                             "void xpa_ok(const XpaOk *a, /* c */ unsigned n); // d\n")
    import ctypes
    assert sig == {"xpa_ok": (None, [ctypes.c_void_p, ctypes.c_uint])} and consts == {"XPA_N": 7}
    assert structs["XpaOk"]._fields_ == [("a", ctypes.c_int), ("b", ctypes.c_int), ("p", ctypes.c_void_p),
                                         ("q", ctypes.c_void_p)]


def test_call_names_the_entry_point_that_failed(lib):
    with pytest.raises(_lib.XpaError, match=r"xpa_gae_scan failed.*invalid argument"):
        _lib.call(lib.xpa_gae_scan, None, None, None, None, None, -1, 4, 0.99, 0.95, 1, None, None, None)


def test_constants_come_from_the_header(lib):
    assert _lib.ABI_VERSION == lib.xpa_abi_version() == 4
    assert _lib.COLSUM_TICKET_INTS == 4096


def test_ops_refuse_cpu_tensors():
    from xuanpolicy_amd import ops
    x = torch.zeros(4, 8)
    with pytest.raises(ValueError, match="ROCm device"):
        ops.gae_scan(x, x, x, torch.zeros(4, 8, dtype=torch.uint8), x, 0.99, 0.95)
    with pytest.raises(ValueError, match="ROCm device"):
        ops.policy_loss("ppo", "gaussian", torch.zeros(4, 2), torch.zeros(2), torch.zeros(4), torch.zeros(8),
                        torch.zeros(4), torch.zeros(4), old_logp=torch.zeros(4))


def test_config_cascade():
    from xuanpolicy_amd.runner import get_arguments
    a = get_arguments("ppo", "synthbox", "SynthBox-v0")
    assert (a.agent, a.parallels, a.n_steps, a.n_epoch, a.n_minibatch) == ("PPO_Clip", 4096, 128, 16, 8)
    assert a.representation_hidden_size == [256] and a.clip_grad_norm == 0.5 and a.use_obsnorm
    b = get_arguments("a2c", "synthbox", "SynthBox-v0")
    assert b.agent == "A2C" and b.discrete and b.clip_grad == 0.5


def test_registries_match_reference_names():
    from xuanpolicy_amd import agents, learners, policies
    assert set(agents.REGISTRY) == {"PPO_Clip", "A2C", "PerDQN"}
    assert set(learners.REGISTRY) == {"PPO_Clip", "A2C", "PerDQN"}
    assert {"Gaussian_AC", "Categorical_AC", "Basic_Q_network"} <= set(policies.REGISTRY)
    assert {"Basic_MLP", "AC_CNN_Atari", "Basic_CNN"} <= set(policies.REGISTRY_Representation)


def test_qnetwork_state_dict_keys_match_reference(golden):
    """BasicQnetwork over Basic_CNN loads the reference's state_dict (deterministic.py:148-182, cnn.py:5-40)."""
    import torch
    from xuanpolicy_amd.policies import BasicQnetwork, Basic_CNN
    g = golden("perdqn.npz")
    B, A = (int(x) for x in g["config"][:2])
    net = [int(x) for x in g["net"]]
    nl = (len(net) - 1) // 3

    class Disc:
        n, shape = A, ()
    rep = Basic_CNN((84, 84, 4), net[nl:2 * nl], net[2 * nl:3 * nl], net[:nl], None, None, torch.nn.ReLU, "cpu")
    pol = BasicQnetwork(Disc(), rep, net[3 * nl:], None, None, torch.nn.ReLU, "cpu")
    sd = {k[4:]: torch.as_tensor(v) for k, v in g.items() if k.startswith("sd0/")}
    assert set(pol.state_dict()) == set(sd)
    pol.load_state_dict(sd)


def test_policy_state_dict_keys_match_reference(golden):
    """Our Gaussian/Categorical AC modules load the reference's state_dict (checkpoint interchange)."""
    from xuanpolicy_amd.policies import Basic_MLP, Categorical_AC_Policy, Gaussian_AC_Policy

    class Box:
        shape = (6,)

    class Disc:
        n, shape = 6, ()
    g = golden("loss.npz")
    for tag, cls, space in (("ppo_gaussian_6", Gaussian_AC_Policy, Box()),
                            ("ppo_categorical_6", Categorical_AC_Policy, Disc())):
        D = g[tag + "/obs"].shape[1]
        rep = Basic_MLP((D,), [64], None, torch.nn.init.orthogonal_, torch.nn.LeakyReLU, "cpu")
        pol = cls(space, rep, [64], [64], None, torch.nn.init.orthogonal_, torch.nn.LeakyReLU, "cpu")
        sd = {k[len(tag) + 5:]: torch.as_tensor(v) for k, v in g.items() if k.startswith(tag + "/sd0/")}
        pol.load_state_dict(sd)
        out, dist, v = pol(g[tag + "/obs"])
        head = dist.mu if hasattr(dist, "mu") else dist.logits
        assert torch.allclose(head, torch.as_tensor(g[tag + "/head"]), atol=1e-5)
        assert torch.allclose(v, torch.as_tensor(g[tag + "/v"]), atol=1e-5)


def test_flat_state_placement_groups():
    """FlatState keeps parameter order/offsets per parameter but lays placement groups back to back
    (the paired actor|critic hidden layer of fused_mlp.head_placement)."""
    from xuanpolicy_amd.flat import ALIGN, FlatState
    from xuanpolicy_amd.fused_mlp import head_placement
    from xuanpolicy_amd.policies import Basic_MLP, Gaussian_AC_Policy

    class Box:
        shape = (6,)
    torch.manual_seed(0)
    rep = Basic_MLP((17,), [256], None, torch.nn.init.orthogonal_, torch.nn.LeakyReLU, "cpu")
    pol = Gaussian_AC_Policy(Box(), rep, [256], [256], None, torch.nn.init.orthogonal_, torch.nn.LeakyReLU, "cpu")
    before = {k: v.clone() for k, v in pol.state_dict().items()}
    groups = head_placement(pol)
    assert len(groups) == 2
    fs = FlatState(pol.parameters(), placement=groups)
    assert [id(p) for p in fs.params] == [id(p) for p in pol.parameters()]
    assert all(o % ALIGN == 0 for o in fs.offsets)
    for g in groups:
        pv, gv = fs.span(g)
        assert pv.numel() == sum(p.numel() for p in g)
        assert pv.data_ptr() == g[0].data_ptr() and gv.data_ptr() == g[0].grad.data_ptr()
    assert fs.span([groups[0][1], groups[0][0]]) is None   # wrong order is not back to back
    for k, v in pol.state_dict().items():
        assert torch.equal(v, before[k]), k
    # offsets are unique and do not overlap
    spans = sorted((o, o + p.numel()) for p, o in zip(fs.params, fs.offsets))
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
