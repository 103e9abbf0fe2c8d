"""CPU: K34's admission predicate and LDS size helper, and the argument checks that run before any launch."""
import ctypes

import pytest

from xuanpolicy_amd import _lib


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def test_admission_and_lds(lib):
    assert lib.xpa_small_q_lds_floats(32, 32, 128, 128, 16) == 34000 <= 40704   # the widest admitted carve
    assert lib.xpa_small_q_lds_floats(1, 4, 32, 32, 2) == lib.xpa_small_q_lds_floats(32, 4, 32, 32, 2)
    for h0 in (32, 64, 128):
        for h1 in (32, 64, 128):
            assert lib.xpa_small_q_ok(128, 4, h0, h1, 2) == 1 and lib.xpa_small_q_lds_floats(32, 4, h0, h1, 2) <= 40704
    assert lib.xpa_small_q_ok(512, 32, 128, 128, 16) == 1 and lib.xpa_small_q_ok(1, 1, 32, 32, 2) == 1


@pytest.mark.parametrize("shape", [(128, 4, 256, 128, 2), (128, 4, 128, 256, 2), (128, 4, 96, 128, 2), (128, 4, 128, 128, 17),
                                   (128, 4, 128, 128, 1), (513, 4, 128, 128, 2), (0, 4, 128, 128, 2), (128, 33, 128, 128, 2)])
def test_refused_shapes(lib, shape):
    assert lib.xpa_small_q_ok(*shape) == 0
    a = _block(*shape)
    assert lib.xpa_small_q_update(ctypes.byref(a), None) == 1


def _block(batch, d_in, h0, h1, k):
    """A block whose every pointer is a fake, 16-B aligned non-null address: only the checked field can fail."""
    a = _lib.XpaSmallQArgs()
    for name, typ in a._fields_:
        if typ is ctypes.c_void_p:
            setattr(a, name, 4096)
    a.batch, a.d_in, a.h0, a.h1, a.k, a.n_groups = batch, d_in, h0, h1, k, (batch + 31) // 32
    a.act_code, a.n_sched, a.n, a.n_rows, a.obs_ld = 1, 256, 1 << 20, 1000, d_in
    return a


def test_null_and_misplaced_pointers_rejected_before_launch(lib):
    assert lib.xpa_small_q_update(None, None) == 1
    assert lib.xpa_small_q_values(None, None, 4, 1, None, None) == 1
    for field in ("obs", "next", "act", "tW1", "param", "grad_part", "td_abs", "cursor"):
        a = _block(128, 4, 128, 128, 2)
        setattr(a, field, None)
        assert lib.xpa_small_q_update(ctypes.byref(a), None) == 1, field
    a = _block(128, 4, 128, 128, 2)
    a.gW1 = 4096 + 4 * ((1 << 20) - 8)   # a gradient view that runs past the flat gradient
    assert lib.xpa_small_q_update(ctypes.byref(a), None) == 1
    a = _block(128, 4, 128, 128, 2)
    a.n_groups = 3                       # not ceil(batch / 32)
    assert lib.xpa_small_q_update(ctypes.byref(a), None) == 1
    a = _block(128, 4, 128, 128, 2)
    assert lib.xpa_small_q_values(ctypes.byref(a), None, 4, 10, ctypes.c_void_p(4096), None) == 1
    assert lib.xpa_small_q_values(ctypes.byref(a), ctypes.c_void_p(4096), 3, 10, ctypes.c_void_p(4096), None) == 1
