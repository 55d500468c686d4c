"""Host-side checks of the half-precision levels forward (include/nq_hip.h): the two entries are declared,
exported and bound, the ABI version stays 7, no second eligibility query exists, and nq_conv_forward3_levels_f16 /
nq_weight_layout3_f16 refuse bad arguments before any device call (the pointers passed here are not device memory: a call that
got as far as a launch would not return one of these codes)."""
import ctypes
import inspect

import pytest

import levels_cases as L

NEW = ("nq_weight_layout3_f16", "nq_conv_forward3_levels_f16")


@pytest.fixture(scope="module")
def lib():
    from neuroquant_amd import _lib
    return _lib.lib()


def test_symbols_declared_exported_and_bound(lib):
    from neuroquant_amd import ops
    declared = L.check_symbols_declared_exported_and_bound(lib, NEW)
    assert len(lib.nq_conv_forward3_levels_f16.argtypes) == len(lib.nq_conv_forward3_levels.argtypes) + 1   # + the flag word
    # eligibility is nq_conv3_levels_supported: no query of its own
    assert not [n for n in declared if "supported" in n and ("f16" in n or "half" in n)]
    assert callable(ops.conv3_forward_levels_f16_raw)
    # ... which is a name for the one wrapper of both entries: that one takes the dtype and the flag word
    assert {"dtype", "sat_flag"} <= set(inspect.signature(ops.conv3_forward_levels_raw).parameters)


def test_arguments_are_checked_before_the_device(lib):
    call = L.check_arguments_before_the_device(lib, "f16")
    # a null flag is refused even where the shape would be, and before it: the same code on every shape
    assert call(sat=None) == -1 and call(sat=None, shape=L.SPLIT) == -1


def test_operand_entry_refuses_bad_arguments(lib):
    n, p = None, ctypes.c_void_p(16)
    assert lib.nq_weight_layout3_f16(n, p, 44, 148, 5, n) == -1 and lib.nq_weight_layout3_f16(p, n, 44, 148, 5, n) == -1
    assert lib.nq_weight_layout3_f16(p, p, 44, 148, 7, n) == -1 and lib.nq_weight_layout3_f16(p, p, 44, 148, 1, n) == -1
    assert lib.nq_weight_layout3_f16(p, p, 0, 148, 5, n) == -1 and lib.nq_weight_layout3_f16(p, p, 44, 0, 5, n) == -1
