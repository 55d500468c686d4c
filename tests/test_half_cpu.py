"""Host-side checks of the half-precision levels forward (include/nq_hip.h): the two entries are declared,
exported and bound, the ABI version stays 7, no second eligibility query exists, and nq_conv_forward3_levels_f16 /
nq_weight_layout3_f16 refuse bad arguments before any device call (the pointers passed here are not device memory: a call that
got as far as a launch would not return one of these codes)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

NEW = ("nq_weight_layout3_f16", "nq_conv_forward3_levels_f16")

# shapes nq_conv3_levels_supported refuses: the heads, a few-pixel layer, a toy layer (tests/test_levels_cpu.py)
REFUSED = [(B, 37, 640, 1280, 3, 3) for B in (1, 2)] + [(B, 24, 640, 1280, 3, 3) for B in (1, 2)] + \
          [(B, 77, 10, 20, 1024, 3) for B in (1, 2)] + [(2, 5, 6, 7, 8, 3)]


@pytest.fixture(scope="module")
def lib():
    from neuroquant_amd import _lib
    return _lib.lib()


def test_symbols_declared_exported_and_bound(lib):
    from neuroquant_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "nq_hip.h")).read()
    declared = set(re.findall(r"\b(nq_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and getattr(lib, name).argtypes is not None, name
    assert len(lib.nq_conv_forward3_levels_f16.argtypes) == len(lib.nq_conv_forward3_levels.argtypes) + 1   # + the flag word
    assert lib.nq_abi_version() == 7
    # eligibility is nq_conv3_levels_supported: no query of its own
    assert not [n for n in declared if "supported" in n and ("f16" in n or "half" in n)]
    assert callable(ops.conv3_forward_levels_f16_raw)


def test_arguments_are_checked_before_the_device(lib):
    n, p = None, ctypes.c_void_p(16)
    ok = (2, 44, 320, 640, 148, 5)                       # a shape the path serves

    def call(x=p, wt=p, scale=p, bias=p, y=p, z=p, sat=p, shape=ok, r=1, epi=0):
        B, cin, H, W, cout, k = shape
        return lib.nq_conv_forward3_levels_f16(x, wt, scale, bias, y, z, sat, B, cin, H, W, cout, k, r, epi, n)

    assert lib.nq_conv3_levels_supported(*ok) == 1
    assert call(x=n) == -1 and call(wt=n) == -1 and call(scale=n) == -1 and call(sat=n) == -1
    assert call(y=n) == -1 and call(y=n, epi=2) == -1    # plain / tanh write y
    assert call(z=n, epi=1, r=2) == -1 and call(z=n, epi=3, r=2) == -1
    assert call(epi=1, r=3) == -1                        # 148 channels do not shuffle by 3
    for i in range(5):
        bad = list(ok)
        bad[i] = 0
        assert call(shape=tuple(bad)) == -1              # a non-positive size
    assert call(epi=4, r=1) == -1                        # the data-gradient epilogue
    assert call(epi=0x100) == -2 and call(epi=0x200) == -2 and call(epi=2 | 0x300) == -2   # split-word bits
    assert call(shape=(2, 44, 320, 640, 148, 7)) == -2   # k = 7 not built
    assert call(shape=(70000, 44, 320, 640, 148, 5)) == -2
    for shape in REFUSED:
        assert lib.nq_conv3_levels_supported(*shape) == 0 and call(shape=shape) == -2, shape
    split = (2, 848, 40, 80, 64, 5)                      # HNeRV dec3's data gradient shape: tiled, split-K
    assert lib.nq_conv3_levels_supported(*split) == 0 and call(shape=split) == -2
    # a null flag is refused even where the shape would be, and before it: the same code on every shape
    assert call(sat=n, shape=split) == -1


def test_operand_entry_refuses_bad_arguments(lib):
    n, p = None, ctypes.c_void_p(16)
    assert lib.nq_weight_layout3_f16(n, p, 44, 148, 5, n) == -1 and lib.nq_weight_layout3_f16(p, n, 44, 148, 5, n) == -1
    assert lib.nq_weight_layout3_f16(p, p, 44, 148, 7, n) == -1 and lib.nq_weight_layout3_f16(p, p, 44, 148, 1, n) == -1
    assert lib.nq_weight_layout3_f16(p, p, 0, 148, 5, n) == -1 and lib.nq_weight_layout3_f16(p, p, 44, 0, 5, n) == -1
