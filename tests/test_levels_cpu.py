"""Host-side checks of the levels forward (include/nq_hip.h): the two entries are declared, exported and bound;
nq_conv3_levels_supported answers what the launch plan says (the unsplit tiled kernel, on a shape the bf16x3 path serves) on
every shape the GPU tests and the shipped models use; nq_conv_forward3_levels refuses bad arguments before any device call."""
import ctypes
import os
import re

import pytest

import conv3_cases as C
from conftest import ROOT

NEW = ("nq_conv3_levels_supported", "nq_conv_forward3_levels")

# full-last-chunk shapes (tail kind 0) beside the table of conv3_cases, for k = 3 and 5: (shape without k, mi, waves per SIMD)
EXTRA = [((2, 16, 169, 67, 5), 1, 3), ((2, 48, 169, 67, 17), 2, 3), ((2, 30, 169, 67, 36), 3, 3), ((2, 32, 169, 67, 68), 5, 2)]
EXTRA_ROWS = [(s + (k,), ("tiled", mi, w)) for k in (3, 5) for s, mi, w in EXTRA]

# layers of the 3M models that take the path, by batch size
MODEL_LAYERS = [(B, 64, 40, 80, 848, 5) for B in (1, 2)] + [(B, 53, 160, 320, 176, 5) for B in (1, 2)] + \
               [(B, 44, 320, 640, 148, 5) for B in (1, 2)] + [(B, 24, 160, 320, 96, 3) for B in (1, 2)] + \
               [(B, 24, 320, 640, 96, 3) for B in (1, 2)] + [(2, 36, 40, 80, 384, 3)]
# ... and shapes that must not: the heads, a few-pixel layer, a toy layer
REFUSED = [(B, 37, 640, 1280, 3, 3) for B in (1, 2)] + [(B, 24, 640, 1280, 3, 3) for B in (1, 2)] + \
          [(B, 77, 10, 20, 1024, 3) for B in (1, 2)] + [(2, 5, 6, 7, 8, 3)]


@pytest.fixture(scope="module")
def lib():
    from neuroquant_amd import _lib
    return _lib.lib()


def plan(lib, shape):
    from neuroquant_amd import _lib
    p = _lib.Conv3Plan()
    assert lib.nq_conv_forward3_plan(*shape, ctypes.byref(p)) == 0, shape
    return {n: getattr(p, n) for n, _ in _lib.Conv3Plan._fields_}


def from_plan(p):
    return int(p["kernel"] == C.TILED and p["supported"] == 1 and p["nsplit"] == 1)


def test_symbols_declared_exported_and_bound(lib):
    from neuroquant_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nq_hip.h")).read()
    declared = set(re.findall(r"\b(nq_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and getattr(lib, name).argtypes is not None, name
    assert lib.nq_abi_version() == 7


def test_supported_is_the_plans_answer(lib):
    seen = {0: 0, 1: 0}
    shapes = [c[0] for c in C.CASES] + [r[0] for r in EXTRA_ROWS] + MODEL_LAYERS + REFUSED + list(C.FORMERLY_REFUSED)
    for shape in shapes:
        got = lib.nq_conv3_levels_supported(*shape)
        assert got == from_plan(plan(lib, shape)), shape
        seen[got] += 1
    assert seen[0] and seen[1]
    for shape in MODEL_LAYERS:
        assert lib.nq_conv3_levels_supported(*shape) == 1, shape
    for shape in REFUSED:
        assert lib.nq_conv3_levels_supported(*shape) == 0, shape
    assert lib.nq_conv3_levels_supported(2, 44, 320, 640, 148, 7) == 0
    assert lib.nq_conv3_levels_supported(0, 44, 320, 640, 148, 5) == 0
    # NeRV-3M's 36 -> 384 at 40 x 80 fills the chip with two frames only: whatever the plan says for one
    assert lib.nq_conv3_levels_supported(1, 36, 40, 80, 384, 3) == from_plan(plan(lib, (1, 36, 40, 80, 384, 3)))


def test_extra_rows_are_what_the_gpu_test_relies_on(lib):
    """tiled, supported, unsplit, a full last chunk, and the build named"""
    for shape, inst in EXTRA_ROWS:
        p = plan(lib, shape)
        assert from_plan(p) == 1 and p["tail"] == 0 and C.inst_of(p) == inst, (shape, p)


def test_arguments_are_checked_before_the_device(lib):
    n, p = None, ctypes.c_void_p(16)
    ok = (2, 44, 320, 640, 148, 5)                       # a shape the path serves

    def call(x=p, wt=p, scale=p, bias=p, y=p, z=p, shape=ok, r=1, epi=0):
        B, cin, H, W, cout, k = shape
        return lib.nq_conv_forward3_levels(x, wt, scale, bias, y, z, B, cin, H, W, cout, k, r, epi, n)

    assert lib.nq_conv3_levels_supported(*ok) == 1
    assert call(x=n) == -1 and call(wt=n) == -1 and call(scale=n) == -1
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
        assert call(shape=shape) == -2, shape            # heads, few-pixel and toy layers
    split = (2, 848, 40, 80, 64, 5)                      # HNeRV dec3's data gradient shape: tiled, split-K
    assert plan(lib, split)["nsplit"] > 1 and call(shape=split) == -2
