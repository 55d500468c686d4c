"""Host-side checks of the levels forward (include/nq_hip.h): the two entries are declared, exported and bound;
nq_conv3_levels_supported answers what the launch plan says (the unsplit tiled kernel, on a shape the bf16x3 path serves) on
every shape the GPU tests and the shipped models use; nq_conv_forward3_levels refuses bad arguments before any device call."""
import pytest

import conv3_cases as C
import levels_cases as L
from levels_cases import REFUSED, plan

NEW = ("nq_conv3_levels_supported", "nq_conv_forward3_levels")

# full-last-chunk shapes (tail kind 0) beside the table of conv3_cases, for k = 3 and 5: (shape, build)
EXTRA_ROWS = [(shape, inst) for shape, inst, _ in L.EXTRA]

# layers of the 3M models that take the path, by batch size
MODEL_LAYERS = [(B, 64, 40, 80, 848, 5) for B in (1, 2)] + [(B, 53, 160, 320, 176, 5) for B in (1, 2)] + \
               [(B, 44, 320, 640, 148, 5) for B in (1, 2)] + [(B, 24, 160, 320, 96, 3) for B in (1, 2)] + \
               [(B, 24, 320, 640, 96, 3) for B in (1, 2)] + [(2, 36, 40, 80, 384, 3)]


@pytest.fixture(scope="module")
def lib():
    from neuroquant_amd import _lib
    return _lib.lib()


def from_plan(p):
    return int(L.unsplit_tiled(p))


def test_symbols_declared_exported_and_bound(lib):
    L.check_symbols_declared_exported_and_bound(lib, NEW)


def test_supported_is_the_plans_answer(lib):
    seen = {0: 0, 1: 0}
    shapes = [c[0] for c in C.CASES] + [r[0] for r in EXTRA_ROWS] + MODEL_LAYERS + REFUSED + list(C.FORMERLY_REFUSED)
    for shape in shapes:
        got = lib.nq_conv3_levels_supported(*shape)
        assert got == from_plan(plan(shape)), shape
        seen[got] += 1
    assert seen[0] and seen[1]
    for shape in MODEL_LAYERS:
        assert lib.nq_conv3_levels_supported(*shape) == 1, shape
    for shape in REFUSED:
        assert lib.nq_conv3_levels_supported(*shape) == 0, shape
    assert lib.nq_conv3_levels_supported(2, 44, 320, 640, 148, 7) == 0
    assert lib.nq_conv3_levels_supported(0, 44, 320, 640, 148, 5) == 0
    # NeRV-3M's 36 -> 384 at 40 x 80 fills the chip with two frames only: whatever the plan says for one
    assert lib.nq_conv3_levels_supported(1, 36, 40, 80, 384, 3) == from_plan(plan((1, 36, 40, 80, 384, 3)))


def test_extra_rows_are_what_the_gpu_test_relies_on(lib):
    """tiled, supported, unsplit, a full last chunk, and the build named"""
    for shape, inst in EXTRA_ROWS:
        p = plan(shape)
        assert from_plan(p) == 1 and p["tail"] == 0 and C.inst_of(p) == inst, (shape, p)


def test_arguments_are_checked_before_the_device(lib):
    L.check_arguments_before_the_device(lib, "bf16")
