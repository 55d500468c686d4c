"""Host-only checks behind tests/test_wgrad3_variants.py: the table of tests/wgrad3_cases.py names every template
instantiation of the bf16x3 weight-gradient kernels and the launch plan really sends each row to its instantiation; the
workspace the library asks for holds what the launch writes; the role-swapped form is not offered where the few-pixel kernel
owns the exchanged shape (its workspace is a 4-float token, the swapped launch would write slabs into it)."""
import ctypes

import pytest
import torch

from wgrad3_cases import (ALL_PCS, CASES, EXTRA_CASES, ROW_PCS, case_id, inputs, nseg_of, reference, slab_floats, swapped_reference,
                          tiles_of)

# Every instantiation conv_wgrad3_k3.hip / conv_wgrad3_k5.hip compile, per kernel size, as (mi, ni, pc) -- written out from the
# dispatch of conv_wgrad3_impl.h, not read from the library:
#   4-wave kernel (pc 0): ni in {1, 5, 6} x mi 1..5, ni 7 x mi 1..4                                                     19
#   producer/consumer, row segments of 1 / 2 / 4 rows (pc 1 / 12 / 14): (mi, ni) in {3,4,5} x {5,6} + {3,4} x {7}    3 x 8
#   producer/consumer, 128-pixel segments (pc 4): ni 1 x mi 2..5                                                         4
PER_K = [
    (1, 1, 0), (2, 1, 0), (3, 1, 0), (4, 1, 0), (5, 1, 0),
    (1, 5, 0), (2, 5, 0), (3, 5, 0), (4, 5, 0), (5, 5, 0),
    (1, 6, 0), (2, 6, 0), (3, 6, 0), (4, 6, 0), (5, 6, 0),
    (1, 7, 0), (2, 7, 0), (3, 7, 0), (4, 7, 0),
    (3, 5, 1), (4, 5, 1), (5, 5, 1), (3, 6, 1), (4, 6, 1), (5, 6, 1), (3, 7, 1), (4, 7, 1),
    (3, 5, 12), (4, 5, 12), (5, 5, 12), (3, 6, 12), (4, 6, 12), (5, 6, 12), (3, 7, 12), (4, 7, 12),
    (3, 5, 14), (4, 5, 14), (5, 5, 14), (3, 6, 14), (4, 6, 14), (5, 6, 14), (3, 7, 14), (4, 7, 14),
    (2, 1, 4), (3, 1, 4), (4, 1, 4), (5, 1, 4),
]
ALLOWED_MISSING = 0
# One of the 94 cannot exist: k = 3, 80 x 384 tile, four-row segments needs 2 x 82032 bytes of LDS, 224 more than the 160 KiB
# a workgroup has (the launch failed with a HIP launch error on an MI355X).  launch_wgrad3p no longer builds that kernel and
# plan_wgrad3 gives such layers two-row segments; the plan must never choose it.
UNLAUNCHABLE = {(3, 5, 6, 14)}


@pytest.fixture(scope="module")
def lib():
    from neuroquant_amd import _lib
    return _lib.lib()


def plan(lib, B, cin, H, W, cout, k):
    v = [ctypes.c_int() for _ in range(4)]
    assert lib.nq_conv_wgrad3_plan(B, cin, H, W, cout, k, *[ctypes.byref(t) for t in v]) == 0
    return tuple(t.value for t in v)      # (mi, ni, nsplit, pc)


@pytest.mark.parametrize("k", (3, 5))
def test_reference_is_anchored(k):
    """the unfold + matmul reference of the GPU file == torch.nn.grad.conv2d_weight in float64, and its exchanged-role reading
    == that function on the exchanged convolution (the identity ops.conv_wgrad_swapped3 rests on)"""
    x, dy = inputs((2, 3, 7, 9, 5, k))
    dw, db = reference(x, dy, k)
    want = torch.nn.grad.conv2d_weight(x.double(), (5, 3, k, k), dy.double(), padding=k // 2)
    torch.testing.assert_close(dw, want, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(db, dy.double().sum((0, 2, 3)), rtol=0, atol=0)
    # the convolution dy (5 channels) -> x (3 channels): its weight gradient from the same two tensors
    want_sw = torch.nn.grad.conv2d_weight(dy.double(), (3, 5, k, k), x.double(), padding=k // 2)
    torch.testing.assert_close(swapped_reference(dw), want_sw, rtol=1e-12, atol=1e-12)


def test_table_is_complete():
    want = {(k, mi, ni, pc) for k in (3, 5) for mi, ni, pc in PER_K}
    assert len(PER_K) == 47 == len(set(PER_K)) and len(want) == 94
    want -= UNLAUNCHABLE
    have = [(shape[5], mi, ni, pc) for shape, (mi, ni, pc) in CASES]
    assert len(have) == len(set(have)), "an instantiation is listed twice"
    assert set(have) <= want, sorted(set(have) - want)
    missing = sorted(want - set(have))
    assert len(missing) <= ALLOWED_MISSING, missing


def test_extra_cases_run_the_reclassified_segment(lib):
    for shape, (mi, ni, pc) in EXTRA_CASES:
        B, cin, H, W, cout, k = shape
        pmi, pni, nsplit, ppc = plan(lib, *shape)
        assert (pmi, pni, ppc) == (mi, ni, pc) and pc == 0 and k == 3 and W % 32 in (1, 2) and W > 64
        assert lib.nq_conv_wgrad3_supported(*shape) == 1 and lib.nq_conv_wgrad3_ws_floats(*shape) >= slab_floats(cin, cout, k, mi, ni, nsplit)
        assert nseg_of(B, H, W, pc) >= 2 * nsplit + 1


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_table_matches_plan(lib, case):
    shape, (mi, ni, pc) = case
    B, cin, H, W, cout, k = shape
    pmi, pni, nsplit, ppc = plan(lib, *shape)
    assert (pmi, pni, ppc) == (mi, ni, pc), f"{shape}: planned {(pmi, pni, ppc)}, recorded {(mi, ni, pc)}"
    # the decoder would really take it, and on the tiled kernel (the few-pixel kernel answers a 4-float token)
    assert lib.nq_conv_wgrad3_supported(*shape) == 1
    assert lib.nq_conv_wgrad3_ws_floats(*shape) > 4
    assert lib.nq_conv_wgrad3_split_io(*shape) == (3 if pc in (1, 12, 14) else 0)
    # ragged edges on every side
    if pc == 4:
        assert W % 128 == 0
    else:
        assert W % 32 != 0
        # left-edge, interior and ragged right-edge segment in every row (interior: the halo row, loaded as whole quads from
        # k//2 left of the segment, ends inside the image row -- the 4-wave kernel stages such segments on a path of its own)
        assert W >= 32 + 4 * ((32 + k - 1 + 3) // 4) - k // 2
    assert cout % (16 * mi) != 0
    if ni > 1:
        assert (cin * k * k) % (64 * ni) != 0
    else:
        assert cin * k * k <= 64
    assert cin >= 2 and H >= 2 * k
    nseg = nseg_of(B, H, W, pc)
    assert 1 <= nsplit <= nseg
    if pc == 0:
        assert nseg >= 2 * nsplit + 1   # some workgroup walks three segments: both buffers, every load site
    else:
        assert nseg // nsplit >= 6      # what the producer/consumer plans promise
    if pc in (12, 14):
        assert H % (pc - 10) == 0


def test_unlaunchable_variant_is_never_planned(lib):
    """the shape the table once held for it, and its neighbours, now take two-row segments"""
    for shape in [(2, 107, 112, 67, 193, 3), (2, 36, 320, 640, 80, 3), (2, 40, 160, 320, 148, 3)]:
        mi, ni, nsplit, pc = plan(lib, *shape)
        assert (mi, ni) == (5, 6) and pc == 12, (shape, mi, ni, pc)


def test_table_covers_frame_edges_tiles_and_uneven_splits(lib):
    assert 3 * sum(1 for shape, _ in CASES if shape[0] >= 2) >= len(CASES)
    for pc in ROW_PCS:
        multi = [shape for shape, (mi, ni, p) in CASES if p == pc and min(tiles_of(shape[1], shape[4], shape[5], mi, ni)) > 1]
        assert multi, f"pc {pc}: no entry with several channel tiles and several n-tiles"
    for pc in ALL_PCS:
        uneven = [shape for shape, (mi, ni, p) in CASES
                  if p == pc and nseg_of(shape[0], shape[2], shape[3], pc) % plan(lib, *shape)[2] != 0]
        assert uneven, f"pc {pc}: no entry whose segment count is not a multiple of nsplit"


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_workspace_is_large_enough(lib, case):
    shape, _ = case
    B, cin, H, W, cout, k = shape
    mi, ni, nsplit, pc = plan(lib, *shape)
    assert lib.nq_conv_wgrad3_ws_floats(*shape) >= slab_floats(cin, cout, k, mi, ni, nsplit)


def _swapped_offered(ops, lib, B, cin, H, W, cout, k):
    """what both Python gates (ops._wgrad_plain, the decoder's wgrad closure) ask; where it says yes, the workspace
    ops.conv_wgrad_swapped3 allocates must hold the slabs of the exchanged problem's plan"""
    offered = ops.conv_wgrad_swapped3_supported(B, cin, H, W, cout, k)
    if offered:
        mi, ni, nsplit, pc = plan(lib, B, cout, H, W, cin, k)
        assert lib.nq_conv_wgrad3_ws_floats(B, cout, H, W, cin, k) >= slab_floats(cout, cin, k, mi, ni, nsplit), (B, cin, H, W, cout, k)
    return offered


def test_swapped_shapes_fall_back(lib):
    """Heads with <= 4 output channels, very many input channels and <= 512 pixels: the exchanged shape belongs to the
    few-pixel kernel, nq_conv_wgrad3_ws_floats answers 4 floats, and the swapped launch (which has no few-pixel form) would
    write nsplit*co_pad*(n_pad+1) floats of slabs there.  The gates send them to the fp32 kernel; that the C entries refuse is checked with real
    buffers in tests/test_wgrad3_variants.py."""
    from neuroquant_amd import ops
    # (B, cout, H, W, cin, k) of the EXCHANGED problem, as the issue lists them
    for B, cout, H, W, cin, k in [(1, 3, 8, 8, 2500, 3), (2, 3, 8, 16, 2432, 3), (2, 1, 8, 16, 2700, 5)]:
        assert lib.nq_conv_wgrad3_supported(B, cout, H, W, cin, k) == 1
        assert lib.nq_conv_wgrad3_ws_floats(B, cout, H, W, cin, k) == 4
        assert not _swapped_offered(ops, lib, B, cin, H, W, cout, k)
    # around the thresholds of the few-pixel kernel (<= 512 pixels, H*W % 8 == 0, Cin*k*k*Cout >= 65536 of the exchanged
    # problem), on geometries with and without the 128 segments the tiled kernel wants: whatever is offered has its slabs
    yes = no = 0
    for k in (3, 5):
        for cout in (1, 2, 3, 4):
            if cout * k * k > 64:
                continue
            edge = -(-65536 // (cout * k * k))        # smallest cin the few-pixel kernel takes
            for B, H, W in [(1, 128, 4), (2, 64, 4), (1, 129, 4), (1, 128, 5), (1, 8, 8), (2, 8, 16), (2, 16, 16), (2, 16, 17), (4, 8, 16)]:
                for cin in (edge - 17, edge - 1, edge, edge + 1, edge + 40):
                    if _swapped_offered(ops, lib, B, cin, H, W, cout, k):
                        yes += 1
                    else:
                        no += 1
                        if lib.nq_conv_wgrad3_supported(B, cout, H, W, cin, k):      # refused although "supported": the token
                            assert lib.nq_conv_wgrad3_ws_floats(B, cout, H, W, cin, k) == 4
    assert yes and no
    # the shapes the swapped form exists for are still offered
    assert _swapped_offered(ops, lib, 2, 37, 640, 1280, 3, 3) and _swapped_offered(ops, lib, 2, 37, 48, 96, 3, 3)
    # ... and every table row with <= 4 input channels is the exchanged problem of an offered head
    for (B, cin, H, W, cout, k), _ in CASES:
        if cin * k * k <= 64 and cin <= 4:
            assert _swapped_offered(ops, lib, B, cout, H, W, cin, k)


def _parent_rule(lib, B, cin, H, W, cout, k):
    """ops.conv_wgrad_swapped3_supported as it was written in Python before ABI v6, on the queries it used"""
    return int(cout <= 4 and cin > 4 and cout * k * k <= 64 and lib.nq_conv_wgrad3_supported(B, cout, H, W, cin, k) == 1
               and lib.nq_conv_wgrad3_ws_floats(B, cout, H, W, cin, k) > 4)


def test_swapped_queries_restate_the_python_rule(lib):
    """nq_conv_wgrad3_swapped_supported / _ws_floats (ABI v6; arguments of the ORIGINAL layer) against the rule the Python
    host used to spell out, over the grid of test_swapped_shapes_fall_back (both sides of the few-pixel kernel's thresholds)"""
    shapes = [(1, 2500, 8, 8, 3, 3), (2, 2432, 8, 16, 3, 3), (2, 2700, 8, 16, 1, 5)]
    for shape in shapes:                                  # the few-pixel kernel owns the exchanged shape
        assert lib.nq_conv_wgrad3_swapped_ws_floats(*shape) == 0 and lib.nq_conv_wgrad3_swapped_supported(*shape) == 0
    for k in (3, 5):
        for cout in (1, 2, 3, 4, 5):
            edge = -(-65536 // (cout * k * k))
            for B, H, W in [(1, 128, 4), (2, 64, 4), (1, 129, 4), (1, 128, 5), (1, 8, 8), (2, 8, 16), (2, 16, 16), (2, 16, 17), (4, 8, 16)]:
                shapes += [(B, cin, H, W, cout, k) for cin in (edge - 17, edge - 1, edge, edge + 1, edge + 40, 4, 5)]
    shapes += [(B, cout, H, W, cin, k) for (B, cin, H, W, cout, k), _ in CASES if cin <= 4]
    yes = no = 0
    for shape in shapes:
        B, cin, H, W, cout, k = shape
        got = lib.nq_conv_wgrad3_swapped_supported(*shape)
        assert got == _parent_rule(lib, *shape), shape
        if got:
            yes += 1
            assert lib.nq_conv_wgrad3_swapped_ws_floats(*shape) == lib.nq_conv_wgrad3_ws_floats(B, cout, H, W, cin, k) > 4, shape
        else:
            no += 1
    assert yes and no
    for shape, want in [((2, 37, 640, 1280, 3, 3), 1), ((2, 37, 48, 96, 3, 3), 1),
                        ((1, 2500, 8, 8, 3, 3), 0),        # the few-pixel kernel owns the exchanged shape
                        ((2, 37, 48, 96, 5, 3), 0),        # Cout > 4
                        ((2, 4, 48, 96, 3, 3), 0),         # Cin <= 4
                        ((2, 37, 48, 96, 3, 5), 0)]:       # Cout * k * k = 75 > 64
        assert lib.nq_conv_wgrad3_swapped_supported(*shape) == want, shape


def test_lean_workspace_kept(lib):
    """the few-pixel layers of both 3M models still leave no slabs: a token workspace"""
    for shape in [(2, 77, 10, 20, 1024, 3), (2, 145, 2, 4, 1800, 3), (2, 72, 10, 20, 576, 3)]:
        assert lib.nq_conv_wgrad3_supported(*shape) == 1
        assert lib.nq_conv_wgrad3_ws_floats(*shape) == 4
