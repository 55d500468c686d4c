"""The routing of the bf16x3 convolution path, pinned: every host query of conv3.hip (forward / data gradient, weight gradient,
operand size) is asked over a fixed grid of shapes and the packed answers are compared with recorded SHA-256 digests.  A change of
the dispatch code that is meant to leave the plans alone must leave the three digests alone; after an INTENDED change of a plan
reprint them with `python tests/test_conv3_plan_digest_cpu.py` (record() below) and paste the three lines over DIGESTS.

Host calls only: nothing is allocated and nothing is launched, so the shapes on both sides of the 32-bit size guards cost nothing.
The few-pixel kernel's own 0x7FFFFF00-byte guard needs >= 2^20 input channels on <= 512 pixels.  With few output channels the
few-pixel plan wants slabs for a K loop that long and the tiled kernel has the shape on both sides; the guard pair therefore has
2304 output channels, where the grid alone passes the plan's cap of 1024 workgroups, no split is left and the few-pixel kernel
takes the shape just inside the guard.
One guard cannot be seen through a query: the weight gradient's Cout*H*W >= 2^31 refusal sits in the launch.  The launch is
called with placeholder pointers AT the refused shapes only (it returns before it touches them); on the near side it would run.

Non-positive H or W: every query answers 0 / NQ_ERR_INVALID (test_non_positive_sizes); such rows are not in the digests."""
import ctypes
import hashlib
import os
import struct
import sys

import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import conv3_cases
import wgrad3_cases

# every switch a plan reads (conv3.hip, conv_flat3.hip, conv_wgrad_flat3.hip, conv_igemm3_impl.h)
PLAN_ENV = ("NQ_FLAT3", "NQ_FLAT3_CPW", "NQ_SPLITK_MIN_CHUNKS", "NQ_IG3_OCC3_STEPS", "NQ_WGRAD_FLAT3", "NQ_WGRAD3_PC", "NQ_WGRAD3_SS",
            "NQ_WGRAD3_MINSEG", "NQ_WGRAD3_SHRINK", "NQ_WGRAD3_HEAD_SPLITS")

# recorded from the library of commit 9d84d7e (the last one before the dispatch resolved each plan in one place)
DIGESTS = {
    "forward": "8a7f6822f801012d7c17936183c6bd12e9193cff250c097c45ed13cb4db94c18",
    "wgrad": "06c500a9dab315f23764caf4106e7d858262338bf4596ab51c2eea140d981b2d",
    "operand": "9e7971edac97036fb640e8cba39962d1ed45ed291187d03fe04d143b12a4ecb1",
}

KS = (3, 5)
BS = (1, 2, 3, 8)
HWS = ((1, 1), (2, 4), (8, 8), (10, 20), (16, 32), (16, 33), (17, 67), (40, 80), (48, 96), (137, 70), (160, 320), (320, 640), (640, 1280))
CHANNELS = (1, 3, 4, 5, 12, 16, 17, 20, 24, 25, 29, 32, 33, 36, 44, 48, 64, 65, 77, 80, 96, 145, 148, 257, 384, 848, 1024, 1712)
GRID = [(B, cin, H, W, cout, k) for k in KS for B in BS for H, W in HWS for cin in CHANNELS for cout in CHANNELS]
TABLES = ([c[0] for c in conv3_cases.CASES] + list(conv3_cases.FORMERLY_REFUSED) + [c[0] for c in wgrad3_cases.CASES]
          + [c[0] for c in wgrad3_cases.EXTRA_CASES])
# (shape just inside, shape at the guard), (B, cin, H, W, cout, k)
FWD_GUARD = [((1, 64, 4095, 4096, 64, k), (1, 64, 4095, 4097, 64, k)) for k in KS]            # B*Cin*H*W*4 = 0xFFFFFF00 at the second
FLAT_GUARD = [((2, 1048575, 16, 16, 2304, k), (2, 1048576, 16, 16, 2304, k)) for k in KS]    # ... >= 0x7FFFFF00 on 512 pixels
WG_X_GUARD = [((2, 64, 2048, 2047, 48, k), (2, 64, 2048, 2048, 48, k)) for k in KS]          # x of 2 GiB at the second
WG_DY_GUARD = [((2, 48, 2048, 2047, 64, k), (2, 48, 2048, 2048, 64, k)) for k in KS]         # dy of 2 GiB at the second
WG_REFUSED = [((1, 16, 4096, 4095, 128, k), (1, 16, 4096, 4096, 128, k)) for k in KS]        # Cout*H*W = 2^31 at the second
WG_REFUSED_X = [(1, 128, 4096, 4096, 16, k) for k in KS]                                     # Cin*H*W = 2^31
GUARDS = FWD_GUARD + FLAT_GUARD + WG_X_GUARD + WG_DY_GUARD + WG_REFUSED
SHAPES = GRID + TABLES + [s for pair in GUARDS for s in pair] + WG_REFUSED_X

FLOOR = 300          # shapes of GRID behind every answer listed in test_every_branch_is_populated
X_SPLIT, Y_SPLIT = conv3_cases.X_SPLIT, conv3_cases.Y_SPLIT


def forward_answers(lib, shape):
    """rc of nq_conv_forward3_plan, the 13 ints of the nq_conv3_plan it fills, supported, split_io | workspace floats"""
    from neuroquant_amd import _lib
    q = _lib.Conv3Plan()
    rc = lib.nq_conv_forward3_plan(*shape, ctypes.byref(q))
    return (struct.pack("<i", rc) + bytes(q)
            + struct.pack("<iiq", lib.nq_conv3_supported(*shape), lib.nq_conv3_split_io(*shape), lib.nq_conv_forward3_ws_floats(*shape)))


def wgrad_answers(lib, shape):
    """rc and (mi, ni, nsplit, pc) of nq_conv_wgrad3_plan, supported, split_io, swapped_supported | workspace floats, swapped ones"""
    v = [ctypes.c_int() for _ in range(4)]
    rc = lib.nq_conv_wgrad3_plan(*shape, *[ctypes.byref(t) for t in v])
    return struct.pack("<8i2q", rc, *[t.value for t in v], lib.nq_conv_wgrad3_supported(*shape), lib.nq_conv_wgrad3_split_io(*shape),
                       lib.nq_conv_wgrad3_swapped_supported(*shape), lib.nq_conv_wgrad3_ws_floats(*shape),
                       lib.nq_conv_wgrad3_swapped_ws_floats(*shape))


def operand_answers(lib):
    """nq_conv3_weight_bytes of every (Cin, Cout, k) among the shapes, as the forward and as the data-gradient operand"""
    keys = sorted({(s[1], s[4], s[5]) for s in SHAPES} | {(s[4], s[1], s[5]) for s in SHAPES})
    return b"".join(struct.pack("<q", lib.nq_conv3_weight_bytes(*key)) for key in keys)


def record(lib):
    """the three digests and the answers behind them: {name: hex digest}, [forward bytes per shape], [weight-gradient bytes]"""
    fwd = [forward_answers(lib, s) for s in SHAPES]
    wg = [wgrad_answers(lib, s) for s in SHAPES]
    digests = {"forward": hashlib.sha256(b"".join(fwd)).hexdigest(), "wgrad": hashlib.sha256(b"".join(wg)).hexdigest(),
               "operand": hashlib.sha256(operand_answers(lib)).hexdigest()}
    return digests, fwd, wg


@pytest.fixture(scope="module", autouse=True)
def untuned_environment():
    """the plans read these (most of them once per process): with one of them set, the digests describe another library"""
    found = [v for v in PLAN_ENV if v in os.environ]
    assert not found, f"unset {', '.join(found)}: the launch plans read them, and the recorded digests are for the defaults"


@pytest.fixture(scope="module")
def lib():
    from neuroquant_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def answers(lib):
    digests, fwd, wg = record(lib)
    return digests, dict(zip(SHAPES, fwd)), dict(zip(SHAPES, wg))


def test_grid():
    assert len(GRID) == 81536 == len(set(GRID))


@pytest.mark.parametrize("name", ("forward", "wgrad", "operand"))
def test_digest(answers, name):
    got = answers[0][name]
    print(f'    "{name}": "{got}",')
    assert got == DIGESTS[name], f"the {name} answers of the bf16x3 dispatch changed (see this module's docstring)"


def test_every_branch_is_populated(answers):
    """a condition on the grid: each answer of the routing decision has at least FLOOR shapes of GRID behind it"""
    _, fwd, wg = answers
    n = {}

    def count(key):
        n[key] = n.get(key, 0) + 1

    for s in GRID:
        f = struct.unpack("<14i", fwd[s][:56])
        plan = dict(zip(("rc", "kernel", "supported", "split_io", "mi", "waves", "flat_nw", "flat_nb", "flat_mi", "nsplit", "per_split",
                         "tail", "lds_bytes", "lds_bytes_dgrad"), f))
        count(("kernel", plan["kernel"]))
        count(("split", plan["nsplit"] > 1))
        count(("supported", plan["supported"]))
        count(("waves", plan["waves"]))
        count(("tail", plan["tail"]))
        count(("split_io", plan["split_io"]))
        rc, mi, ni, nsplit, pc, sup, sio, swsup, ws, swws = struct.unpack("<8i2q", wg[s])
        count(("pc", pc))
        count(("token", ws == 4))
        count(("swapped", swsup))
        count(("swapped_ws0", swws == 0))
    want = ([("kernel", conv3_cases.TILED), ("kernel", conv3_cases.FLAT), ("split", True), ("split", False), ("supported", 1),
             ("supported", 0), ("waves", 0), ("waves", 2), ("waves", 3), ("tail", 0), ("tail", 1), ("tail", 2), ("tail", 3),
             ("split_io", 0), ("split_io", X_SPLIT), ("split_io", Y_SPLIT), ("split_io", X_SPLIT | Y_SPLIT)]
            + [("pc", pc) for pc in (0, 1, 12, 14, 4)] + [("token", True), ("swapped", 1), ("swapped_ws0", True)])
    for key in want:
        print(key, n.get(key, 0))
    thin = {key: n.get(key, 0) for key in want if n.get(key, 0) < FLOOR}
    assert not thin, thin
    # nothing answers outside the listed values
    assert {k for k in n if k[0] in ("kernel", "waves", "tail", "split_io", "pc")} <= set(want)


def test_guard_shapes_change_an_answer(lib, answers):
    _, fwd, wg = answers
    for inside, at in FWD_GUARD:        # the tiled kernel's 32-bit buffer offsets: offered just inside, not at 0xFFFFFF00 bytes
        assert inside[0] * inside[1] * inside[2] * inside[3] * 4 < 0xFFFFFF00 == at[0] * at[1] * at[2] * at[3] * 4
        assert (lib.nq_conv3_supported(*inside), lib.nq_conv3_supported(*at)) == (1, 0)
        assert fwd[inside] != fwd[at]
    for guard in (WG_X_GUARD, WG_DY_GUARD):   # the producer/consumer kernel's 32-bit offsets: the 4-wave kernel from 2 GiB on
        for inside, at in guard:
            assert struct.unpack("<8i2q", wg[inside])[4] == 14 and struct.unpack("<8i2q", wg[at])[4] == 0
            assert struct.unpack("<8i2q", wg[inside])[6] == 3 and struct.unpack("<8i2q", wg[at])[6] == 0      # split words
    for inside, at in WG_X_GUARD:
        assert inside[0] * inside[1] * inside[2] * inside[3] * 4 < 2 ** 31 == at[0] * at[1] * at[2] * at[3] * 4
    for inside, at in WG_DY_GUARD:
        assert inside[0] * inside[4] * inside[2] * inside[3] * 4 < 2 ** 31 == at[0] * at[4] * at[2] * at[3] * 4
    for inside, at in FLAT_GUARD:       # the few-pixel kernel's signed 32-bit offsets: the tiled kernel from 0x7FFFFF00 bytes on
        assert inside[0] * inside[1] * inside[2] * inside[3] * 4 < 0x7FFFFF00 <= at[0] * at[1] * at[2] * at[3] * 4
        a, b = struct.unpack("<14i", fwd[inside][:56]), struct.unpack("<14i", fwd[at][:56])
        assert (a[1], b[1]) == (conv3_cases.FLAT, conv3_cases.TILED)
        assert (a[3], a[9]) == (Y_SPLIT, 1) and b[3] == X_SPLIT and b[9] > 1          # split words, K split
        assert fwd[inside] != fwd[at]
    # The launch's own refusal (module docstring): placeholder pointers, called AT the refused shapes only.  Safe only because
    # conv_wgrad3_impl refuses these sizes BEFORE it plans or launches anything: an edit that moves that check behind the
    # launch must drop these calls first (on a machine with a GPU they would start kernels on these addresses).
    p, n = ctypes.c_void_p(16), None
    for inside, at in WG_REFUSED:
        assert inside[4] * inside[2] * inside[3] < 2 ** 31 == at[4] * at[2] * at[3]
        assert lib.nq_conv_wgrad3_supported(*inside) == 1 == lib.nq_conv_wgrad3_supported(*at)       # the queries do not see it
        assert lib.nq_conv_wgrad3(p, p, p, p, p, *at, 0, n, n) == -2
    for at in WG_REFUSED_X:
        assert at[1] * at[2] * at[3] == 2 ** 31
        assert lib.nq_conv_wgrad3(p, p, p, p, p, *at, 0, n, n) == -2


@pytest.mark.parametrize("shape", [(2, 64, 0, 64, 64, 3), (2, 64, 16, 0, 64, 5), (2, 64, -8, 64, 64, 3), (2, 64, 16, -40, 64, 5),
                                   (2, 64, 0, 64, 3, 3), (2, 1024, 0, 8, 1024, 3)])
def test_non_positive_sizes(lib, shape):
    """no kernel is asked a convolution without pixels: every query says so instead of planning one"""
    from neuroquant_amd import _lib
    assert lib.nq_conv_forward3_plan(*shape, ctypes.byref(_lib.Conv3Plan())) == -1
    assert lib.nq_conv_wgrad3_plan(*shape, *[ctypes.byref(ctypes.c_int()) for _ in range(4)]) == -1
    for query in ("nq_conv3_supported", "nq_conv3_split_io", "nq_conv_forward3_ws_floats", "nq_conv_wgrad3_supported",
                  "nq_conv_wgrad3_split_io", "nq_conv_wgrad3_ws_floats", "nq_conv_wgrad3_swapped_supported",
                  "nq_conv_wgrad3_swapped_ws_floats"):
        assert getattr(lib, query)(*shape) == 0, query


if __name__ == "__main__":
    from neuroquant_amd import _lib
    for key, value in record(_lib.lib())[0].items():
        print(f'    "{key}": "{value}",')
