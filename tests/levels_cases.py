"""What the tests of the levels forward (dtype 'bf16') and of its half-precision build (dtype 'f16', §15) share: the
row table with its plan helpers and coverage check, the input builders (the seed is the caller's), the exact-integer and
run-to-run checks and the refusal check by dtype, the player tests' file builders, and the argument checks both C entries make
before any device call.  A plain module like conv3_cases.py: no fixtures, nothing collected."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import bitstream_ref as R
import conv3_cases as C
from conftest import BITS, ROOT, T, TINY_HNERV, TINY_NERV, state_dict_from_npz

DEV = "cuda"
CODE = {"plain": 0, "psgelu": 1, "tanh": 2, "ps": 3}      # NQ_EPI_* (include/nq_hip.h)
ENTRY = {"bf16": "nq_conv_forward3_levels", "f16": "nq_conv_forward3_levels_f16"}


# ------------------------------------------------------------------------------------------ rows and plans
def plan(shape):
    from neuroquant_amd import _lib
    q = _lib.Conv3Plan()
    assert _lib.lib().nq_conv_forward3_plan(*shape, ctypes.byref(q)) == 0, shape
    return {n: getattr(q, n) for n, _ in q._fields_}


def unsplit_tiled(p):
    return p["kernel"] == C.TILED and p["supported"] == 1 and p["nsplit"] == 1


# full last chunk (tail kind 0): (shape without k, mi, waves per SIMD); plain with bias, the 36-channel rows PS_GELU r 2 as well
_EXTRA = [((2, 16, 169, 67, 5), 1, 3), ((2, 48, 169, 67, 17), 2, 3), ((2, 30, 169, 67, 36), 3, 3), ((2, 32, 169, 67, 68), 5, 2)]
EXTRA = [(s + (k,), ("tiled", mi, w), [("plain", 1, True)] + ([("psgelu", 2, True)] if s[4] % 4 == 0 else []))
         for k in (3, 5) for s, mi, w in _EXTRA]
# Every tiled row of the table that has a forward epilogue, taken from the table alone (nothing is asked of the library while
# the module is collected, and the test ids do not move with the plan).  The rows whose plan is the UNSPLIT tiled kernel are the
# ones the levels entries serve -- SERVED today, counted in check_rows_cover...; on a split-K row the tests check that it is refused.
CANDIDATES = [(shape, inst, [e for e in epis if e[0] != "dgrad"]) for shape, inst, epis in C.CASES
              if inst[0] == "tiled" and any(e[0] != "dgrad" for e in epis)]
ROWS = CANDIDATES + EXTRA
IDS = [C.case_id(r) for r in ROWS]
SERVED = 34
TWO_CALLS = [((2, 7, 169, 67, 17, 3), ("plain", 1, True)), ((2, 7, 169, 67, 36, 5), ("ps", 2, True)),
             ((2, 7, 81, 67, 99, 3), ("psgelu", 3, True))]   # one register-staged tile (mi 2) and two LDS-DMA tiles (mi 3, mi 4)


def check_plan(ops, row):
    shape, inst, _ = row
    p = plan(shape)
    assert unsplit_tiled(p) and C.inst_of(p) == inst, "the plan no longer sends this shape to the build it is listed for"
    assert ops.conv3_levels_supported(*shape)
    return p


def check_rows_cover_every_build_tail_and_epilogue():
    """what the parametrised tests rely on: a tuning change of the plan shows up here, not as a thinner test"""
    served = [r for r in ROWS if unsplit_tiled(plan(r[0]))]
    assert len(served) - len(EXTRA) == SERVED and len(EXTRA) == 8 and served[-len(EXTRA):] == EXTRA
    assert len(CANDIDATES) > SERVED                  # ... and some split-K rows, for the refusal
    feats = [(r, C.Feat(r[0], plan(r[0]))) for r in served]
    for k in (3, 5):
        fk = [(r, f) for r, f in feats if r[0][5] == k]
        assert {f.inst[1:] for _, f in fk} == set(C.TILED_INSTS)
        for fam in ("reg", "dma"):
            assert {f.tail for _, f in fk if f.family == fam} == {0, 1, 2, 3}, (k, fam)
        epis = {(e[0], e[1], e[2], r[0][3] % 2) for r, _ in fk for e in r[2]}
        names = {(e[0], e[1], e[2]) for e in epis}
        assert {("plain", 1, True), ("plain", 1, False), ("tanh", 1, True), ("ps", 3, True), ("psgelu", 3, True), ("ps", 4, True),
                ("psgelu", 4, True)} <= names
        for name in ("ps", "psgelu"):
            assert (name, 2, True, 0) in epis and (name, 2, True, 1) in epis     # r 2: even W (DPP stores) and odd W
    for (shape, inst, _), f in feats[-len(EXTRA):]:
        assert f.tail == 0 and f.inst == inst


_SERVED_BEFORE = {}


def n_bits(idx):
    """2 .. 8, cycling over the rows that are served"""
    if not _SERVED_BEFORE:
        c = 0
        for i, r in enumerate(ROWS):
            _SERVED_BEFORE[i] = c
            c += int(unsplit_tiled(plan(r[0])))
    return 2 + _SERVED_BEFORE[idx] % 7


# ------------------------------------------------------------------------------------------ inputs and launches
def _extreme_levels(g, cout, cin, k, L):
    """integer weights n = level - zero_point with both extreme levels in every output channel and both extreme zero points"""
    lv = torch.randint(0, L, (cout, cin, k, k), generator=g)
    lv.view(cout, -1)[:, 0] = 0
    lv.view(cout, -1)[:, 1] = L - 1
    zp = torch.randint(0, L, (cout,), generator=g)
    zp[0], zp[-1] = 0, L - 1
    return lv, zp


def levels_inputs(shape, n_bits, seed):
    """(x, n, delta, b) on the CPU: Gaussian activations, integer weights (_extreme_levels), steps that give the weights the scale
    of conv3_cases.forward_inputs"""
    B, cin, H, W, cout, k = shape
    g = C._gen(shape, seed)
    x = torch.randn(B, cin, H, W, generator=g)
    L = 2 ** n_bits
    lv, zp = _extreme_levels(g, cout, cin, k, L)
    delta = (0.5 + torch.rand(cout, generator=g)) * math.sqrt(3) / (L * math.sqrt(cin * k * k))
    b = torch.randn(cout, generator=g) * 0.1
    n = (lv - zp.view(-1, 1, 1, 1)).float()
    return x, n, delta, b


def new_flag():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


def run(ops, dtype, xg, wt, scale, bias, shape, epi, flag=None):
    name, r, has_bias = epi
    return ops.conv3_forward_levels_raw(xg, wt, scale, bias if has_bias else None, shape[4], shape[5], CODE[name], r, dtype, flag)


def refused(ops, row, dtype):
    """a row the plan splits over K (or gives to another kernel): not offered, and the launch says unsupported"""
    from neuroquant_amd import _lib
    shape = row[0]
    B, cin, H, W, cout, k = shape
    assert not ops.conv3_levels_supported(*shape)
    x, n, scale = torch.zeros(B, cin, H, W, device=DEV), torch.zeros(cout, cin, k, k, device=DEV), torch.ones(cout, device=DEV)
    y, flag = torch.empty(B, cout, H, W, device=DEV), new_flag() if dtype == "f16" else None
    wt = ops.levels_operand(n, dtype=dtype)
    rc = getattr(_lib.lib(), ENTRY[dtype])(x.data_ptr(), wt.data_ptr(), scale.data_ptr(), None, y.data_ptr(), None,
                                           *([] if flag is None else [flag.data_ptr()]), B, cin, H, W, cout, k, 1, 0,
                                           torch.cuda.current_stream().cuda_stream)
    assert rc == -2
    with pytest.raises(_lib.NQLibraryError):
        ops.conv3_forward_levels_raw(x, wt, scale, None, cout, k, 0, 1, dtype, flag)
    assert flag is None or int(flag.item()) == 0


def exact_epis(epis):
    """plain (with / without bias) and ps: a shuffle is a permutation; a PS_GELU entry contributes its shuffle"""
    out = []
    for name, r, bias in epis:
        e = (name, r, bias) if name in ("plain", "ps") else ("ps", r, bias) if name == "psgelu" else None
        if e is not None and e not in out:
            out.append(e)
    return out


EXACT_IDX = [i for i in range(len(ROWS)) if exact_epis(ROWS[i][2])]


def check_exact_on_integer_inputs(ops, idx, dtype, seed):
    """small-integer activations, 8-bit levels, power-of-two steps, biases that are multiples of the step: every product and sum
    is exact in fp32 (and the operands in bf16 and in half), so the output must equal float64 bit for bit"""
    row = ROWS[idx]
    shape, inst, epis = row
    B, cin, H, W, cout, k = shape
    if not unsplit_tiled(plan(shape)):
        return refused(ops, row, dtype)
    check_plan(ops, row)
    K = cin * k * k
    assert K <= (1179 if k == 3 else 1275) and 4 * 255 * K + 8 < 2 ** 24     # every partial sum is an integer fp32 holds
    g = C._gen(shape, seed)
    x = torch.randint(-4, 5, (B, cin, H, W), generator=g).float()
    lv, zp = _extreme_levels(g, cout, cin, k, 256)
    n = (lv - zp.view(-1, 1, 1, 1)).float()
    assert float(n.max()) == 255 and float(n.min()) == -255
    assert torch.equal(n.half().float(), n) and torch.equal(x.half().float(), x)
    delta = torch.tensor([2.0 ** -(co % 7) for co in range(cout)])
    b = torch.randint(-8, 9, (cout,), generator=g).float() * delta
    conv = C.forward_conv(x, n, k) * delta.double().view(1, -1, 1, 1)        # integers times a power of two: exact
    assert float(conv.abs().max()) < 2 ** 24
    xg, scale, bg, flag = x.to(DEV), delta.to(DEV), b.to(DEV), new_flag() if dtype == "f16" else None
    wt = ops.levels_operand(n.to(DEV), dtype=dtype)
    for epi in exact_epis(epis):
        ry, rz = C.forward_reference(conv, b, epi)
        y, z = run(ops, dtype, xg, wt, scale, bg, shape, epi, flag)
        for got, ref in ((y, ry), (z, rz)):
            assert (got is None) == (ref is None)
            if ref is not None:
                want = ref.float()
                assert torch.equal(want.double(), ref), "the reference itself is not exact in fp32"
                assert torch.equal(got.cpu(), want), f"{epi}: {int((got.cpu() != want).sum())} of {want.numel()} outputs differ"
    assert flag is None or int(flag.item()) == 0


def check_two_calls_agree_bit_for_bit(ops, shape, epi, dtype, seed):
    p = plan(shape)
    assert unsplit_tiled(p) and (p["mi"] <= 2) == (shape[4] == 17)
    x, n, delta, b = levels_inputs(shape, 5, seed)
    xg, scale, bg, flag = x.to(DEV), delta.to(DEV), b.to(DEV), new_flag() if dtype == "f16" else None
    first = run(ops, dtype, xg, ops.levels_operand(n.to(DEV), dtype=dtype), scale, bg, shape, epi, flag)
    again = run(ops, dtype, xg, ops.levels_operand(n.to(DEV), dtype=dtype), scale, bg, shape, epi, flag)
    for a, c in zip(first, again):
        assert (a is None and c is None) or torch.equal(a.view(torch.int32), c.view(torch.int32))


# ------------------------------------------------------------------------------------------ player files
N = 8      # frames of the tiny models


def quant_model(golden, name, arch, had, bits=BITS, channel_wise=True):
    """a tiny model of tests/golden under uncalibrated 'max' scales, one quantised forward done"""
    from neuroquant_amd.models import HNeRV, NeRV
    from neuroquant_amd.quantization import QuantModel
    z = golden(name)
    model = (HNeRV if arch == "hnerv" else NeRV)(TINY_HNERV if arch == "hnerv" else TINY_NERV)
    missing, unexpected = model.load_state_dict(state_dict_from_npz(z, "sd:"), strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    qnn = QuantModel(model.to(DEV).eval(), hadamard=had,
                     weight_quant_params=dict(n_bits=8, channel_wise=channel_wise, scale_method="max"))
    qnn.set_bitwidth(bits)
    qnn.eval()
    qnn.set_quant_state(True)
    emb = T(z["emb"]).to(DEV)
    with torch.no_grad():
        qnn(emb[:2])
    return qnn, emb


def hnerv_file(golden, tmp_path, name="m.nqv", bits=BITS, channel_wise=True, **kw):
    from neuroquant_amd.bitstream import write_stream
    qnn, emb = quant_model(golden, "traj_hnerv.npz", "hnerv", False, bits=bits, channel_wise=channel_wise)
    path = str(tmp_path / name)
    write_stream(qnn, path, "hnerv", dict(TINY_HNERV), embeddings=emb, **kw)
    return path


def nerv_file(tmp_path):
    """a NeRV file outside the Hadamard domain (randomly initialised: no fixture holds one)"""
    from neuroquant_amd.bitstream import write_stream
    from neuroquant_amd.models import NeRV
    from neuroquant_amd.quantization import QuantModel
    torch.manual_seed(7)
    qnn = QuantModel(NeRV(TINY_NERV).to(DEV).eval(), hadamard=False,
                     weight_quant_params=dict(n_bits=8, channel_wise=True, scale_method="max"))
    qnn.set_bitwidth(BITS)
    qnn.eval()
    qnn.set_quant_state(True)
    with torch.no_grad():
        qnn(qnn.encode(torch.tensor([0.0, 0.125], device=DEV)))
    path = str(tmp_path / "nerv.nqv")
    write_stream(qnn, path, "nerv", dict(TINY_NERV), frames=N)
    return path


def hadamard_nerv_file(golden, tmp_path):
    """Hadamard-domain files store the levels of the transformed weights"""
    from neuroquant_amd.bitstream import write_stream
    qnn, emb = quant_model(golden, "traj_nerv_had.npz", "nerv", True)
    path = str(tmp_path / "n.nqv")
    write_stream(qnn, path, "nerv", dict(TINY_NERV), frames=N)
    return path


def check_driver_names_the_layers(golden, tmp_path, arithmetic):
    """methods/decode_stream.py with --arithmetic: -> what it printed"""
    path = hnerv_file(golden, tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "neuroquant_amd.methods.decode_stream", "--stream", path, "--arithmetic", arithmetic,
                        "--synthetic", str(N)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert f"arithmetic {arithmetic}: batch 1: layers [5]" in p.stdout and "float: PSNR" in p.stdout and "decode FPS" in p.stdout
    return p.stdout


def spy(dec):
    """record every layer's input on its way through dec._conv: {(B, layer): x}"""
    seen, orig = {}, dec._conv

    def conv(i, x):
        seen[(x.shape[0], i)] = x
        return orig(i, x)

    dec._conv = conv
    return seen


def all_frames(dec, B, **kw):
    return torch.cat([dec.decode(list(range(j, j + B)), **kw) for j in range(0, N, B)])


def file_layer(path, i):
    """(n = level - zero_point, delta per channel, bias) of layer i in float64, read with tests/bitstream_ref.py alone"""
    header, sec, _ = R.read(path)
    lay = header["layers"][i]
    co, ci, k, k2 = lay["shape"]
    lv = R.unpack(sec[f"w{i}.levels"], co * ci * k * k2, lay["n_bits"]).astype(np.float64).reshape(co, ci, k, k2)
    zp = sec[f"w{i}.zero_point"].astype(np.float64).reshape(-1, 1, 1, 1)
    delta = np.broadcast_to(sec[f"w{i}.delta"].astype(np.float64).reshape(-1), (co,))     # one step per channel or one in all
    assert header["bias"] == "soft"
    return T(lv - zp), T(np.ascontiguousarray(delta)), T(sec[f"b{i}.soft"].astype(np.float64))


# ------------------------------------------------------------------------------------------ host-side checks (no GPU)
# shapes nq_conv3_levels_supported refuses: the heads, a few-pixel layer, a toy layer
REFUSED = [(B, 37, 640, 1280, 3, 3) for B in (1, 2)] + [(B, 24, 640, 1280, 3, 3) for B in (1, 2)] + \
          [(B, 77, 10, 20, 1024, 3) for B in (1, 2)] + [(2, 5, 6, 7, 8, 3)]
SPLIT = (2, 848, 40, 80, 64, 5)     # HNeRV dec3's data gradient shape: tiled, split-K


def check_symbols_declared_exported_and_bound(lib, names):
    """-> the names include/nq_hip.h declares"""
    from neuroquant_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nq_hip.h")).read()
    declared = set(re.findall(r"\b(nq_[a-z0-9_]+)\s*\(", hdr))
    for name in names:
        assert name in declared and name in _lib.EXPORTS and getattr(lib, name).argtypes is not None, name
    assert lib.nq_abi_version() == 7
    return declared


def check_arguments_before_the_device(lib, dtype):
    """what both entries refuse before any device call (the pointers passed here are not device memory: a call that got as far
    as a launch would not return one of these codes); -> call(**changed arguments) for what is particular to an entry"""
    n, p = None, ctypes.c_void_p(16)
    ok = (2, 44, 320, 640, 148, 5)                       # a shape the path serves

    def call(x=p, wt=p, scale=p, bias=p, y=p, z=p, sat=p, shape=ok, r=1, epi=0):
        B, cin, H, W, cout, k = shape
        return getattr(lib, ENTRY[dtype])(x, wt, scale, bias, y, z, *([sat] if dtype == "f16" else []), B, cin, H, W, cout, k, r,
                                          epi, n)

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
        assert lib.nq_conv3_levels_supported(*shape) == 0 and call(shape=shape) == -2, shape   # heads, few-pixel and toy layers
    assert plan(SPLIT)["nsplit"] > 1 and lib.nq_conv3_levels_supported(*SPLIT) == 0 and call(shape=SPLIT) == -2
    return call
