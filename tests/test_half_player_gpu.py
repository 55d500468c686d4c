"""The player's opt-in `half` arithmetic (StreamDecoder(arithmetic="half")) on the tiny models: it takes exactly
the layers `levels` takes, those layers are right against float64 on the file's own integers at the derived bound of
tests/test_half_conv_gpu.py (check 3), whole frames stay within a cap computed from that bound, and the `exact` and `levels`
players are what they were."""
import pytest
import torch

import conv3_cases as C
from conftest import BITS, T, TINY_HNERV
from levels_cases import (DEV, all_frames, check_driver_names_the_layers, file_layer, hadamard_nerv_file, hnerv_file, nerv_file,
                          quant_model, spy)

pytestmark = pytest.mark.gpu

U =2.0 ** -11                  # unit roundoff of IEEE half
GELU_SLOPE = 1.13               # max gelu' = 1.129


@pytest.fixture(scope="module")
def ops():
    from neuroquant_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


@pytest.fixture(scope="module")
def frames(golden):
    return (T(golden("frames_320x640.npz")["frames"]).float() / 255.0).to(DEV)


def _layer_reference(x, n, delta, b, k, r):
    """float64 on the file's integers: (activation y, its derived bound, E = the largest bound of the PRE-activation).  The bound is
    check 3 of tests/test_half_conv_gpu.py: conv3_cases.bound + slope * (2^-11 * conv64(|x|, |n| delta) + conv64(s, |n| delta)),
    s = |x| on half subnormals"""
    x = x.cpu().double()
    w = n * delta.view(-1, 1, 1, 1)
    conv = C.forward_conv(x, w, k)
    ax = x.abs()
    s = torch.where((ax > 0) & (ax < 2.0 ** -14), ax, torch.zeros_like(ax))
    extra = C.forward_conv(U * ax + s, w.abs(), k)
    pre = conv + b.view(1, -1, 1, 1)
    y, _ = C.forward_reference(conv, b, ("psgelu", r, True))
    bound_y = C.bound(y) + GELU_SLOPE * torch.nn.functional.pixel_shuffle(extra, r)
    return y, bound_y, float((C.bound(pre) + extra).max())


@pytest.mark.parametrize("channel_wise", (True, False), ids=("channelwise", "layerwise"))
@pytest.mark.parametrize("bits", (BITS, [2] * 7, [8] * 7), ids=("mixed", "2bit", "8bit"))
def test_half_player(ops, golden, frames, tmp_path, bits, channel_wise):
    from neuroquant_amd.bitstream import StreamDecoder
    path = hnerv_file(golden, tmp_path, bits=bits, channel_wise=channel_wise)
    exact, lev = StreamDecoder(path, arithmetic="exact"), StreamDecoder(path, arithmetic="levels")
    before = {B: (all_frames(exact, B), all_frames(lev, B)) for B in (1, 2)}      # before any half decoder exists
    half = StreamDecoder(path, arithmetic="half")
    assert half.arithmetic == "half" and half.levels_used == {} and half.saturated() is False
    assert half.levels_ineligible == lev.levels_ineligible and sorted(half.levels_ineligible) == [0, 1]
    seen = spy(half)
    out, E = {}, {}
    for B in (1, 2):
        out[B] = all_frames(half, B)
        # the path taken: exactly the layers `levels` takes
        assert half.levels_used[B] == lev.levels_used[B] == [len(half.weights) - 2], (B, half.levels_used, lev.levels_used)
        for i in half.levels_used[B]:
            x = seen[(B, i)]
            cout, cin, k, _ = half.weights[i].shape
            n, delta, b = file_layer(path, i)
            ref, bound, E[B] = _layer_reference(x, n, delta, b, k, half._r[i])
            assert half._takes_levels(i, x) and not exact._takes_levels(i, x)
            err = (half._conv(i, x).cpu().double() - ref).abs()
            e_half = float((err / bound).max())
            print(f"layer {i} B {B} ({cin} -> {cout}, k {k}, {bits[i]} bits): error / derived bound {e_half:.4f} "
                  f"({float((err / C.bound(ref)).max()):.2f} x the bf16x3 bound)")
            assert e_half <= 1.0
    gain = float(half.weights[-1].abs().sum(dim=(1, 2, 3)).max())       # the head is linear: max_co sum |w_head[co]|
    for B in (1, 2):
        fe, fh = before[B][0], out[B]
        cap = 2 * (C.ATOL + C.RTOL * float(fe.abs().max())) + 0.5 * GELU_SLOPE * gain * E[B]
        diff = float((fe - fh).abs().max())
        pe, ph = (float(ops.frame_psnr(f, frames).double().mean()) for f in (fe, fh))
        print(f"B {B}: largest |half - exact| {diff:.3e} (cap {cap:.3e}: head gain {gain:.3f}, E {E[B]:.3e}); PSNR exact {pe:.5f} dB, "
              f"half {ph:.5f} dB, difference {ph - pe:+.6f} dB")
        assert diff <= cap
        assert abs(ph - pe) < 0.02
        for layout in ("chw", "hwc"):
            ue, uh = all_frames(exact, B, out="u8", layout=layout), all_frames(half, B, out="u8", layout=layout)
            d8 = (ue.int() - uh.int()).abs()
            print(f"B {B} u8 {layout}: {float((d8 != 0).float().mean()) * 100:.4f} % of the bytes differ")
            assert int(d8.max()) <= 1
    assert half.saturated() is False and exact.saturated() is False and lev.saturated() is False
    # the other two arithmetics, decoders opened before and after the half decoder ran: the same bits
    exact2, lev2 = StreamDecoder(path), StreamDecoder(path, arithmetic="levels")
    for B in (1, 2):
        assert torch.equal(all_frames(exact, B), before[B][0]) and torch.equal(all_frames(exact2, B), before[B][0])
        assert torch.equal(all_frames(lev, B), before[B][1]) and torch.equal(all_frames(lev2, B), before[B][1])
    assert torch.equal(all_frames(half, 1), out[1])


def test_entropy_coded_files_give_the_same_half_decoder(ops, golden, tmp_path):
    from neuroquant_amd.bitstream import StreamDecoder, write_stream
    qnn, emb = quant_model(golden, "traj_hnerv.npz", "hnerv", False)
    outs = {}
    for coding in ("packed", "rans", "auto"):
        path = str(tmp_path / f"{coding}.nqv")
        write_stream(qnn, path, "hnerv", dict(TINY_HNERV), embeddings=emb, coding=coding)
        dec = StreamDecoder(path, arithmetic="half")
        outs[coding] = (all_frames(dec, 1), all_frames(dec, 2), dec)
    assert outs["rans"][2].level_tensors["rans"] == 7 and outs["packed"][2].level_tensors["rans"] == 0
    for coding in ("rans", "auto"):
        assert outs[coding][2].levels_used == outs["packed"][2].levels_used and outs[coding][2].levels_used[1]
        assert torch.equal(outs[coding][0], outs["packed"][0]) and torch.equal(outs[coding][1], outs["packed"][1])
        assert outs[coding][2].saturated() is False


def test_nerv_last_block_takes_the_3x3_build(ops, tmp_path):
    """a NeRV file outside the Hadamard domain (randomly initialised: no fixture holds one): the last block, k = 3"""
    from neuroquant_amd.bitstream import StreamDecoder
    path = nerv_file(tmp_path)
    exact, half = StreamDecoder(path), StreamDecoder(path, arithmetic="half")
    seen = spy(half)
    gain = float(half.weights[-1].abs().sum(dim=(1, 2, 3)).max())
    for B in (1, 2):
        fe, fh = all_frames(exact, B), all_frames(half, B)
        assert half.levels_used[B] == [5] and half.weights[5].shape[2] == 3
        n, delta, b = file_layer(path, 5)
        _, _, E = _layer_reference(seen[(B, 5)], n, delta, b, 3, half._r[5])
        cap = 2 * (C.ATOL + C.RTOL * float(fe.abs().max())) + 0.5 * GELU_SLOPE * gain * E
        diff = float((fe - fh).abs().max())
        print(f"NeRV, B {B}: layers {half.levels_used[B]}, largest |half - exact| {diff:.3e} (cap {cap:.3e})")
        assert diff <= cap
    assert half.saturated() is False


def test_saturated_reports_a_clamped_activation_and_stays_set(ops, golden, tmp_path):
    """embeddings scaled by 1e8 drive the last block's input far beyond 65504 (the layers in front of it are GELU-linear at that
    size and stay finite in fp32): the flag goes up, stays up on clean frames, and belongs to that decoder alone"""
    from neuroquant_amd.bitstream import StreamDecoder
    path = hnerv_file(golden, tmp_path)
    half, other, exact = StreamDecoder(path, arithmetic="half"), StreamDecoder(path, arithmetic="half"), StreamDecoder(path)
    clean = half.decode([0])
    assert half.saturated() is False
    seen = spy(half)
    half._emb = [e * 1e8 for e in half._emb]
    half.decode([0])
    x = seen[(1, 5)]
    assert bool(torch.isfinite(x).all()) and float(x.abs().max()) > 65504.0
    assert half.saturated() is True
    half._emb = list(half.embeddings.split(1))
    assert torch.equal(half.decode([0]), clean) and half.saturated() is True
    assert other.saturated() is False and exact.saturated() is False


def test_refusals(ops, golden, tmp_path):
    from neuroquant_amd.bitstream import StreamDecoder
    assert StreamDecoder.ARITHMETICS == ("exact", "levels", "half")
    path = hnerv_file(golden, tmp_path)
    for bad in ("fast", "f16", "Half", None):
        with pytest.raises(ValueError):
            StreamDecoder(path, arithmetic=bad)
    had = hadamard_nerv_file(golden, tmp_path)
    with pytest.raises(ValueError):
        StreamDecoder(had, arithmetic="half")
    assert StreamDecoder(had).decode([0]).shape == (1, 3, 320, 640)


def test_driver_names_the_layers(golden, tmp_path):
    assert "clamped" not in check_driver_names_the_layers(golden, tmp_path, "half")
