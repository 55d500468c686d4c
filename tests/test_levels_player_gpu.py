"""The player's opt-in `levels` arithmetic (StreamDecoder(arithmetic="levels")) on the tiny models: which
layers take the integer-level convolution, that those layers are right against float64 on the file's own integers, and how far
whole frames move from the default (`exact`) player, which stays bit-identical to what it was."""
import pytest
import torch

import conv3_cases as C
from conftest import BITS, T, TINY_HNERV
from levels_cases import (DEV, all_frames, check_driver_names_the_layers, file_layer, hadamard_nerv_file, hnerv_file, nerv_file,
                          quant_model, spy)

pytestmark = pytest.mark.gpu

CAP = 2 * (C.ATOL + C.RTOL)     # both players are within ATOL + RTOL * |ref| (|ref| <= 1: frames) of ONE float64 value at the
#                                 last block; the head behind it is the same launch on inputs that far apart


@pytest.fixture(scope="module")
def ops():
    from neuroquant_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


@pytest.fixture(scope="module")
def frames(golden):
    return (T(golden("frames_320x640.npz")["frames"]).float() / 255.0).to(DEV)


@pytest.mark.parametrize("channel_wise", (True, False), ids=("channelwise", "layerwise"))
@pytest.mark.parametrize("bits", (BITS, [2] * 7, [8] * 7), ids=("mixed", "2bit", "8bit"))
def test_levels_player(ops, golden, frames, tmp_path, bits, channel_wise):
    from neuroquant_amd.bitstream import StreamDecoder
    path = hnerv_file(golden, tmp_path, bits=bits, channel_wise=channel_wise)
    exact, lev = StreamDecoder(path, arithmetic="exact"), StreamDecoder(path, arithmetic="levels")
    assert exact.arithmetic == "exact" and lev.arithmetic == "levels" and lev.levels_used == {}
    # only the 1 x 1 layers (the stem and the first block) can never take the path, and the decoder says why
    assert [i for i, w in enumerate(lev.weights) if w.shape[2] == 1] == [0, 1] == sorted(lev.levels_ineligible)
    assert all("1 x 1" in why for why in lev.levels_ineligible.values()) and exact.levels_ineligible == {}
    seen = spy(lev)
    out = {}
    for B in (1, 2):
        out[B] = (all_frames(exact, B), all_frames(lev, B))
        # the path taken: exactly the layers the library offers it for, here the last block
        want = []
        for i, w in enumerate(lev.weights):
            cout, cin, k, _ = w.shape
            _, _, H, W = seen[(B, i)].shape
            if k in (3, 5) and ops.conv3_levels_supported(B, cin, H, W, cout, k):
                want.append(i)
        assert lev.levels_used[B] == want and want, (B, lev.levels_used, want)
        assert want == [len(lev.weights) - 2] and exact.levels_used[B] == []
        # those layers, both paths on the SAME input, against float64 on the file's own integers
        for i in want:
            x = seen[(B, i)]
            cout, cin, k, _ = lev.weights[i].shape
            n, delta, b = file_layer(path, i)
            conv = C.forward_conv(x.cpu(), n * delta.view(-1, 1, 1, 1), k)
            ref, _ = C.forward_reference(conv, b, ("psgelu", lev._r[i], True))
            assert lev._takes_levels(i, x) and not exact._takes_levels(i, x)
            e_lev = float(((lev._conv(i, x).cpu().double() - ref).abs() / C.bound(ref)).max())
            e_exact = float(((exact._conv(i, x).cpu().double() - ref).abs() / C.bound(ref)).max())
            print(f"layer {i} B {B} ({cin} -> {cout}, k {k}, {bits[i]} bits): error / bound levels {e_lev:.4f}, exact {e_exact:.4f}")
            assert e_lev <= 1.0 and e_exact <= 1.0
    for B in (1, 2):
        fe, fl = out[B]
        diff = float((fe - fl).abs().max())
        pe, pl = (float(ops.frame_psnr(f, frames).double().mean()) for f in (fe, fl))
        print(f"B {B}: largest |levels - exact| {diff:.3e} (cap {CAP:.1e}); PSNR exact {pe:.5f} dB, levels {pl:.5f} dB, "
              f"difference {pl - pe:+.6f} dB")
        assert diff <= CAP
        assert abs(pl - pe) < 0.02
        for layout in ("chw", "hwc"):
            ue, ul = all_frames(exact, B, out="u8", layout=layout), all_frames(lev, B, out="u8", layout=layout)
            d8 = (ue.int() - ul.int()).abs()
            print(f"B {B} u8 {layout}: {float((d8 != 0).float().mean()) * 100:.4f} % of the bytes differ")
            assert int(d8.max()) <= 1
    # one batch size's result does not depend on which was decoded first, and the record of the path is written once
    used = {B: list(v) for B, v in lev.levels_used.items()}
    assert torch.equal(all_frames(lev, 1), out[1][1]) and lev.levels_used == used


def test_entropy_coded_files_give_the_same_levels_decoder(ops, golden, tmp_path):
    from neuroquant_amd.bitstream import StreamDecoder, write_stream
    qnn, emb = quant_model(golden, "traj_hnerv.npz", "hnerv", False)
    outs = {}
    for coding in ("packed", "rans", "auto"):
        path = str(tmp_path / f"{coding}.nqv")
        write_stream(qnn, path, "hnerv", dict(TINY_HNERV), embeddings=emb, coding=coding)
        dec = StreamDecoder(path, arithmetic="levels")
        outs[coding] = (all_frames(dec, 1), all_frames(dec, 2), dec)
    assert outs["rans"][2].level_tensors["rans"] == 7 and outs["packed"][2].level_tensors["rans"] == 0
    for coding in ("rans", "auto"):
        assert outs[coding][2].levels_used == outs["packed"][2].levels_used and outs[coding][2].levels_used[1]
        assert torch.equal(outs[coding][0], outs["packed"][0]) and torch.equal(outs[coding][1], outs["packed"][1])


def test_hard_bias_file(ops, golden, tmp_path):
    from neuroquant_amd.bitstream import StreamDecoder
    path = hnerv_file(golden, tmp_path, name="h.nqv", bias="hard")
    exact, lev = StreamDecoder(path), StreamDecoder(path, arithmetic="levels")
    for B in (1, 2):
        diff = float((all_frames(exact, B) - all_frames(lev, B)).abs().max())
        print(f"hard biases, B {B}: largest |levels - exact| {diff:.3e}")
        assert lev.levels_used[B] == [5] and diff <= CAP


def test_nerv_last_block_takes_the_3x3_build(ops, tmp_path):
    """a NeRV file outside the Hadamard domain (randomly initialised: no fixture holds one): the last block, k = 3"""
    from neuroquant_amd.bitstream import StreamDecoder
    path = nerv_file(tmp_path)
    exact, lev = StreamDecoder(path), StreamDecoder(path, arithmetic="levels")
    for B in (1, 2):
        fe, fl = all_frames(exact, B), all_frames(lev, B)
        diff = float((fe - fl).abs().max())
        print(f"NeRV, B {B}: layers {lev.levels_used[B]}, largest |levels - exact| {diff:.3e}")
        assert lev.levels_used[B] == [5] and lev.weights[5].shape[2] == 3
        assert diff <= CAP


def test_refusals_and_the_default(ops, golden, tmp_path):
    from neuroquant_amd.bitstream import StreamDecoder
    path = hnerv_file(golden, tmp_path)
    with pytest.raises(ValueError):
        StreamDecoder(path, arithmetic="fast")
    plain, exact = StreamDecoder(path), StreamDecoder(path, arithmetic="exact")
    for B in (1, 2):
        assert torch.equal(all_frames(plain, B), all_frames(exact, B))
    assert plain.arithmetic == "exact"
    had = hadamard_nerv_file(golden, tmp_path)
    with pytest.raises(ValueError):
        StreamDecoder(had, arithmetic="levels")
    assert StreamDecoder(had).decode([0]).shape == (1, 3, 320, 640)


def test_driver_names_the_layers(golden, tmp_path):
    check_driver_names_the_layers(golden, tmp_path, "levels")
