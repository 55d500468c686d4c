"""Scale init by search on the GPU: csrc/scale_init.hip against the numpy restatement of the definition
(tests/scale_init_ref.py) on every route of its launch plan, against what the real reference returned (tests/golden/
scale_init.npz), through the quantiser, the calibration loop, the driver and bit_assign's table.

The plan changes route at rows of 512 / 513 elements (a wave per row -> a workgroup per row) and 8192 / 8193 (-> rows cut into
pieces); (1, 70001) is one row over nine pieces, (300, 27) many rows that share workgroups four at a time."""
import copy
import logging
import os
import types

import numpy as np
import pytest
import torch

import scale_init_ref as S
from conftest import T, TINY_HNERV, state_dict_from_npz
from oracle import nq_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(1, 1), (1, 9), (3, 63), (3, 64), (3, 65), (5, 255), (5, 256), (5, 257), (2, 1025), (300, 27), (1, 70001),
          (3, 512), (3, 513), (2, 8192), (2, 8193)]
LEVELS = (4, 8, 16, 256)
CANARY = 12345.0
TIE = 2.0 ** -36


@pytest.fixture(scope="module")
def ops():
    from neuroquant_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def bits(t):
    """the bit pattern of a float tensor, so that NaNs compare"""
    t = t.detach().cpu()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32).numpy()


def same(got, want):
    """fp32 values equal bit for bit (a NaN equals a NaN, whatever its sign: 0 / 0 differs between the host and the device)"""
    got, want = np.array(got, np.float32), np.array(want, np.float32)
    return bool(np.all((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))


def data_of(rows, row_len):
    """random weight rows, then the five constructed ones (zeros, constant, all-positive, all-negative, one outlier)"""
    return np.concatenate([S.make_rows(rows, row_len, seed=rows * 100003 + row_len), S.constructed_rows(row_len, seed=row_len)])


def run_search(ops, x, K, p):
    """two calls into buffers with canaries behind them -> the outputs of the first as numpy, after the common checks"""
    rows = x.shape[0]
    outs = []
    for _ in range(2):
        d, z = (torch.full((rows + 8,), CANARY, device=DEV) for _ in range(2))
        c = torch.full((rows + 8,), 77, device=DEV, dtype=torch.int32)
        s = torch.full((rows + 2, S.NC), CANARY, device=DEV, dtype=torch.float64)
        ops.scale_init_search_raw(x, K, p, out=(d[:rows], z[:rows], c[:rows], s[:rows]))
        assert bool((d[rows:] == CANARY).all() and (z[rows:] == CANARY).all() and (c[rows:] == 77).all() and (s[rows:] == CANARY).all())
        outs.append((d[:rows], z[:rows], c[:rows], s[:rows]))
    for a, b in zip(*outs):
        assert np.array_equal(bits(a), bits(b))                        # two calls: the same bits
    d, z, c, s = outs[0]
    return d.cpu().numpy(), z.cpu().numpy(), c.cpu().numpy(), s.cpu().numpy()


def check_search(ops, x_np, K, p, tag):
    """choice equal (near-ties within 2^-36 relative either way, at most 2 % of the rows), delta / zp the bits of the chosen
    candidate, scores within 1e-12 relative"""
    d, z, c, s = run_search(ops, torch.from_numpy(x_np).to(DEV), K, p)
    ties = 0
    for r, row in enumerate(x_np):
        win, _, _, sc, cands = S.search_row(row, K, p)
        assert np.all(np.abs(s[r] - sc) <= 1e-12 * np.abs(sc)), (tag, r, s[r], sc)
        assert 0 <= c[r] < S.NC, (tag, r, c[r])
        if c[r] != win:
            assert abs(sc[c[r]] - sc[win]) <= TIE * sc[win], (tag, r, c[r], win, sc)
            ties += 1
        cd, cz = cands[c[r]]
        assert same([d[r], z[r]], [cd, cz]), (tag, r)
    assert ties <= 0.02 * len(x_np), (tag, ties)
    return c


def check_gaussian(ops, x_np, K, tag):
    """bit-equal on the rows whose float64 mean and variance lie further than 2^-36 relative from an fp32 rounding midpoint;
    the others (at most 1 %) are skipped"""
    rows = x_np.shape[0]
    x = torch.from_numpy(x_np).to(DEV)
    outs = []
    for _ in range(2):
        d, z = (torch.full((rows + 8,), CANARY, device=DEV) for _ in range(2))
        st = torch.full((rows + 2, 2), CANARY, device=DEV)
        ops.scale_init_gaussian_raw(x, K, out=(d[:rows], z[:rows], st[:rows]))
        assert bool((d[rows:] == CANARY).all() and (z[rows:] == CANARY).all() and (st[rows:] == CANARY).all())
        outs.append((d[:rows], z[:rows], st[:rows]))
    for a, b in zip(*outs):
        assert np.array_equal(bits(a), bits(b))
    rd, rz, rst, m64 = S.gaussian(x_np, K)
    skipped = 0
    d, z, st = outs[0]
    for r in range(rows):
        if x_np.shape[1] > 1 and min(S.fp32_midpoint_distance(m64[r, 0]), S.fp32_midpoint_distance(m64[r, 1])) <= TIE:
            skipped += 1
            continue
        got = torch.stack([d[r], z[r], st[r, 0], st[r, 1]]).cpu().numpy()
        assert same(got, [rd[r], rz[r], rst[r, 0], rst[r, 1]]), (tag, r, got, rd[r], rz[r], rst[r])
    assert skipped <= 0.01 * rows, (tag, skipped)
    return st.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_search_equals_the_restatement(ops, shape):
    rows, row_len = shape
    x = data_of(rows, row_len)
    for K in LEVELS:
        for p in (3.5, 1.0):
            c = check_search(ops, x, K, p, (shape, K, p))
            assert c[rows] == 0 and c[rows + 1] == 0                   # zeros and the constant row: the full (empty) range
            if K == 4:                                                 # the outlier row: the search leaves candidate 0
                assert (c[rows + S.OUTLIER] > 0) == (row_len in S.OUTLIER_CLIPS_AT_4_LEVELS), (shape, p, c[rows:])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_gaussian_equals_the_restatement(ops, shape):
    rows, row_len = shape
    x = data_of(rows, row_len)
    for K in LEVELS:
        st = check_gaussian(ops, x, K, (shape, K))
        if row_len > 1:
            assert st[rows + 1, 1] == 0.0 and st[rows + 1, 0] == np.float32(0.37)      # the constant row: var = 0 exactly


def test_a_row_of_more_than_256_pieces(ops):
    """(1, 257 * 8192 + 5): a layer-wise tensor of over 2 M elements is cut into 258 pieces, so the passes over the per-piece
    ranges, sums and partial scores (256 threads, one piece each) go round a second time"""
    x = S.make_rows(1, 257 * 8192 + 5, seed=258)
    x[0, 256 * 8192 + 17], x[0, 257 * 8192 + 3] = x.max() * 1.5, x.min() * 1.25      # the range lives in pieces 257 and 258
    for p in (3.5, 1.0):
        check_search(ops, x, 16, p, ("258 pieces", 16, p))
    check_gaussian(ops, x, 16, ("258 pieces", 16))


def test_out_buffers_are_checked_before_the_launch(ops):
    """out=: a buffer of the wrong size, dtype, device or layout is a ValueError, not a write past its end"""
    x = torch.from_numpy(S.make_rows(6, 40, seed=3)).to(DEV)
    f = lambda n, dt=torch.float32: torch.zeros(n, device=DEV, dtype=dt)      # noqa: E731
    good = (f(6), f(6), f(6, torch.int32), f(60, torch.float64))
    ops.scale_init_search_raw(x, 16, 3.5, out=good)
    ops.scale_init_search_raw(x, 16, 3.5, out=good[:3] + (None,))
    for i, bad in ((0, f(5)), (1, f(6, torch.float64)), (2, f(6)), (2, None), (3, f(59, torch.float64)), (3, f(60)),
                   (0, torch.zeros(6)), (1, f(12)[::2])):
        with pytest.raises(ValueError):
            ops.scale_init_search_raw(x, 16, 3.5, out=good[:i] + (bad,) + good[i + 1:])
    with pytest.raises(ValueError):
        ops.scale_init_search_raw(x, 16, 3.5, out=good[:3])
    ops.scale_init_gaussian_raw(x, 16, out=(f(6), f(6), None))
    for bad in ((f(6), f(6), f(11)), (f(7), f(6), f(12)), (f(6), None, f(12)), (f(6), f(6))):
        with pytest.raises(ValueError):
            ops.scale_init_gaussian_raw(x, 16, out=bad)


def test_search_leaves_the_full_range_where_it_should(ops):
    """weight rows at 2-4 bits: most rows take a clipped range (the reason for the feature), none at 8 bits"""
    x = S.make_rows(64, 144, seed=5)
    for p in (3.5, 1.0):
        assert (check_search(ops, x, 16, p, ("clip", 16, p)) > 0).mean() > 0.5
        assert (check_search(ops, x, 256, p, ("clip", 256, p)) == 0).all()


def test_a_row_without_a_winner(ops):
    """a NaN or an Inf in a row: choice -1 and NaN scales for that row in the raw entry, the other rows of the call stay
    correct; the dispatcher raises a ValueError that names the first such row"""
    for rows, row_len in ((6, 100), (6, 700), (3, 9000)):
        x = S.make_rows(rows, row_len, seed=row_len)
        x[1, row_len // 3] = np.nan
        if rows > 4:
            x[4, 5] = np.inf
        bad = [1, 4] if rows > 4 else [1]
        xg = torch.from_numpy(x).to(DEV)
        for K, p in ((16, 3.5), (4, 1.0)):
            d, z, c, s = run_search(ops, xg, K, p)
            for r in range(rows):
                if r in bad:
                    assert c[r] == -1 and np.isnan(d[r]) and np.isnan(z[r])
                else:
                    win, rd, rz, sc, _ = S.search_row(x[r], K, p)
                    assert c[r] == win and same([d[r], z[r]], [rd, rz])
                    assert np.all(np.abs(s[r] - sc) <= 1e-12 * np.abs(sc))
        w = xg.view(rows, -1, 1, 1)
        for method in ("mse", "l1", "gaussian"):
            with pytest.raises(ValueError, match="row 1 of %d" % rows):
                ops.scale_init(w, 16, True, method)
        with pytest.raises(ValueError, match="row 0 of 1"):
            ops.scale_init(w, 16, False, "mse")
    assert ops.scale_init(torch.from_numpy(S.make_rows(4, 30, 1)).to(DEV).view(4, 30, 1, 1), 16, True, "l1")[0].shape == (4, 1, 1, 1)


def test_kernels_equal_the_reference(ops, golden):
    """the rule of tests/test_scale_init_cpu.py, with the kernels in the restatement's place"""
    def on_gpu(x, K, cw, method):
        d, z = ops.scale_init(torch.from_numpy(np.ascontiguousarray(x)).to(DEV), K, cw, method)
        return d.cpu().numpy(), z.cpu().numpy()

    S.check_against_fixture(golden("scale_init.npz"), on_gpu)


@pytest.mark.parametrize("method", ("mse", "l1", "gaussian"))
def test_through_the_quantiser(ops, method):
    """UniformAffineQuantizer(scale_method=m): result shapes as for 'max', the fake-quantised tensor is the oracle's with the
    restatement's scales"""
    from neuroquant_amd.quantization import UniformAffineQuantizer
    g = torch.Generator().manual_seed(11)
    w = torch.randn(12, 6, 3, 3, generator=g) * 0.05 * (1 + 3 * torch.rand(12, 1, 1, 1, generator=g))
    b = torch.randn(12, generator=g) * 0.1
    for x, cw in ((w, True), (b, True), (w, False)):
        for nb in (3, 4, 8):
            q = UniformAffineQuantizer(n_bits=nb, channel_wise=cw, scale_method=method)
            qmax = UniformAffineQuantizer(n_bits=nb, channel_wise=cw, scale_method="max")
            y, ymax = q(x.to(DEV)), qmax(x.to(DEV))
            assert q.inited and isinstance(q.delta, torch.nn.Parameter)
            assert q.delta.shape == qmax.delta.shape and q.zero_point.shape == qmax.zero_point.shape
            rd, rz = S.scale_init(x.numpy(), 2 ** nb, cw, method)
            assert same(q.delta.detach().cpu().numpy(), rd) and same(q.zero_point.cpu().numpy(), rz), (method, cw, nb)
            assert torch.equal(y.cpu(), O.uaq_fake_quant(x, T(rd), T(rz), 2 ** nb)), (method, cw, nb)
            if nb == 3 and method != "gaussian" and cw and x.dim() == 4:
                assert not torch.equal(y, ymax)                          # new ground: not the 'max' scales


# ------------------------------------------------------------------------------------------ the tiny HNeRV
def _build(sd):
    from neuroquant_amd.models import HNeRV
    model = HNeRV(TINY_HNERV)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    return model.to(DEV).eval()


class _Replay:
    def __init__(self, frames, order, n):
        self.frames, self.order, self.n, self.pos = frames, order, n, 0

    def __len__(self):
        return self.order.shape[1]

    def __iter__(self):
        ep = self.order[self.pos]
        self.pos += 1
        for idx in ep:
            idx_t = torch.as_tensor(idx, dtype=torch.int64, device=DEV)
            yield {"img": self.frames[idx_t], "idx": idx_t, "norm_idx": idx_t.float() / self.n}


def test_calibration_loop_from_searched_scales(ops, golden):
    """model_reconstruction from scale_method='mse' against oracle.calibrate started from the restatement's scales: the tiny
    HNeRV of tests/test_hip_parity.py's trajectory test at 3-4 bits, 2 phase-1 + 38 phase-2 iterations, and that test's
    tolerances (first losses 2e-4; the rest by the multiples of the oracle's own spread stated there; PSNR 0.02 dB)."""
    import json
    from neuroquant_amd.quantization import QuantModel, model_reconstruction
    z = golden("traj_hnerv.npz")
    frames = T(golden("frames_320x640.npz")["frames"]).float() / 255.0
    sd = state_dict_from_npz(z, "sd:")
    wbits = [4, 4, 3, 4, 4, 4, 4]
    order, iters, emb = z["order"].reshape(-1, 2, 2), 40, T(z["emb"])

    dec = O.Decoder.from_state_dict(sd, "hnerv", [5, 4, 4, 2, 2], (1, 1))
    qs = O.QuantStack(dec, wbits, hadamard=False)
    clamped = 0
    for L, nb in zip(dec.layers, wbits):
        (wd, wz), (bd, bz) = S.scale_init(L.w.numpy(), 2 ** nb, True, "mse"), S.scale_init(L.b.numpy(), 2 ** nb, True, "mse")
        L.wd, L.wz, L.bd, L.bz = T(wd), T(wz), T(bd), T(bz)
        lv = torch.round(L.w / L.wd) + L.wz
        clamped += int(((lv < 0) | (lv > 2 ** nb - 1)).sum())
    assert clamped > 100                                                # new ground: weights outside the clamped range
    ref = np.array(O.calibrate(qs, emb, frames, order, iters))
    with torch.no_grad():
        ref_psnr = float(O.psnr_per_frame(qs.forward(emb), frames).mean())

    ops.set_conv_precision("fp32")
    try:
        qnn = QuantModel(_build(sd), hadamard=False, weight_quant_params=dict(n_bits=8, channel_wise=True, scale_method="mse"))
        qnn.set_bitwidth(wbits)
        qnn.eval()
        qnn.set_quant_state(True)
        fr, em = frames.to(DEV), emb.to(DEV)
        with torch.no_grad():
            qnn(em[:2])
        for m, L in zip(qnn.quant_modules(), dec.layers):
            assert m.weight_quantizer.scale_method == "mse" == m.bias_quantizer.scale_method
        rec = []
        model_reconstruction(qnn, cali_data=em, gt=_Replay(fr, order, 8), arch="hnerv", batch_size=2, iters=iters, weight=0.01,
                             opt_mode="mse", hadamard=False, b_range=(20, 2), warmup=0.2, p=2.0, lr=0.003, recorder=rec)
        qnn.set_quant_state(True)
        with torch.no_grad():
            psnr = float(torch.cat([ops.frame_psnr(qnn(em[i:i + 1])[0], fr[i:i + 1]) for i in range(8)]).mean())
    finally:
        ops.set_conv_precision(None)
    log = np.array(rec)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "traj_sensitivity.json")) as f:
        sp = json.load(f)["hnerv"]["spread"]
    assert log.shape == ref.shape
    np.testing.assert_array_equal(log[:, 2:], ref[:, 2:])
    rel = np.abs(log[:, 0] - ref[:, 0]) / np.abs(ref[:, 0])
    same = tot = 0
    d_rel = []
    for m, L in zip(qnn.quant_modules(), dec.layers):
        same += int(((m.weight_quantizer.alpha >= 0).cpu() == (L.wa >= 0)).sum())
        tot += L.wa.numel()
        d = m.weight_quantizer.delta.detach().cpu().reshape(-1)
        d_rel.append(((d - L.wd.reshape(-1)).abs() / L.wd.reshape(-1).abs()).numpy())
    d_rel = np.concatenate(d_rel)
    print("loop from mse scales: loss rel first3 %.2e, all %.2e; final delta rel median %.2e; masks equal %.4f; PSNR %.4f vs oracle "
          "%.4f; %d weights outside the clamped range" % (rel[:3].max(), rel.max(), np.median(d_rel), same / tot, psnr, ref_psnr, clamped))
    np.testing.assert_allclose(log[:3, 0], ref[:3, 0], rtol=2e-4)
    assert rel.max() <= 3.0 * sp["loss_rel_all"]
    assert np.median(d_rel) <= 3.0 * sp["final_delta_rel_median"]
    assert same / tot >= sp["mask_agreement"] - 0.10
    assert abs(psnr - ref_psnr) < 0.02


def test_driver_init_mse_exports_a_stream_that_plays_the_live_model(tmp_path):
    """calibrate_network --init mse --synthetic 4 ... --export_stream for a few iterations: StreamDecoder's float frames are
    bit for bit the live model's evaluation"""
    from neuroquant_amd.bitstream import StreamDecoder
    from neuroquant_amd.methods import calibrate_network as cn
    root = logging.getLogger()
    saved = (root.level, list(root.handlers))
    stream = tmp_path / "out" / "model.nqv"
    args = cn.parse_args(["--arch", "hnerv", "--synthetic", "4", "--batch_size", "2", "--channel_wise", "--init", "mse",
                          "--iters_w", "8", "--weight", "0.01", "--warmup", "0.2", "--lr", "0.003",
                          "--precision", "4", "4", "3", "4", "4", "4", "4", "--export_stream", str(stream)])
    args.outf = str(tmp_path / "run")
    try:
        cn.seed_all(903)
        cn.calibrate(args, dict(TINY_HNERV))
        for h in list(root.handlers):
            if h not in saved[1]:
                h.close()
                root.removeHandler(h)
    finally:
        root.setLevel(saved[0])
        for h in list(root.handlers):
            if h not in saved[1]:
                root.removeHandler(h)
    log = "".join(open(os.path.join(args.outf, f)).read() for f in sorted(os.listdir(args.outf)) if f.endswith(".log"))
    assert "Init time" in log and "Weight quantization w/ opt" in log
    assert any("mse-init" in f for f in os.listdir(args.outf))
    qnn = args.qnn
    assert all(m.weight_quantizer.n_bits in (3, 4) for m in qnn.quant_modules())
    dec = StreamDecoder(str(stream))
    qnn.set_quant_state(True)
    with torch.no_grad():
        for idx in ([0], [1, 2], [3]):
            assert torch.equal(dec.decode(idx), qnn(dec.embeddings[idx[0]:idx[-1] + 1])[0])


@pytest.mark.parametrize("hadamard", (False, True))
def test_bit_assign_table_shares_the_quant_models_scales(ops, golden, hadamard):
    """bit_assign's table with init='mse': bit for bit the perturbations of a lazily initialised QuantModel(scale_method='mse')"""
    from neuroquant_amd.methods import bit_assign
    from neuroquant_amd.quantization import QuantModel
    zt = golden("traj_hnerv.npz")
    model = _build(state_dict_from_npz(zt, "sd:"))
    emb = T(zt["emb"]).to(DEV)
    choices = (3, 4, 8)
    args = types.SimpleNamespace(channel_wise=True, hadamard=hadamard, init="mse")
    table = bit_assign.perturbation_table(model, choices, args)[0]
    tmax = bit_assign.perturbation_table(model, choices, types.SimpleNamespace(channel_wise=True, hadamard=hadamard, init="max"))[0]
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(table, tmax))       # 3 bits: not the 'max' table
    for ci, c in enumerate(choices):
        qnn = QuantModel(copy.deepcopy(model), hadamard=hadamard, weight_quant_params=dict(n_bits=8, channel_wise=True, scale_method="mse"))
        qnn.eval()
        qnn.set_bitwidth([c] * 7)
        qnn.set_quant_state(True)
        with torch.no_grad():
            qnn(emb[:2])
        pert = qnn.get_perturbation()
        assert len(pert) == 7
        for l, v in enumerate(pert):
            assert torch.equal(table[l][ci], v), (c, l)
