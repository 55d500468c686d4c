"""Network-wise calibration driver (counterpart of the reference's methods/calibrate_network.py).

Same flags, same sequence (FP eval -> QuantModel -> set_bitwidth -> lazy scale init -> eval quant off / on ->
model_reconstruction -> final eval -> torch.save), with the reference's PNG DataLoader replaced by a GPU-resident
uint8 frame cache (frames are decoded ONCE; the reference re-decodes every frame every epoch in 4 worker processes,
which alone caps it at ~55 it/s) and PSNR and MS-SSIM computed by HIP kernels (ops.frame_psnr, ops.ms_ssim:
the definition of pytorch_msssim.ms_ssim; last-bit parity with that pip package is not pinned, see ops.ms_ssim).

    python -m neuroquant_amd.methods.calibrate_network --arch hnerv --config cfg.yaml --data_path bunny/ --vid Bunny \
        --ckpt epoch300.pth --batch_size 2 --channel_wise --init max --iters_w 21000 --weight 0.01 --b_start 20 \
        --b_end 2 --warmup 0.2 --lr 0.003 --precision 6 5 4 5 5 6 6
    (--precision_file bits.json takes the bit-widths from `bit_assign --budget_bytes N --out bits.json`;
    --synthetic N uses N synthetic Bunny-shaped frames instead of --data_path; --data_path clip.y4m / clip.yuv reads an 8-bit
    YUV 4:2:0 clip instead of a directory of PNGs (--yuv_size, --yuv_matrix, --yuv_range, --yuv_frames);
    the reconstruction objective is one entry of objective.TABLE (objective_of), squared error unless asked:
    --loss_domain yuv420 (--yuv_weights WY WU WV, default 6 1 1; matrix and range from --yuv_matrix / --yuv_range: §19),
    --rec_loss ssim | Fusion1 | Fusion3 | Fusion5 or --rec_weights W_MSE W_SSIM (the reference's MSE + (1 - SSIM) losses: §21),
    --rec_loss msssim or --rec_ms_weights W_MSE W_MS (1 - MS-SSIM; frames whose smaller side exceeds 160: §22); every evaluation
    then also logs the figure that objective is after;
    --export_stream FILE.nqv also writes the calibrated model as a bit stream that
    `python -m neuroquant_amd.methods.decode_stream` plays back; --stream_coding packed | rans | auto chooses between levels
    packed at their bit-width and entropy-coded levels; --embed_bits B (HNeRV) quantises the frame embeddings to B bits, calibrates
    and evaluates on the embeddings a player restores, and stores them as levels: DESIGN.md §17;
    --rate_lambda L (default 0: off) adds L * bits per pixel of the weight levels, priced by a static per-tensor model of the
    hard levels, to the phase-2 objective (ops.level_rate; the pixels are those of the frame cache), logs 'rate: ..' lines and,
    with --export_stream, the model's bytes beside the coded ones: DESIGN.md §23)
"""
import argparse
import logging
import os
import random
import sys
import time
from datetime import datetime

import numpy as np
import torch

from ..models import HNeRV, NeRV
from ..quantization import QuantModel, model_reconstruction
from ..utils import (CacheLoader, FrameCache, RoundTensor, data_split, get_config, setup_logger, synthetic_frames)
from .. import objective, ops
from ..objective import SSIM_METRIC_NAME, YUV_METRIC_NAMES   # added to the metrics by the SSIM / the YUV 4:2:0 objective


def parse_args(argv):
    p = argparse.ArgumentParser(description='running parameters', formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--seed', default=903, type=int)
    p.add_argument('--outf', default='unify')
    p.add_argument('--config', type=str)
    p.add_argument('--arch', type=str)
    p.add_argument('-p', '--print-freq', default=50, type=int)
    p.add_argument('--data_path', type=str)
    p.add_argument('--synthetic', type=int, default=0, help='use N synthetic frames instead of --data_path')
    add_yuv_args(p)
    p.add_argument('--loss_domain', type=str, default='rgb', choices=['rgb', 'yuv420'],
                   help='reconstruction loss of the calibration: RGB mean squared error, or the weighted plane MSEs of the 8-bit '
                        'YUV 4:2:0 codes (--yuv_matrix, --yuv_range, --yuv_weights; DESIGN.md §19)')
    add_yuv_loss_args(p)
    add_rec_loss_args(p)
    p.add_argument('--vid', type=str, default='Bunny')
    p.add_argument('--data_split', type=str, default='1_1_1')
    p.add_argument('--batch_size', default=12, type=int)
    prec = p.add_mutually_exclusive_group()
    prec.add_argument('--precision', type=int, nargs='+', default=None, help='per-layer bit-widths (default: 8 for all 7 layers)')
    prec.add_argument('--precision_file', type=str, default=None,
                      help='read the bit-widths from the JSON that `bit_assign --out` writes (its "bits" list)')
    p.add_argument('--channel_wise', action='store_true')
    p.add_argument('--hadamard', action='store_true')
    p.add_argument('--iters_w', default=20000, type=int)
    p.add_argument('--weight', default=0.01, type=float)
    p.add_argument('--b_start', default=20, type=int)
    p.add_argument('--b_end', default=2, type=int)
    p.add_argument('--warmup', default=0.2, type=float)
    p.add_argument('--input_prob', default=1.0, type=float)
    p.add_argument('--lr', default=0.0015, type=float)
    p.add_argument('--norm_p', default=2.0, type=float)
    p.add_argument('--init', default='max', type=str, choices=['max', 'mse', 'gaussian', 'l1', 'l2'])
    p.add_argument('--opt_mode', default='mse', type=str, choices=['mse', 'fisher_diag', 'fisher_full', 'lp_norm'])
    p.add_argument('--ckpt', default='None', type=str)
    p.add_argument('--dump_vis', action='store_true', default=False)
    p.add_argument('--export_stream', type=str, default=None,
                   help='write the calibrated model as a packed bit stream (.nqv, neuroquant_amd/bitstream.py) to this path')
    p.add_argument('--stream_coding', type=str, default='packed', choices=['packed', 'rans', 'auto'],
                   help='levels of --export_stream: packed at their bit-width, rANS coded, or whichever is smaller per tensor')
    p.add_argument('--embed_bits', type=int, default=None, choices=range(2, 9), metavar='2..8',
                   help='HNeRV: quantise the frame embeddings to this many bits (one scale per embedding channel); the calibration, '
                        'every evaluation after the FP one and --export_stream use the embeddings a player restores from the levels')
    p.add_argument('--rate_lambda', type=float, default=0.0,
                   help='weight of the rate term of phase 2: lambda * bits per pixel of the weight levels under a static '
                        'per-tensor model of the hard levels (DESIGN.md §23); 0 = off')
    args = p.parse_args(argv)
    rate_params(args, 1)   # a negative or non-finite --rate_lambda stops here
    if args.precision_file is not None:
        args.precision = read_precision_file(args.precision_file)
    elif args.precision is None:
        args.precision = [8] * 7
    return args


def read_precision_file(path, n_layers=None):
    """The "bits" list of the JSON `bit_assign --out` writes; ValueError if it is not a list of widths in 2..8 or, given
    n_layers, not of that length."""
    import json
    with open(path) as f:
        bits = json.load(f).get('bits')
    if not isinstance(bits, list) or not bits or not all(isinstance(b, int) and 2 <= b <= 8 for b in bits):
        raise ValueError(f'{path}: "bits" must be a list of bit-widths in 2..8, got {bits!r}')
    if n_layers is not None and len(bits) != n_layers:
        raise ValueError(f'{path} lists {len(bits)} bit-widths, the decoder has {n_layers} quantised layers')
    return bits


def seed_all(seed=903):
    random.seed(seed)
    np.random.seed(seed)
    os.environ['PYTHONHASHSEED'] = str(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)


def dist_setup():
    """Data-parallel launch: under `python -m torch.distributed.run --nproc-per-node N ... -m
    neuroquant_amd.methods.calibrate_network ...` every rank binds its GPU and joins the RCCL group BEFORE any other GPU call.
    -> (rank, world, device).  Single process: (0, 1, 'cuda').  NQ_DP_REHEARSAL=1 runs the collective path on a 1-rank
    group (one GPU)."""
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if 'RANK' not in os.environ or (world == 1 and not os.environ.get('NQ_DP_REHEARSAL')):
        return 0, 1, 'cuda'
    import torch.distributed as dist
    rank, local = int(os.environ['RANK']), int(os.environ.get('LOCAL_RANK', '0'))
    # the HSA runtime reads its environment when it initialises, i.e. at the first GPU call below: the variable that makes
    # RCCL's cross-process buffer sharing use dmabuf (the only IPC mode this host driver supports) must be set BEFORE it
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    torch.cuda.set_device(local)
    if not dist.is_initialized():
        dist.init_process_group('nccl', device_id=torch.device('cuda', local))
    return rank, world, f'cuda:{local}'


def add_yuv_args(p):
    """The flags that describe a .y4m / .yuv --data_path (load_frames reads them with getattr defaults)."""
    p.add_argument('--yuv_size', type=str, default=None, help='WxH of a raw .yuv clip whose name does not carry _<W>x<H>')
    p.add_argument('--yuv_matrix', type=str, default='bt709', choices=['bt709', 'bt601'], help='colour matrix of a YUV clip')
    p.add_argument('--yuv_range', type=str, default=None, choices=['limited', 'full'],
                   help="range of a YUV clip's codes (default: the file's XCOLORRANGE, else limited)")
    p.add_argument('--yuv_frames', type=int, default=None, help='use the first N frames of a YUV clip')


def add_yuv_loss_args(p):
    """The flag of the YUV 4:2:0 objective that calibration and training share (matrix and range: add_yuv_args)."""
    p.add_argument('--yuv_weights', type=float, nargs=3, default=[6.0, 1.0, 1.0], metavar=('WY', 'WU', 'WV'),
                   help='plane weights of the YUV 4:2:0 objective (--loss_domain yuv420 / loss: yuv420; DESIGN.md §19)')


# the reference's losses of MSE and single-scale SSIM (reference utils.py:119-130): name -> (w_mse, w_ssim); the one table of the
# calibration driver (--rec_loss) and the trainer (regress.SSIM_LOSSES, `loss:` of a config)
SSIM_LOSSES = {'ssim': (0.0, 1.0), 'Fusion1': (0.3, 0.7), 'Fusion3': (0.5, 0.5), 'Fusion5': (0.7, 0.3)}


# the MS-SSIM objective: the name --rec_loss and a config's `loss:` share, and its default (w_mse, w_ms)
MSSSIM_LOSS, MSSSIM_WEIGHTS = 'msssim', (0.0, 1.0)


def add_rec_loss_args(p):
    """The flags of the calibration's MSE + SSIM objective: a name of the reference's, or free weights."""
    g = p.add_mutually_exclusive_group()
    g.add_argument('--rec_loss', type=str, default='l2', choices=['l2'] + list(SSIM_LOSSES) + [MSSSIM_LOSS],
                   help='reconstruction loss of the calibration: squared error, or w_mse * MSE + w_ssim * (1 - SSIM) with the '
                        "reference's weights: " + ', '.join(f'{k} {v}' for k, v in SSIM_LOSSES.items()) +
                        f'; or {MSSSIM_LOSS}: 1 - MS-SSIM, the five-scale figure every evaluation logs (DESIGN.md §22)')
    g.add_argument('--rec_weights', type=float, nargs=2, default=None, metavar=('W_MSE', 'W_SSIM'),
                   help='free weights of the MSE + SSIM reconstruction loss')
    g.add_argument('--rec_ms_weights', type=float, nargs=2, default=None, metavar=('W_MSE', 'W_MS'),
                   help='free weights of the MSE + MS-SSIM reconstruction loss w_mse * MSE + w_ms * (1 - MS-SSIM)')


def objective_of(args):
    """The reconstruction objective the flags ask for (objective.Objective): --loss_domain yuv420 with the yuv_*
    flags, --rec_loss ssim / Fusion* or --rec_weights, --rec_loss msssim or --rec_ms_weights, else the squared error.  ValueError for
    an unknown name, flags that exclude each other, bad weights and --loss_domain yuv420 beside an objective defined on RGB frames."""
    name = getattr(args, 'rec_loss', None) or 'l2'
    free = [(flag, obj) for flag, obj in (('rec_weights', 'ssim'), ('rec_ms_weights', MSSSIM_LOSS)) if getattr(args, flag, None) is not None]
    if len(free) + (name != 'l2') > 1:
        raise ValueError('--rec_loss, --rec_weights and --rec_ms_weights exclude each other')
    if free:
        (flag, name), w = free[0], getattr(args, free[0][0])
    elif name in SSIM_LOSSES:
        flag, name, w = 'rec_loss', 'ssim', SSIM_LOSSES[name]
    elif name == MSSSIM_LOSS:
        flag, w = 'rec_loss', MSSSIM_WEIGHTS
    elif name != 'l2':
        raise ValueError(f"rec_loss must be one of {['l2'] + list(SSIM_LOSSES)}, got {name!r}")
    yuv420 = getattr(args, 'loss_domain', 'rgb') == 'yuv420'
    if name == 'l2':
        return objective.resolve('yuv420', yuv_loss_params(args), '--loss_domain yuv420') if yuv420 else objective.resolve('l2')
    keys = tuple(objective.TABLE[name]['defaults'])
    if len(w) != len(keys):
        raise ValueError(f"--{flag} takes {' '.join(k.upper() for k in keys)}, got {w!r}")
    if yuv420:
        raise ValueError(f"the MSE + {objective.TABLE[name]['title']} objective is defined on RGB frames: it does not combine with "
                         '--loss_domain yuv420')
    return objective.resolve(name, dict(zip(keys, w)), '--' + flag)


def rec_loss_params(args):
    """-> None unless the flags ask for an MSE + SSIM objective (--rec_loss ssim / Fusion*, --rec_weights), else dict(w_mse,
    w_ssim) of model_reconstruction(ssim=...); objective_of's refusals."""
    obj = objective_of(args)
    return dict(obj.params) if obj.name == 'ssim' else None


def rec_msssim_params(args):
    """-> None unless --rec_loss msssim (weights (0, 1)) or --rec_ms_weights W_MSE W_MS is given, else dict(w_mse, w_ms) of
    model_reconstruction(msssim=...); objective_of's refusals."""
    obj = objective_of(args)
    return dict(obj.params) if obj.name == MSSSIM_LOSS else None


def rate_params(args, pixels):
    """-> None for --rate_lambda 0 (off), else dict(weight, pixels) of model_reconstruction(rate=...); pixels = frames * H * W of
    the frame cache.  ValueError for a negative or non-finite weight."""
    lam = ops.level_rate_args('--rate_lambda', getattr(args, 'rate_lambda', 0.0) or 0.0)
    return dict(weight=lam, pixels=int(pixels)) if lam > 0.0 else None


@torch.no_grad()
def hard_level_rate(qnn, hadamard):
    """R_hard of the calibrated weight quantisers in bits (ops.level_rate_raw: the stored levels priced by the static model the
    rate term optimises), summed over the layers; one host read."""
    from ..quantization.calib_model import _quant_modules
    items = []
    for m in _quant_modules(qnn):
        wq = m.weight_quantizer
        items.append(((m.hadamard_weight if hadamard else m.org_weight).data, wq.alpha.data, wq.delta.data, wq.zero_point,
                      wq.n_levels))
    return float(ops.level_rate_raw(items, 0.0).total[1])


def yuv_loss_params(args):
    """matrix / full_range / weights of the YUV 4:2:0 objective (ops.yuv420_loss) and of the PSNR-Y / U / V evaluation: the
    --yuv_matrix and --yuv_range that describe a clip (bt709, limited when unset; a .y4m / .yuv --data_path without --yuv_range
    gives its own range) and --yuv_weights."""
    from ..videoio import is_video_file
    rng = getattr(args, 'yuv_range', None)
    if rng not in (None, 'limited', 'full'):
        raise ValueError(f"yuv_range must be 'limited' or 'full', got {rng!r}")
    full = rng == 'full'
    path = getattr(args, 'data_path', None)
    if rng is None and not getattr(args, 'synthetic', 0) and path and is_video_file(path):
        full = open_yuv_clip(args, path)[3]
    return dict(matrix=getattr(args, 'yuv_matrix', None) or 'bt709', full_range=bool(full),
                weights=tuple(getattr(args, 'yuv_weights', None) or ops.YUV_LOSS_WEIGHTS))


def open_yuv_clip(args, path):
    """The clip at `path` as the yuv_* attributes of args describe it -> (YuvFile, frames to use, matrix, full_range)."""
    from ..videoio import open_yuv, parse_size
    size = getattr(args, 'yuv_size', None)
    clip = open_yuv(path, size=parse_size(size) if isinstance(size, str) else size)
    rng = getattr(args, 'yuv_range', None)
    if rng not in (None, 'limited', 'full'):
        raise ValueError(f"yuv_range must be 'limited' or 'full', got {rng!r}")
    full = bool(clip.full_range) if rng is None else rng == 'full'
    n = getattr(args, 'yuv_frames', None)
    n = clip.frames if n is None else int(n)
    if not 0 < n <= clip.frames:
        raise ValueError(f'{path} holds {clip.frames} frames, yuv_frames asks for {n}')
    return clip, n, getattr(args, 'yuv_matrix', None) or 'bt709', full


def load_yuv_frames(args, cfg, device, batch=16):
    """-> uint8 (N,3,crop_h,crop_w) on `device` from a .y4m / .yuv clip: ops.yuv420_to_rgb_u8 on at most `batch` frames at a
    time, then the centre crop of the PNG path."""
    from ..videoio import centre_crop_offsets
    h, w = cfg['crop_h'], cfg['crop_w']
    clip, n, matrix, full = open_yuv_clip(args, args.data_path)
    top, left = centre_crop_offsets(clip.H, clip.W, h, w)
    out = torch.empty((n, 3, h, w), dtype=torch.uint8, device=device)
    for j in range(0, n, batch):
        k = min(batch, n - j)
        rgb = ops.yuv420_to_rgb_u8(torch.from_numpy(clip.read(j, k)).to(device), clip.H, clip.W, matrix, full)
        out[j:j + k] = rgb[:, :, top:top + h, left:left + w]
    return out


def load_frames(args, cfg, device):
    """-> uint8 (N,3,crop_h,crop_w) on `device`: sorted PNGs, center crop (reference videosets/datasets.py:8-30), or the
    frames of a .y4m / .yuv clip (8-bit 4:2:0; optional args.yuv_size / yuv_matrix / yuv_range / yuv_frames)."""
    h, w = cfg['crop_h'], cfg['crop_w']
    if args.synthetic:
        return synthetic_frames(args.synthetic, h, w, seed=args.seed, device=device)
    from ..videoio import is_video_file
    if is_video_file(args.data_path):
        return load_yuv_frames(args, cfg, device)
    from PIL import Image
    files = [os.path.join(args.data_path, x) for x in sorted(os.listdir(args.data_path))]
    out = torch.empty((len(files), 3, h, w), dtype=torch.uint8)
    for i, f in enumerate(files):
        a = torch.from_numpy(np.asarray(Image.open(f).convert('RGB')).copy()).permute(2, 0, 1)
        top, left = int(round((a.shape[1] - h) / 2.0)), int(round((a.shape[2] - w) / 2.0))
        out[i] = a[:, top:top + h, left:left + w]
    return out.to(device)


METRIC_NAMES = ['pred_seen_psnr', 'pred_seen_ssim', 'pred_unseen_psnr', 'pred_unseen_ssim']   # reference args.metric_names


@torch.no_grad()
def evaluate(model, cache: FrameCache, args, cfg, embeddings=None, msssim=None):
    """Per-frame decode + PSNR + MS-SSIM (reference calibrate_network.py:82-145); returns ([seen_psnr, unseen_psnr],
    embeddings) and leaves all four means on args.eval_metrics, keyed by METRIC_NAMES (as the reference leaves args.fps).
    Frames too small for five scales (min(H, W) <= 160) are evaluated for PSNR only: MS-SSIM is logged as n/a and stored
    as NaN.  embeddings (N, c, h, w): frame i is decoded from row i instead of model.encode's output.  msssim: dict(w_mse,
    w_ms) of an MS-SSIM objective the caller optimises (the trainer's `loss: msssim`; the calibration driver's flags are read
    from args): one more line names it beside the MS-SSIM it is after."""
    model.eval()
    n = len(cache)
    dev = cache.frames.device
    with_ssim = min(cache.frames.shape[-2:]) > 160
    # also the figure the objective is after (objective.TABLE): PSNR-Y / U / V for --loss_domain yuv420, the single-scale SSIM
    # for --rec_loss ssim / Fusion* / --rec_weights, one more line beside the MS-SSIM for an MS-SSIM objective
    obj = objective.resolve(MSSSIM_LOSS, msssim, 'evaluate(msssim=)') if msssim is not None else objective_of(args)
    extra = []
    psnr, ssim, embeds, dec_times = [], [], [], []
    for i in range(n):
        idx = torch.tensor([i], device=dev)
        img = cache.batch(idx)
        if embeddings is not None:
            emb = embeddings[i:i + 1]
        else:
            emb = model.encode(img) if args.arch == 'hnerv' else model.encode(idx.float() / n)
        out, embed_list, dec_time = model.decode(emb)
        embeds.append(embed_list[0])
        dec_times.append(dec_time)
        psnr.append(ops.frame_psnr(out, img))
        if with_ssim:
            ssim.append(ops.ms_ssim(out, img))
        fig = obj.eval_frame(out, img)
        if fig is not None:
            extra.append(fig)
        if i % args.print_freq == 0 or i == n - 1:
            logging.info('[{}], Eval at Step [{}/{}], FPS {}, PSNR {}, MS-SSIM {}'.format(
                datetime.now().strftime("%Y/%m/%d %H:%M:%S"), i + 1, n,
                round(cfg.get('batch_size', 1) / (sum(dec_times) / len(dec_times)), 1),
                RoundTensor(torch.cat(psnr).mean().cpu(), 2),
                RoundTensor(torch.cat(ssim).mean().cpu(), 4) if with_ssim else 'n/a'))
    psnr = torch.cat(psnr).cpu()
    ssim = torch.cat(ssim).cpu() if with_ssim else torch.full((n,), float('nan'))
    seen = [i for i in range(n) if i not in args.val_ind_list]
    unseen = list(args.val_ind_list)
    res = [psnr[seen].mean() if seen else torch.zeros(()), psnr[unseen].mean() if unseen else torch.zeros(())]
    args.eval_metrics = dict(zip(METRIC_NAMES, [res[0], ssim[seen].mean() if seen else torch.zeros(()),
                                                res[1], ssim[unseen].mean() if unseen else torch.zeros(())]))
    more, line = obj.eval_report(torch.cat(extra).cpu() if extra else None, ssim.mean() if with_ssim else None)   # over all frames
    args.eval_metrics.update(more)
    if line is not None:
        logging.info(line)
    model.train()
    return res, embeds


def report_line(tag, args):
    """'<tag>: best_pred_seen_psnr: .. | best_pred_seen_ssim: .. | best_pred_unseen_psnr: .. | best_pred_unseen_ssim: ..' from the
    metrics the last evaluate() left on args (the reference's print_str, calibrate_network.py:212-217)."""
    return (tag + ': ' if tag else '') + ' | '.join(
        f'best_{k}: {RoundTensor(v, 4 if k.endswith("ssim") else 2)}' for k, v in args.eval_metrics.items() if k in METRIC_NAMES)


def calibrate(args, cfg):
    if not torch.cuda.is_available():
        raise RuntimeError('neuroquant_amd needs an AMD GPU (no CPU path); the reference CPU path lives in oracle/ for tests')
    # one process per GPU: --batch_size is the GLOBAL batch, each rank takes batch_size/world frames of every batch; all
    # ranks hold all frames / embeddings / parameters, evaluate identically (replicas are bit-identical), rank 0 logs + saves
    rank, world, device = dist_setup()
    if args.batch_size % world:
        raise ValueError(f'--batch_size {args.batch_size} must divide over {world} ranks')
    frames = load_frames(args, cfg, device)
    cache = FrameCache(frames)
    n = len(cache)
    split = [int(x) for x in args.data_split.split('_')]
    train_ind, args.val_ind_list = data_split(list(range(n)), split, False, 0)
    train_loader = CacheLoader(cache, train_ind, args.batch_size, seed=args.seed, rank=rank, world=world)

    model = (HNeRV if args.arch == 'hnerv' else NeRV)(cfg).to(device)
    dec_param = sum(p.numel() for p in model.decoder.parameters()) / 1e6
    if rank == 0:
        os.makedirs(args.outf, exist_ok=True)
        setup_logger(os.path.join(args.outf, time.strftime('%Y%m%d_%H%M%S') + '.log'))
    else:
        logging.getLogger().setLevel(logging.WARNING)
    logging.info(f'Decoder_{round(dec_param, 2)}M' + (f' | data-parallel over {world} GPUs, {args.batch_size // world} frames per GPU' if world > 1 else ''))
    if args.ckpt != 'None':
        logging.info("=> loading checkpoint '{}'".format(args.ckpt))
        model.load_state_dict(torch.load(args.ckpt, map_location='cpu'), strict=False)
    else:
        logging.info('no --ckpt: random-initialised weights (throughput runs only)')
    model.to(device)

    def report(tag, res):   # res: evaluate()'s return value, whose four metrics are on args.eval_metrics
        logging.info(report_line(tag, args))

    logging.info('=======================Full-precision model========================')
    res, embedding_list = evaluate(model, cache, args, cfg)
    report('FP', res)

    embed_bits, qemb, stored = getattr(args, 'embed_bits', None), None, None
    if embed_bits is not None:
        if args.arch != 'hnerv':
            raise ValueError('--embed_bits applies to HNeRV: NeRV stores no embeddings')
        from ..bitstream import quantise_embeddings
        qemb = quantise_embeddings(embedding_list, embed_bits)
        stored = qemb.restored      # what a player rebuilds from the levels: everything below runs on it
        evaluate(model, cache, args, cfg, embeddings=stored)
        report('FP, embeddings quantised to {} bits'.format(embed_bits), None)

    wq_params = {'n_bits': 8, 'channel_wise': args.channel_wise, 'scale_method': args.init}
    qnn = QuantModel(model=model, hadamard=args.hadamard, weight_quant_params=wq_params).to(device)
    if getattr(args, 'precision_file', None):
        read_precision_file(args.precision_file, len(qnn.quant_modules()))
    args.qbits = qnn.set_bitwidth(args.precision)
    qnn.eval()
    cali_data = torch.cat(embedding_list, dim=0) if stored is None else stored
    logging.info('input embedding shape: {}'.format(cali_data.shape))

    qnn.set_quant_state(True)
    t0 = time.time()
    with torch.no_grad():
        qnn(cali_data[:args.batch_size])
    torch.cuda.synchronize()
    logging.info('Init time: {}'.format(time.time() - t0))

    qnn.set_quant_state(False)
    report('Close quantization', evaluate(qnn, cache, args, cfg, embeddings=stored)[0])
    qnn.set_quant_state(True)
    report('Weight quantization w/o opt', evaluate(qnn, cache, args, cfg, embeddings=stored)[0])

    logging.info('average bit-width: {}'.format(args.qbits))
    obj = objective_of(args)
    if obj.log_line() is not None:
        logging.info(obj.log_line())
    rate_obj = rate_params(args, n * cache.frames.shape[-2] * cache.frames.shape[-1])
    if rate_obj is not None:
        logging.info('rate term: lambda * bits per pixel of the weight levels, {}'.format(rate_obj))
    start = datetime.now()
    qnn.set_quant_state(weight_quant=True)
    model_reconstruction(qnn, cali_data=cali_data, gt=train_loader, arch=args.arch, batch_size=args.batch_size,
                         iters=args.iters_w, weight=args.weight, opt_mode='mse', hadamard=args.hadamard,
                         b_range=(args.b_start, args.b_end), warmup=args.warmup, p=args.norm_p, lr=args.lr,
                         **obj.engine_kwargs(), **(dict(rate=rate_obj) if rate_obj is not None else {}))
    torch.cuda.synchronize()
    logging.info(f"Training complete in: {str(datetime.now() - start)}")

    qnn.set_quant_state(weight_quant=True)
    res = evaluate(qnn, cache, args, cfg, embeddings=stored)[0]
    report('Weight quantization w/ opt', res)
    tag = 'CW' if args.channel_wise else 'LW'
    if rank == 0:
        torch.save(qnn, "{}/{}_W{}_prob{}_{}-init_{}.pth".format(args.outf, args.arch, args.qbits, args.input_prob, args.init, tag))
        if getattr(args, 'export_stream', None):
            from ..bitstream import write_stream
            s = write_stream(qnn, args.export_stream, args.arch, cfg, frames=n,
                             embeddings=(qemb if qemb is not None else cali_data) if args.arch == 'hnerv' else None,
                             coding=getattr(args, 'stream_coding', 'packed'))
            logging.info('bit stream: {} ({} bytes, {} bpp; nominal {} bytes; coding {}: levels {} bytes, '
                         'gap to entropy {} bytes)'.format(
                             args.export_stream, s['file_bytes'], round(s.get('bpp', float('nan')), 5), s['total_bytes_nominal'],
                             s['coding'], s['coded_level_bytes'], s['gap_to_entropy_bytes']))
            if rate_obj is not None:
                args.rate_hard_bytes = hard_level_rate(qnn, args.hadamard) / 8
                logging.info('rate model: R_hard / 8 = {} bytes of weight levels (bit stream: coded levels {} bytes, entropy {} '
                             'bytes, biases included)'.format(round(args.rate_hard_bytes, 1), s['coded_level_bytes'],
                                                              s['entropy_level_bytes']))
            if 'embedding' in s:
                e = s['embedding']
                logging.info('bit stream embeddings: {} bits, stored {} ({} bytes; packed / rans / temporal: {})'.format(
                    e['bits'], e['mode'], e['bytes'], ' / '.join(str(e['mode_bytes'][m]) for m in ('packed', 'rans', 'temporal'))))
    args.qnn = qnn
    return res


def main(argv):
    args = parse_args(argv)
    cfg = get_config(args.config)
    seed_all(args.seed)   # NB the reference defines seed_all but never calls it (calibrate_network.py:68-78, 311-324)
    exp_id = f"{args.vid}_e{cfg.get('epoch')}_b{cfg.get('batch_size')}_lr{cfg.get('learning_rate')}_{cfg.get('loss')}"
    args.outf = os.path.join('results', args.outf, exp_id,
                             "network-wise_calib/hadamard-{}_{}-init_batch{}_CW_weight{}_brange{}-{}_warmup{}_lr{}".format(
                                 args.hadamard, args.init, args.batch_size, args.weight, args.b_start, args.b_end,
                                 args.warmup, args.lr))
    try:
        return calibrate(args, cfg)
    finally:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            dist.destroy_process_group()


if __name__ == '__main__':
    main(sys.argv[1:])
