"""FP32 INR trainer (counterpart of the reference's methods/regress.py:151-322; SURVEY §8f-4, a "next" row).

Same flags and schedule (Adam, weight_decay 0, `--lr_type cosine_0.1_1_0.1` / hybrid, a config's `loss:` = one objective of
objective.TABLE: `l2`, `yuv420`, the reference's `ssim` / `Fusion1` / `Fusion3` / `Fusion5`, `msssim`, or `lp`
(`loss_p: P`, `loss_weights: [W_ABS, W_MSE]`: the absolute-error losses on csrc/lp_loss.hip), per-epoch
`model_latest.pth`, final `epoch{N}.pth` state_dicts that `calibrate_network` loads).  The decoder runs as the fused
HIP stack (`ops.decoder_stack`: implicit-GEMM convs, fused PixelShuffle/GELU/tanh, data/weight gradients), frames come
from the GPU-resident cache; Adam and, by default, the ConvNeXt encoder stay in PyTorch (`--enc_kernels hip` runs the
encoder's Blocks on csrc/convnext.hip; `--enc_kernels hip_all` also its downsampling stages, patchify conv +
channels-first LayerNorm, on csrc/patchify.hip).  Evaluations report PSNR and MS-SSIM
(ops.ms_ssim); tensorboard is not produced.  `--qat ffnerv|hinerv --qat_bits B` trains the quantisation-aware baselines of the
reference's QATQuantizer: every decoder weight passes through csrc/qat.hip in front of the decoder node;
with `--export_stream FILE.nqv [--stream_coding packed|rans|auto] [--stream_encoder host|gpu]` the trained model (or, with
`--eval_only --weight ckpt`, a checkpoint) is also written as a bit stream that `python -m neuroquant_amd.methods.decode_stream`
plays back to the frames of the evaluation.  `--prune_ratio R` is the papers' other baseline, global unstructured
magnitude pruning: the R smallest part of the decoder's convolution weights, by magnitude over all of them at once, is set to zero
once the model and `--weight` are loaded (csrc/prune.hip) and held there through every optimiser step.

    python -m neuroquant_amd.methods.regress --arch hnerv --config cfg.yaml --data_path bunny/ --vid Bunny
"""
import argparse
import logging
import math
import os
import sys
import time
from datetime import datetime

import torch

from ..models import HNeRV, NeRV
from ..utils import CacheLoader, FrameCache, RoundTensor, data_split, get_config, setup_logger
from .. import objective, ops
from .calibrate_network import (MSSSIM_LOSS, MSSSIM_WEIGHTS, SSIM_LOSSES, add_yuv_args, add_yuv_loss_args, evaluate, load_frames, report_line, seed_all,
                                yuv_loss_params)


def parse_args(argv):
    p = argparse.ArgumentParser(description='running parameters', formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--seed', default=903, type=int)
    p.add_argument('--outf', default='unify')
    p.add_argument('--config', type=str)
    p.add_argument('--arch', type=str)
    p.add_argument('--data_path', type=str)
    p.add_argument('--synthetic', type=int, default=0)
    add_yuv_args(p)
    add_yuv_loss_args(p)
    p.add_argument('--vid', type=str, default='Bunny')
    p.add_argument('--data_split', type=str, default='1_1_1')
    p.add_argument('-p', '--print-freq', default=50, type=int)
    p.add_argument('--lr_type', type=str, default='cosine_0.1_1_0.1')
    p.add_argument('--weight', default='None', type=str)
    p.add_argument('--eval_only', action='store_true', default=False)
    p.add_argument('--enc_kernels', choices=('torch', 'hip', 'hip_all'), default='torch',
                   help="what runs the HNeRV encoder: PyTorch ops; 'hip': its ConvNeXt blocks on csrc/convnext.hip; 'hip_all': "
                        "the blocks and the downsampling stages (csrc/patchify.hip)")
    p.add_argument('--qat', choices=('ffnerv', 'hinerv'), default=None,
                   help="quantisation-aware training (the reference's QATQuantizer): every decoder weight, layer 0 and the head "
                        "included, is quantised in front of the decoder; biases and the encoder stay fp32")
    p.add_argument('--qat_bits', type=int, default=8, help='bit width of --qat, 2 .. 8')
    p.add_argument('--qat_seed', type=int, default=0, help="seed of the 'hinerv' noise mask")
    p.add_argument('--export_stream', type=str, default=None,
                   help='--qat: write the trained model as a bit stream (.nqv, bitstream.write_qat_stream) to this path')
    p.add_argument('--stream_coding', type=str, default='packed', choices=['packed', 'rans', 'auto'],
                   help='symbols of --export_stream: packed at their bit-width, rANS coded, or whichever is smaller per tensor')
    p.add_argument('--stream_encoder', type=str, default='host', choices=['host', 'gpu'],
                   help='who runs the rANS encoder of --export_stream: numpy on the host, or the HIP encoder on the device')
    p.add_argument('--prune_ratio', type=float, default=None,
                   help='global unstructured magnitude pruning: this part, in [0, 1], of the decoder convolution weights is zeroed '
                        'after the model and --weight are loaded and kept at zero while training; not with --qat')
    p.add_argument('--prune_scope', choices=('decoder',), default='decoder',
                   help="what --prune_ratio prunes: 'decoder', its convolution weights (biases, encoder and embeddings stay)")
    return p.parse_args(argv)


def prune_check(args):
    """--prune_ratio's rules, before anything runs"""
    ratio = getattr(args, 'prune_ratio', None)
    if ratio is None:
        return
    if getattr(args, 'qat', None) is not None:
        raise ValueError('--prune_ratio with --qat: mixing the two baselines is not defined here')
    if not 0.0 <= ratio <= 1.0:
        raise ValueError(f'--prune_ratio must lie in [0, 1], got {ratio}')


class WeightPruner:
    """--prune_ratio: the decoder's convolution weights (every 4-D parameter outside the encoder) pruned ONCE, globally by
    magnitude (ops.magnitude_prune_), and the mask of that moment; `hold` writes the zeros back into weights, gradients and both
    Adam moments in one launch after an optimiser step, so checkpoints keep their keys and hold the pruned weights as zeros."""

    def __init__(self, model, ratio):
        self.names, self.params = zip(*[(n, p) for n, p in model.named_parameters() if not n.startswith('encoder') and p.dim() == 4])
        self.tensors = [p.data for p in self.params]
        self.mask, self.sel = ops.magnitude_prune_(self.tensors, ratio)
        self.pruned = ops.prune_counts(self.tensors, self.mask)

    def hold(self, optimizer):
        state = [optimizer.state.get(p, {}) for p in self.params]
        ops.prune_apply_(self.tensors, self.mask, [p.grad for p in self.params], [s.get('exp_avg') for s in state],
                         [s.get('exp_avg_sq') for s in state])

    def sparsity(self):
        """{name: pruned part of the tensor, ..., 'total': of all of them}, from the mask"""
        out = {n: k / t.numel() for n, k, t in zip(self.names, self.pruned, self.tensors)}
        out['total'] = sum(self.pruned) / sum(t.numel() for t in self.tensors)
        return out

    def log(self):
        sp = self.sparsity()
        logging.info('sparsity: total {:.4f} ({} of {}) | '.format(sp['total'], sum(self.pruned), sum(t.numel() for t in self.tensors))
                     + ' '.join('{}: {:.4f}'.format(n, sp[n]) for n in self.names))


def prune_model(model, args):
    """-> the WeightPruner of --prune_ratio (the model is pruned when this returns), or None without the flag"""
    prune_check(args)
    ratio = getattr(args, 'prune_ratio', None)
    return None if ratio is None else WeightPruner(model, ratio)


class WeightQAT:
    """The `weight_qat` hook of models/_decode.run_decoder: the decoder's [(W, b)] -> [(QATQuantizer(W), b)] in ONE ops.qat_weight
    call over all weights.  'hinerv' noise is on exactly while the model is in training mode, so evaluations decode with every
    weight quantised; `step`, the device counter the noise mask reads, advances in front of every training forward.  Not a
    module: checkpoints hold the latent fp32 weights under the model's own keys.  `last`: the weights of the latest decode."""

    def __init__(self, model, mode, bits, seed=0):
        ops.qat_args('--qat', None, bits, mode, seed)
        self.model, self.mode, self.bits, self.seed = model, mode, bits, seed
        self.step, self.last = None, None

    def __call__(self, weights):
        Ws = [W for W, _ in weights]
        noise = self.mode == 'hinerv' and self.model.training
        if noise:
            if self.step is None:
                self.step = torch.zeros(1, dtype=torch.int32, device=Ws[0].device)
            self.step += 1
        self.last = ops.qat_weight(Ws, self.bits, self.mode, noise, self.seed, self.step)
        return [(Wq, b) for Wq, (_, b) in zip(self.last, weights)]


def build_model(args, cfg, device):
    """The model `train` optimises: HNeRV / NeRV of the config; with --qat its decoder reads quantised weights (WeightQAT)."""
    if args.arch == 'hnerv':
        cfg = dict(cfg, enc_kernels=getattr(args, 'enc_kernels', 'torch'))   # a flag, not a config line: the reference's YAML files stay usable
    model = (HNeRV if args.arch == 'hnerv' else NeRV)(cfg).to(device)
    mode = getattr(args, 'qat', None)
    model.weight_qat = WeightQAT(model, mode, args.qat_bits, getattr(args, 'qat_seed', 0)) if mode is not None else None
    return model


def export_stream(model, args, cfg, embeddings, frames):
    """--export_stream: the QAT-trained model as a .nqv file; embeddings: what the evaluation decoded the frames from"""
    from ..bitstream import write_qat_stream
    s = write_qat_stream(model, args.export_stream, args.arch, cfg, args.qat, args.qat_bits, frames=frames,
                         embeddings=embeddings if args.arch == 'hnerv' else None, coding=args.stream_coding,
                         encoder=args.stream_encoder)
    logging.info('bit stream: {} ({} bytes, {} bpp; nominal {} bytes; {} at {} bits, coding {})'.format(
        args.export_stream, s['file_bytes'], round(s.get('bpp', float('nan')), 5), s['total_bytes_nominal'], s['mode'],
        args.qat_bits, s['coding']))
    return s


def adjust_lr(optimizer, cur_epoch, args, eta_min=0.05):
    """reference utils.py:77-97."""
    if 'hybrid' in args.lr_type:
        up_ratio, up_pow, down_pow, min_lr, final_lr = [float(x) for x in args.lr_type.split('_')[1:]]
        if cur_epoch < up_ratio:
            lr_mult = min_lr + (1. - min_lr) * (cur_epoch / up_ratio) ** up_pow
        else:
            lr_mult = 1 - (1 - final_lr) * ((cur_epoch - up_ratio) / (1. - up_ratio)) ** down_pow
    elif 'cosine' in args.lr_type:
        up_ratio, up_pow, min_lr = [float(x) for x in args.lr_type.split('_')[1:]]
        if cur_epoch < up_ratio:
            lr_mult = min_lr + (1. - min_lr) * (cur_epoch / up_ratio) ** up_pow
        else:
            lr_mult = max(0.5 * (math.cos(math.pi * (cur_epoch - up_ratio) / (1 - up_ratio)) + 1.0), eta_min)
    else:
        raise NotImplementedError
    for g in optimizer.param_groups:
        g['lr'] = args.lr * lr_mult
    return args.lr * lr_mult


# SSIM_LOSSES (imported above): the members of the reference's loss table (utils.py:119-130) made of MSE and single-scale SSIM
# only, name -> (w_mse, w_ssim); one table with the calibration driver's --rec_loss (calibrate_network.py)


def loss_params(args, cfg):
    """cfg['loss'] -> None for 'l2', the keywords of ops.yuv420_loss for 'yuv420' (the weighted plane MSEs of the 8-bit YUV
    4:2:0 codes; --yuv_matrix, --yuv_range, --yuv_weights; evaluations then also report PSNR-Y / U / V), the keywords of
    ops.ssim_loss for 'ssim' / 'Fusion1' / 'Fusion3' / 'Fusion5' (DESIGN.md §20), dict(w_mse, w_ms) of ops.ms_ssim_loss for
    'msssim' (weights (0, 1), or the config's `loss_weights: [W_MSE, W_MS]`), dict(p, w_abs, w_mse) of ops.lp_loss
    for 'lp' (the config's `loss_p: P`, default 1, and `loss_weights: [W_ABS, W_MSE]`, default (1, 0): w_abs * mean |d|^p + w_mse *
    MSE, i.e. the reference's `l1` = (1, [1, 0]), `Fusion7` = (1, [0.3, 0.7]), `Fusion8` = (1, [0.5, 0.5])); anything
    else raises."""
    loss_name = cfg.get('loss', 'l2')
    if loss_name == 'l2':
        return None
    if loss_name == 'lp':
        w = cfg.get('loss_weights', (1.0, 0.0))
        if not isinstance(w, (list, tuple)) or len(w) != 2:
            raise ValueError(f'loss_weights takes [W_ABS, W_MSE], got {w!r}')
        return objective.resolve('lp', dict(p=cfg.get('loss_p', 1.0), w_abs=w[0], w_mse=w[1]), 'loss_p / loss_weights').params
    if loss_name == MSSSIM_LOSS:
        w = cfg.get('loss_weights', MSSSIM_WEIGHTS)
        if not isinstance(w, (list, tuple)) or len(w) != 2:
            raise ValueError(f'loss_weights takes [W_MSE, W_MS], got {w!r}')
        return objective.resolve(MSSSIM_LOSS, dict(w_mse=w[0], w_ms=w[1]), 'loss_weights').params   # finite, >= 0, a positive sum
    if loss_name in SSIM_LOSSES:
        w_mse, w_ssim = SSIM_LOSSES[loss_name]
        return dict(w_mse=w_mse, w_ssim=w_ssim)
    if loss_name != 'yuv420':
        raise NotImplementedError("only the l2 loss of the shipped configs, 'yuv420' (DESIGN.md §19) and 'ssim' / 'Fusion1' / "
                                  "'Fusion3' / 'Fusion5' (DESIGN.md §20) are built")
    args.loss_domain = 'yuv420'
    return yuv_loss_params(args)


def step_loss(img_out, img, yuv=None):
    """the scalar one training step differentiates: per-channel mean of the loss (`yuv`: what loss_params returned, or the Objective
    resolved from it; l2 is F.mse_loss(...).flatten(1).mean(1).mean(), the SSIM losses the reference's per-frame loss, then .mean())"""
    return objective.of_params(yuv).step_loss(img_out, img)


def train_step(model, optimizer, sample, args, obj, pruner=None):
    """one optimiser step on one batch of the loader -> the decoded frames; pruner: --prune_ratio's mask, held through the step"""
    img = sample['img']
    img_out, _, _ = model(img if args.arch == 'hnerv' else sample['norm_idx'])
    loss = step_loss(img_out, img, obj)
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    optimizer.step()
    if pruner is not None:
        pruner.hold(optimizer)
    return img_out


def train(args, cfg):
    prune_check(args)
    if not torch.cuda.is_available():
        raise RuntimeError('neuroquant_amd needs an AMD GPU')
    obj = objective.of_params(loss_params(args, cfg))
    device = 'cuda'
    cache = FrameCache(load_frames(args, cfg, device))
    n = len(cache)
    train_ind, args.val_ind_list = data_split(list(range(n)), [int(x) for x in args.data_split.split('_')], False, 0)
    loader = CacheLoader(cache, train_ind, cfg['batch_size'], seed=args.seed)
    model = build_model(args, cfg, device)
    want_stream = getattr(args, 'export_stream', None)
    if want_stream and model.weight_qat is None:
        raise ValueError('--export_stream writes a --qat model; a calibrated model is written by calibrate_network --export_stream')
    os.makedirs(args.outf, exist_ok=True)
    setup_logger(os.path.join(args.outf, time.strftime('%Y%m%d_%H%M%S') + '.log'))
    if args.weight != 'None':
        model.load_state_dict(torch.load(args.weight, map_location='cpu'), strict=False)
    pruner = prune_model(model, args)
    msssim = obj.params if obj.name == MSSSIM_LOSS else None   # evaluations then log the objective's line
    if args.eval_only:
        res, embeds = evaluate(model, cache, args, cfg, msssim=msssim)
        logging.info(report_line('', args))
        if pruner is not None:
            pruner.log()
        if want_stream:
            export_stream(model, args, cfg, embeds, n)
        return res
    optimizer = torch.optim.Adam(model.parameters(), weight_decay=0.)
    args.lr = cfg['learning_rate']
    start = datetime.now()
    for epoch in range(cfg['epoch']):
        model.train()
        psnrs = []
        for i, sample in enumerate(loader):
            lr = adjust_lr(optimizer, (epoch + float(i) / len(loader)) / cfg['epoch'], args)
            img = sample['img']
            img_out = train_step(model, optimizer, sample, args, obj, pruner)
            psnrs.append(ops.frame_psnr(img_out, img))
            if i % args.print_freq == 0 or i == len(loader) - 1:
                logging.info('[{}], Epoch[{}/{}], Step [{}/{}], lr:{:.2e} pred_PSNR: {}'.format(
                    datetime.now().strftime("%Y/%m/%d %H:%M:%S"), epoch + 1, cfg['epoch'], i + 1, len(loader), lr,
                    RoundTensor(torch.cat(psnrs).mean().cpu(), 2)))
        if (epoch + 1) % cfg.get('eval_freq', 30) == 0 or (cfg['epoch'] - epoch) in [1, 3, 5]:
            res, _ = evaluate(model, cache, args, cfg, msssim=msssim)
            logging.info(f'Eval at epoch {epoch + 1}: pred_seen_psnr: {RoundTensor(res[0], 2)} | pred_seen_ssim: '
                         f'{RoundTensor(args.eval_metrics["pred_seen_ssim"], 4)}')
            if pruner is not None:
                pruner.log()
        torch.save(model.state_dict(), '{}/model_latest.pth'.format(args.outf))
        if (epoch + 1) % cfg['epoch'] == 0:
            torch.save(model.state_dict(), f'{args.outf}/epoch{epoch + 1}.pth')
    logging.info(f"Training complete in: {str(datetime.now() - start)}")
    if want_stream:
        export_stream(model, args, cfg, evaluate(model, cache, args, cfg, msssim=msssim)[1], n)
    return model


def main(argv):
    args = parse_args(argv)
    cfg = get_config(args.config)
    seed_all(args.seed)
    exp_id = f"{args.vid}_e{cfg['epoch']}_b{cfg['batch_size']}_lr{cfg['learning_rate']}_{cfg['loss']}"
    args.outf = os.path.join('results', args.outf, exp_id)
    return train(args, cfg)


if __name__ == '__main__':
    main(sys.argv[1:])
