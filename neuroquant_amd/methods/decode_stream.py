"""Player driver: decode every frame of a bit stream (`.nqv`, packed or entropy-coded levels; neuroquant_amd/bitstream.py) on the GPU.

    python -m neuroquant_amd.methods.decode_stream --stream model.nqv [--out DIR] [--frames DIR | --synthetic N]
        [--batch_size B] [--arithmetic exact|levels|half]

The file is all it needs: no checkpoint, no QuantModel, no configuration.  --out writes frame%05d.png through the 8-bit
interleaved path (ops.frames_to_u8).  --frames (sorted PNGs, centre-cropped as the calibration driver crops them) or
--synthetic N (the calibration driver's synthetic frames; same --seed) reports PSNR and MS-SSIM (ops.frame_psnr /
ops.ms_ssim) of the float output and of the 8-bit frames.  FPS covers decode only (ground truth and metrics excluded).
With --batch_size 1 (the default, and what calibrate_network's evaluation uses) the float PSNR is the one that driver logged
for 'Weight quantization w/ opt'.  --arithmetic levels runs the big 3 x 3 / 5 x 5 layers on the stored integer levels with two
MFMAs per product (not bit-identical to the live model, within its float64 bounds) and names the layers that
took that path.  --arithmetic half runs the same layers on half-precision activations with one MFMA per product (DESIGN.md
§15: an approximation, about ten times outside those bounds), names them likewise, and exits non-zero if an activation left the
range of IEEE half.
"""
import argparse
import os
import sys
import time
from types import SimpleNamespace

import torch

from .. import ops
from ..bitstream import StreamDecoder
from ..utils import RoundTensor


def parse_args(argv):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0], formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--stream', type=str, required=True)
    p.add_argument('--out', type=str, default=None, help='write the decoded frames as PNGs into this directory')
    p.add_argument('--frames', type=str, default=None, help='directory of ground-truth PNGs: report PSNR / MS-SSIM')
    p.add_argument('--synthetic', type=int, default=0, help='ground truth = N synthetic frames (calibrate_network --synthetic)')
    p.add_argument('--seed', default=903, type=int)
    p.add_argument('--batch_size', default=1, type=int)
    p.add_argument('--arithmetic', default='exact', choices=StreamDecoder.ARITHMETICS,
                   help="'levels': integer-level convolutions where the unsplit tiled bf16x3 kernel has the layer; "
                        "'half': those layers on half-precision activations (an approximation)")
    return p.parse_args(argv)


@torch.no_grad()
def run(args):
    if not torch.cuda.is_available():
        raise RuntimeError('neuroquant_amd needs an AMD GPU (no CPU path)')
    t0 = time.time()
    dec = StreamDecoder(args.stream, arithmetic=args.arithmetic)
    open_s = time.time() - t0
    n, B = dec.frames, max(1, args.batch_size)
    gt = None
    if args.frames or args.synthetic:
        from .calibrate_network import load_frames
        gt = load_frames(SimpleNamespace(synthetic=args.synthetic, seed=args.seed, data_path=args.frames), dec.cfg, 'cuda')
        if gt.shape[0] != n:
            raise ValueError(f'{gt.shape[0]} ground-truth frames, the stream holds {n}')
    if args.out:
        from PIL import Image
        os.makedirs(args.out, exist_ok=True)
    with_ssim = min(dec.cfg['crop_h'], dec.cfg['crop_w']) > 160
    acc = {k: [] for k in ('psnr', 'ssim', 'psnr_u8', 'ssim_u8')}
    dec.decode(list(range(min(B, n))))          # warm-up: builds the operands, loads the kernels
    torch.cuda.synchronize()
    dec_time = 0.0
    for j in range(0, n, B):
        idx = list(range(j, min(j + B, n)))
        t0 = time.time()
        img = dec.decode(idx)
        torch.cuda.synchronize()
        dec_time += time.time() - t0
        u8 = ops.frames_to_u8(img, 'hwc') if (args.out or gt is not None) else None
        if args.out:
            for i, a in zip(idx, u8.cpu().numpy()):
                Image.fromarray(a).save(os.path.join(args.out, 'frame%05d.png' % i))
        if gt is not None:
            ref = ops.gather_frames_u8(gt, torch.tensor(idx, device=gt.device))
            img8 = u8.permute(0, 3, 1, 2).float() / 255.0
            acc['psnr'].append(ops.frame_psnr(img, ref))
            acc['psnr_u8'].append(ops.frame_psnr(img8, ref))
            if with_ssim:
                acc['ssim'].append(ops.ms_ssim(img, ref))
                acc['ssim_u8'].append(ops.ms_ssim(img8, ref))
    res = dict(frames=n, batch_size=B, open_seconds=open_s, fps=n / dec_time, file_bytes=os.path.getsize(args.stream),
               level_bytes=dec.level_bytes, level_tensors=dec.level_tensors, arithmetic=dec.arithmetic,
               saturated=dec.saturated(),     # once, after the last frame
               levels_used={b: list(v) for b, v in dec.levels_used.items()})
    for k, v in acc.items():
        if v:
            res[k] = torch.cat(v).cpu().mean()
    return res


def main(argv):
    args = parse_args(argv)
    res = run(args)
    print('stream {}: {} bytes, {} frames, opened in {:.3f} s, decode FPS {} (batch {})'.format(
        args.stream, res['file_bytes'], res['frames'], res['open_seconds'], round(res['fps'], 1), res['batch_size']))
    print('levels: rans {} bytes in {} tensors, packed {} bytes in {} tensors'.format(
        res['level_bytes']['rans'], res['level_tensors']['rans'], res['level_bytes']['packed'], res['level_tensors']['packed']))
    if res['arithmetic'] in ('levels', 'half'):
        print('arithmetic {}: '.format(res['arithmetic']) + '; '.join('batch {}: layers {}'.format(b, v if v else 'none')
                                                           for b, v in sorted(res['levels_used'].items())))
    if 'psnr' in res:
        fmt = lambda k, d: RoundTensor(res[k], d) if k in res else 'n/a'
        print('float: PSNR {} | MS-SSIM {}'.format(fmt('psnr', 2), fmt('ssim', 4)))
        print('8-bit: PSNR {} | MS-SSIM {}'.format(fmt('psnr_u8', 2), fmt('ssim_u8', 4)))
    if args.out:
        print('wrote {} PNGs to {}'.format(res['frames'], args.out))
    if res['saturated']:
        print('arithmetic half: an activation left the range of IEEE half (|x| > 65504) and was clamped: '
              'the frames are NOT the stream\'s; decode it with --arithmetic levels or exact')
    return res


if __name__ == '__main__':
    sys.exit(1 if main(sys.argv[1:])['saturated'] else 0)
