"""Player driver: decode every frame of a bit stream (`.nqv`, packed or entropy-coded levels; neuroquant_amd/bitstream.py) on the GPU.

    python -m neuroquant_amd.methods.decode_stream --stream model.nqv [--out DIR | --out clip.y4m | --out clip.yuv]
        [--frames DIR | --frames clip.y4m | --frames clip_WxH.yuv | --synthetic N] [--batch_size B]
        [--arithmetic exact|levels|half] [--fps NUM[:DEN]] [--matrix bt709|bt601] [--range limited|full] [--yuv_size WxH]

The file is all it needs: no checkpoint, no QuantModel, no configuration.  --out X.y4m / X.yuv writes ONE video file of 8-bit
YUV 4:2:0 frames (ops.frames_to_yuv420 of the float frames: --matrix, --range; --fps goes into the y4m header); any other
--out is a directory that receives frame%05d.png through the 8-bit interleaved path (ops.frames_to_u8).  --frames (sorted
PNGs, or a .y4m / .yuv clip converted by ops.yuv420_to_rgb_u8 with the same --matrix and, unless the clip states its own,
--range; centre-cropped as the calibration driver crops them) or --synthetic N (the calibration driver's synthetic frames;
same --seed) reports PSNR and MS-SSIM (ops.frame_psnr / ops.ms_ssim) of the float output and of the 8-bit frames.  Against a
YUV clip it also reports the PSNR of the Y, U and V planes between the decoded 4:2:0 frames and the clip's own bytes, and
their 6:1:1 mean.  FPS covers decode only (ground truth, conversion, metrics and file output excluded).
With --batch_size 1 (the default, and what calibrate_network's evaluation uses) the float PSNR is the one that driver logged
for 'Weight quantization w/ opt'.  --arithmetic levels runs the big 3 x 3 / 5 x 5 layers on the stored integer levels with two
MFMAs per product (not bit-identical to the live model, within its float64 bounds) and names the layers that
took that path.  --arithmetic half runs the same layers on half-precision activations with one MFMA per product (DESIGN.md
§15: an approximation, about ten times outside those bounds), names them likewise, and exits non-zero if an activation left the
range of IEEE half.  A file whose embeddings are stored as levels plays like any other; their bits, coding and
bytes are printed and returned as `embedding_info`.
"""
import argparse
import contextlib
import os
import sys
import time
from types import SimpleNamespace

import torch

from .. import ops, videoio
from ..bitstream import StreamDecoder
from ..utils import RoundTensor


def parse_args(argv):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0], formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--stream', type=str, required=True)
    p.add_argument('--out', type=str, default=None,
                   help='X.y4m / X.yuv: write the decoded frames as one 8-bit YUV 4:2:0 video file; anything else: PNGs into this directory')
    p.add_argument('--frames', type=str, default=None,
                   help='ground truth, a directory of PNGs or a .y4m / .yuv clip: report PSNR / MS-SSIM')
    p.add_argument('--fps', type=str, default='30', help='NUM[:DEN], the frame rate written into a .y4m header')
    p.add_argument('--matrix', type=str, default='bt709', choices=['bt709', 'bt601'], help='colour matrix of YUV input and output')
    p.add_argument('--range', type=str, default=None, choices=['limited', 'full'],
                   help="range of the YUV codes (default: limited; for --frames, the clip's own XCOLORRANGE if it has one)")
    p.add_argument('--yuv_size', type=str, default=None, help='WxH of a raw .yuv --frames clip whose name does not carry _<W>x<H>')
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
    h, w = dec.cfg['crop_h'], dec.cfg['crop_w']
    matrix = getattr(args, 'matrix', None) or 'bt709'
    rng = getattr(args, 'range', None)
    gt = clip = None
    if args.frames or args.synthetic:
        from .calibrate_network import load_frames, open_yuv_clip
        src = SimpleNamespace(synthetic=args.synthetic, seed=args.seed, data_path=args.frames, yuv_matrix=matrix, yuv_range=rng,
                              yuv_size=getattr(args, 'yuv_size', None))
        if not args.synthetic and videoio.is_video_file(args.frames):
            # the clip's own bytes are the 4:2:0 ground truth: its planes must crop where the RGB frames crop
            clip, _, _, clip_full = open_yuv_clip(src, args.frames)
            top, left = videoio.centre_crop_offsets(clip.H, clip.W, h, w)
            if top % 2 or left % 2:
                raise ValueError(f'the centre crop of {w}x{h} from a {clip.W}x{clip.H} 4:2:0 clip starts at top={top}, '
                                 f'left={left}: both offsets must be even (chroma is cropped at half of them)')
        gt = load_frames(src, dec.cfg, 'cuda')
        if gt.shape[0] != n:
            raise ValueError(f'{gt.shape[0]} ground-truth frames, the stream holds {n}')
    video = None
    if videoio.is_video_file(args.out):
        video = videoio.open_writer(args.out, h, w, fps=videoio.parse_fps(getattr(args, 'fps', None) or '30'),
                                    full_range=rng == 'full')
    elif args.out:
        from PIL import Image
        os.makedirs(args.out, exist_ok=True)
    with_ssim = min(h, w) > 160
    acc = {k: [] for k in ('psnr', 'ssim', 'psnr_u8', 'ssim_u8', 'psnr_yuv')}
    with video if video is not None else contextlib.nullcontext():   # the file closes whatever happens
        dec.decode(list(range(min(B, n))))          # warm-up: builds the operands, loads the kernels
        torch.cuda.synchronize()
        dec_time = 0.0
        for j in range(0, n, B):
            idx = list(range(j, min(j + B, n)))
            t0 = time.time()
            img = dec.decode(idx)
            torch.cuda.synchronize()
            dec_time += time.time() - t0
            u8 = ops.frames_to_u8(img, 'hwc') if ((args.out and video is None) or gt is not None) else None
            if video is not None:      # the bytes decode(idx, out='yuv420', ...) returns: one rounding from the float frame
                video.write(ops.frames_to_yuv420(img, matrix, video.full_range).cpu().numpy())
            elif args.out:
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
            if clip is not None:
                own = videoio.crop_yuv420(clip.read(j, len(idx)), clip.H, clip.W, top, left, h, w)
                acc['psnr_yuv'].append(ops.yuv420_psnr(ops.frames_to_yuv420(img, matrix, clip_full),
                                                       torch.from_numpy(own).to(img.device), h, w))
    res = dict(frames=n, batch_size=B, open_seconds=open_s, fps=n / dec_time, file_bytes=os.path.getsize(args.stream),
               level_bytes=dec.level_bytes, level_tensors=dec.level_tensors, arithmetic=dec.arithmetic,
               embedding_info=dec.embedding_info,
               saturated=dec.saturated(),     # once, after the last frame
               levels_used={b: list(v) for b, v in dec.levels_used.items()})
    yuv = acc.pop('psnr_yuv')
    for k, v in acc.items():
        if v:
            res[k] = torch.cat(v).cpu().mean()
    if yuv:
        p = torch.cat(yuv).cpu()                  # (frames, 3) float64
        res['psnr_y'], res['psnr_u'], res['psnr_v'] = p.mean(0)
        res['psnr_yuv_611'] = ((6.0 * p[:, 0] + p[:, 1] + p[:, 2]) / 8.0).mean()
    return res


def main(argv):
    args = parse_args(argv)
    res = run(args)
    print('stream {}: {} bytes, {} frames, opened in {:.3f} s, decode FPS {} (batch {})'.format(
        args.stream, res['file_bytes'], res['frames'], res['open_seconds'], round(res['fps'], 1), res['batch_size']))
    print('levels: rans {} bytes in {} tensors, packed {} bytes in {} tensors'.format(
        res['level_bytes']['rans'], res['level_tensors']['rans'], res['level_bytes']['packed'], res['level_tensors']['packed']))
    if res['embedding_info']:
        e = res['embedding_info']
        print('embeddings: {} bits, {}{}, {} bytes'.format(e['bits'], e['coding'], ', frame-to-frame differences' if e['temporal'] else '',
                                                           e['bytes']))
    if res['arithmetic'] in ('levels', 'half'):
        print('arithmetic {}: '.format(res['arithmetic']) + '; '.join('batch {}: layers {}'.format(b, v if v else 'none')
                                                           for b, v in sorted(res['levels_used'].items())))
    if 'psnr' in res:
        fmt = lambda k, d: RoundTensor(res[k], d) if k in res else 'n/a'
        print('float: PSNR {} | MS-SSIM {}'.format(fmt('psnr', 2), fmt('ssim', 4)))
        print('8-bit: PSNR {} | MS-SSIM {}'.format(fmt('psnr_u8', 2), fmt('ssim_u8', 4)))
    if 'psnr_y' in res:
        print('yuv420: PSNR-Y {} U {} V {} | 6:1:1 {}'.format(*(RoundTensor(res[k], 2)
                                                                for k in ('psnr_y', 'psnr_u', 'psnr_v', 'psnr_yuv_611'))))
    if videoio.is_video_file(args.out):
        print('wrote {} frames to {}'.format(res['frames'], args.out))
    elif args.out:
        print('wrote {} PNGs to {}'.format(res['frames'], args.out))
    if res['saturated']:
        print('arithmetic half: an activation left the range of IEEE half (|x| > 65504) and was clamped: '
              'the frames are NOT the stream\'s; decode it with --arithmetic levels or exact')
    return res


if __name__ == '__main__':
    sys.exit(1 if main(sys.argv[1:])['saturated'] else 0)
