"""The reconstruction objectives of calibration and training, said once.

TABLE is keyed by objective name; `resolve` validates parameters against it and returns the Objective that the engine
(`model_reconstruction`, `LossFunction`), the calibration driver (`calibrate_network.objective_of`) and the trainer
(`regress.step_loss`) call.  The rate term adds to every objective and is checked by `rate_kwarg`.
"""
import contextlib
import functools

from . import ops
from .utils import RoundTensor

SSIM_METRIC_NAME = 'ssim_single_scale'    # added to args.eval_metrics by an MSE + SSIM objective
YUV_METRIC_NAMES = ['psnr_y', 'psnr_u', 'psnr_v', 'psnr_yuv_611']    # added by the YUV 4:2:0 objective (the player's keys)


def _two_weights(args_fn, side):   # check of a (w_mse, w_x) objective: the ops validator on the smallest legal probe shape
    shape = (1, 1, side, side)
    return lambda what, p: dict(zip(p, args_fn(what, shape, shape, *p.values())))


def _yuv_frame(out, img, p):   # PSNR of the 8-bit Y / U / V planes of the output against the ground truth's, in the player's format
    h, w = img.shape[-2:]
    return ops.yuv420_psnr(ops.frames_to_yuv420(out, p['matrix'], p['full_range']),
                           ops.frames_to_yuv420(img, p['matrix'], p['full_range']), h, w)


def _yuv_report(vals, ms_ssim, p):   # vals (frames, 3) float64: means of decibels, 6:1:1 per frame, as the player reports them
    y, u, v = vals.mean(0)
    m611 = ((6.0 * vals[:, 0] + vals[:, 1] + vals[:, 2]) / 8.0).mean()
    return (dict(zip(YUV_METRIC_NAMES, [y, u, v, m611])),
            'yuv420: PSNR-Y {} U {} V {} | 6:1:1 {}'.format(*(RoundTensor(t, 2) for t in (y, u, v, m611))))


def _ssim_report(vals, ms_ssim, p):
    s1 = vals.mean()
    return {SSIM_METRIC_NAME: s1}, 'ssim objective {}: SSIM {}'.format(p, RoundTensor(s1, 4))


def _msssim_report(vals, ms_ssim, p):   # the figure this objective is after is the MS-SSIM every evaluation logs
    return {}, (None if ms_ssim is None else
                'msssim objective ({}, {}): MS-SSIM {}'.format(p['w_mse'], p['w_ms'], RoundTensor(ms_ssim, 4)))


# name -> defaults: parameter names and defaults, in keyword order; exact: the engine's keyword must give them all (else any subset)
#   check(what, params) -> validated params, ValueError naming `what` before anything is launched
#   excludes: objectives it does not combine with (title: its name in those refusals)
#   head_grad: the ops function behind the decoder's head; rec: the element of its first result that is logged
#   loss: the differentiable ops function; lp_mul(C): its factor on the scale of lp_loss (LossFunction); step_div(C): its divisor
#     for the trainer's per-channel mean (regress.step_loss); None: the loss as it is, nothing more is launched
#   fused_head: the decoder may compute it behind the head convolution (ops.fused_head_loss); log: the calibration's log line
#   frame(out, img, params) -> a per-frame extra evaluation figure; report(those on the CPU, mean MS-SSIM or None, params) ->
#     (metrics to add, log line or None)
TABLE = {
    'l2': dict(defaults={}, exact=False, check=lambda what, p: p, excludes=(), title='squared error',
               head_grad=ops.l2_loss_head_grad, rec=None, loss=ops.l2_loss, lp_mul=None, step_div=lambda C: C,
               fused_head=True, log=None, frame=None, report=None),
    'yuv420': dict(defaults=dict(matrix='bt709', full_range=False, weights=ops.YUV_LOSS_WEIGHTS), exact=False,
                   check=lambda what, p: dict(p, weights=ops.yuv420_loss_args(what, (1, 3, 2, 2), *p.values())[2]), excludes=(), title='YUV 4:2:0', head_grad=ops.yuv420_loss_head_grad, rec=0, loss=ops.yuv420_loss, lp_mul=None,
                   step_div=lambda C: 3, fused_head=False, log='reconstruction loss: YUV 4:2:0 plane MSEs, {}',
                   frame=_yuv_frame, report=_yuv_report),
    'ssim': dict(defaults=dict(w_mse=0.0, w_ssim=1.0), exact=True, check=_two_weights(ops.ssim_loss_args, 11),
                 excludes=('yuv420',), title='SSIM', head_grad=ops.ssim_loss_head_grad, rec=0, loss=ops.ssim_loss,
                 lp_mul=lambda C: C, step_div=None, fused_head=False,
                 log='reconstruction loss: C * (w_mse * MSE + w_ssim * (1 - SSIM)), {}',
                 frame=lambda out, img, p: ops.ssim(out, img), report=_ssim_report),
    'msssim': dict(defaults=dict(w_mse=0.0, w_ms=1.0), exact=True, check=_two_weights(ops.ms_ssim_loss_args, 161),
                   excludes=('ssim', 'yuv420'), title='MS-SSIM', head_grad=ops.msssim_loss_head_grad, rec=0, loss=ops.ms_ssim_loss,
                   lp_mul=lambda C: C, step_div=None, fused_head=False,
                   log='reconstruction loss: C * (w_mse * MSE + w_ms * (1 - MS-SSIM)), {}', frame=None, report=_msssim_report),
}


class Objective:
    """One resolved objective: `name`, validated `params`, and what the loops call."""

    def __init__(self, name, params):
        e = TABLE[name]
        self.name, self.params, self.entry = name, params, e
        self._head_grad = functools.partial(e['head_grad'], **params)
        self._loss = functools.partial(e['loss'], **params)
        self._rec, self._fused_head = e['rec'], e['fused_head']    # (what an iteration reads: no table lookup in the step)

    def head_request(self, target):
        """the context the calibration step enters around the decoder forward: the fused head-loss request, or nothing"""
        if not self._fused_head:
            return contextlib.nullcontext()
        return ops.fused_head_loss(cache_u8=target[0], idx=target[1]) if isinstance(target, tuple) else ops.fused_head_loss(tgt=target)

    def head_grad(self, img_out, target, node=None):
        """-> (rec, dimg): the logged loss and the gradient `img_out.backward(dimg)` (or decoder_backward_steps(node, dimg))
        continues from; target = float frames or (cache_u8, idx) of the uint8 frame cache"""
        cached = isinstance(target, tuple)
        out = self._head_grad(img_out, cache_u8=target[0], idx=target[1], node=node) if cached \
            else self._head_grad(img_out, tgt=target, node=node)
        if out is None:   # l2 only: no hand-over slot, or the fused tanh-head kernel does not apply
            return ops.l2_loss_and_grad(img_out, ops.gather_frames_u8(*target) if cached else target)
        return (out[0] if self._rec is None else out[0][self._rec]), out[1]

    def lp_loss(self, pred, tgt):
        """the differentiable loss on the scale of lp_loss(p=2), as the calibration logs it"""
        loss, mul = self._loss(pred, tgt), self.entry['lp_mul']
        return loss if mul is None else loss * mul(pred.shape[1])

    def step_loss(self, pred, tgt):
        """the differentiable loss as the trainer's per-channel mean"""
        loss, div = self._loss(pred, tgt), self.entry['step_div']
        return loss if div is None else loss / div(tgt.shape[1])

    def engine_kwargs(self):
        """the keywords of model_reconstruction that ask for this objective (from_kwargs reads them back)"""
        kw = dict(loss_domain='yuv420' if self.name == 'yuv420' else 'rgb', yuv=None, ssim=None, msssim=None)
        if self.name != 'l2':
            kw['yuv' if self.name == 'yuv420' else self.name] = dict(self.params)
        return kw

    def log_line(self):
        return None if self.entry['log'] is None else self.entry['log'].format(self.params)

    def eval_frame(self, out, img):
        return None if self.entry['frame'] is None else self.entry['frame'](out, img, self.params)

    def eval_report(self, vals, ms_ssim=None):
        return ({}, None) if self.entry['report'] is None else self.entry['report'](vals, ms_ssim, self.params)


def resolve(name, params=None, what='model_reconstruction'):
    """-> Objective `name` with `params` over its defaults; ValueError for an unknown name, unknown keys or bad values"""
    if name not in TABLE:
        raise ValueError(f'objective must be one of {list(TABLE)}, got {name!r}')
    e = TABLE[name]
    params = dict(params or {})
    if set(params) - set(e['defaults']):
        raise ValueError(f"{name} takes {', '.join(e['defaults']) or 'no parameters'}, got {sorted(params)}")
    return Objective(name, e['check'](what, dict(e['defaults'], **params)))


def from_kwargs(loss_domain='rgb', yuv=None, ssim=None, msssim=None, what='model_reconstruction'):
    """The objective model_reconstruction's keywords ask for; bad keys, bad values and what does not combine stop here."""
    if loss_domain not in ('rgb', 'yuv420'):
        raise ValueError(f"loss_domain must be 'rgb' or 'yuv420', got {loss_domain!r}")
    yuv = dict(yuv or {})
    if set(yuv) - set(TABLE['yuv420']['defaults']):
        raise ValueError(f"yuv takes matrix, full_range and weights, got {sorted(yuv)}")
    asked = {n: p for n, p in (('yuv420', yuv if loss_domain == 'yuv420' else None), ('ssim', ssim), ('msssim', msssim)) if p is not None}
    for n, p in asked.items():
        e = TABLE[n]
        if e['exact'] and (not isinstance(p, dict) or set(p) != set(e['defaults'])):
            raise ValueError(f"{n} takes dict({', '.join(e['defaults'])}), got {sorted(p) if isinstance(p, dict) else p!r}")
        for other in e['excludes']:
            if other in asked:
                raise ValueError(f"the {e['title']} objective is defined on RGB frames: it does not combine with loss_domain 'yuv420'"
                                 if other == 'yuv420' else f"{n} and {other} are two objectives: give one")
    name = next(reversed(asked), 'l2')
    return resolve(name, asked.get(name), what)


def of_params(params, what='loss'):
    """The objective that regress.loss_params' result (None for l2, else the keywords of its ops loss) stands for: the entry with
    exactly those parameter names.  An Objective passes through."""
    if isinstance(params, Objective):
        return params
    if params is None:
        return resolve('l2', None, what)
    for name, e in TABLE.items():
        if e['defaults'] and set(params) == set(e['defaults']):
            return resolve(name, params, what)
    raise ValueError(f'no objective takes the parameters {sorted(params)}')


def rate_kwarg(rate, what='model_reconstruction(rate=)'):
    """model_reconstruction's rate= keyword -> None or dict(weight, pixels), validated (ops.level_rate)"""
    if rate is None:
        return None
    if not isinstance(rate, dict) or set(rate) != {'weight', 'pixels'}:
        raise ValueError(f"rate takes dict(weight, pixels), got {sorted(rate) if isinstance(rate, dict) else rate!r}")
    px = rate['pixels']
    if isinstance(px, bool) or not isinstance(px, int) or px <= 0:
        raise ValueError(f"rate: pixels must be a positive int (frames * H * W), got {px!r}")
    return dict(weight=ops.level_rate_args(what, rate['weight']), pixels=px)
