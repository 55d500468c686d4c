"""Unit-wise reconstruction: the one implementation under block_reconstruction (BRECQ / QDrop) and layer_reconstruction (AdaRound),
reference quantization/calib_block.py and calib_layer.py.  An iteration has no autograd tape and needs no data gradient:

    idx = randperm(N)[:batch_size]                       as the reference draws it
    x = QDrop mix / gather of the cached inputs          nq_qdrop_mix
    soft AdaRound weight and bias of THIS unit           nq_adaround_forward
    convolution (+ PixelShuffle + GELU, saving gelu')    nq_conv_forward
    loss and the gradient at the convolution output      nq_unit_rec_loss   
    weight / bias gradient                               nq_conv_wgrad
    d(alpha) + regulariser gradient, Adam                nq_adaround_backward, nq_adam_step

The convolutions run on the fp32 kernels.  Hadamard-domain weights are out of scope here."""
import logging
import time

import torch

from .. import ops
from .data_utils import LinearTempDecay, save_grad_data, save_inp_oup_data, unit_parts
from .quantizer import AdaRoundQuantizer

OPT_MODES = ('mse', 'fisher_diag', 'fisher_full')


class UnitStep:
    """The explicit iteration of one unit on cached data.  gradients(idx) -> (rec loss (1,), d(alpha_w), d(alpha_b)) with the
    regulariser's gradient of weight `reg_weight` at temperature `reg_b` added to d(alpha_w) (0: off)."""

    def __init__(self, unit, inps, sym, outs, grads, opt_mode, p, input_prob, seed=0):
        self.conv, self.r, self.act = unit_parts(unit)
        if self.conv.hadamard:
            raise ValueError('unit-wise calibration of Hadamard-domain weights is not built (use --granularity network)')
        self.wq, self.bq = self.conv.weight_quantizer, self.conv.bias_quantizer
        self.w, self.b = self.conv.weight.data, self.conv.bias.data
        self.inps, self.sym, self.outs, self.grads = inps, sym, outs, grads
        self.mode, self.p = ops.UNIT_REC_MODES[opt_mode], float(p)
        self.prob, self.seed = float(input_prob), seed
        self.step = torch.zeros(1, dtype=torch.int32, device=inps.device)   # the generator's step word, read on the device

    def gradients(self, idx, reg_weight=0.0, reg_b=0.0):
        wq, bq = self.wq, self.bq
        cout, _, k, _ = self.w.shape
        x = ops.qdrop_mix(self.inps, self.sym if self.prob < 1.0 else None, idx, self.prob, self.seed, self.step)
        self.step += 1
        W = ops.adaround_forward(self.w, wq.alpha.data, wq.delta.data, wq.zero_point, wq.n_levels, True)
        b = ops.adaround_forward(self.b, bq.alpha.data, bq.delta.data, bq.zero_point, bq.n_levels, True)
        wt, dims, _, _ = ops.weight_layouts(W, False)
        y, z = ops.conv_forward_raw(x, wt, dims, b, cout, k, ops.EPI_PS_GELU if self.act else ops.EPI_PLAIN, self.r)
        loss, dconv = ops.unit_rec_loss_raw(y, self.outs, self.mode, self.p, self.grads, z if self.act else None, self.r, idx)
        dW, db = ops.conv_wgrad_raw(x, dconv, cout, k, True)
        da_w = ops.adaround_backward(self.w, dW, wq.alpha.data, wq.delta.data, wq.zero_point, wq.n_levels, reg_weight, reg_b)
        da_b = ops.adaround_backward(self.b, db, bq.alpha.data, bq.delta.data, bq.zero_point, bq.n_levels)
        return loss, da_w, da_b


def prepare_unit(model, unit):
    """The reference's set-up: model FP, unit quantised, the unit's two quantisers replaced by AdaRoundQuantizers with soft targets"""
    conv = unit_parts(unit)[0]
    model.set_quant_state(False)
    unit.set_quant_state(True)
    for name, tensor in (('weight_quantizer', conv.org_weight.data), ('bias_quantizer', conv.bias.data)):
        q = getattr(conv, name)
        if not isinstance(q, AdaRoundQuantizer):
            if not q.inited:
                q(tensor)   # the lazy scale init of UniformAffineQuantizer
            q = AdaRoundQuantizer(uaq=q, round_mode='learned_hard_sigmoid', weight_tensor=tensor)
            setattr(conv, name, q)
        q.soft_targets = True
    return conv


def reconstruct_unit(model, unit, cali_data, batch_size, iters, weight, opt_mode, asym, b_range, warmup, input_prob, p, lr):
    if opt_mode not in OPT_MODES:
        raise ValueError('Not supported reconstruction loss function: {}'.format(opt_mode))
    ops.lp_loss_args('unit reconstruction', (1, 1, 1, 1), (1, 1, 1, 1), p, 1.0, 0.0)
    conv = prepare_unit(model, unit)
    wq, bq = conv.weight_quantizer, conv.bias_quantizer
    t0 = time.time()
    (inps, sym), outs = save_inp_oup_data(model, unit, cali_data, asym, batch_size=10, input_prob=True, keep_gpu=True)
    logging.info('Cached init time: {}'.format(time.time() - t0))
    grads = save_grad_data(model, unit, cali_data, batch_size=1) if opt_mode != 'mse' else None
    step = UnitStep(unit, inps, sym, outs, grads, opt_mode, p, input_prob)
    decay = LinearTempDecay(iters, rel_start_decay=warmup, start_b=b_range[0], end_b=b_range[1])   # decay_start = 0
    loss_start = iters * warmup
    moments = [torch.zeros_like(q.alpha.data) for q in (wq, wq, bq, bq)]
    for count in range(1, iters + 1):
        idx = torch.randperm(inps.size(0))[:batch_size].to(inps.device)
        b = decay(count)
        on = count >= loss_start
        rec, da_w, da_b = step.gradients(idx, weight if on else 0.0, b if on else 0.0)
        ops.adam_step(wq.alpha.data, da_w, moments[0], moments[1], lr, count)
        ops.adam_step(bq.alpha.data, da_b, moments[2], moments[3], lr, count)
        if count % 500 == 0:
            rnd = float(ops.round_loss(wq.alpha.data, b, weight)) if on else 0.0
            logging.info('Total loss:\t{:.4f} (rec:{:.4f}, round:{:.4f})\tb={:.2f}\tcount={}'.format(
                float(rec) + rnd, float(rec), rnd, b if on else 0, count))
    wq.soft_targets = bq.soft_targets = False
