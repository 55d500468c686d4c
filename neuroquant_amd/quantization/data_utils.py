"""Temperature schedule of the rounding regulariser (reference quantization/data_utils.py:24-41) and the caches of the
unit-wise (layer / block) reconstruction (reference data_utils.py:45-272)."""
import torch
import torch.nn.functional as F

from ..models._layers import OutImg


class LinearTempDecay:
    def __init__(self, t_max: int, rel_start_decay: float = 0.2, start_b: int = 10, end_b: int = 2):
        self.t_max = t_max
        self.start_decay = rel_start_decay * t_max
        self.start_b = start_b
        self.end_b = end_b

    def __call__(self, t):
        if t < self.start_decay:
            return self.start_b
        rel_t = (t - self.start_decay) / (self.t_max - self.start_decay)
        return self.end_b + (self.start_b - self.end_b) * max(0.0, 1 - rel_t)


def unit_parts(unit):
    """-> (the unit's QuantModule, PixelShuffle factor r, has GELU): a QuantNeRVBlock is reconstructed behind PixelShuffle + GELU,
    a QuantModule (decoder[0], the head, or the convolution inside a block) at its convolution output"""
    from .quant_block import QuantNeRVBlock
    from .quant_layer import QuantModule
    if isinstance(unit, QuantNeRVBlock):
        if not unit._fusable:
            raise ValueError('unit-wise calibration takes blocks of convolution + PixelShuffle + exact GELU')
        return unit.conv, unit._r, True
    if isinstance(unit, QuantModule):
        return unit, 1, False
    raise ValueError(f'a calibration unit is a QuantModule or a QuantNeRVBlock, got {type(unit).__name__}')


def _stages(model, unit):
    """-> (decoder stages in order, index of the stage that is or holds `unit`, unit is the convolution INSIDE that stage)"""
    stages = list(model.model.decoder) + [model.model.head_layer]
    for i, st in enumerate(stages):
        if st is unit or getattr(st, 'conv', None) is unit:
            return stages, i, st is not unit
    raise ValueError("the unit is not a stage of the model's decoder")


def _reshape(model, h):
    """the channel -> space reshape behind decoder[0] (models/_decode.run_decoder)"""
    net = model.model
    if net.fc_h == 1 and net.fc_w == 1:
        return h
    n, _, hh, ww = h.shape
    return h.view(n, -1, net.fc_h, net.fc_w, hh, ww).permute(0, 1, 4, 2, 5, 3).reshape(n, -1, net.fc_h * hh, net.fc_w * ww)


def _run(model, stages, lo, hi, h):
    """stages [lo, hi) on h, one launch per layer"""
    for i in range(lo, hi):
        h = stages[i](h)
        if i == 0:
            h = _reshape(model, h)
    return h


def _unit_output(stage, inner, h):
    return stage.conv(h) if inner else stage(h)


def _cache(batches, what):
    """the batches as one device tensor; RuntimeError with the byte count where the device cannot hold it (there is no CPU spill)"""
    need = sum(b.numel() for b in batches) * 4
    free = torch.cuda.mem_get_info(batches[0].device)[0]
    if need > free:
        raise RuntimeError(f'{what}: the cache needs {need} bytes on the device, {free} are free (caches are not spilled to the host)')
    return torch.cat(batches)


def _batches(what, cali_data, batch_size, keep_gpu):
    if not keep_gpu:
        raise ValueError(f'{what}: the caches live on the device (keep_gpu=False, the host spill, is not built)')
    bs = min(batch_size, cali_data.size(0))
    return [cali_data[i * bs:(i + 1) * bs] for i in range(cali_data.size(0) // bs)]   # whole batches only, as the reference


def save_inp_oup_data(model, layer, cali_data: torch.Tensor, asym: bool = False, batch_size: int = 8, keep_gpu: bool = True,
                      input_prob: bool = False):
    """Input and FP output of a unit over the calibration set (reference data_utils.py:45-88): ((inps, sym), outs) with
    input_prob, else ((inps,), outs).  inps: the unit's input with the whole model quantised (asym) or FP; sym: its FP input;
    outs: the unit's FP output.  The decoder runs layer by layer up to the unit -- no hooks, no exception to stop it -- and the
    caches stay on the device.  Leaves the model FP and the unit quantised, as the reference."""
    stages, at, inner = _stages(model, layer)
    inps, syms, outs = [], [], []
    with torch.no_grad():
        for x in _batches('save_inp_oup_data', cali_data, batch_size, keep_gpu):
            model.set_quant_state(False)
            fp_in = _run(model, stages, 0, at, x)
            outs.append(_unit_output(stages[at], inner, fp_in))
            syms.append(fp_in)
            if asym:
                model.set_quant_state(True)
                inps.append(_run(model, stages, 0, at, x))
            else:
                inps.append(fp_in)
    model.set_quant_state(False)
    layer.set_quant_state(True)
    inps, outs = _cache(inps, 'save_inp_oup_data'), _cache(outs, 'save_inp_oup_data')
    return ((inps, _cache(syms, 'save_inp_oup_data')) if input_prob else (inps,)), outs


def save_grad_data(model, layer, cali_data: torch.Tensor, batch_size: int = 8, keep_gpu: bool = True):
    """|g| + 1 over the calibration set (reference data_utils.py:91-119, 222-272): g is the gradient, at the unit's output, of
    F.mse_loss(out_fp, out_q, reduction='none').flatten(1).mean(1) of every sample, out_q the frames of the model quantised up
    to and including the unit (quantize_model_till).  The layers behind the unit run under autograd on the HIP convolutions,
    whose backward is the data-gradient kernels.  Leaves the model FP and the unit quantised."""
    stages, at, inner = _stages(model, layer)
    last = len(stages) - 1
    grads = []
    for x in _batches('save_grad_data', cali_data, batch_size, keep_gpu):
        with torch.no_grad():
            model.set_quant_state(False)
            out_fp = OutImg(_run(model, stages, 0, last + 1, x), model.model.out_bias)
            for st in stages[:at + 1]:
                st.set_quant_state(True)
            u = _unit_output(stages[at], inner, _run(model, stages, 0, at, x))
        u.requires_grad_(True)
        with torch.enable_grad():
            h = stages[at].act(stages[at].pixelshuffle(u)) if inner else (_reshape(model, u) if at == 0 else u)
            out_q = OutImg(_run(model, stages, at + 1, last + 1, h), model.model.out_bias)
            loss = F.mse_loss(out_fp, out_q, reduction='none').flatten(1).mean(1).sum()
        grads.append(torch.autograd.grad(loss, u)[0].abs() + 1.0)
    model.set_quant_state(False)
    layer.set_quant_state(True)
    return _cache(grads, 'save_grad_data')
