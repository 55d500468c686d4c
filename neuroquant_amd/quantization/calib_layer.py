"""Layer-wise calibration (reference quantization/calib_layer.py: AdaRound at every convolution output)."""
import torch

from .calib_unit import reconstruct_unit
from .quant_layer import QuantModule
from .quant_model import QuantModel


def layer_reconstruction(model: QuantModel, layer: QuantModule, cali_data: torch.Tensor,
                         batch_size: int = 8, iters: int = 20000, weight: float = 0.01,
                         opt_mode: str = 'mse', asym: bool = False, b_range: tuple = (20, 2),
                         warmup: float = 0.0, input_prob: float = 1.0, p: float = 2.0, lr: float = 0.0015):
    """Learn the AdaRound variables of one QuantModule against its cached FP convolution output, in place; the reference's
    signature (calib_layer.py:89-93).  The reference's body raises NameError at its line 130, `opt_params` being undefined where
    the alphas are collected: it is taken as the empty list it evidently meant, which makes this block_reconstruction's loop on
    a unit without PixelShuffle or activation.  quantization/calib_unit.py runs it."""
    reconstruct_unit(model, layer, cali_data, batch_size, iters, weight, opt_mode, asym, b_range, warmup, input_prob, p, lr)
