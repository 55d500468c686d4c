"""Block-wise calibration (reference quantization/calib_block.py: BRECQ reconstruction with QDrop's input mix)."""
import torch

from .calib_unit import reconstruct_unit
from .quant_block import BaseQuantBlock
from .quant_model import QuantModel


def block_reconstruction(model: QuantModel, block: BaseQuantBlock, cali_data: torch.Tensor,
                         batch_size: int = 8, iters: int = 20000, weight: float = 0.01,
                         opt_mode: str = 'mse', asym: bool = False, b_range: tuple = (20, 2),
                         warmup: float = 0.0, input_prob: float = 1.0, p: float = 2.0, lr: float = 0.0015):
    """Learn the AdaRound variables of one block (or of a bare layer: decoder[0], the head) against the block's cached FP
    output, in place; the reference's signature and schedule (calib_block.py:91-183).  asym: the cached input comes from the
    quantised model; input_prob < 1: QDrop, each element of the input taken from the quantised input with that probability,
    else from the FP one; opt_mode 'mse' (lp_loss(p)), 'fisher_diag', 'fisher_full'.  quantization/calib_unit.py runs it."""
    reconstruct_unit(model, block, cali_data, batch_size, iters, weight, opt_mode, asym, b_range, warmup, input_prob, p, lr)
