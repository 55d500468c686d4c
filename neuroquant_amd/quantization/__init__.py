from .quant_block import BaseQuantBlock, QuantNeRVBlock
from .quant_layer import QuantModule
from .quant_model import QuantModel
from .quantizer import AdaRoundQuantizer, QATQuantizer, UniformAffineQuantizer, lp_loss
from .data_utils import LinearTempDecay, save_grad_data, save_inp_oup_data
from .calib_block import block_reconstruction
from .calib_layer import layer_reconstruction
from .calib_model import LossFunction, model_reconstruction
