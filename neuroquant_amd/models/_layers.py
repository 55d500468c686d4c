"""Building blocks of the NeRV / HNeRV video INRs (reference models/_layers.py), parameter names kept so the
reference's checkpoints load unchanged (e.g. `decoder.3.conv.0.weight`, `encoder.stages.1.0.pwconv1.weight`).

The decoder block is the hot path: once wrapped by QuantModel it runs on the fused HIP conv+PixelShuffle+GELU
kernel.  The ConvNeXt encoder is a one-time precompute for calibration and plain PyTorch by default;
the trainer can put its Blocks on the HIP kernels of csrc/convnext.hip (`kernels='hip'`) and, with
`kernels='hip_all'`, its downsampling stages on those of csrc/patchify.hip as well.
"""
from math import ceil, pi

import torch
import torch.nn as nn
import torch.nn.functional as F


def OutImg(x, out_bias='tanh'):
    if out_bias == 'sigmoid':
        return torch.sigmoid(x)
    if out_bias == 'tanh':
        return torch.tanh(x) * 0.5 + 0.5
    return x + float(out_bias)


class Sin(nn.Module):
    def forward(self, input):
        return torch.sin(input)


_ACTS = {
    'relu': lambda: nn.ReLU(True),
    'leaky': lambda: nn.LeakyReLU(inplace=True),
    'leaky01': lambda: nn.LeakyReLU(negative_slope=0.1, inplace=True),
    'relu6': lambda: nn.ReLU6(inplace=True),
    'gelu': lambda: nn.GELU(),
    'sin': lambda: Sin(),
    'swish': lambda: nn.SiLU(inplace=True),
    'softplus': lambda: nn.Softplus(),
    'hardswish': lambda: nn.Hardswish(inplace=True),
}


def ActivationLayer(act_type):
    if act_type not in _ACTS:
        raise KeyError(f"Unknown activation function {act_type}.")
    return _ACTS[act_type]()


def NormLayer(norm_type, ch_width):
    if norm_type == 'none':
        return nn.Identity()
    if norm_type == 'batch':
        return nn.BatchNorm2d(num_features=ch_width, track_running_stats=False)
    if norm_type == 'instance':
        return nn.InstanceNorm2d(num_features=ch_width)
    raise NotImplementedError


class NeRVBlock(nn.Module):
    """conv (stride 1, 'same') -> PixelShuffle(stride) -> norm -> act   (reference _layers.py:20-36)."""

    def __init__(self, in_channel, out_channel, kernel_size, stride, bias, norm, act):
        super().__init__()
        self.conv = nn.Sequential(
            nn.Conv2d(in_channel, out_channel * stride * stride, kernel_size, stride=1,
                      padding=ceil((kernel_size - 1) // 2), bias=bias),
            nn.PixelShuffle(stride) if stride != 1 else nn.Identity(),
        )
        self.norm = NormLayer(norm, out_channel)
        self.act = ActivationLayer(act)

    def forward(self, x):
        return self.act(self.norm(self.conv(x)))


class PositionEncoding(nn.Module):
    """NeRV frame-index embedding: [sin(b^i * pi * t), cos(b^i * pi * t)] (reference _layers.py:77-86)."""

    def __init__(self, base, level):
        super().__init__()
        self.pe_bases = base ** torch.arange(int(level)) * pi

    def forward(self, pos):
        value_list = pos * self.pe_bases.to(pos.device)
        pe_embed = torch.cat([torch.sin(value_list), torch.cos(value_list)], dim=-1)
        return pe_embed.view(pos.size(0), -1, 1, 1)


class LayerNorm(nn.Module):
    def __init__(self, normalized_shape, eps=1e-6, data_format="channels_last"):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(normalized_shape))
        self.bias = nn.Parameter(torch.zeros(normalized_shape))
        self.eps = eps
        if data_format not in ("channels_last", "channels_first"):
            raise NotImplementedError
        self.data_format = data_format
        self.normalized_shape = (normalized_shape,)

    def forward(self, x):
        if self.data_format == "channels_last":
            return F.layer_norm(x, self.normalized_shape, self.weight, self.bias, self.eps)
        u = x.mean(1, keepdim=True)
        s = (x - u).pow(2).mean(1, keepdim=True)
        x = (x - u) / torch.sqrt(s + self.eps)
        return self.weight[:, None, None] * x + self.bias[:, None, None]


BLOCK_KERNELS = ('torch', 'hip')


class Block(nn.Module):
    """ConvNeXt block: 7x7 depthwise conv -> LN -> 1x1 (4x) -> GELU -> 1x1 -> layer scale -> residual."""

    def __init__(self, dim, drop_path=0., layer_scale_init_value=1e-6, kernels='torch'):
        super().__init__()
        if kernels not in BLOCK_KERNELS:
            raise ValueError(f"Block kernels must be one of {BLOCK_KERNELS}, got {kernels!r}")
        self.kernels = kernels
        self.dwconv = nn.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim)
        self.norm = LayerNorm(dim, eps=1e-6)
        self.pwconv1 = nn.Linear(dim, 4 * dim)
        self.act = nn.GELU()
        self.pwconv2 = nn.Linear(4 * dim, dim)
        self.gamma = nn.Parameter(layer_scale_init_value * torch.ones((dim)),
                                  requires_grad=True) if layer_scale_init_value > 0 else None
        if drop_path > 0.:
            raise NotImplementedError("stochastic depth is not used by the shipped configs (drop_path_rate=0)")
        self.drop_path = nn.Identity()
        if kernels == 'hip':   # no silent fallback: a block the kernels cannot serve is refused here
            from .. import ops
            if dim not in ops.CONVNEXT_WIDTHS or self.gamma is None:
                raise ValueError(f"Block(dim={dim}, kernels='hip'): the HIP block serves a multiple of 8 up to 64 channels "
                                 "with layer scale")

    def forward(self, x):
        if self.kernels == 'hip':
            from .. import ops
            return ops.convnext_block(x, self.dwconv.weight, self.dwconv.bias, self.norm.weight, self.norm.bias,
                                      self.pwconv1.weight, self.pwconv1.bias, self.pwconv2.weight, self.pwconv2.bias, self.gamma)
        y = self.dwconv(x).permute(0, 2, 3, 1)
        y = self.pwconv2(self.act(self.pwconv1(self.norm(y))))
        if self.gamma is not None:
            y = self.gamma * y
        return x + y.permute(0, 3, 1, 2)


class Downsample(nn.Sequential):
    """A downsampling stage of the encoder: the reference's nn.Sequential of a stride-s patchify conv and a channels-first
    LayerNorm -- conv at index 0 and LayerNorm at index 1 (`order='post'`, stage 0) or the other way round (`order='pre'`) --
    so parameter names and checkpoints are the reference's.  `kernels='hip'` forwards through ops.patchify_ln
    (csrc/patchify.hip); a shape those kernels do not serve is refused here, there is no fallback."""

    def __init__(self, in_channel, out_channel, stride, order, kernels='torch'):
        if kernels not in BLOCK_KERNELS:
            raise ValueError(f"Downsample kernels must be one of {BLOCK_KERNELS}, got {kernels!r}")
        conv = nn.Conv2d(in_channel, out_channel, kernel_size=stride, stride=stride)
        norm = LayerNorm(out_channel if order == 'post' else in_channel, eps=1e-6, data_format="channels_first")
        super().__init__(*((conv, norm) if order == 'post' else (norm, conv)))
        self.order, self.kernels = order, kernels
        if kernels == 'hip':
            from .. import ops
            ops.patchify_ln_shape(f"Downsample({in_channel}, {out_channel}, stride={stride}, kernels='hip')", in_channel,
                                  out_channel, stride, order)

    def forward(self, x):
        if self.kernels != 'hip':
            return super().forward(x)
        from .. import ops
        conv, norm = (self[0], self[1]) if self.order == 'post' else (self[1], self[0])
        return ops.patchify_ln(x, conv.weight, conv.bias, norm.weight, norm.bias, self.order)


ENCODER_KERNELS = ('torch', 'hip', 'hip_all')   # PyTorch ops | Blocks in HIP | Blocks and downsampling stages in HIP


class ConvNeXt(nn.Module):
    """HNeRV frame encoder (reference _layers.py:134-193): per stage a strided patchify conv + `stage_blocks` Blocks.
    `kernels`: 'torch', 'hip' (the Blocks on csrc/convnext.hip) or 'hip_all' (and the stages on csrc/patchify.hip)."""

    def __init__(self, stage_blocks=0, strds=[2, 2, 2, 2], dims=[96, 192, 384, 768], in_chans=3, drop_path_rate=0.,
                 layer_scale_init_value=1e-6, kernels='torch'):
        super().__init__()
        if kernels not in ENCODER_KERNELS:
            raise ValueError(f"ConvNeXt kernels must be one of {ENCODER_KERNELS}, got {kernels!r}")
        block_kernels = 'torch' if kernels == 'torch' else 'hip'
        down_kernels = 'hip' if kernels == 'hip_all' else 'torch'
        self.downsample_layers = nn.ModuleList()
        self.stages = nn.ModuleList()
        self.stage_num = len(dims)
        for i in range(self.stage_num):
            if i > 0:
                down = Downsample(dims[i - 1], dims[i], strds[i], 'pre', kernels=down_kernels)
            else:
                down = Downsample(in_chans, dims[0], strds[i], 'post', kernels=down_kernels)
            self.downsample_layers.append(down)
            self.stages.append(nn.Sequential(*[Block(dim=dims[i], layer_scale_init_value=layer_scale_init_value,
                                                     kernels=block_kernels) for _ in range(stage_blocks)]))
        self.apply(self._init_weights)

    @staticmethod
    def _init_weights(m):
        if isinstance(m, (nn.Conv2d, nn.Linear)):
            nn.init.trunc_normal_(m.weight, std=.02)
            nn.init.constant_(m.bias, 0)

    def forward(self, x):
        for down, stage in zip(self.downsample_layers, self.stages):
            x = stage(down(x))
        return x
