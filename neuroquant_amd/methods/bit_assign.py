"""Sensitivity-guided mixed-precision bit allocation (counterpart of the reference's methods/bit_assign.py).

Same entry points and flow as the reference (file:line are the reference's):
  gradtensor_to_vec             bit_assign.py:36-55
  run_hessian_vector_product    bit_assign.py:57-118   H·v of nn.MSELoss w.r.t. the decoder conv weights, summed over the
                                                       first 10 batches, by double backward (autograd.grad(create_graph=True)
                                                       then prod.backward()) -- here through ops.decoder_stack_dd, i.e.
                                                       the HIP convolution kernels composed as twice-differentiable
                                                       autograd Functions (conv is bilinear: F, dgrad, wgrad are closed
                                                       under differentiation)
  run_approx_param_fisher       bit_assign.py:120-168  accumulated dL/dW
  sensitivity_criterion         bit_assign.py:171-217  'omega' = sum_l <v_l,(Hv)_l>,  'fisher_diag' = sum_l <v_l^2, g_l^2>
  assign / main                 bit_assign.py:276-446  FP eval -> per candidate: QuantModel, set_bitwidth, lazy scale init,
                                                       score; the lowest score wins

    python -m neuroquant_amd.methods.bit_assign --arch hnerv --config cfg.yaml --data_path bunny/ --vid Bunny \
        --ckpt epoch300.pth --batch_size 2 --channel_wise --init max --mode omega
    (--synthetic N uses N synthetic frames; --candidates "2 3 4 6 4 4 2" "6 5 4 5 5 6 6" overrides the toy candidates)

Under a size budget (--budget_bytes N | --budget_avg_bits X) nothing is typed in: Omega is a quadratic form, so the Gram
table of the L x K per-layer perturbations (gram_table, L K second-order passes per batch) holds the exact Omega of all K^L
allocations, and a HIP kernel enumerates them under the budget (search_allocation):
    python -m neuroquant_amd.methods.bit_assign ... --budget_bytes 1400000 --out bits.json
    python -m neuroquant_amd.methods.calibrate_network ... --precision_file bits.json --export_stream video.nqv

Frames come from the GPU-resident uint8 cache instead of the PNG DataLoader; batches are drawn shuffle=True,
drop_last=False like the reference's full_dataloader (bit_assign.py:281-283).  Candidates are independent, so on a
multi-GPU node rank r scores candidates r, r+world, ... and the scores are all-gathered (replicas, no data-path
collective).
"""
import argparse
import copy
import json
import logging
import math
import os
import random
import sys
import time
from datetime import datetime

import numpy as np
import torch
import torch.nn as nn

from ..models import HNeRV, NeRV
from ..models._decode import _fused_stack
from ..quantization import QuantModel
from ..quantization.quant_block import specials
from ..quantization.quantizer import StraightThrough
from ..utils import FrameCache, data_split, get_config, setup_logger
from .. import ops
from .calibrate_network import add_yuv_args, evaluate, load_frames, report_line

# toy example (bit_assign.py:26-35)
hnerv_candidate = {
    'candidate1': [2, 3, 4, 6, 4, 4, 2],  # 4.96 bit
    'candidate2': [6, 5, 4, 5, 5, 6, 6],  # 4.79 bit
}
nerv_candidate = {
    'candidate1': [5, 6, 3, 4, 5, 4, 3],  # 5.47 bit
    'candidate2': [6, 5, 5, 6, 7, 6, 7],  # 5.12 bit
}
MAX_BATCHES = 10  # bit_assign.py:116-118
DEFAULT_BIT_CHOICES = (2, 3, 4, 5, 6, 7, 8)


class FullLoader:
    """The reference's `full_dataloader` (bit_assign.py:281-283: shuffle=True, drop_last=False) over a FrameCache."""

    def __init__(self, cache: FrameCache, batch_size, seed=903):
        self.cache, self.bs = cache, batch_size
        self.gen = torch.Generator().manual_seed(seed)

    def __len__(self):
        return (len(self.cache) + self.bs - 1) // self.bs

    def __iter__(self):
        n = len(self.cache)
        perm = torch.randperm(n, generator=self.gen).to(self.cache.frames.device)
        for i in range(0, n, self.bs):
            idx = perm[i:i + self.bs]
            yield {'img': self.cache.batch(idx), 'idx': idx, 'norm_idx': idx.float() / n}


def gradtensor_to_vec(net):
    """Gradients of the decoder's weight tensors, in named_parameters order (bit_assign.py:36-55)."""
    return [v.grad.data for k, v in net.named_parameters() if 'encoder' not in k and 'weight' in k]


def _decode_dd(arch, net, sample):
    """Twice-differentiable forward of `net` on one batch.  The encoder output does not depend on the decoder weights,
    so it is computed without a graph (the reference builds one through the encoder and never uses it)."""
    spec_provs = _fused_stack(net)
    if spec_provs is None:
        raise NotImplementedError('bit allocation needs the shipped decoder shape (conv/PixelShuffle/GELU blocks, tanh head)')
    spec, provs = spec_provs
    img = sample['img']
    with torch.no_grad():
        emb = net.encode(img) if arch == 'hnerv' else net.encode(sample['norm_idx'])
    return ops.decoder_stack_dd(emb, spec, [p() for p in provs]), img


def run_hessian_vector_product(arch, vec, params, net, criterion, dataloader, use_cuda=True):
    """H·vec accumulated into the .grad of `params` (bit_assign.py:57-118)."""
    if not use_cuda:
        raise RuntimeError('neuroquant_amd has no CPU path (the CPU restatement lives in oracle/ for tests)')
    net.cuda()
    vec = [v.detach().cuda() for v in vec]
    net.eval()
    net.zero_grad()
    for count, sample in enumerate(dataloader):
        if count >= MAX_BATCHES:
            break
        img_out, img = _decode_dd(arch, net, sample)
        loss = criterion(img_out, img)
        grad_f = torch.autograd.grad(loss, inputs=params, create_graph=True, allow_unused=True)
        prod = sum((g * v).sum() for g, v in zip(grad_f, vec) if g is not None)
        prod.backward()


def run_approx_param_fisher(arch, vec, params, net, criterion, dataloader, use_cuda=True):
    """dL/dW accumulated into the .grad of `params` over the first 10 batches (bit_assign.py:120-168)."""
    if not use_cuda:
        raise RuntimeError('neuroquant_amd has no CPU path (the CPU restatement lives in oracle/ for tests)')
    net.cuda()
    net.eval()
    net.zero_grad()
    for count, sample in enumerate(dataloader):
        if count >= MAX_BATCHES:
            break
        img_out, img = _decode_dd(arch, net, sample)
        criterion(img_out, img).backward()


def sensitivity_criterion(mode, arch, net, qnn, dataloader, use_cuda=True):
    """Sensitivity score of one mixed-precision candidate (bit_assign.py:171-217): net = FP model, qnn = the
    QuantModel whose `get_perturbation()` gives v_l = W_l - Q(W_l)."""
    params = []
    for k, v in net.named_parameters():
        if 'encoder' in k:
            continue
        if 'weight' in k:
            v.requires_grad = True
            params.append(v)
    with torch.no_grad():
        vec = [v.detach() for v in qnn.get_perturbation()]
    criterion = nn.MSELoss()
    if mode == 'omega':
        run_hessian_vector_product(arch, vec, params, net, criterion, dataloader, use_cuda)
        total = 0.
        for count, (g, v) in enumerate(zip(gradtensor_to_vec(net), vec)):
            cur = (g * v).sum()
            total = total + cur
            logging.info(f"[{count:d}-th layer] {float(cur):.3e}")
        return total
    if mode == 'fisher_diag':
        run_approx_param_fisher(arch, vec, params, net, criterion, dataloader, use_cuda)
        total = 0.
        for count, (g, v) in enumerate(zip(gradtensor_to_vec(net), vec)):
            cur = (v.pow(2) * g.pow(2)).sum()
            total = total + cur
            logging.info(f"[{count:d}-th layer] {float(cur):.3e}")
        return total
    raise ValueError('Not implemented sensitivity criteria: {}'.format(mode))


def owned_candidates(names, rank=0, world=1):
    """Candidates scored by `rank`: round-robin in dict order (candidates are independent -> replicas, no collective
    on the data path)."""
    return [n for i, n in enumerate(names) if i % world == rank]


def gather_scores(scores, world):
    """Union of the per-rank {name: score} dicts on every rank (torch.distributed.all_gather_object)."""
    if world <= 1:
        return dict(scores)
    import torch.distributed as dist
    gathered = [None] * world
    dist.all_gather_object(gathered, scores)
    return {k: v for d in gathered for k, v in d.items()}


def pick_best(candidate_dict, scores):
    """Lowest score wins; ties go to the earlier candidate (bit_assign.py:361-365 uses a strict '<')."""
    names = list(candidate_dict)
    best = min(names, key=lambda c: (scores[c], names.index(c)))
    return best, candidate_dict[best], scores[best]


def score_candidates(model, candidate_dict, cali_data, cache, args, rank=0, world=1):
    """-> {name: score} for the candidates this rank owns."""
    device = next(model.parameters()).device
    scores = {}
    mine = set(owned_candidates(list(candidate_dict), rank, world))
    for candidate, bits in candidate_dict.items():
        if candidate not in mine:
            continue
        wq_params = {'n_bits': 8, 'channel_wise': args.channel_wise, 'scale_method': args.init}
        qnn = QuantModel(model=copy.deepcopy(model), hadamard=args.hadamard, weight_quant_params=wq_params).to(device)
        qnn.eval()
        avg_bits = float(qnn.set_bitwidth(bits))
        qnn.set_quant_state(True)
        with torch.no_grad():
            qnn(cali_data[:args.batch_size].to(device))      # lazy scale init (bit_assign.py:353-355)
        logging.info(f"[{candidate}: {bits}] Average Quantization Bit-Width:\t{avg_bits:.4f}")
        loader = FullLoader(cache, args.batch_size, seed=args.seed)   # same batches for every candidate
        score = float(sensitivity_criterion(args.mode, args.arch, copy.deepcopy(model), qnn, loader, use_cuda=True))
        logging.info(f"[{candidate}: {bits}] The {args.mode} sensitivity score =\t{score:.3e}")
        scores[candidate] = score
    return scores


# ------------------------------------------------------------------------------------------ table and search
def decoder_convs(model):
    """The decoder's convolutions in the order QuantModel.quant_modules() lists their quantised counterparts (the same walk
    as QuantModel.quant_module_refactor: children named '*encoder*' are left alone, a NeRVBlock contributes its conv)."""
    out = []
    for name, child in model.named_children():
        if 'encoder' in name or isinstance(child, StraightThrough):
            continue
        if type(child) in specials:
            out.append(child.conv[0])
        elif isinstance(child, nn.Conv2d):
            out.append(child)
        else:
            out += decoder_convs(child)
    return out


def _hard_levels(x, delta, zp, n_levels):
    """export._levels for a UniformAffineQuantizer: the integer grid tensor an entropy coder stores."""
    return torch.clamp(torch.round(x / delta) + zp, 0, n_levels - 1).round().to(torch.uint8)


def size_tables(numels, bit_choices, entropy_bits=None):
    """Integer sizes in bits of layer l at choice c.  numels: [(weight.numel(), bias.numel())] per layer.
    'nominal': c (weight.numel() + bias.numel()), export_quantized's nominal_bits; 'entropy' (given entropy_bits[l][c], the
    zeroth-order entropy of the hard levels of weight plus bias): its ceiling, an estimate made before calibration of what
    --stream_coding rans realises."""
    tables = {'nominal': [[int(c) * (int(nw) + int(nb)) for c in bit_choices] for nw, nb in numels]}
    if entropy_bits is not None:
        tables['entropy'] = [[int(math.ceil(e)) for e in row] for row in entropy_bits]
    return tables


@torch.no_grad()
def perturbation_table(model, bit_choices, args):
    """-> (table, hists, sizes): table[l][c] = v_l(c) = W_l - Q_c(W_l), bit for bit what QuantModel.get_perturbation()[l] is
    after set_bitwidth([c] * L) and the lazy-init forward, from the same kernels (ops.scale_init with --init's method, ops.uaq_forward_multi)
    without a QuantModel copy or a decoder forward; hists[l][c] = (weight, bias) level histograms of the hard UAQ levels
    (what export_quantized would store); sizes = size_tables(...).  With args.hadamard the scales come from the transformed,
    zero-padded weight and are applied to the weight itself, as QuantModule.get_weight_perturbation does."""
    from ..export import _entropy_bits
    convs = decoder_convs(model)
    table, hists, ent = [[] for _ in convs], [[] for _ in convs], [[] for _ in convs]
    srcs = [ops.hadamard_weight_of(m.weight.data) if args.hadamard else m.weight.data for m in convs]
    for c in bit_choices:
        nl = 2 ** int(c)
        scales = [ops.scale_init(src, nl, args.channel_wise, args.init) for src in srcs]
        fq = ops.uaq_forward_multi([(m.weight.data, d, z, nl) for m, (d, z) in zip(convs, scales)])
        for l, (m, src, (d, z), q) in enumerate(zip(convs, srcs, scales, fq)):
            table[l].append(m.weight.data - q)
            bd, bz = ops.scale_init(m.bias.data, nl, args.channel_wise, args.init)
            wl, bl = _hard_levels(src, d, z, nl), _hard_levels(m.bias.data, bd, bz, nl)
            hists[l].append((torch.bincount(wl.flatten().long(), minlength=nl), torch.bincount(bl.flatten().long(), minlength=nl)))
            ent[l].append(_entropy_bits(wl, nl) + _entropy_bits(bl, nl))
    sizes = size_tables([(m.weight.numel(), m.bias.numel()) for m in convs], bit_choices, ent)
    return table, hists, sizes


def direction_names(n_layers, n_choices):
    """Column names of the Gram table, column j = l K + c <-> 'l:c' (what owned_candidates / gather_scores share out)."""
    return [f'{l}:{c}' for l in range(n_layers) for c in range(n_choices)]


def _decoder_weights(net):
    params = []
    for k, v in net.named_parameters():
        if 'encoder' not in k and 'weight' in k:
            v.requires_grad = True
            params.append(v)
    return params


def gram_table(mode, arch, net, table, dataloader, rank=0, world=1):
    """G (L K, L K) float64 on the device: G[(l,c),(m,d)] = <v_l(c), (H e_{m,d})_l>, H the Hessian of the MSE loss at the FP
    weights summed over the first MAX_BATCHES batches, e_{m,d} = v_m(d) on layer m and zero elsewhere.  Batches are the outer
    loop: one twice-differentiable forward and one autograd.grad(create_graph=True) per batch, then one autograd.grad of
    <dL/dW_m, v_m(d)> per direction on the retained graph; ops.rows_dot turns layer l's slice of H e_j into G[(l,.), j].  The
    .grad fields are not touched.  Rank r computes the columns r, r + world, ... (owned_candidates / gather_scores).
    'fisher_diag': one first-order accumulation g_l; only G[(l,c),(l,c)] = sum v_l(c)^2 g_l^2 is non-zero."""
    params = _decoder_weights(net)
    n_layers, K = len(table), len(table[0])
    if len(params) != n_layers or any(p.shape != row[0].shape or len(row) != K for p, row in zip(params, table)):
        raise ValueError('the perturbation table does not match the decoder\'s weight tensors')
    n = n_layers * K
    dev = params[0].device
    stacks = [torch.stack([v.detach() for v in row]) for row in table]
    criterion = nn.MSELoss()
    net.eval()
    if mode == 'fisher_diag':
        acc = None
        for count, sample in enumerate(dataloader):
            if count >= MAX_BATCHES:
                break
            img_out, img = _decode_dd(arch, net, sample)
            g = torch.autograd.grad(criterion(img_out, img), params, allow_unused=True)
            g = [torch.zeros_like(p) if x is None else x for x, p in zip(g, params)]
            acc = g if acc is None else [a + x for a, x in zip(acc, g)]
        G = torch.zeros(n, n, device=dev, dtype=torch.float64)
        for l in range(n_layers):
            d = ops.rows_dot(stacks[l].pow(2), acc[l].pow(2))
            G[l * K:(l + 1) * K, l * K:(l + 1) * K] = torch.diag(d)
        return G
    if mode != 'omega':
        raise ValueError('Not implemented sensitivity criteria: {}'.format(mode))
    names = direction_names(n_layers, K)
    mine = owned_candidates(list(range(n)), rank, world)
    cols = {names[j]: torch.zeros(n, device=dev, dtype=torch.float64) for j in mine}
    for count, sample in enumerate(dataloader):
        if count >= MAX_BATCHES:
            break
        img_out, img = _decode_dd(arch, net, sample)
        grad_f = torch.autograd.grad(criterion(img_out, img), inputs=params, create_graph=True, allow_unused=True)
        live = [j for j in mine if grad_f[j // K] is not None]
        for pos, j in enumerate(live):
            m, d = divmod(j, K)
            prod = (grad_f[m] * table[m][d].detach()).sum()
            hv = torch.autograd.grad(prod, params, retain_graph=pos + 1 < len(live), allow_unused=True)
            for l, h in enumerate(hv):
                if h is not None:
                    cols[names[j]][l * K:(l + 1) * K] += ops.rows_dot(stacks[l], h)
        del grad_f
    if world > 1:
        cols = {k: v.cpu() for k, v in cols.items()}
    cols = gather_scores(cols, world)
    return torch.stack([cols[k].to(dev) for k in names], dim=1)


def omega_from_table(G, bits, bit_choices=DEFAULT_BIT_CHOICES):
    """Omega of one allocation from the table, on the host: sum_l sum_m G[(l,b_l),(m,b_m)], l ascending in the outer and m in
    the inner loop, plain float64 additions from 0.0 -- the order of the search kernel."""
    G = G.detach().cpu().numpy() if isinstance(G, torch.Tensor) else np.asarray(G, dtype=np.float64)
    choices = [int(c) for c in bit_choices]
    K = len(choices)
    idx = [l * K + choices.index(int(b)) for l, b in enumerate(bits)]
    if G.shape != (len(idx) * K, len(idx) * K):
        raise ValueError(f'a table of shape {G.shape} does not hold {len(idx)} layers of {K} choices')
    acc = 0.0
    for i in idx:
        for j in idx:
            acc = acc + float(G[i, j])
    return acc


def index_to_bits(index, n_layers, bit_choices=DEFAULT_BIT_CHOICES):
    """Mixed-radix candidate index, layer 0 the least significant digit -> per-layer bit-widths."""
    K = len(bit_choices)
    return [int(bit_choices[(index // K ** l) % K]) for l in range(n_layers)]


def search_allocation(G, size_bits, budget_bits, bit_choices=DEFAULT_BIT_CHOICES):
    """-> (bits, omega, size_bits_total): the allocation of least Omega among those with sum_l size_bits[l][b_l] <=
    budget_bits, by ops.bit_search over all K^L of them.  ValueError when G is not finite or nothing fits."""
    sizes = torch.as_tensor(size_bits, dtype=torch.int64)
    n_layers, K = sizes.shape
    if K != len(bit_choices):
        raise ValueError(f'size table has {K} choices per layer, bit_choices {len(bit_choices)}')
    if not bool(torch.isfinite(G).all()):
        raise ValueError('the Omega table holds non-finite entries')
    omega, index = ops.bit_search(G, sizes.to(G.device), int(budget_bits))
    if index is None:
        least = int(sizes.min(dim=1).values.sum())
        raise ValueError(f'no allocation fits {int(budget_bits)} bits: the smallest feasible size is {least} bits '
                         f'({math.ceil(least / 8)} bytes)')
    bits = index_to_bits(index, n_layers, bit_choices)
    total = sum(int(sizes[l, (index // K ** l) % K]) for l in range(n_layers))
    return bits, omega, total


def frontier(G, size_bits, budgets, bit_choices=DEFAULT_BIT_CHOICES, numels=None):
    """One search per budget (bits) -> [{budget, bits, omega, size_bits, avg_bits}]; avg_bits is QuantModel.set_bitwidth's
    parameter-weighted average when the per-layer (weight, bias) element counts are given."""
    out = []
    for budget in budgets:
        bits, omega, total = search_allocation(G, size_bits, budget, bit_choices)
        out.append(dict(budget=int(budget), bits=bits, omega=omega, size_bits=total,
                        avg_bits=average_bits(bits, numels) if numels else None))
    return out


def average_bits(bits, numels):
    """QuantModel.set_bitwidth's return value: the parameter-weighted average bit-width, in its arithmetic."""
    total, num = 0., 0.
    for b, (nw, nb) in zip(bits, numels):
        total += b * nw + b * nb
        num += nw + nb
    return total / num


def budget_to_bits(numels, budget_bytes=None, budget_avg_bits=None):
    """The budget in bits of the size model: --budget_bytes N <-> ceil(sum / 8) <= N; --budget_avg_bits X <-> sum / params <= X
    in the float division of QuantModel.set_bitwidth (the largest integer sum that satisfies it)."""
    if budget_bytes is not None:
        return 8 * int(budget_bytes)
    num = float(sum(nw + nb for nw, nb in numels))
    s = int(math.floor(budget_avg_bits * num))
    while (s + 1) / num <= budget_avg_bits:
        s += 1
    while s > 0 and s / num > budget_avg_bits:
        s -= 1
    return s


def assign_under_budget(args, model, cache, rank, world):
    """Table, search, log, --out: what `assign` does when a budget is given."""
    choices = [int(c) for c in args.bit_choices]
    table, _, sizes = perturbation_table(model, choices, args)
    convs = decoder_convs(model)
    numels = [(m.weight.numel(), m.bias.numel()) for m in convs]
    size_bits = sizes[args.size_model]
    budget = budget_to_bits(numels, args.budget_bytes, args.budget_avg_bits)
    least = sum(min(row) for row in size_bits)
    if least > budget:    # before the table is paid for; search_allocation says the same of a table it is handed
        raise ValueError(f'no allocation fits {budget} bits: the smallest feasible size is {least} bits '
                         f'({math.ceil(least / 8)} bytes)')
    t0 = time.time()
    loader = FullLoader(cache, args.batch_size, seed=args.seed)
    G = gram_table(args.mode, args.arch, copy.deepcopy(model), table, loader, rank, world)
    torch.cuda.synchronize()
    logging.info(f'{args.mode} table: {len(convs)} layers x {len(choices)} choices = {G.shape[0]} directions in '
                 f'{time.time() - t0:.2f} s; max|G - G^T| / max|G| = {float((G - G.t()).abs().max() / G.abs().max()):.2e}')
    bits, omega, total = search_allocation(G, size_bits, budget, choices)
    avg = average_bits(bits, numels)
    result = dict(bits=bits, omega=omega, size_bits=total, avg_bits=avg, mode=args.mode, bit_choices=choices,
                  budget=dict(bits=budget, bytes=args.budget_bytes, avg_bits=args.budget_avg_bits, size_model=args.size_model))
    if args.frontier:
        in_bytes = args.budget_bytes is not None      # the frontier's budgets are in the unit of the budget flag
        budgets = [budget_to_bits(numels, int(b) if in_bytes else None, None if in_bytes else float(b)) for b in args.frontier]
        result['frontier'] = frontier(G, size_bits, budgets, choices, numels)
        for f in result['frontier']:
            logging.info(f"[frontier] budget {f['budget']} bits: {f['bits']}  {args.mode} = {f['omega']:.3e}  "
                         f"size {f['size_bits']} bits, {f['avg_bits']:.4f} bit average")
    toy = hnerv_candidate if args.arch == 'hnerv' else nerv_candidate
    for name, tb in toy.items():
        if len(tb) != len(convs) or any(b not in choices for b in tb):
            continue
        tsize = sum(size_bits[l][choices.index(b)] for l, b in enumerate(tb))
        if tsize <= budget:
            logging.info(f"[{name}: {tb}] fits the budget ({tsize} bits); table {args.mode} =\t{omega_from_table(G, tb, choices):.3e}")
    logging.info(f"[search: {bits}] Average Quantization Bit-Width:\t{avg:.4f}  size {total} of {budget} bits ({args.size_model})")
    if args.out and rank == 0:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or '.', exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)
    args.result = result
    return 'search', bits, omega


def assign(args, cfg):
    if not torch.cuda.is_available():
        raise RuntimeError('neuroquant_amd needs an AMD GPU (no CPU path); the reference CPU path lives in oracle/ for tests')
    import torch.distributed as dist
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    rank = dist.get_rank() if world > 1 else 0
    device = 'cuda'
    frames = load_frames(args, cfg, device)
    cache = FrameCache(frames)
    n = len(cache)
    split = [int(x) for x in args.data_split.split('_')]
    _, args.val_ind_list = data_split(list(range(n)), split, False, 0)

    model = (HNeRV if args.arch == 'hnerv' else NeRV)(cfg).to(device)
    os.makedirs(args.outf, exist_ok=True)
    setup_logger(os.path.join(args.outf, time.strftime('%Y%m%d_%H%M%S') + f'_r{rank}.log'))
    if args.ckpt != 'None':
        logging.info("=> loading checkpoint '{}'".format(args.ckpt))
        model.load_state_dict(torch.load(args.ckpt, map_location='cpu'), strict=False)
    else:
        logging.info('no --ckpt: random-initialised weights (throughput runs only)')
    model.to(device)

    logging.info('=======================Full-precision model========================')
    res, embedding_list = evaluate(model, cache, args, cfg)
    logging.info(report_line('FP', args))
    cali_data = torch.cat(embedding_list, dim=0)

    if getattr(args, 'budget_bytes', None) is not None or getattr(args, 'budget_avg_bits', None) is not None:
        best_candidate, best_bits, best_score = assign_under_budget(args, model, cache, rank, world)
    else:
        if args.candidates:
            candidate_dict = {f'candidate{i + 1}': [int(b) for b in c.split()] for i, c in enumerate(args.candidates)}
        else:
            candidate_dict = hnerv_candidate if args.arch == 'hnerv' else nerv_candidate
        scores = gather_scores(score_candidates(model, candidate_dict, cali_data, cache, args, rank, world), world)
        best_candidate, best_bits, best_score = pick_best(candidate_dict, scores)
    logging.info("=" * 60)
    logging.info(f"Best Candidate: {best_candidate}")
    logging.info(f"Bit Configuration: {best_bits}")
    logging.info(f"Minimum Score: {best_score:.4e}")
    logging.info("=" * 60)
    return best_candidate, best_bits, best_score


def parse_args(argv):
    p = argparse.ArgumentParser(description='running parameters', formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--seed', default=903, type=int)
    p.add_argument('--outf', default='unify')
    p.add_argument('--config', type=str)
    p.add_argument('--arch', type=str)
    p.add_argument('-p', '--print-freq', default=50, type=int)
    p.add_argument('--data_path', type=str)
    p.add_argument('--synthetic', type=int, default=0, help='use N synthetic frames instead of --data_path')
    add_yuv_args(p)
    p.add_argument('--vid', type=str, default='Bunny')
    p.add_argument('--data_split', type=str, default='1_1_1')
    p.add_argument('--batch_size', default=12, type=int)
    p.add_argument('--hadamard', action='store_true')
    p.add_argument('--channel_wise', action='store_true')
    p.add_argument('--init', default='max', type=str, choices=['max', 'mse', 'gaussian', 'l1', 'l2'])
    p.add_argument('--mode', default='omega', type=str, choices=['omega', 'fisher_diag'])
    p.add_argument('--candidates', type=str, nargs='*', default=None,
                   help='bit lists, one quoted string per candidate; default: the reference\'s toy candidates')
    p.add_argument('--ckpt', default='None', type=str)
    budget = p.add_mutually_exclusive_group()
    budget.add_argument('--budget_bytes', type=int, default=None,
                        help='search the allocation of least score with ceil(size / 8) <= N bytes instead of scoring candidates')
    budget.add_argument('--budget_avg_bits', type=float, default=None,
                        help='the same under an average bit-width (QuantModel.set_bitwidth(bits) <= X)')
    p.add_argument('--bit_choices', type=int, nargs='+', default=list(DEFAULT_BIT_CHOICES), help='bit-widths every layer may take')
    p.add_argument('--size_model', default='nominal', type=str, choices=['nominal', 'entropy'],
                   help='size of a layer at a width: width x parameters, or the entropy of its hard levels')
    p.add_argument('--frontier', type=float, nargs='*', default=None,
                   help='further budgets (in the unit of the budget flag) to search; listed in --out')
    p.add_argument('--out', type=str, default=None, help='write {bits, omega, size_bits, avg_bits, ...} as JSON to this path')
    args = p.parse_args(argv)
    if sorted(set(args.bit_choices)) != list(args.bit_choices) or not all(2 <= c <= 8 for c in args.bit_choices):
        p.error('--bit_choices must be distinct ascending widths in 2..8')
    return args


def seed_all(seed=903):
    random.seed(seed)
    np.random.seed(seed)
    os.environ['PYTHONHASHSEED'] = str(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)


def main(argv):
    args = parse_args(argv)
    seed_all(args.seed)
    cfg = get_config(args.config)
    if 'RANK' in os.environ and int(os.environ.get('WORLD_SIZE', '1')) > 1:
        import torch.distributed as dist
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')))
        dist.init_process_group('nccl')
    exp_id = f"{args.vid}_e{cfg.get('epoch')}_b{cfg.get('batch_size')}_lr{cfg.get('learning_rate')}_{cfg.get('loss')}"
    args.outf = os.path.join('results', args.outf, exp_id,
                             "sensitivity-{}_{}-init_batch{}_CW".format(args.mode, args.init, args.batch_size))
    return assign(args, cfg)


if __name__ == '__main__':
    main(sys.argv[1:])
