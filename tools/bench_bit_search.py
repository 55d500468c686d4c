#!/usr/bin/env python3
"""Times the bit allocation under a size budget (methods/bit_assign.py) at HNeRV-3M, 640 x 1280, B = 2, synthetic
frames, one GPU, against candidate scoring (`score_candidates`, unchanged from before the table existed) in the same process.

    python tools/bench_bit_search.py [--out profiles/bit_search.json] [--frames 20] [--search_repeats 50]

Records: seconds to build the 49-direction Omega table (perturbations + Gram table) and per direction; seconds
`score_candidates` takes per candidate (the two toy candidates, one warm-up candidate first); the search at (L, K) = (7, 7) --
host clock around ops.bit_search (launches + read-back) and HIP events around back-to-back calls of the C entry; the
frontier over five average-bit budgets; for the two toy candidates the table's Omega against the directly scored one; and
max|G - G^T| / max|G|.  No threshold: the figures are written down.  The model is randomly initialised (timing does not
depend on the weights; the Omega VALUES of a random model mean nothing beyond table-against-direct agreement).  Prints ONE JSON
object and writes it to --out.  Needs the GPU."""
import argparse
import copy
import ctypes
import json
import logging
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neuroquant_amd import _lib as L, ops  # noqa: E402
from neuroquant_amd.methods import bit_assign  # noqa: E402
from neuroquant_amd.utils import FrameCache, get_config, synthetic_frames  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bit_search.json"))
    ap.add_argument("--frames", type=int, default=20, help="synthetic frames; 20 = the 10 batches of two the criterion uses")
    ap.add_argument("--search_repeats", type=int, default=50)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_bit_search.py needs a GPU"
    logging.getLogger().setLevel(logging.WARNING)
    cfg = get_config(os.path.join(ROOT, "tools", "hnerv_bunny_3m.yaml"))
    args = types.SimpleNamespace(arch="hnerv", mode="omega", batch_size=2, seed=903, channel_wise=True, hadamard=False, init="max")
    torch.manual_seed(903)
    model = bit_assign.HNeRV(cfg).to("cuda").eval()
    cache = FrameCache(synthetic_frames(a.frames, cfg["crop_h"], cfg["crop_w"], seed=903, device="cuda"))
    with torch.no_grad():
        emb = torch.cat([model.encode(cache.batch(torch.tensor([i], device="cuda"))) for i in range(a.frames)])
    choices = list(bit_assign.DEFAULT_BIT_CHOICES)
    toy = bit_assign.hnerv_candidate
    batches = min(bit_assign.MAX_BATCHES, (a.frames + 1) // 2)

    # candidate scoring as it was: a warm-up candidate (first-use costs of the kernels), then the two toy candidates
    bit_assign.score_candidates(model, {"warmup": [8] * 7}, emb, cache, args)
    direct, t_direct = timed(lambda: bit_assign.score_candidates(model, toy, emb, cache, args))

    torch.cuda.reset_peak_memory_stats()
    (table, _, sizes), t_pert = timed(lambda: bit_assign.perturbation_table(model, choices, args))
    loader = bit_assign.FullLoader(cache, 2, seed=903)
    G, t_gram = timed(lambda: bit_assign.gram_table("omega", "hnerv", copy.deepcopy(model), table, loader))
    peak = torch.cuda.max_memory_allocated()
    n = G.shape[0]

    numels = [(m.weight.numel(), m.bias.numel()) for m in bit_assign.decoder_convs(model)]
    size_bits = torch.tensor(sizes["nominal"], dtype=torch.int64, device="cuda")
    budget = bit_assign.budget_to_bits(numels, budget_avg_bits=5.0)
    wall = []
    for _ in range(a.search_repeats):
        _, t = timed(lambda: ops.bit_search(G, size_bits, budget))
        wall.append(t)
    ws = torch.empty(L.lib().nq_bit_search_ws_bytes(7, 7) // 8, device="cuda", dtype=torch.float64)
    om = torch.empty(1, device="cuda", dtype=torch.float64)
    ix = torch.empty(1, device="cuda", dtype=torch.int64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(a.search_repeats):
        L.check(L.lib().nq_bit_search(p(G), p(size_bits), 7, 7, budget, p(om), p(ix), p(ws), stream), "bit_search")
    e.record()
    torch.cuda.synchronize()

    front = bit_assign.frontier(G, sizes["nominal"], [bit_assign.budget_to_bits(numels, budget_avg_bits=x) for x in (3.0, 4.0, 5.0, 6.0, 7.0)],
                                choices, numels)
    toys = {}
    for name, bits in toy.items():
        t_om = bit_assign.omega_from_table(G, bits, choices)
        toys[name] = dict(bits=bits, omega_table=t_om, omega_direct=direct[name],
                          rel_gap=abs(t_om - direct[name]) / max(abs(direct[name]), 1e-300))
    res = dict(model="HNeRV-3M 640x1280, random weights", batch=2, batches=batches, frames=a.frames, directions=n,
               table_seconds=round(t_pert + t_gram, 3), perturbation_seconds=round(t_pert, 4), gram_seconds=round(t_gram, 3),
               seconds_per_direction=round(t_gram / n, 4),
               score_candidates_seconds_per_candidate=round(t_direct / len(toy), 3),
               table_cost_in_candidates=round((t_pert + t_gram) / (t_direct / len(toy)), 2),
               peak_memory_mib_table=round(peak / 2 ** 20, 1),
               search_7x7=dict(allocations=7 ** 7, wall_ms_median=round(1e3 * statistics.median(wall), 4),
                               wall_ms_min=round(1e3 * min(wall), 4),
                               kernels_ms_per_call=round(s.elapsed_time(e) / a.search_repeats, 4)),
               frontier=front, toy_candidates=toys,
               asymmetry=float((G - G.t()).abs().max() / G.abs().max()))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
