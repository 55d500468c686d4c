"""Measures the HIP ConvNeXt block (ops.convnext_block, csrc/convnext.hip) -> profiles/convnext_block.json.

  block      forward + backward (all ten gradients) of one block at (1, 64, 128, 256), (1, 64, 32, 64) and (1, 16, 2, 4): the HIP
             block against models/_layers.py Block on PyTorch ops, in one process, alternating inside every repeat
  trainer    steps/s of the trainer's step on HNeRV-3M (640 x 1280, B = 2, l2) with enc_kernels 'torch' and 'hip', and, with
             --parent_tree DIR (a checkout of the parent commit; it runs on this tree's libnqhip.so through NQ_LIB, the ABI is
             additive), of the parent's trainer: one fresh child process per run, the candidates alternating; the spread of the
             runs of one candidate is the run-to-run spread the others are read against

    python tools/bench_convnext.py [--out profiles/convnext_block.json] [--repeats 9] [--calls 50] [--steps 300] [--rounds 3]
                                   [--parent_tree DIR] [--skip block,trainer]

Block: HIP events around `calls` back-to-back forward + backward calls on one stream (launch gaps and allocations included, the
same for both), median over `repeats` windows after a warm-up of each.  Trainer: host clock between two device synchronisations,
steps 20 .. `steps` of a run.  Recorded, not asserted.  Prints ONE JSON object and writes it to --out.  Needs the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK_SHAPES = [(1, 64, 128, 256), (1, 64, 32, 64), (1, 16, 2, 4)]


def spread(v, digits=1):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits), "runs": len(v)}


def trainer_child(root, kernels, steps):
    """one trainer run of the tree at `root` -> prints its steps/s"""
    sys.path[:0] = [root, os.path.join(root, "tools")]
    import torch
    from bench import HNERV_3M
    from bench_ssim_loss import train
    frames = torch.randint(0, 256, (8, 3, 640, 1280), device="cuda", dtype=torch.uint8, generator=torch.Generator(device="cuda").manual_seed(1))
    cfg = dict(HNERV_3M) if kernels == "parent" else dict(HNERV_3M, enc_kernels=kernels)
    print(json.dumps({"steps_per_s": train(cfg, frames, "l2", steps, first=20)[1]}))


def trainer_run(root, kernels, steps):
    env = dict(os.environ, NQ_LIB=os.path.join(ROOT, "neuroquant_amd", "libnqhip.so"))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, kernels, str(steps)], env=env, check=True,
                         capture_output=True, text=True, timeout=600).stdout
    return json.loads(out.strip().splitlines()[-1])["steps_per_s"]


def bench_block(shape, repeats, calls):
    import torch
    sys.path.insert(0, ROOT)
    from neuroquant_amd.models._layers import Block
    N, C, H, W = shape
    torch.manual_seed(C + H)
    blocks = {k: Block(C, kernels=k).cuda() for k in ("torch", "hip")}
    blocks["hip"].load_state_dict(blocks["torch"].state_dict())
    x = torch.randn(shape, device="cuda", requires_grad=True)
    dy = torch.randn(shape, device="cuda")

    def step(blk):
        torch.autograd.grad(blk(x), [x] + list(blk.parameters()), dy)

    def window_us(blk):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(calls):
            step(blk)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / calls

    for blk in blocks.values():
        for _ in range(20):
            step(blk)
    t = {k: [] for k in blocks}
    for _ in range(repeats):
        for k, blk in blocks.items():
            t[k].append(window_us(blk))
    flops = 3 * 2 * 2 * N * H * W * C * 4 * C          # the two pointwise products, forward + both backward products of each
    row = {"shape": list(shape), "us_per_forward_backward": {k: spread(v) for k, v in t.items()},
           "hip_over_torch_time": round(statistics.median(t["hip"]) / statistics.median(t["torch"]), 3),
           "pointwise_gflop_per_call": round(flops / 1e9, 3)}
    return row


def main(argv):
    if argv[:1] == ["--child"]:
        return trainer_child(argv[1], argv[2], int(argv[3]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convnext_block.json"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent_tree", default=None, help="a checkout of the parent commit: its default trainer against this tree's")
    ap.add_argument("--skip", default="", help="comma-separated: block, trainer")
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_convnext needs the GPU (nothing is measured without one)")
    skip = set(filter(None, a.skip.split(",")))
    res = {}
    if os.path.exists(a.out):                    # sections measured by an earlier call are kept
        with open(a.out) as fh:
            res = json.load(fh)
    res["device"] = torch.cuda.get_device_name(0)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)

    if "trainer" not in skip:                    # child processes first, before this process holds the GPU
        cands = {"torch": (ROOT, "torch"), "hip": (ROOT, "hip")}
        if a.parent_tree:
            cands["parent"] = (os.path.abspath(a.parent_tree), "parent")
        rates = {k: [] for k in cands}
        for _ in range(a.rounds):
            for k, (root, kernels) in cands.items():
                rates[k].append(trainer_run(root, kernels, a.steps))
        med = {k: statistics.median(v) for k, v in rates.items()}
        res["trainer"] = {"note": "HNeRV-3M 640x1280: model + step_loss + backward + Adam at B = 2, l2, steps 20 .. %d of a run, one "
                                  "process per run, %d runs per candidate, alternating" % (a.steps, a.rounds),
                          "steps_per_s": {k: spread(v) for k, v in rates.items()},
                          "hip_over_torch": round(med["hip"] / med["torch"], 4),
                          "default_over_parent": round(med["torch"] / med["parent"], 4) if "parent" in med else "not measured"}
        save()
    if "block" not in skip:
        res["block"] = {"calls_per_window": a.calls, "repeats": a.repeats,
                        "note": "forward + backward (ten gradients) of one Block through autograd, back-to-back calls on one stream: "
                                "launch gaps and allocations included; microseconds per call",
                        "shapes": [bench_block(s, a.repeats, a.calls) for s in BLOCK_SHAPES]}
        save()
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])
