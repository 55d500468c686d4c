"""Measures the HIP encoder stages (ops.patchify_ln, csrc/patchify.hip) -> profiles/patchify.json.

  stages     forward + backward (every gradient; stage 0 without a data gradient, its input is the image) of the five
             downsampling stages of HNeRV-3M at B = 2: models/_layers.py Downsample with kernels='hip' against the same two
             modules on PyTorch ops, in one process, alternating inside every repeat
  trainer    steps/s of the trainer's step on HNeRV-3M (640 x 1280, B = 2, l2) with enc_kernels 'torch', 'hip' and 'hip_all', and,
             with --parent_tree DIR (a checkout of the parent commit; it runs on this tree's libnqhip.so through NQ_LIB, the ABI
             is additive), of the parent's default trainer: one fresh child process per run, the candidates alternating; the
             spread of the runs of one candidate is the run-to-run spread the others are read against

    python tools/bench_patchify.py [--out profiles/patchify.json] [--repeats 9] [--calls 50] [--steps 300] [--rounds 3]
                                   [--parent_tree DIR] [--skip stages,trainer]

Windows and clocks are those of tools/bench_convnext.py (its trainer child runs the steps).  Recorded, not asserted.  Prints ONE
JSON object and writes it to --out.  Needs the GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
from bench_convnext import spread, trainer_run  # noqa: E402

# (N, C_in, H, W, C_out, s, order): HNeRV-3M at 640 x 1280, enc_strides 5, 4, 4, 2, 2, enc_channel 64, 64, 64, 64, 16
STAGES = [(2, 3, 640, 1280, 64, 5, "post"), (2, 64, 128, 256, 64, 4, "pre"), (2, 64, 32, 64, 64, 4, "pre"),
          (2, 64, 8, 16, 64, 2, "pre"), (2, 64, 4, 8, 16, 2, "pre")]


def bench_stage(case, repeats, calls):
    import torch
    from neuroquant_amd.models._layers import Downsample
    N, Cin, H, W, Cout, s, order = case
    torch.manual_seed(Cin + H)
    mods = {k: Downsample(Cin, Cout, s, order, kernels=k).cuda() for k in ("torch", "hip")}
    mods["hip"].load_state_dict(mods["torch"].state_dict())
    x = torch.randn(N, Cin, H, W, device="cuda", requires_grad=order == "pre")
    dy = torch.randn(N, Cout, H // s, W // s, device="cuda")

    def step(m):
        torch.autograd.grad(m(x), ([x] if order == "pre" else []) + list(m.parameters()), dy)

    def window_us(m):
        s_, e_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s_.record()
        for _ in range(calls):
            step(m)
        e_.record()
        torch.cuda.synchronize()
        return s_.elapsed_time(e_) * 1e3 / calls

    for m in mods.values():
        for _ in range(20):
            step(m)
    t = {k: [] for k in mods}
    for _ in range(repeats):
        for k, m in mods.items():
            t[k].append(window_us(m))
    return {"case": list(case), "us_per_forward_backward": {k: spread(v) for k, v in t.items()},
            "hip_over_torch_time": round(statistics.median(t["hip"]) / statistics.median(t["torch"]), 3),
            "product_gflop_per_call": round((3 if order == "pre" else 2) * 2 * N * (H // s) * (W // s) * Cout * Cin * s * s / 1e9, 3)}


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patchify.json"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent_tree", default=None, help="a checkout of the parent commit: its default trainer against this tree's")
    ap.add_argument("--skip", default="", help="comma-separated: stages, trainer")
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_patchify needs the GPU (nothing is measured without one)")
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
        cands = {k: (ROOT, k) for k in ("torch", "hip", "hip_all")}
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
                          "hip_all_over_hip": round(med["hip_all"] / med["hip"], 4),
                          "hip_all_over_torch": round(med["hip_all"] / med["torch"], 4),
                          "default_over_parent": round(med["torch"] / med["parent"], 4) if "parent" in med else "not measured"}
        save()
    if "stages" not in skip:
        res["stages"] = {"calls_per_window": a.calls, "repeats": a.repeats,
                         "note": "forward + backward of one downsampling stage through autograd (stage 0 without a data gradient), "
                                 "back-to-back calls on one stream: launch gaps and allocations included; microseconds per call",
                         "shapes": [bench_stage(c, a.repeats, a.calls) for c in STAGES]}
        save()
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])
