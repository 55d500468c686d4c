"""Measures the QAT weight quantisers (ops.qat_weight, csrc/qat.hip) -> profiles/qat.json.

  kernels    one forward call and one backward call over the seven decoder weights of HNeRV-3M, 'ffnerv' (1 + 1 launches) and
             'hinerv' with noise (2 + 2 launches), against the same arithmetic written in PyTorch ops (the reference's
             QATQuantizer.forward under autograd, tensor by tensor), in one process, alternating inside every repeat
  trainer    steps/s of the trainer's step on HNeRV-3M (640 x 1280, B = 2, l2, --enc_kernels hip_all) with --qat off, ffnerv
             and hinerv, and, with --parent_tree DIR (a checkout of the parent commit; it runs on this tree's libnqhip.so through
             NQ_LIB, the ABI is additive), of the parent's trainer: one fresh child process per run, the candidates alternating;
             the spread of the runs of one candidate is the run-to-run spread the others are read against

    python tools/bench_qat.py [--out profiles/qat.json] [--repeats 9] [--calls 50] [--steps 300] [--rounds 3] [--bits 6]
                              [--parent_tree DIR] [--skip kernels,trainer]

Kernels: HIP events around `calls` back-to-back calls on one stream (launch gaps and allocations included, the same for both
sides), median over `repeats` windows after a warm-up of each: durations per CALL; a call's single launches are not timed apart.
Trainer: host clock between two device synchronisations, steps 20 .. `steps` of a run.  Recorded, not asserted.  Prints ONE JSON
object and writes it to --out.  Needs the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spread(v, digits=1):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits), "runs": len(v)}


def trainer_child(root, qat, steps, bits):
    """one trainer run of the tree at `root` -> prints its steps/s"""
    sys.path[:0] = [root, os.path.join(root, "tools")]
    import torch
    from bench import HNERV_3M
    from neuroquant_amd.methods import regress
    from neuroquant_amd.methods.calibrate_network import seed_all
    from neuroquant_amd.models import HNeRV
    from neuroquant_amd.utils import CacheLoader, FrameCache
    frames = torch.randint(0, 256, (8, 3, 640, 1280), device="cuda", dtype=torch.uint8, generator=torch.Generator(device="cuda").manual_seed(1))
    seed_all(903)
    args = regress.parse_args(["--arch", "hnerv"])
    args.lr = 1e-3
    loader = CacheLoader(FrameCache(frames), list(range(8)), 2, seed=903)
    model = HNeRV(dict(HNERV_3M, enc_kernels="hip_all")).to("cuda").train()
    if qat not in ("off", "parent"):
        model.weight_qat = regress.WeightQAT(model, qat, bits, 903)
    opt = torch.optim.Adam(model.parameters(), weight_decay=0.)
    done, marks, first = 0, {}, 20
    while done < steps:
        for sample in loader:
            regress.adjust_lr(opt, done / steps, args)
            img = sample["img"]
            loss = regress.step_loss(model(img)[0], img, None)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            done += 1
            if done in (first, steps):
                torch.cuda.synchronize()
                marks[done] = time.perf_counter()
            if done == steps:
                break
    print(json.dumps({"steps_per_s": (steps - first) / (marks[steps] - marks[first])}))


def trainer_run(root, qat, steps, bits):
    env = dict(os.environ, NQ_LIB=os.path.join(ROOT, "neuroquant_amd", "libnqhip.so"))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, qat, str(steps), str(bits)], env=env, check=True,
                         capture_output=True, text=True, timeout=600).stdout
    return json.loads(out.strip().splitlines()[-1])["steps_per_s"]


def torch_qat(w, bits, mode):
    """QATQuantizer.forward of the reference on PyTorch ops (noise on)"""
    import torch
    if mode == "ffnerv":
        t, n = torch.tanh(w), float(2 ** (bits - 1) - 1)
        q = torch.floor(t.abs() * n) / n * torch.sign(t)
        return t + (q - t).detach()                      # qfn: straight-through
    s = 2 * w.abs().max(dim=0, keepdim=True)[0] / (2. ** bits - 1.) + 1e-6
    q = torch.round(w / s).clamp(-2 ** (bits - 1), 2 ** (bits - 1) - 1).detach()
    m = (torch.rand_like(w) > 0.9).to(w.dtype)
    return w * m + q * s * (1. - m)


def bench_kernels(mode, bits, repeats, calls):
    import torch
    sys.path.insert(0, ROOT)
    from bench import HNERV_3M
    from neuroquant_amd import ops
    from neuroquant_amd.models import HNeRV
    torch.manual_seed(0)
    model = HNeRV(HNERV_3M).cuda()
    ws = [p.detach().clone().requires_grad_(True) for n, p in model.named_parameters() if not n.startswith("encoder") and p.dim() == 4]
    gs = [torch.randn_like(w) for w in ws]
    step = torch.ones(1, dtype=torch.int32, device="cuda")
    sides = {"hip": lambda: ops.qat_weight(ws, bits, mode, True, 903, step), "torch": lambda: [torch_qat(w, bits, mode) for w in ws]}

    def window_us(fn, backward):
        ys = fn() if backward else None
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(calls):
            if backward:
                torch.autograd.grad(ys, ws, gs, retain_graph=True)
            else:
                with torch.no_grad():
                    fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / calls

    t = {(k, d): [] for k in sides for d in ("forward", "backward")}
    for r in range(repeats + 1):                          # the first round warms up
        for (k, d), v in t.items():
            us = window_us(sides[k], d == "backward")
            if r:
                v.append(us)
    return {"shapes": [list(w.shape) for w in ws], "elements": sum(w.numel() for w in ws),
            "launches_per_call": {"forward": 1 + (mode == "hinerv"), "backward": 1 + (mode == "hinerv")},
            "us_per_call": {f"{k}_{d}": spread(v) for (k, d), v in t.items()},
            "hip_over_torch_time": {d: round(statistics.median(t["hip", d]) / statistics.median(t["torch", d]), 3) for d in ("forward", "backward")}}


def main(argv):
    if argv[:1] == ["--child"]:
        return trainer_child(argv[1], argv[2], int(argv[3]), int(argv[4]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qat.json"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bits", type=int, default=6)
    ap.add_argument("--parent_tree", default=None, help="a checkout of the parent commit: its default trainer against this tree's")
    ap.add_argument("--skip", default="", help="comma-separated: kernels, trainer")
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_qat needs the GPU (nothing is measured without one)")
    skip = set(filter(None, a.skip.split(",")))
    res = {}
    if os.path.exists(a.out):                    # sections measured by an earlier call are kept
        with open(a.out) as fh:
            res = json.load(fh)
    res["device"] = torch.cuda.get_device_name(0)
    res["not_measured"] = "the launches of a call apart from each other; equal-step trainings against post-training rounding"

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)

    if "trainer" not in skip:                    # child processes first, before this process holds the GPU
        cands = {"off": ROOT, "ffnerv": ROOT, "hinerv": ROOT}
        if a.parent_tree:
            cands["parent"] = os.path.abspath(a.parent_tree)
        rates = {k: [] for k in cands}
        for _ in range(a.rounds):
            for k, root in cands.items():
                rates[k].append(trainer_run(root, k, a.steps, a.bits))
        med = {k: statistics.median(v) for k, v in rates.items()}
        res["trainer"] = {"note": "HNeRV-3M 640x1280: model + step_loss + backward + Adam at B = 2, l2, enc_kernels hip_all, %d bits, steps "
                                  "20 .. %d of a run, one process per run, %d runs per candidate, alternating" % (a.bits, a.steps, a.rounds),
                          "steps_per_s": {k: spread(v) for k, v in rates.items()},
                          "ffnerv_over_off": round(med["ffnerv"] / med["off"], 4), "hinerv_over_off": round(med["hinerv"] / med["off"], 4),
                          "default_over_parent": round(med["off"] / med["parent"], 4) if "parent" in med else "not measured"}
        save()
    if "kernels" not in skip:
        res["kernels"] = {"calls_per_window": a.calls, "repeats": a.repeats, "bits": a.bits,
                          "note": "one call over the seven HNeRV-3M decoder weights, back-to-back calls on one stream: launch gaps and "
                                  "allocations included; microseconds per call (backward: through autograd)",
                          "ffnerv": bench_kernels("ffnerv", a.bits, a.repeats, a.calls),
                          "hinerv": bench_kernels("hinerv", a.bits, a.repeats, a.calls)}
        save()
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])
