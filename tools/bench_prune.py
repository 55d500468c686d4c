"""Measures the magnitude-pruning baseline (ops.magnitude_select / prune_mask / prune_apply_, csrc/prune.hip)
-> profiles/prune.json.

  kernels    select + mask + apply over the seven decoder weights of HNeRV-3M (one list, 2.64 M elements, ratio 0.4) against
             torch.kthvalue of the concatenated magnitudes plus masking on PyTorch ops (which reads the threshold's tensor on
             the device but breaks ties arbitrarily), in one process, alternating inside every repeat; and the select, the mask
             and the apply (with gradient and both Adam moments) apart
  trainer    steps/s of the trainer's step on HNeRV-3M (640 x 1280, B = 2, l2, --enc_kernels hip_all) without and with
             --prune_ratio 0.4, and, with --parent_tree DIR (a checkout of the parent commit; it runs on this tree's libnqhip.so
             through NQ_LIB, the ABI is additive), of the parent's trainer: one fresh child process per run, the candidates
             alternating; the spread of the runs of one candidate is the run-to-run spread the others are read against, and the
             default path counts as unchanged when the ranges of 'off' and 'parent' overlap

    python tools/bench_prune.py [--out profiles/prune.json] [--repeats 9] [--calls 50] [--steps 300] [--rounds 3]
                                [--parent_tree DIR] [--skip kernels,trainer]

Kernels: HIP events around `calls` back-to-back calls on one stream (launch gaps and allocations included, the same for both
sides), median over `repeats` windows after a warm-up of each.  Trainer: host clock between two device synchronisations, steps
20 .. `steps` of a run.  Recorded, not asserted.  Prints ONE JSON object and writes it to --out.  Needs the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIO = 0.4
NOT_MEASURED = ("packed and rans file bytes and PSNR of the trained fixture after pruning at 0.2 / 0.4 / 0.6 and a short fine-tune; how "
                "many pruned weights are still at their zero level after calibrate_network; the launches of a call apart from each "
                "other; the first call of a window, on the dense list, apart from the calls on the pruned one")


def spread(v, digits=1):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits), "runs": len(v)}


def trainer_child(root, mode, steps):
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
    args = regress.parse_args(["--arch", "hnerv"] + (["--prune_ratio", str(RATIO)] if mode == "prune" else []))
    args.lr = 1e-3
    loader = CacheLoader(FrameCache(frames), list(range(8)), 2, seed=903)
    model = HNeRV(dict(HNERV_3M, enc_kernels="hip_all")).to("cuda").train()
    pruner = regress.prune_model(model, args) if mode == "prune" else None
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
            if pruner is not None:
                pruner.hold(opt)
            done += 1
            if done in (first, steps):
                torch.cuda.synchronize()
                marks[done] = time.perf_counter()
            if done == steps:
                break
    print(json.dumps({"steps_per_s": (steps - first) / (marks[steps] - marks[first])}))


def trainer_run(root, mode, steps):
    env = dict(os.environ, NQ_LIB=os.path.join(ROOT, "neuroquant_amd", "libnqhip.so"))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, mode, str(steps)], env=env, check=True,
                         capture_output=True, text=True, timeout=600).stdout
    return json.loads(out.strip().splitlines()[-1])["steps_per_s"]


def bench_kernels(repeats, calls):
    import torch
    sys.path.insert(0, ROOT)
    from bench import HNERV_3M
    from neuroquant_amd import ops
    from neuroquant_amd.models import HNeRV
    torch.manual_seed(0)
    model = HNeRV(HNERV_3M).cuda()
    dense = [p.detach().clone() for n, p in model.named_parameters() if not n.startswith("encoder") and p.dim() == 4]
    ws = [w.clone() for w in dense]
    comp = [[torch.randn_like(w) for w in ws] for _ in range(3)]
    n = sum(w.numel() for w in ws)
    k = int(RATIO * n)
    sel = ops.magnitude_select(ws, k)
    mask = ops.prune_mask(ws, sel)

    def torch_prune():
        thr = torch.kthvalue(torch.cat([w.reshape(-1) for w in ws]).abs(), k)[0]
        for w in ws:
            w.mul_(w.abs() > thr)

    def restore():                                # every window prunes the same dense weights
        for w, d in zip(ws, dense):
            w.copy_(d)

    sides = {"hip_select_mask_apply": lambda: ops.magnitude_prune_(ws, RATIO), "torch_kthvalue_mask": torch_prune,
             "hip_select": lambda: ops.magnitude_select(ws, k), "hip_mask": lambda: ops.prune_mask(ws, sel),
             "hip_apply_with_grad_and_moments": lambda: ops.prune_apply_(ws, mask, *comp)}

    def window_us(fn):
        restore()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(calls):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / calls

    t = {key: [] for key in sides}
    for r in range(repeats + 1):                  # the first round warms up
        for key, v in t.items():
            us = window_us(sides[key])
            if r:
                v.append(us)
    return {"shapes": [list(w.shape) for w in ws], "elements": n, "k": k, "run": ops.L.lib().nq_prune_run(),
            "launches_per_call": {"select": 8, "mask": 3, "apply": 1},
            "us_per_call": {key: spread(v) for key, v in t.items()},
            "hip_over_torch_time": round(statistics.median(t["hip_select_mask_apply"]) / statistics.median(t["torch_kthvalue_mask"]), 3),
            "note": "after the first call of a window the list is already pruned: 40 % of it ties at magnitude 0, the dominating bin"}


def main(argv):
    if argv[:1] == ["--child"]:
        return trainer_child(argv[1], argv[2], int(argv[3]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prune.json"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent_tree", default=None, help="a checkout of the parent commit: its default trainer against this tree's")
    ap.add_argument("--skip", default="", help="comma-separated: kernels, trainer")
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_prune needs the GPU (nothing is measured without one)")
    skip = set(filter(None, a.skip.split(",")))
    res = {}
    if os.path.exists(a.out):                    # sections measured by an earlier call are kept
        with open(a.out) as fh:
            res = json.load(fh)
    res["device"] = torch.cuda.get_device_name(0)
    res["not_measured"] = NOT_MEASURED

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)

    if "trainer" not in skip:                    # child processes first, before this process holds the GPU
        cands = {"off": ROOT, "prune": ROOT}
        if a.parent_tree:
            cands["parent"] = os.path.abspath(a.parent_tree)
        rates = {key: [] for key in cands}
        for _ in range(a.rounds):
            for key, root in cands.items():
                rates[key].append(trainer_run(root, key, a.steps))
        med = {key: statistics.median(v) for key, v in rates.items()}
        tr = {"note": "HNeRV-3M 640x1280: model + step_loss + backward + Adam (+ the mask held) at B = 2, l2, enc_kernels hip_all, steps "
                      "20 .. %d of a run, one process per run, %d runs per candidate, alternating" % (a.steps, a.rounds),
              "prune_ratio": RATIO, "steps_per_s": {key: spread(v) for key, v in rates.items()},
              "spread_of_off_percent": round(100 * (max(rates["off"]) - min(rates["off"])) / med["off"], 2),
              "prune_over_off": round(med["prune"] / med["off"], 4)}
        if "parent" in med:
            tr["default_over_parent"] = round(med["off"] / med["parent"], 4)
            tr["default_ranges_overlap_parent"] = min(rates["off"]) <= max(rates["parent"]) and min(rates["parent"]) <= max(rates["off"])
        else:
            tr["default_over_parent"] = "not measured"
        res["trainer"] = tr
        save()
    if "kernels" not in skip:
        res["kernels"] = dict(bench_kernels(a.repeats, a.calls), calls_per_window=a.calls, repeats=a.repeats, ratio=RATIO)
        save()
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])
