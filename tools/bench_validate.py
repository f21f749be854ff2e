#!/usr/bin/env python3
"""Time one validation batch: ``FastSCNN.validate`` against the unfused step (needs the GPU).

    python tools/bench_validate.py [--batches 1,8 --height 1024 --width 2048
                                    --iters 10 --warmup 3 --rounds 3 --only SUBSTRING]

The two arms compute the same two results, the criterion's loss and the SegmentationMetric
counters, on the same eval-mode model, input and target, under ``no_grad``:

    unfused:  outputs = model(x); loss = criterion(outputs, t)
              metric.update(torch.argmax(outputs[0], 1), t)
    fused:    loss = model.validate(x, t, criterion=criterion, metric=metric)

Configurations: batch 1 (the reference's validation batch) and 8 at 3 x 1024 x 2048; 19 classes
with the CE criterion and 2 classes with ``MixDiceLoss``; fp32 and fp16 autocast; aux head off
and on (the criterion's ``aux`` follows the model's).  Per configuration both arms are warmed
up, then timed as alternating blocks (unfused, fused, ..., unfused) of ``--iters`` calls between
two HIP events.  Prints one JSON line: per configuration every block's per-call microseconds,
the medians, the spread between repeated unfused blocks (the noise floor), the route
``validate`` took, both losses and whether the counters agree; ``all_fused_faster`` at the end.
For kernel times run it under ``rocprofv3 --kernel-trace --stats`` with ``--only`` and few rounds.
"""
import argparse
import contextlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def events_ms(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="", help="run the configurations whose name contains this")
    args = ap.parse_args()

    import numpy as np
    import torch
    import _fscnn_boot
    _fscnn_boot.load()
    from fast_scnn_pytorch_amd import arch
    from fast_scnn_pytorch_amd.loss import MixDiceLoss, MixSoftmaxCrossEntropyLoss
    from fast_scnn_pytorch_amd.metric import SegmentationMetric
    from models.fast_scnn import FastSCNN

    if not torch.cuda.is_available():
        raise SystemExit("bench_validate: no GPU visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    H, W = args.height, args.width
    gen = torch.Generator(device=dev).manual_seed(0)
    results = []
    for C, head in ((19, "ce"), (2, "mix_dice")):
        for aux in (False, True):
            model = FastSCNN(C, aux=aux)
            model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in
                                   arch.portable_state_dict(C, aux, 0, "bnrand").items()})
            model = model.to(dev).eval()
            crit = (MixSoftmaxCrossEntropyLoss(aux=aux, aux_weight=0.2) if head == "ce" else
                    MixDiceLoss(aux=aux, aux_weight=0.4))
            for B in [int(b) for b in args.batches.split(",")]:
                x = torch.randn(B, 3, H, W, device=dev, generator=gen)
                if C == 2:  # lane-like: about 10 % ones
                    t = (torch.rand(B, H, W, device=dev, generator=gen) < 0.1).long()
                else:
                    t = torch.randint(0, C, (B, H, W), device=dev, generator=gen)
                    t[:, :, :64] = -1  # ignored pixels
                for prec in ("fp32", "fp16_autocast"):
                    name = "%dx3x%dx%d C=%d %s %s aux=%d" % (B, H, W, C, head, prec, int(aux))
                    if args.only not in name:
                        continue
                    results.append(run_config(args, name, model, crit, x, t, C, prec,
                                              SegmentationMetric))
    print(json.dumps({"tool": "bench_validate", "iters": args.iters, "rounds": args.rounds,
                      "configs": results,
                      "all_fused_faster": all(r["fused_median_us"] < r["unfused_median_us"]
                                              for r in results)}))


def run_config(args, name, model, crit, x, t, C, prec, SegmentationMetric):
    import torch
    last = {}
    metrics = {"unfused": SegmentationMetric(C), "fused": SegmentationMetric(C)}

    def ctx():
        if prec == "fp16_autocast":
            return torch.autocast("cuda", dtype=torch.float16)
        return contextlib.nullcontext()

    def unfused():
        with torch.no_grad(), ctx():
            outputs = model(x)
            last["unfused"] = crit(outputs, t)
            metrics["unfused"].update(torch.argmax(outputs[0], 1), t)

    def fused():
        with ctx():
            last["fused"] = model.validate(x, t, criterion=crit, metric=metrics["fused"])

    peak = {}
    for arm, fn in (("unfused", unfused), ("fused", fused)):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[arm] = torch.cuda.max_memory_allocated() - base
    route = bool(model._last_validate_fused)
    for m in metrics.values():
        m.reset()
    blocks = {"unfused": [], "fused": []}
    for _ in range(args.rounds):
        blocks["unfused"].append(events_ms(unfused, args.iters))
        blocks["fused"].append(events_ms(fused, args.iters))
    blocks["unfused"].append(events_ms(unfused, args.iters))
    # the same number of batches in both metrics before they are compared
    for _ in range(args.iters):
        fused()
    torch.cuda.synchronize()
    u, f = blocks["unfused"], blocks["fused"]
    spread = max(abs(a - b) for a, b in zip(u, u[1:]))
    mu, mf = statistics.median(u), statistics.median(f)
    same = bool((metrics["unfused"].counts() == metrics["fused"].counts()).all())
    return {"config": name, "validate_fused_route": route,
            "unfused_us": [round(v * 1e3, 1) for v in u],
            "fused_us": [round(v * 1e3, 1) for v in f],
            "unfused_median_us": round(mu * 1e3, 1), "fused_median_us": round(mf * 1e3, 1),
            "unfused_pair_spread_us": round(spread * 1e3, 1),
            "gain_us": round((mu - mf) * 1e3, 1),
            "fused_wins_beyond_spread": bool(mu - mf > spread),
            "unfused_peak_MB": round(peak["unfused"] / 2 ** 20, 1),
            "fused_peak_MB": round(peak["fused"] / 2 ** 20, 1),
            "loss_unfused": float(last["unfused"].item()), "loss_fused": float(last["fused"].item()),
            "counters_equal": same}


if __name__ == "__main__":
    main()
