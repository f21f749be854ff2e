#!/usr/bin/env python3
"""Time the fused OHEM train step against the unfused route and the plain CE step (needs the GPU).

    python tools/ohem_head_time.py [--batch 8 --height 1024 --width 2048 --classes 19
                                    --thresh 0.7 --min-kept 256 --no-weight --dtype bf16]

One train step = forward, loss, backward (no optimiser).  The three arms run in the same process
on the same model, input and target, as alternating blocks (unfused, fused, ce, unfused, ...):

    unfused:  criterion(model(x), target).backward()       full-resolution logits + dlogits
    fused:    model.forward_loss_ohem(x, target, criterion).backward()
    ce:       model.forward_loss(x, target).backward()     plain fused cross entropy: the floor

``--thresh`` / ``--min-kept`` choose the branch of the threshold rule: with the defaults
(0.7, 256) a random-init net keeps every labelled pixel and the head's second pass returns at
once; a small ``--thresh`` with a large ``--min-kept`` (0.01, 100000) takes the k-th smallest
probability, so the second pass recomputes loss and gradient.  The JSON line reports the device
threshold and the kept fraction of the fused arm, so the branch taken is on record.

Each block is ``--iters`` steps between two HIP events after ``--warmup`` steps of every arm.
Prints one JSON line: every block's per-step microseconds, the medians, the spread between
repeated unfused blocks (max |difference| of consecutive unfused blocks: the noise floor a gain
has to exceed), the fused step's distance to the CE step (the cost of OHEM) and the peak memory
of one step of each arm.
"""
import argparse
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
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--classes", type=int, default=19)
    ap.add_argument("--thresh", type=float, default=0.7)
    ap.add_argument("--min-kept", type=int, default=256)
    ap.add_argument("--no-weight", action="store_true",
                    help="no class weights (required unless --classes 19)")
    ap.add_argument("--dtype", choices=["bf16", "fp16", "fp32"], default="bf16")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()

    import numpy as np
    import torch
    import _fscnn_boot
    _fscnn_boot.load()
    from fast_scnn_pytorch_amd import arch
    from fast_scnn_pytorch_amd.loss import MixSoftmaxCrossEntropyOHEMLoss
    from models.fast_scnn import FastSCNN

    if not torch.cuda.is_available():
        raise SystemExit("ohem_head_time: no GPU visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    B, H, W, C = args.batch, args.height, args.width, args.classes
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[args.dtype]
    use_weight = not args.no_weight and C == 19
    crit = MixSoftmaxCrossEntropyOHEMLoss(thresh=args.thresh, min_kept=args.min_kept,
                                          use_weight=use_weight)
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, 3, H, W, device=dev, generator=gen).to(dt)
    t = torch.randint(0, C, (B, H, W), device=dev, generator=gen)
    t[torch.rand(B, H, W, device=dev, generator=gen) < 0.1] = -1  # 10 % ignored
    model = FastSCNN(C)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in
                           arch.portable_state_dict(C, seed=0).items()})
    model = model.to(dev).train()
    last = {}

    def unfused():
        model.zero_grad(set_to_none=True)
        loss = crit(model(x), t)
        loss.backward()
        last["unfused"] = loss

    def fused():
        model.zero_grad(set_to_none=True)
        loss = model.forward_loss_ohem(x, t, crit)
        loss.backward()
        last["fused"] = loss

    def ce():
        model.zero_grad(set_to_none=True)
        loss = model.forward_loss(x, t)
        loss.backward()
        last["ce"] = loss

    arms = (("unfused", unfused), ("fused", fused), ("ce", ce))
    peak = {}
    for name, fn in arms:
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
    # the branch the fused arm takes, read once outside the timed blocks
    model._keep_ws = True
    fused()
    torch.cuda.synchronize()
    dbg = model._debug["ohem"]
    thr = float(dbg["thr"].item())
    labelled = int(dbg["counts"][0].item())
    kept = int(((dbg["prob"] <= dbg["thr"]) & (dbg["prob"] < 1.5)).sum().item())
    model._keep_ws = False
    model._debug = None
    del dbg
    blocks = {name: [] for name, _ in arms}
    for _ in range(args.rounds):
        for name, fn in arms:
            blocks[name].append(events_ms(fn, args.iters))
    blocks["unfused"].append(events_ms(unfused, args.iters))
    u, f, c = blocks["unfused"], blocks["fused"], blocks["ce"]
    spread = max(abs(a - b) for a, b in zip(u, u[1:]))
    mu, mf, mc = statistics.median(u), statistics.median(f), statistics.median(c)
    print(json.dumps({
        "shape": "%dx3x%dx%d %s, %d classes, OHEM(thresh=%g, min_kept=%d, weights %s)"
                 % (B, H, W, args.dtype, C, args.thresh, args.min_kept,
                    "on" if use_weight else "off"),
        "device_threshold": thr, "labelled": labelled, "kept": kept,
        "second_pass": "skipped" if thr == float(np.float32(args.thresh)) else "recomputes",
        "unfused_us": [round(v * 1e3, 1) for v in u], "fused_us": [round(v * 1e3, 1) for v in f],
        "ce_us": [round(v * 1e3, 1) for v in c],
        "unfused_median_us": round(mu * 1e3, 1), "fused_median_us": round(mf * 1e3, 1),
        "ce_median_us": round(mc * 1e3, 1),
        "unfused_pair_spread_us": round(spread * 1e3, 1),
        "gain_us": round((mu - mf) * 1e3, 1),
        "fused_wins_beyond_spread": bool(mu - mf > spread),
        "ohem_cost_over_ce_us": round((mf - mc) * 1e3, 1),
        "unfused_step_peak_MB": round(peak["unfused"] / 2 ** 20, 1),
        "fused_step_peak_MB": round(peak["fused"] / 2 ** 20, 1),
        "ce_step_peak_MB": round(peak["ce"] / 2 ** 20, 1),
        "loss_unfused": round(float(last["unfused"].item()), 6),
        "loss_fused": round(float(last["fused"].item()), 6),
        "loss_ce": round(float(last["ce"].item()), 6)}))


if __name__ == "__main__":
    main()
