#!/usr/bin/env python3
"""Time the fused Dice / Focal+Dice train step against the unfused route (needs the GPU).

    python tools/dice_head_time.py [--batch 8 --height 1024 --width 2048 --classes 19
                                    --criterion dice|mix_dice|focal_dice --dtype bf16]

One train step = forward, loss, backward (no optimiser).  The two arms run in the same process on
the same model, input and target, as alternating blocks (unfused, fused, unfused, fused, ...):

    unfused:  criterion(model(x)[0], target).backward()      full-resolution logits + dlogits
    fused:    model.forward_loss(x, target, criterion=criterion).backward()

Each block is ``--iters`` steps between two HIP events after ``--warmup`` steps of both arms.
Prints one JSON line: every block's per-step microseconds, the medians, the spread between
repeated unfused blocks (max |difference| of consecutive unfused blocks: the noise floor a gain
has to exceed) and the peak memory of one step of each arm.
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
    ap.add_argument("--criterion", choices=["dice", "mix_dice", "focal_dice"], default="dice")
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
    from fast_scnn_pytorch_amd.loss import DiceLoss, FocalDiceLoss, MixDiceLoss
    from models.fast_scnn import FastSCNN

    if not torch.cuda.is_available():
        raise SystemExit("dice_head_time: no GPU visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    B, H, W, C = args.batch, args.height, args.width, args.classes
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[args.dtype]
    crit = {"dice": DiceLoss(), "mix_dice": MixDiceLoss(aux=False),
            "focal_dice": FocalDiceLoss()}[args.criterion]
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, 3, H, W, device=dev, generator=gen).to(dt)
    if C == 2:  # lane-like: about 10 % ones
        t = (torch.rand(B, H, W, device=dev, generator=gen) < 0.1).long()
    else:
        t = torch.randint(0, C, (B, H, W), device=dev, generator=gen)
    model = FastSCNN(C)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in
                           arch.portable_state_dict(C, seed=0).items()})
    model = model.to(dev).train()
    last = {}

    def unfused():
        model.zero_grad(set_to_none=True)
        loss = crit(model(x)[0], t)
        loss.backward()
        last["unfused"] = loss

    def fused():
        model.zero_grad(set_to_none=True)
        loss = model.forward_loss(x, t, criterion=crit)
        loss.backward()
        last["fused"] = loss

    peak = {}
    for name, fn in (("unfused", unfused), ("fused", fused)):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
    blocks = {"unfused": [], "fused": []}
    for _ in range(args.rounds):
        blocks["unfused"].append(events_ms(unfused, args.iters))
        blocks["fused"].append(events_ms(fused, args.iters))
    blocks["unfused"].append(events_ms(unfused, args.iters))
    u, f = blocks["unfused"], blocks["fused"]
    spread = max(abs(a - b) for a, b in zip(u, u[1:]))
    mu, mf = statistics.median(u), statistics.median(f)
    print(json.dumps({
        "shape": "%dx3x%dx%d %s, %d classes, %s" % (B, H, W, args.dtype, C, args.criterion),
        "unfused_us": [round(v * 1e3, 1) for v in u], "fused_us": [round(v * 1e3, 1) for v in f],
        "unfused_median_us": round(mu * 1e3, 1), "fused_median_us": round(mf * 1e3, 1),
        "unfused_pair_spread_us": round(spread * 1e3, 1),
        "gain_us": round((mu - mf) * 1e3, 1),
        "fused_wins_beyond_spread": bool(mu - mf > spread),
        "unfused_step_peak_MB": round(peak["unfused"] / 2 ** 20, 1),
        "fused_step_peak_MB": round(peak["fused"] / 2 ** 20, 1),
        "loss_unfused": round(float(last["unfused"].item()), 6),
        "loss_fused": round(float(last["fused"].item()), 6)}))


if __name__ == "__main__":
    main()
