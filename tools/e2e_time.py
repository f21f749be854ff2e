#!/usr/bin/env python3
"""Time the deployment pipeline: ``EndToEndFastSCNN`` against the unfused composition (needs the
GPU).

    python tools/e2e_time.py [--batches 1,8 --iters 20 --warmup 5 --rounds 3 --only SUBSTRING]

Both arms take the same uint8 frames, 640 x 360, through base 1024 back to 640 x 360, on the same
eval-mode model with the ImageNet mean / std, under ``no_grad``:

    unfused:  x = F.interpolate(frames.float(), (1024, 1024), bilinear, align_corners=False)
              x = ((x / 255 - mean) / std).to(dtype)
              y = F.interpolate(model(x)[0], (360, 640), bilinear, align_corners=False)
              p = F.softmax(y, 1)                       # what the pieces before this module offer
    fused:    p = e2e(frames)
    predict:  mask = e2e.predict(frames, scale=255)     # against p.argmax(1) * 255 of the unfused arm

Configurations: fp16 and fp32, 2 and 19 classes, batch 1 and 8.  Per configuration the arms are
warmed up, then timed as alternating blocks (unfused, fused, predict, ..., unfused) of ``--iters``
calls between two HIP events.  Prints one JSON line: per configuration every block's per-call
microseconds, the medians, the spread between repeated unfused blocks (the noise floor), the peak
memory of one call of each arm and the largest difference between the two arms' probabilities.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
W, H, BASE = 640, 360, 1024


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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="", help="run the configurations whose name contains this")
    args = ap.parse_args()

    import numpy as np
    import torch
    import torch.nn.functional as F
    import _fscnn_boot
    _fscnn_boot.load()
    from fast_scnn_pytorch_amd import arch
    from fast_scnn_pytorch_amd.deploy import EndToEndFastSCNN
    from models.fast_scnn import FastSCNN

    if not torch.cuda.is_available():
        raise SystemExit("e2e_time: no GPU visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    gen = torch.Generator(device=dev).manual_seed(0)
    mean = torch.tensor(MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(STD, device=dev).view(1, 3, 1, 1)
    results = []
    for C in (2, 19):
        model = FastSCNN(C)
        model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in
                               arch.portable_state_dict(C, False, 0, "bnrand").items()})
        model = model.to(dev).eval()
        for B in [int(b) for b in args.batches.split(",")]:
            # smooth frames: a coarse random image enlarged, like a camera frame's low frequencies
            coarse = torch.rand(B, 3, 9, 16, device=dev, generator=gen) * 255
            frames = F.interpolate(coarse, size=(H, W), mode="bicubic",
                                   align_corners=False).clamp(0, 255).round().to(torch.uint8)
            for dt, prec in ((torch.float16, "fp16"), (torch.float32, "fp32")):
                name = "%dx3x%dx%d -> %d^2 -> %dx%d C=%d %s" % (B, H, W, BASE, W, H, C, prec)
                if args.only not in name:
                    continue
                e2e = EndToEndFastSCNN(model, (W, H), BASE, MEAN, STD, dtype=dt)
                e2e.preprocessor.to(dev)
                e2e.eval()
                last = {}

                def unfused():
                    with torch.no_grad():
                        x = F.interpolate(frames.float(), size=(BASE, BASE), mode="bilinear",
                                          align_corners=False)
                        x = ((x / 255.0 - mean) / std).to(dt)
                        y = F.interpolate(model(x)[0], size=(H, W), mode="bilinear",
                                          align_corners=False)
                        last["unfused"] = F.softmax(y, 1)

                def fused():
                    last["fused"] = e2e(frames)

                def predict():
                    last["predict"] = e2e.predict(frames, scale=255)

                results.append(run_config(args, name, unfused, fused, predict, last, e2e))
    print(json.dumps({"tool": "e2e_time", "iters": args.iters, "rounds": args.rounds,
                      "configs": results,
                      "all_fused_faster": all(r["fused_median_us"] < r["unfused_median_us"]
                                              for r in results)}))


def run_config(args, name, unfused, fused, predict, last, e2e):
    import torch
    arms = (("unfused", unfused), ("fused", fused), ("predict", predict))
    peak = {}
    for arm, fn in arms:
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[arm] = torch.cuda.max_memory_allocated() - base
    route = bool(e2e._last_fused)
    blocks = {arm: [] for arm, _ in arms}
    for _ in range(args.rounds):
        for arm, fn in arms:
            blocks[arm].append(events_ms(fn, args.iters))
    blocks["unfused"].append(events_ms(unfused, args.iters))
    u = blocks["unfused"]
    spread = max(abs(a - b) for a, b in zip(u, u[1:]))
    med = {arm: statistics.median(v) for arm, v in blocks.items()}
    pu, pf = last["unfused"].float(), last["fused"].float()
    mask_u = (pu.argmax(1) * 255).to(torch.uint8)
    out = {"config": name, "fused_route": route}
    for arm, _ in arms:
        out[arm + "_us"] = [round(v * 1e3, 1) for v in blocks[arm]]
        out[arm + "_median_us"] = round(med[arm] * 1e3, 1)
        out[arm + "_peak_MB"] = round(peak[arm] / 2 ** 20, 1)
    out.update({"unfused_pair_spread_us": round(spread * 1e3, 1),
                "gain_us": round((med["unfused"] - med["fused"]) * 1e3, 1),
                "fused_wins_beyond_spread": bool(med["unfused"] - med["fused"] > spread),
                "max_abs_prob_diff": float((pu - pf).abs().max().item()),
                "mask_disagreement": float((mask_u != last["predict"]).float().mean().item())})
    return out


if __name__ == "__main__":
    main()
