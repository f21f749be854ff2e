#!/usr/bin/env python3
"""Time the overlay tail of the deployment pipeline (needs the GPU).

    python tools/overlay_time.py [--iters 20 --warmup 3 --rounds 3 --limit 240
                                  --md profiles/overlay_time.md]

uint8 NHWC camera frames, base 1024, 2 classes, fp16 arithmetic, ``input_size`` 640 x 360, the
reference's green at alpha 0.5.  Configurations: 640 x 360 frames at batch 1 and 8 (frame and mask
of one size), and 1920 x 1080 frames at batch 1 (the mask is resized to the frame).  Three arms
produce the overlay:

    fused:  e2e.overlay(frames, fused=True)      front end, backbone, one overlay launch
    two:    e2e.overlay(frames, fused=False)     ... e2e_head (the mask), fscnn_overlay_mask
    torch:  e2e.predict(frames, 255), then full-frame torch ops: (index for the resize,) compare,
            where, multiply, add, round, clamp, cast

Every configuration runs in a process of its own under ``--limit`` seconds (this process never
opens the GPU); in it the arms are warmed up and then timed in interleaved rounds (fused, two,
torch, fused, ...), ``--iters`` calls per block between two HIP events.  Prints one JSON line;
``--md`` also writes the table.  Nothing is asserted on the timings.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
W, H, BASE = 640, 360, 1024
CONFIGS = {"640x360_b1": (1, 640, 360), "640x360_b8": (8, 640, 360), "1920x1080_b1": (1, 1920, 1080)}


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


def child(args):
    import numpy as np
    import torch
    import torch.nn.functional as F
    import _fscnn_boot
    _fscnn_boot.load()
    from fast_scnn_pytorch_amd import arch
    from fast_scnn_pytorch_amd.deploy import EndToEndFastSCNN
    from models.fast_scnn import FastSCNN

    if not torch.cuda.is_available():
        raise SystemExit("overlay_time: no GPU visible")
    B, w, h = CONFIGS[args.child]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    gen = torch.Generator(device=dev).manual_seed(0)
    model = FastSCNN(2)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in
                           arch.portable_state_dict(2, False, 0, "bnrand").items()})
    model = model.to(dev).eval()
    e2e = EndToEndFastSCNN(model, (W, H), BASE, MEAN, STD, dtype=torch.float16, channels_last=True)
    e2e.preprocessor.to(dev)
    e2e.eval()
    # smooth frames: a coarse random image enlarged, like a camera frame's low frequencies
    coarse = torch.rand(B, 3, 9, 16, device=dev, generator=gen) * 255
    frames = F.interpolate(coarse, size=(h, w), mode="bicubic", align_corners=False)
    frames = frames.clamp(0, 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    green = torch.tensor([0, 255, 0], dtype=torch.uint8, device=dev)
    zero = torch.zeros((), dtype=torch.uint8, device=dev)
    sy = (torch.arange(h, device=dev) * H) // h
    sx = (torch.arange(w, device=dev) * W) // w
    last = {}

    def fused():
        last["fused"] = e2e.overlay(frames, fused=True)

    def two():
        last["two"] = e2e.overlay(frames, fused=False)

    def torch_ops():
        mask = e2e.predict(frames, scale=255)
        if (h, w) != (H, W):
            mask = mask[:, sy[:, None], sx[None, :]]
        colour = torch.where((mask != 0)[..., None], green, zero)
        t = frames.float() * 1.0 + colour.float() * 0.5
        last["torch"] = t.round().clamp(0, 255).to(torch.uint8)

    arms = (("fused", fused), ("two", two), ("torch", torch_ops))
    routes = {}
    for a, fn in arms:
        for _ in range(args.warmup):
            fn()
        routes[a] = bool(e2e._last_fused)
    blocks = {a: [] for a, _ in arms}
    for _ in range(args.rounds):
        for a, fn in arms:
            blocks[a].append(events_ms(fn, args.iters))
    e2e.overlay(frames)
    r = {"config": args.child, "batch": B, "frame": "%dx%d" % (w, h),
         "default_route": "fused" if e2e._last_fused else "two",
         "fused_arm_ran_fused": routes["fused"],
         "coloured_share": round(float((last["two"] != frames).any(-1).float().mean()), 3),
         "arms_identical": bool(torch.equal(last["fused"], last["two"])
                                and torch.equal(last["two"], last["torch"])),
         "two_spread_us": round((max(blocks["two"]) - min(blocks["two"])) * 1e3, 1)}
    for a in blocks:
        r[a + "_us"] = [round(v * 1e3, 1) for v in blocks[a]]
        r[a + "_median_us"] = round(statistics.median(blocks[a]) * 1e3, 1)
    print("RESULT " + json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds per configuration's process")
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--md", default="")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    results = []
    for name in args.configs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--iters",
               str(args.iters), "--warmup", str(args.warmup), "--rounds", str(args.rounds)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit("overlay_time: %s ran past %d s; nothing more is started"
                             % (name, args.limit))
        line = [s for s in p.stdout.splitlines() if s.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit("overlay_time: %s ended with status %d; nothing more is started"
                             % (name, p.returncode))
        results.append(json.loads(line[0][7:]))
        print("# " + json.dumps(results[-1]), flush=True)
    print(json.dumps({"tool": "overlay_time", "iters": args.iters, "rounds": args.rounds,
                      "configs": results}))
    if args.md:
        lines = ["# Overlay tail: fused against two launches against torch ops", "",
                 "`tools/overlay_time.py`: uint8 NHWC frames, base 1024, `input_size` 640 x 360, 2 "
                 "classes, fp16, green at alpha 0.5; medians of %d interleaved rounds of %d calls, "
                 "whole pipeline per call, microseconds." % (args.rounds, args.iters), "",
                 "| batch | frame | fused | two launches | spread of two | predict + torch ops | "
                 "default route | arms identical |", "|---|---|---|---|---|---|---|---|"]
        for r in results:
            lines.append("| %d | %s | %.1f | %.1f | %.1f | %.1f | %s | %s |" % (
                r["batch"], r["frame"], r["fused_median_us"], r["two_median_us"],
                r["two_spread_us"], r["torch_median_us"], r["default_route"],
                "yes" if r["arms_identical"] else "no"))
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
