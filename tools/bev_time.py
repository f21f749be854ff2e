#!/usr/bin/env python3
"""Time the bird's-eye tail of the deployment pipeline (needs the GPU).

    python tools/bev_time.py [--batches 1,8 --ppu 1,5,20 --iters 20 --warmup 3 --rounds 3
                              --md profiles/bev_time.md]

640 x 360 uint8 frames, base 1024, 2 classes, fp16 arithmetic, the corrected calibration's
full-image view at ``--ppu`` pixels per cm (208 x 108, 1043 x 542, 4173 x 2168), ``min_width`` 10.
Three arms produce the bird's-eye mask and the row table:

    fused:  e2e.bird_eye(frames, view, fused=True)      front end, backbone, one bird's-eye launch
    two:    e2e.bird_eye(frames, view, fused=False)     ... e2e_head (frame mask), fscnn_bev_mask
    host:   e2e.predict(frames, 255).cpu() -> the float64 numpy warp and row table of
            tests/bev_ref.py  (the reference's route: mask off the device, warp and scan on the
            host; OpenCV and the per-pixel Python loop are not reproduced, numpy stands in)

Per configuration the arms are warmed up and then timed in interleaved rounds in one process
(fused, two, host, fused, two, ...), ``--iters`` calls per block between two HIP events (wall
clock and fewer calls for the host arm).  Prints one JSON line; ``--md`` also writes the table.
``not slower``: the fused median is not above the two-launch median by more than the spread of
the two-launch arm's own rounds.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
W, H, BASE, MIN_WIDTH = 640, 360, 1024, 10


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


def wall_ms(fn, iters):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--ppu", default="1,5,20")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-iters", type=int, default=1)
    ap.add_argument("--md", default="")
    args = ap.parse_args()

    import numpy as np
    import torch
    import torch.nn.functional as F
    import _fscnn_boot
    _fscnn_boot.load()
    import bev_ref
    from fast_scnn_pytorch_amd import arch, bev
    from fast_scnn_pytorch_amd.deploy import EndToEndFastSCNN
    from models.fast_scnn import FastSCNN

    if not torch.cuda.is_available():
        raise SystemExit("bev_time: no GPU visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    gen = torch.Generator(device=dev).manual_seed(0)
    model = FastSCNN(2)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in
                           arch.portable_state_dict(2, False, 0, "bnrand").items()})
    model = model.to(dev).eval()
    e2e = EndToEndFastSCNN(model, (W, H), BASE, MEAN, STD, dtype=torch.float16)
    e2e.preprocessor.to(dev)
    e2e.eval()
    view = bev.BirdEyeView()
    results = []
    for B in [int(b) for b in args.batches.split(",")]:
        coarse = torch.rand(B, 3, 9, 16, device=dev, generator=gen) * 255
        frames = F.interpolate(coarse, size=(H, W), mode="bicubic",
                               align_corners=False).clamp(0, 255).round().to(torch.uint8)
        for ppu in [int(p) for p in args.ppu.split(",")]:
            (wb, hb), _, _, vp = view.params(ppu, 0.1, True, source_size=(W, H))
            m = bev.inverse_map(vp)
            last = {}

            def fused():
                last["fused"] = e2e.bird_eye(frames, vp, 255, MIN_WIDTH, fused=True)

            def two():
                last["two"] = e2e.bird_eye(frames, vp, 255, MIN_WIDTH, fused=False)

            def host():
                mask = e2e.predict(frames, scale=255).cpu().numpy()
                out = bev_ref.warp(mask, m, hb, wb)
                last["host"] = (out, bev_ref.row_table(out, MIN_WIDTH))

            arms = (("fused", fused, events_ms, args.iters), ("two", two, events_ms, args.iters),
                    ("host", host, wall_ms, args.host_iters))
            for _, fn, _, _ in arms[:2]:
                for _ in range(args.warmup):
                    fn()
            blocks = {a: [] for a, _, _, _ in arms}
            for _ in range(args.rounds):
                for a, fn, timer, iters in arms:
                    blocks[a].append(timer(fn, iters))
            med = {a: statistics.median(v) for a, v in blocks.items()}
            spread = max(blocks["two"]) - min(blocks["two"])
            same = (torch.equal(last["fused"][0], last["two"][0])
                    and torch.equal(last["fused"][1], last["two"][1])
                    and np.array_equal(last["two"][0].cpu().numpy(), last["host"][0])
                    and np.array_equal(last["two"][1].cpu().numpy(), last["host"][1]))
            r = {"batch": B, "ppu": ppu, "view": "%dx%d" % (wb, hb),
                 "nonzero_share": round(float((last["two"][0] != 0).float().mean()), 3),
                 "arms_identical": bool(same), "two_spread_us": round(spread * 1e3, 1),
                 "fused_not_slower": bool(med["fused"] - med["two"] <= spread),
                 "default_route": "fused" if e2e.bird_eye(frames, vp, 255, MIN_WIDTH) is not None
                 and e2e._last_fused else "two"}
            for a in blocks:
                r[a + "_us"] = [round(v * 1e3, 1) for v in blocks[a]]
                r[a + "_median_us"] = round(med[a] * 1e3, 1)
            results.append(r)
            print("# " + json.dumps(r), flush=True)
    print(json.dumps({"tool": "bev_time", "iters": args.iters, "rounds": args.rounds,
                      "configs": results}))
    if args.md:
        lines = ["# Bird's-eye tail: fused against two launches against the host route", "",
                 "`tools/bev_time.py`: 640 x 360 uint8 frames, base 1024, 2 classes, fp16, the "
                 "corrected calibration's full-image view, `min_width` 10; medians of %d "
                 "interleaved rounds of %d calls (host arm: %d), whole pipeline per call, "
                 "microseconds." % (args.rounds, args.iters, args.host_iters), "",
                 "| batch | px/cm | view | fused | two launches | spread of two | host route | "
                 "fused not slower | default route | arms identical |",
                 "|---|---|---|---|---|---|---|---|---|---|"]
        for r in results:
            lines.append("| %d | %d | %s | %.1f | %.1f | %.1f | %.1f | %s | %s | %s |" % (
                r["batch"], r["ppu"], r["view"], r["fused_median_us"], r["two_median_us"],
                r["two_spread_us"], r["host_median_us"], "yes" if r["fused_not_slower"] else "no",
                r["default_route"], "yes" if r["arms_identical"] else "no"))
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
