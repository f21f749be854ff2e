#!/usr/bin/env python3
"""Time the GPU augmentation against the train step it feeds (needs the GPU; no fallback).

    python tools/sync_transform_time.py [--batch 8 --height 1024 --width 2048 --base 1024 --crop 768]

B x H x W uint8 images + masks -> B x 3 x crop x crop bf16 + targets with sampled parameters:
HIP events around 50 calls after warm-up (the whole ``__call__``: host tables, staging copy and
the launch, back to back), the host time of one call, the device time of one call (the same
calls queued behind other device work, so the host is not the limit), and, in the same process, the bf16 train
step (forward_loss + backward + FusedSGD) on the produced batch.  Prints one JSON line with
microseconds, the algorithmic bytes (source window of every crop read once + outputs written)
and the resulting GB/s; exits non-zero if the transform is slower than the step it feeds.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def algorithmic_bytes(params, H, W, crop, out_bytes):
    """Per sample: the source window the crop covers, image (3 B) + mask (1 B) per source pixel,
    read once; x (3 channels), the int64 target written."""
    total = 0
    for p in params:
        sw = min(crop, p.ow - p.x1) * W / p.ow
        sh = min(crop, p.oh - p.y1) * H / p.oh
        total += sw * sh * 4 + crop * crop * (3 * out_bytes + 8)
    return total


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
    ap.add_argument("--base", type=int, default=1024)
    ap.add_argument("--crop", type=int, default=768)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()

    import numpy as np
    import torch
    import _fscnn_boot
    _fscnn_boot.load()
    from fast_scnn_pytorch_amd import arch
    from fast_scnn_pytorch_amd.data import SyncTransform
    from fast_scnn_pytorch_amd.optim import FusedSGD
    from models.fast_scnn import FastSCNN

    if not torch.cuda.is_available():
        raise SystemExit("sync_transform_time: no GPU visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    B, H, W, crop = args.batch, args.height, args.width, args.crop
    gen = torch.Generator(device=dev).manual_seed(0)
    imgs = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev, generator=gen)
    masks = torch.randint(0, 34, (B, H, W), dtype=torch.uint8, device=dev, generator=gen)
    st = SyncTransform(args.base, crop, dtype=torch.bfloat16, seed=0)

    # a fixed cycle of sampled parameter sets, so the timed launches do the sampler's mix of work
    sets = [[st.sample(W, H) for _ in range(B)] for _ in range(args.iters)]
    it = [0]

    def transform():
        p = sets[it[0] % len(sets)]
        it[0] += 1
        return st(imgs, masks, p)

    for _ in range(args.warmup):
        x, t = transform()
    it[0] = 0
    t_ms = events_ms(transform, args.iters)
    # host time of one call (tables + enqueue), with the device idle
    torch.cuda.synchronize()
    h0 = time.perf_counter()
    for _ in range(args.iters):
        transform()
    host_ms = (time.perf_counter() - h0) * 1e3 / args.iters
    torch.cuda.synchronize()
    # device side alone: a call is host-bound when the device is idle, so queue the timed calls
    # behind ~50 ms of other device work (a ring deep enough that no staging slot is reused
    # inside the window, slots allocated beforehand) and time them back to back
    st.RING = args.iters + 1
    for _ in range(2 * st.RING):
        transform()
    torch.cuda.synchronize()
    big = torch.randn(8192, 8192, device=dev).to(torch.bfloat16)
    big @ big
    torch.cuda.synchronize()
    for _ in range(60):
        big @ big
    it[0] = 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        transform()
    e1.record()
    torch.cuda.synchronize()
    dev_ms = e0.elapsed_time(e1) / args.iters
    del big
    nbytes = sum(algorithmic_bytes(p, H, W, crop, 2) for p in sets) / len(sets)

    model = FastSCNN(19)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in
                           arch.portable_state_dict(19, seed=0).items()})
    model = model.to(dev).train()
    opt = FusedSGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    torch.manual_seed(0)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = model.forward_loss(x, t)
        loss.backward()
        opt.step()
        return loss

    for _ in range(args.warmup):
        loss = step()
    s_ms = events_ms(step, args.iters)

    print(json.dumps({
        "shape": "%dx%dx%d u8 -> %dx3x%dx%d bf16 + int64 targets" % (B, H, W, B, crop, crop),
        "transform_us": round(t_ms * 1e3, 1), "transform_host_us": round(host_ms * 1e3, 1),
        "transform_device_us": round(dev_ms * 1e3, 1), "algorithmic_bytes": int(nbytes),
        "transform_GBps": round(nbytes / (t_ms * 1e-3) / 1e9, 1),
        "transform_device_GBps": round(nbytes / (dev_ms * 1e-3) / 1e9, 1),
        "train_step_us": round(s_ms * 1e3, 1), "loss": round(float(loss.item()), 4),
        "transform_faster_than_step": bool(t_ms < s_ms)}))
    if not t_ms < s_ms:
        raise SystemExit("the transform (%.3f ms) is slower than the step it feeds (%.3f ms)"
                         % (t_ms, s_ms))


if __name__ == "__main__":
    main()
