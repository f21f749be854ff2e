"""AdamW step time on FastSCNN(19)'s parameter arena: FusedAdamW against torch.optim.AdamW
(fused=True, the yardstick, and foreach=True) in one process, with the gradients of one real
backward, for a single group and for the decay / no-decay (BatchNorm + bias) grouping.

Blocks of --steps optimizer steps alternate between the contenders, every shape warmed up.  Two
numbers per contender: device time per step (events around a block that is queued behind blocker
matmuls sized to 1.5 x the contender's own enqueue time, so the host stays ahead and the steps
run back to back) and host enqueue time per step (host clock around a block with nothing in
front, no synchronise inside).  Reported as the median over the blocks and the block-to-block
spread (max - min).  Prints one JSON line; fails without a GPU.

    python tools/optim_time.py [--steps 200] [--blocks 7]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--classes", type=int, default=19)
    args = ap.parse_args()
    if args.steps < 200:
        ap.error("--steps must be at least 200")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("optim_time: no GPU (there is no CPU path to time)")
    import _fscnn_boot
    _fscnn_boot.load()
    from fast_scnn_pytorch_amd import arch, portable_init
    from fast_scnn_pytorch_amd.optim import FusedAdamW
    from models.fast_scnn import FastSCNN

    dev = torch.device("cuda", 0)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in
          arch.portable_state_dict(args.classes, seed=0).items()}
    x = torch.from_numpy(portable_init.input_tensor(1, (2, 3, 256, 512))).to(dev)
    t = torch.from_numpy(portable_init.target_tensor(3, (2, 256, 512), args.classes, 0.05)).to(dev)

    def arena_model():
        m = FastSCNN(args.classes)
        m.load_state_dict(sd)
        m = m.to(dev).train()
        m.forward_loss(x, t).backward()  # .grad: views of one flat gradient arena
        return m

    def groups_of(params, grouping):
        if grouping == "single":
            return [{"params": params}]
        nd = [p for p in params if p.dim() == 1]
        return [{"params": [p for p in params if p.dim() != 1], "weight_decay": 1e-2},
                {"params": nd, "weight_decay": 0.0}]

    contenders = {}
    numel = 0
    for grouping in ("single", "decay_nodecay"):
        m = arena_model()
        ours = list(m.parameters())
        numel = sum(p.numel() for p in ours)
        contenders[(grouping, "FusedAdamW")] = (m, FusedAdamW(groups_of(ours, grouping), lr=1e-3))
        for name, kw in (("torch_fused", {"fused": True}), ("torch_foreach", {"foreach": True})):
            ps = [p.detach().clone().requires_grad_(True) for p in ours]
            for p, q in zip(ps, ours):
                p.grad = q.grad.detach().clone()
            contenders[(grouping, name)] = (ps, torch.optim.AdamW(groups_of(ps, grouping),
                                                                  lr=1e-3, **kw))

    blocker = torch.randn(8192, 8192, device=dev)

    def block(opt, steps, nblock):
        """-> (device us / step, host enqueue us / step).  nblock blocker matmuls in front keep
        the GPU busy while the host enqueues the block (device time); 0: the GPU keeps pace and
        the host never waits for room in the queue (host time)."""
        torch.cuda.synchronize()
        for _ in range(nblock):
            torch.mm(blocker, blocker)
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        h0 = time.perf_counter()
        for i in range(steps):
            opt.param_groups[0]["lr"] = 1e-3 * (1.0 - i / (2.0 * steps))  # a schedule, as :249-251
            opt.step()
        h1 = time.perf_counter()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / steps, 1e6 * (h1 - h0) / steps

    torch.mm(blocker, blocker)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.mm(blocker, blocker)
    e1.record()
    torch.cuda.synchronize()
    mm_us = 1e3 * e0.elapsed_time(e1)
    nblock = {}
    for k, (_, opt) in contenders.items():  # warm every shape up; size each one's blocker
        _, host = block(opt, 20, 0)
        _, host = block(opt, 20, 0)
        nblock[k] = int(1.5 * host * args.steps / mm_us) + 2
    res = {k: [] for k in contenders}
    for _ in range(args.blocks):
        for k, (_, opt) in contenders.items():
            dev_us, _ = block(opt, args.steps, nblock[k])
            _, host_us = block(opt, args.steps, 0)
            res[k].append((dev_us, host_us))

    def stat(v):
        v = sorted(v)
        return {"median": round(v[len(v) // 2], 2), "spread": round(v[-1] - v[0], 2)}

    out = {"tool": "optim_time", "device": torch.cuda.get_device_name(0), "numel": numel,
           "steps_per_block": args.steps, "blocks": args.blocks, "unit": "us per step",
           "blocker_us": round(mm_us, 1),
           "blocker_matmuls": {"%s/%s" % k: v for k, v in nblock.items()},
           "results": {}, "expectation_holds": {}}
    for (grouping, name), v in res.items():
        out["results"].setdefault(grouping, {})[name] = {
            "device": stat([a for a, _ in v]), "host_enqueue": stat([b for _, b in v])}
    for grouping, r in out["results"].items():
        y = r["torch_fused"]
        out["expectation_holds"][grouping] = {
            k: r["FusedAdamW"][k]["median"] <= y[k]["median"] + y[k]["spread"]
            for k in ("device", "host_enqueue")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
