#!/usr/bin/env python3
"""Time the colour bird's-eye view kernel, fscnn_bev_image (needs the GPU).

    python tools/bev_image_time.py [--iters 50 --warmup 5 --rounds 3] --json OUT.json
    rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d DIR -- \
        python tools/bev_image_time.py --iters 20 --rounds 1 --json OUT2.json
    python tools/bev_image_time.py --report OUT.json --trace-json OUT2.json \
        --kernel-trace DIR/..._kernel_trace.csv [--copy-trace DIR/..._memory_copy_trace.csv] \
        --md profiles/bev_image_time.md

640 x 360 uint8 channels_last frames (smooth, like a camera frame), the corrected calibration's
full-image view at 1 pixel per cm (208 x 108) and at 20 (4173 x 2168), batch 1 and 8, the image
alone and the image with the segmented picture.  Outputs are allocated once; a configuration's
launches go to the stream back to back between two HIP events ("call" time: it includes what the
host needs to issue a launch), in rounds interleaved with a device-to-device copy of as many bytes
as the launch writes.  The kernel's own time comes from a rocprofv3 kernel trace of a second run
of this tool: its launches are matched to the configurations by their order.  Nothing is asserted
on the timings."""
import argparse
import csv
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 640, 360
CONFIGS = [(n, ppu, blend) for ppu in (1, 20) for n in (1, 8) for blend in (False, True)]


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


def measure(args):
    import torch
    import torch.nn.functional as F
    import _fscnn_boot
    _fscnn_boot.load()
    from fast_scnn_pytorch_amd import _lib, bev

    if not torch.cuda.is_available():
        raise SystemExit("bev_image_time: no GPU visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    lib = _lib.load()
    gen = torch.Generator(device=dev).manual_seed(0)
    view = bev.BirdEyeView()
    green = (ctypes.c_ubyte * 3)(0, 255, 0)
    results = []
    for n, ppu, blend in CONFIGS:
        coarse = torch.rand(n, 3, 9, 16, device=dev, generator=gen) * 255
        frames = F.interpolate(coarse, size=(H, W), mode="bicubic", align_corners=False)
        frames = frames.clamp(0, 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        (wb, hb), _, _, vp = view.params(ppu, 0.1, True)
        m = bev.inverse_map(vp)
        cm = (ctypes.c_double * 9)(*[float(v) for v in m])
        image = torch.empty((n, hb, wb, 3), dtype=torch.uint8, device=dev)
        blended = torch.empty_like(image) if blend else None
        mask = None
        if blend:  # a lane-like mask: the middle third of every row
            mask = torch.zeros((n, hb, wb), dtype=torch.uint8, device=dev)
            mask[:, :, wb // 3:2 * wb // 3] = 255
        out_bytes = image.numel() * (2 if blend else 1)
        src = torch.empty(out_bytes, dtype=torch.uint8, device=dev).fill_(7)
        dst = torch.empty_like(src)
        stream = _lib.stream_ptr(dev)

        def launch():
            rc = lib.fscnn_bev_image(_lib.ptr(frames), 1, n, H, W, cm, hb, wb, _lib.ptr(image),
                                     _lib.ptr(mask), green if blend else None, 1.0, 0.5, 0.0,
                                     _lib.ptr(blended), stream)
            if rc:
                _lib.check(rc, "fscnn_bev_image")

        def copy():
            dst.copy_(src)

        for _ in range(args.warmup):
            launch()
            copy()
        k, c = [], []
        for _ in range(args.rounds):
            k.append(events_ms(launch, args.iters))
            c.append(events_ms(copy, args.iters))
        ref = bev.warp_image(frames, m, (wb, hb), channels_last=True)
        results.append({"batch": n, "px_per_cm": ppu, "view": "%dx%d" % (wb, hb), "blend": blend,
                        "out_bytes": out_bytes, "launches": args.warmup + args.rounds * args.iters,
                        "call_us": [round(v * 1e3, 2) for v in k],
                        "copy_us": [round(v * 1e3, 2) for v in c],
                        "same_as_warp_image": bool(torch.equal(ref, image)),
                        "nonzero_share": round(float((image != 0).float().mean()), 3)})
        print("# " + json.dumps(results[-1]), flush=True)
        del image, blended, mask, src, dst, frames, ref
        torch.cuda.empty_cache()
    doc = {"tool": "bev_image_time", "iters": args.iters, "rounds": args.rounds,
           "warmup": args.warmup, "configs": results}
    print(json.dumps(doc))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)) or ".", exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(doc, f)


def trace_ns(path, match):
    """Durations in ns of the rows of a rocprofv3 CSV whose name column contains ``match`` (any
    row when ``match`` is empty), in start order."""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name") or r.get("Name") or r.get("Direction") or ""
            if match in name:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort()
    return [e - s for s, e in rows]


def report(args):
    with open(args.report) as f:
        doc = json.load(f)
    kern = copies = None
    if args.kernel_trace:
        with open(args.trace_json) as f:
            tdoc = json.load(f)
        kern = trace_ns(args.kernel_trace, "bev_image_kernel")
        # every configuration ends with one warp_image call of the same shape (the identity check)
        counts = [c["launches"] + 1 for c in tdoc["configs"]]
        if sum(counts) != len(kern):
            raise SystemExit("bev_image_time: %d launches in the trace, %d expected"
                             % (len(kern), sum(counts)))
        if args.copy_trace:
            copies = trace_ns(args.copy_trace, "DEVICE_TO_DEVICE")
            if len(copies) != sum(c["launches"] for c in tdoc["configs"]):
                copies = None
    lines = ["# Colour bird's-eye view: kernel time against a copy of the same bytes", "",
             "`tools/bev_image_time.py`: 640 x 360 uint8 channels_last frames, the corrected "
             "calibration's full-image view, outputs allocated once. \"call\": %d rounds of %d "
             "back-to-back launches between two HIP events, median, host issue time included. "
             "\"kernel\": median duration of the same launches in a rocprofv3 kernel trace of a "
             "second run. \"copy\": a device-to-device copy of as many bytes as the launch writes, "
             "timed like \"call\" in interleaved rounds%s. Rates are bytes written over time."
             % (doc["rounds"], doc["iters"],
                ", and its own duration in the memory-copy trace" if copies else ""), "",
             "| batch | view | outputs | bytes written | call us | kernel us | kernel GB/s | copy "
             "call us | copy GB/s |%s kernel rate / copy rate |" % (" copy trace us |" if copies else ""),
             "|---|---|---|---|---|---|---|---|---|%s---|" % ("---|" if copies else "")]
    at = cat = 0
    for i, c in enumerate(doc["configs"]):
        call, cp = statistics.median(c["call_us"]), statistics.median(c["copy_us"])
        kus = None
        cus = None
        if kern is not None:
            t = tdoc["configs"][i]
            mine = kern[at + tdoc["warmup"]:at + t["launches"]]
            at += t["launches"] + 1
            kus = statistics.median(mine) / 1e3
            if copies:
                cm = copies[cat + tdoc["warmup"]:cat + t["launches"]]
                cat += t["launches"]
                cus = statistics.median(cm) / 1e3
        best_copy = min(cp, cus) if cus else cp
        krate = c["out_bytes"] / (kus * 1e3) if kus else None
        crate = c["out_bytes"] / (best_copy * 1e3)
        lines.append("| %d | %s | %s | %d | %.1f | %s | %s | %.1f | %.1f |%s %s |" % (
            c["batch"], c["view"], "image + blended" if c["blend"] else "image", c["out_bytes"],
            call, "%.1f" % kus if kus else "not measured",
            "%.1f" % krate if krate else "not measured", cp, crate,
            (" %.1f |" % cus) if copies else "",
            "%.2f" % (krate / crate) if krate else "not measured"))
    with open(args.md, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default="")
    ap.add_argument("--report", default="", help="JSON of the timed run: write the table")
    ap.add_argument("--trace-json", default="", help="JSON of the traced run")
    ap.add_argument("--kernel-trace", default="")
    ap.add_argument("--copy-trace", default="")
    ap.add_argument("--md", default="profiles/bev_image_time.md")
    args = ap.parse_args()
    return report(args) if args.report else measure(args)


if __name__ == "__main__":
    main()
