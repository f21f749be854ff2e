#!/usr/bin/env python3
"""Time raw frames -> wheel PWM, on the device against the host route (needs the GPU).

    python tools/steer_time.py [--batches 1,8 --ppu 1,4 --iters 20 --warmup 3 --rounds 5
                                --md profiles/steer_time.md]

640 x 360 uint8 frames, base 1024, 2 classes, fp16 arithmetic, the corrected calibration's
full-image view at ``--ppu`` pixels per cm (208 x 108 and 834 x 433), ``plan_complete_path``'s
defaults (fast mode, degree 2, 20 waypoints, anchor on), the default controller with smoothing.
Two arms take frames to ``(pwm_left, pwm_right)`` per frame, both ending with the values on the
host, timed by a host clock around a call that ends in the copy (a device synchronise):

    steer:  e2e.steer(frames, view, controller)[:, PWM_LEFT:PWM_RIGHT + 1].cpu()
            front end, backbone, the bird's-eye launch, the path launch, one 16-byte-per-frame copy
    host:   e2e.bird_eye(frames, view, return_mask=False)[1].cpu(), then per frame
            bev.centerline + np.polyfit + the controller (``host_steer`` below: the fit with
            the weighted anchor, np.linspace waypoints, the preview search, the EMA and the wheel
            law, nothing else): the route a user of this library had before ``steer``

``tail`` is the same pair without the backbone, from a row table already on the device
(``path.plan(rows)...cpu()`` against ``rows.cpu()`` + the host arithmetic).  The arms are warmed up
and timed in interleaved rounds in one process; the table gives medians and each arm's spread
(max - min of its rounds).  Prints one JSON line; ``--md`` also writes the table.  The two arms'
wheel values are compared (largest distance printed): they agree to the tolerance of the tests, not
to the bit, since the fits are different factorisations.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
W, H, BASE = 640, 360, 1024


def wall_ms(fn, iters):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def host_steer(world, p, state):
    """The host route's arithmetic for one frame, as the reference's smooth_path,
    generate_waypoints, _find_preview_point and compute_wheel_pwm do it: centreline world points
    -> ((pwm_left, pwm_right), new EMA state).  No rank test, no path length, no status."""
    import numpy as np
    raw = 0.0
    if world:
        pts = np.array(world, dtype=np.float64)
        y, x, w = pts[:, 1], pts[:, 0], np.ones(len(pts))
        if p["force_bottom_center"]:
            y, x, w = np.append(y, p["anchor_y"]), np.append(x, p["anchor_x"]), np.append(w, 1e6)
        if len(y) > p["degree"]:
            ys = np.linspace(p["min_y"], p["max_y"], p["num_waypoints"])
            xs = np.poly1d(np.polyfit(y, x, p["degree"], w=w))(ys)
            ahead = ys < p["car_y"]
            if ahead.any():
                d = np.abs(np.sqrt((xs - p["car_x"]) ** 2 + (ys - p["car_y"]) ** 2)
                           - p["preview_distance"])
                raw = float(xs[np.flatnonzero(ahead)[np.argmin(d[ahead])]] - p["car_x"])
            else:
                raw = float(xs[np.argmin(ys)] - p["car_x"])
    e = raw if state is None else p["ema_alpha"] * raw + (1 - p["ema_alpha"]) * state
    steering = p["steering_gain"] * e
    dynamic = float(np.clip(p["base_pwm"] / (1 + p["curvature_damping"] * abs(e)), p["min_pwm"],
                            p["max_pwm"]))
    return (float(np.clip(dynamic + steering, -1000, 1000)),
            float(np.clip(dynamic - steering, -1000, 1000))), e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--ppu", default="1,4")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--md", default="")
    args = ap.parse_args()

    import numpy as np
    import torch
    import _fscnn_boot
    _fscnn_boot.load()
    from fast_scnn_pytorch_amd import arch, bev
    from fast_scnn_pytorch_amd import path as P
    from fast_scnn_pytorch_amd.deploy import EndToEndFastSCNN
    from models.fast_scnn import FastSCNN

    if not torch.cuda.is_available():
        raise SystemExit("steer_time: no GPU visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
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
        # a lane-like picture: a bright band bending across each frame, so that the random-weight
        # backbone's mask has rows to fit (the share of rows with a centreline point is reported)
        yy, xx = np.mgrid[0:H, 0:W]
        frames = np.zeros((B, 3, H, W), dtype=np.uint8)
        for b in range(B):
            centre = 320 + (b - B / 2) * 12 + 0.0009 * (359 - yy) ** 2
            band = np.abs(xx - centre) < 40 + yy * 0.35
            frames[b] = np.where(band, 200, 40)[None] + (np.arange(3) * 10)[:, None, None]
        frames = torch.from_numpy(frames).to(dev)
        for ppu in [int(p) for p in args.ppu.split(",")]:
            (wb, hb), _, _, vp = view.params(ppu, 0.1, True, source_size=(W, H))
            last = {}
            ctl = {a: P.VisualLateralErrorController() for a in ("steer", "tail")}
            host_state = {a: [None] * B for a in ("host", "host_tail")}
            params = P.plan_params(vp, ctl["steer"])
            # (Python floats, so that centerline's world points are float64 under every numpy)
            vp_host = dict(vp, view_bounds=tuple(float(v) for v in vp["view_bounds"]))

            def host_math(rows, arm):
                out = np.empty((B, 2))
                for f in range(B):
                    _, world = bev.centerline(rows[f], vp_host, fast=True,
                                              min_width=params["min_width"],
                                              skip_rows=params["skip_rows"])
                    out[f], host_state[arm][f] = host_steer(world, params, host_state[arm][f])
                return out

            def steer():
                last["steer"] = e2e.steer(frames, vp, ctl["steer"])[
                    :, P.PWM_LEFT:P.PWM_RIGHT + 1].cpu().numpy()

            def host():
                rows = e2e.bird_eye(frames, vp, return_mask=False)[1]
                last["host"] = host_math(rows.cpu().numpy(), "host")

            rows_dev = e2e.bird_eye(frames, vp, return_mask=False)[1]

            def tail():
                last["tail"] = P.plan(rows_dev, vp, ctl["tail"])[
                    :, P.PWM_LEFT:P.PWM_RIGHT + 1].cpu().numpy()

            def host_tail():
                last["host_tail"] = host_math(rows_dev.cpu().numpy(), "host_tail")

            arms = (("steer", steer), ("host", host), ("tail", tail), ("host_tail", host_tail))
            for _, fn in arms:
                for _ in range(args.warmup):
                    fn()
            blocks = {a: [] for a, _ in arms}
            for _ in range(args.rounds):
                for a, fn in arms:
                    blocks[a].append(wall_ms(fn, args.iters))
            # every arm has made the same number of calls, so the EMA states correspond
            points = int((rows_dev[:, :, 2] > 0).sum())
            r = {"batch": B, "ppu": ppu, "view": "%dx%d" % (wb, hb),
                 "rows_with_mask_share": round(points / (B * hb), 3),
                 "pwm_distance_steer_host": float(np.abs(last["steer"] - last["host"]).max()),
                 "pwm_distance_tail_host": float(np.abs(last["tail"] - last["host_tail"]).max())}
            for a in blocks:
                r[a + "_us"] = [round(v * 1e3, 1) for v in blocks[a]]
                r[a + "_median_us"] = round(statistics.median(blocks[a]) * 1e3, 1)
                r[a + "_spread_us"] = round((max(blocks[a]) - min(blocks[a])) * 1e3, 1)
            results.append(r)
            print("# " + json.dumps(r), flush=True)
    print(json.dumps({"tool": "steer_time", "iters": args.iters, "rounds": args.rounds,
                      "configs": results}))
    if args.md:
        lines = ["# Frames to wheel PWM: `steer` against the host route", "",
                 "`tools/steer_time.py`: 640 x 360 uint8 frames, base 1024, 2 classes, fp16, the "
                 "corrected calibration's full-image view, `plan_complete_path`'s defaults, the "
                 "default controller with smoothing; medians of %d interleaved rounds of %d calls, "
                 "host clock around calls that end with the wheel values on the host, "
                 "microseconds per call (spread = max - min of the arm's rounds)."
                 % (args.rounds, args.iters), "",
                 "`steer`: front end, backbone, bird's-eye launch, path launch, one small copy.  "
                 "`host`: `bird_eye` + `rows.cpu()` + `bev.centerline` + `np.polyfit` + the "
                 "controller in numpy (`host_steer` of the tool: fit, waypoints, preview search, EMA, wheel "
                 "law and nothing else), the route before `steer`.  `tail` / "
                 "`host tail`: the same two from a row table already on the device, without the "
                 "backbone.", "",
                 "| batch | px/cm | view | steer | spread | host | spread | tail | spread | "
                 "host tail | spread | rows with mask | PWM distance |",
                 "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in results:
            lines.append("| %d | %d | %s | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | "
                         "%.3f | %.2g |" % (
                             r["batch"], r["ppu"], r["view"], r["steer_median_us"],
                             r["steer_spread_us"], r["host_median_us"], r["host_spread_us"],
                             r["tail_median_us"], r["tail_spread_us"], r["host_tail_median_us"],
                             r["host_tail_spread_us"], r["rows_with_mask_share"],
                             r["pwm_distance_steer_host"]))
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
