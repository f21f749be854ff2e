#!/usr/bin/env python3
"""Generate the deployment-pipeline fixtures by importing the REFERENCE wrapper (survey container
only, CPU):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_e2e_golden.py

Imports ``EndToEndFastSCNN`` from the reference's ``export_onnx_fixed.py``, wraps the reference
``FastSCNN`` loaded with the calibrated weights already committed in ``tests/golden/eval_c2_calib``
/ ``eval_c19_calib`` (``helpers.golden_sd``; the portable-init weights alone predict one class
everywhere), and writes ``tests/golden/e2e_<case>_c<C>.npz``:

    frames          uint8 [3, 3, h, w] (stored: smooth random images, a 6x8 random image enlarged
                    bicubically, clamped and rounded); batch 1 is frames[:1]
    probs           fp32 output of the reference wrapper (C = 2: all of it; C = 19: at the seeded
                    positions ``probs_idx`` of the flattened [3, C, H, W] tensor)
    argmax, margin  argmax and top-2 margin of the resampled logits, evaluated in fp64
    input_size, base_size, norm (0 / 1: ImageNet mean / std), num_classes, weights

and ``e2e_schema.npz`` with the wrapper's ``state_dict`` key lists.  Data only.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("FSCNN_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, REF)  # `models` and `export_onnx_fixed` are the reference's own
from export_onnx_fixed import EndToEndFastSCNN  # noqa: E402
from models.fast_scnn import FastSCNN  # noqa: E402

sys.path.append(ROOT)
sys.path.append(os.path.join(ROOT, "tests"))
import _fscnn_boot  # noqa: E402

_fscnn_boot.load()
import helpers  # noqa: E402

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
# name, frame (w, h), input_size (w, h) or None = the frame's, base_size, ImageNet mean / std
CASES = [
    ("80x48", (80, 48), None, 128, True),
    ("200x70", (200, 70), None, 160, True),
    ("61x45", (61, 45), None, 100, False),
    ("50x40_to_37x33", (50, 40), (37, 33), 96, True),
    ("128x128", (128, 128), None, 128, True),
]
WEIGHTS = {2: "eval_c2_calib", 19: "eval_c19_calib"}
NSAMPLE = 8192


def smooth_frames(seed, n, h, w):
    rng = np.random.RandomState(seed)
    lo = torch.from_numpy(rng.uniform(0.0, 255.0, (n, 3, 6, 8)))
    up = F.interpolate(lo, size=(h, w), mode="bicubic", align_corners=False)
    return up.clamp(0, 255).round().to(torch.uint8)


def wrapper(nc, size, base, norm, softmax):
    bb = FastSCNN(nc)
    bb.load_state_dict(helpers.golden_sd(helpers.load_golden(WEIGHTS[nc])))
    m = EndToEndFastSCNN(bb, input_size=size, base_size=base, mean=MEAN if norm else None,
                         std=STD if norm else None, apply_softmax=softmax)
    return m.eval()


def gen_case(idx, name, frame, size, base, norm, nc):
    w, h = frame
    size = size or frame
    frames = smooth_frames(100 + idx, 3, h, w)
    with torch.no_grad():
        probs = wrapper(nc, size, base, norm, True)(frames)
        lg64 = wrapper(nc, size, base, norm, False).double()(frames.double())
    srt = torch.sort(lg64, dim=1).values
    margin = (srt[:, -1] - srt[:, -2]).numpy()
    am = lg64.argmax(1).numpy().astype(np.uint8)
    p64 = torch.softmax(lg64, 1)
    out = {"frames": frames.numpy(), "argmax": am, "margin": margin.astype(np.float32),
           "input_size": np.array(size), "base_size": np.int64(base), "norm": np.int64(norm),
           "num_classes": np.int64(nc), "weights": np.array(WEIGHTS[nc])}
    pr = probs.numpy().astype(np.float32)
    if nc == 2:
        out["probs"] = pr
    else:
        rng = np.random.RandomState(7 + idx)
        pidx = np.unique(rng.randint(0, pr.size, NSAMPLE)).astype(np.int64)
        out["probs_idx"] = pidx
        out["probs"] = pr.ravel()[pidx]
    path = os.path.join(OUT, "e2e_%s_c%d.npz" % (name, nc))
    np.savez_compressed(path, **out)
    hist = np.bincount(am.ravel(), minlength=nc)
    print("%-16s C=%-2d  off-majority %.1f %%  margin<=1e-4 %.3f %%  fp32 vs fp64 %.1e  %d KB"
          % (name, nc, 100.0 * (1 - hist.max() / am.size), 100.0 * (margin <= 1e-4).mean(),
             (probs.double() - p64).abs().max().item(), os.path.getsize(path) // 1024))


def main():
    torch.set_num_threads(8)
    os.makedirs(OUT, exist_ok=True)
    for nc in (2, 19):
        for i, (name, frame, size, base, norm) in enumerate(CASES):
            gen_case(i, name, frame, size, base, norm, nc)
    keys = {}
    for nc in (2, 19):
        keys["c%d_norm" % nc] = np.array(list(wrapper(nc, (64, 48), 64, True, True).state_dict()))
        keys["c%d_plain" % nc] = np.array(list(wrapper(nc, (64, 48), 64, False, True).state_dict()))
    np.savez_compressed(os.path.join(OUT, "e2e_schema.npz"), **keys)


if __name__ == "__main__":
    main()
