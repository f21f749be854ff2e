#!/usr/bin/env python3
"""Generate the augmentation goldens by running the REFERENCE's own transform (needs the
reference checkout and PIL; like tools/gen_golden.py it runs only where those are present).

    FSCNN_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tools/gen_sync_golden.py

Loads ``data_loader/cityscapes.py`` by file path (the package ``__init__`` pulls torchvision),
builds a ``CitySegmentation`` without files, and for every seed calls its ``_sync_transform``
(after ``random.seed(seed)``) and once its ``_val_sync_transform`` on a synthetic source.  The
random draws and resize sizes the reference makes are recorded by wrapping ``random`` and
``Image.resize`` while it runs.  One ``tests/golden/sync_<cfg>.npz`` per configuration: source,
seeds, drawn parameters, expected uint8 crops, expected targets (int8), PIL version.  Data only.
"""
import importlib.util
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("FSCNN_REFERENCE")  # checkout of the reference repository
OUT = os.path.join(ROOT, "tests", "golden")

# name -> (H, W, base, crop, seeds)
CONFIGS = {
    "A": (96, 192, 64, 48, range(48)),
    "B": (90, 60, 64, 48, range(24)),
    "C": (150, 210, 120, 90, range(16)),
}
MIN_CASES = 4


def load_reference():
    spec = importlib.util.spec_from_file_location(
        "ref_cityscapes", os.path.join(REF, "data_loader", "cityscapes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_dataset(mod, base, crop):
    ds = mod.CitySegmentation.__new__(mod.CitySegmentation)
    ds.base_size, ds.crop_size = base, crop
    ds._key = np.array([-1, -1, -1, -1, -1, -1, -1, -1, 0, 1, -1, -1, 2, 3, 4, -1, -1, -1, 5, -1,
                        6, 7, 8, 9, 10, 11, 12, 13, 14, 15, -1, -1, 16, 17, 18])
    ds._mapping = np.array(range(-1, len(ds._key) - 1)).astype("int32")
    return ds


def synthetic_source(H, W, seed):
    """Image: per-channel gradients + noise (interpolation and rounding both matter); mask:
    blocky random label ids 0..33."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([(xx * 255.0 / max(W - 1, 1)), (yy * 255.0 / max(H - 1, 1)),
                    ((xx + yy) * 255.0 / max(H + W - 2, 1))], -1)
    img = np.clip(img + rng.normal(0, 24, img.shape), 0, 255).astype(np.uint8)
    bh, bw = max(H // 12, 1), max(W // 12, 1)
    blocks = rng.integers(0, 34, ((H + bh - 1) // bh, (W + bw - 1) // bw)).astype(np.uint8)
    mask = np.kron(blocks, np.ones((bh, bw), np.uint8))[:H, :W]
    return img, np.ascontiguousarray(mask)


class _Recorder:
    """Stands in for the ``random`` module inside the reference while it runs."""

    def __init__(self):
        self.log = []

    def random(self):
        v = random.random()
        self.log.append(("random", v))
        return v

    def randint(self, a, b):
        v = random.randint(a, b)
        self.log.append(("randint", a, b, v))
        return v


def run_case(mod, ds, img, mask, seed, crop):
    from PIL import Image
    rec = _Recorder()
    sizes = []
    orig_resize = Image.Image.resize

    def resize(self, size, *a, **k):
        sizes.append(tuple(size))
        return orig_resize(self, size, *a, **k)

    random.seed(seed)
    mod.random, Image.Image.resize = rec, resize
    try:
        u8, tgt = ds._sync_transform(Image.fromarray(img), Image.fromarray(mask))
    finally:
        mod.random, Image.Image.resize = random, orig_resize
    lg = rec.log
    assert [e[0] for e in lg[:5]] == ["random", "randint", "randint", "randint", "random"]
    flip = lg[0][1] < 0.5
    short = lg[1][3]
    ow, oh = sizes[0]
    assert sizes[1] == (ow, oh) and short == min(ow, oh)
    padw, padh = lg[2][2] + crop - ow, lg[3][2] + crop - oh
    x1, y1 = lg[2][3], lg[3][3]
    blur = lg[5][1] if lg[4][1] < 0.5 else -1.0
    assert len(lg) == (6 if blur >= 0 else 5)
    params = np.array([flip, ow, oh, padw, padh, x1, y1], np.int32)
    return params, blur, np.asarray(u8), tgt.numpy()


def run_val(ds, img, mask):
    from PIL import Image
    sizes, boxes = [], []
    orig_resize, orig_crop = Image.Image.resize, Image.Image.crop

    def resize(self, size, *a, **k):
        sizes.append(tuple(size))
        return orig_resize(self, size, *a, **k)

    def crop(self, box=None):
        boxes.append(tuple(box))
        return orig_crop(self, box)

    Image.Image.resize, Image.Image.crop = resize, crop
    try:
        u8, tgt = ds._val_sync_transform(Image.fromarray(img), Image.fromarray(mask))
    finally:
        Image.Image.resize, Image.Image.crop = orig_resize, orig_crop
    assert sizes[0] == sizes[1] and boxes[0] == boxes[1]
    params = np.array(sizes[0] + boxes[0][:2], np.int32)  # ow, oh, x1, y1
    return params, np.asarray(u8), tgt.numpy()


def check_branches(name, H, W, crop, params, blur):
    flip = params[:, 0] == 1
    padded = (params[:, 3] > 0) | (params[:, 4] > 0)
    blurred = blur >= 0
    up = np.minimum(params[:, 1], params[:, 2]) > min(H, W)
    down = np.minimum(params[:, 1], params[:, 2]) < min(H, W)
    xmax, ymax = params[:, 1] + params[:, 3] - crop, params[:, 2] + params[:, 4] - crop
    border = ((params[:, 5] == 0) | (params[:, 5] == xmax) | (params[:, 6] == 0)
              | (params[:, 6] == ymax))
    counts = {"flip": flip.sum(), "no flip": (~flip).sum(), "padded": padded.sum(),
              "blurred": blurred.sum(), "padded+blurred": (padded & blurred).sum(),
              "upscale": up.sum(), "downscale": down.sum(), "crop at border": border.sum()}
    print(name, {k: int(v) for k, v in counts.items()})
    for k, v in counts.items():
        assert v >= MIN_CASES, "config %s has only %d '%s' cases" % (name, v, k)


def main():
    import PIL
    if not REF:
        raise SystemExit("set FSCNN_REFERENCE to a checkout of the reference repository")
    mod = load_reference()
    os.makedirs(OUT, exist_ok=True)
    for name, (H, W, base, crop, seeds) in CONFIGS.items():
        ds = make_dataset(mod, base, crop)
        img, mask = synthetic_source(H, W, 1000 + ord(name))
        P, B, U, T = [], [], [], []
        for s in seeds:
            p, b, u8, tgt = run_case(mod, ds, img, mask, s, crop)
            assert u8.shape == (crop, crop, 3) and tgt.shape == (crop, crop)
            P.append(p), B.append(b), U.append(u8), T.append(tgt.astype(np.int8))
        P, B = np.stack(P), np.array(B, np.float64)
        check_branches(name, H, W, crop, P, B)
        vp, vu8, vt = run_val(ds, img, mask)
        path = os.path.join(OUT, "sync_%s.npz" % name)
        np.savez_compressed(
            path, image=img, mask=mask, base=np.int64(base), crop=np.int64(crop),
            seeds=np.array(list(seeds), np.int64), params=P, blur=B, crop_u8=np.stack(U),
            target=np.stack(T), val_params=vp, val_u8=vu8, val_target=vt.astype(np.int8),
            pil_version=np.array(PIL.__version__))
        size = os.path.getsize(path)
        assert size < 1000000, (path, size)
        print(path, size, "bytes")


if __name__ == "__main__":
    main()
