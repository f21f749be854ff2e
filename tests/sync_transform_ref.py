"""numpy restatement of the reference's train / val augmentation
(``CitySegmentation._sync_transform`` / ``_val_sync_transform``, data_loader/cityscapes.py:93-150)
as PIL computes it: fixed-point bilinear resize (Resample.c), nearest mask resize (Geometry.c
``ImagingScaleAffine``), zero pad, crop, 3-pass box "Gaussian" blur (BoxBlur.c) and the label
remap.  Pinned to the reference's own outputs by ``tests/golden/sync_*.npz``; the HIP path is
checked against it where no golden exists (full size, other label tables).

Parameters are the tuple (flip, ow, oh, padw, padh, x1, y1, blur) with blur None or a radius < 1.
"""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2


# ---- parameters ------------------------------------------------------------------------------
def val_params(w, h, crop):
    """_val_sync_transform (cityscapes.py:93-110): short edge -> crop, centre crop."""
    if w > h:
        oh = crop
        ow = int(1.0 * w * oh / h)
    else:
        ow = crop
        oh = int(1.0 * h * ow / w)
    x1 = int(round((ow - crop) / 2.))
    y1 = int(round((oh - crop) / 2.))
    return (False, ow, oh, 0, 0, x1, y1, None)


# ---- tables ---------------------------------------------------------------------------------
def bilinear_tables(insize, outsize, start, count):
    """Resample.c precompute_coeffs (triangle filter) + normalize_coeffs_8bpc for the output
    positions start .. start+count-1; positions >= outsize (the zero pad) get no taps.
    Returns (xmin[count], cnt[count], k[count][ksize]) as int32."""
    scale = float(np.float32(insize)) / float(np.float32(outsize))
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    xmin = np.zeros(count, np.int32)
    cnt = np.zeros(count, np.int32)
    kk = np.zeros((count, ksize), np.int32)
    ss = 1.0 / fs
    for j in range(count):
        xx = start + j
        if xx >= outsize:
            xmin[j] = insize
            continue
        center = (xx + 0.5) * scale
        lo = int(center - support + 0.5)
        if lo < 0:
            lo = 0
        hi = int(center + support + 0.5)
        if hi > insize:
            hi = insize
        n = hi - lo
        w = [0.0] * n
        ww = 0.0
        for i in range(n):
            v = (i + lo - center + 0.5) * ss
            v = -v if v < 0.0 else v
            w[i] = 1.0 - v if v < 1.0 else 0.0
            ww += w[i]
        for i in range(n):
            if ww != 0.0:
                w[i] /= ww
            kk[j, i] = int(0.5 + w[i] * (1 << PRECISION_BITS)) if w[i] >= 0 else \
                int(-0.5 + w[i] * (1 << PRECISION_BITS))
        xmin[j] = lo
        cnt[j] = n
    return xmin, cnt, kk


def nearest_table(insize, outsize, start, count):
    """Geometry.c ImagingScaleAffine for a plain resize: xo = a/2, then xo += a per output
    (sequential additions from position 0).  Pad positions get -1."""
    a = float(insize) / outsize
    xo = a * 0.5
    idx = np.full(count, -1, np.int32)
    for xx in range(min(outsize, start + count)):
        if xx >= start:
            idx[xx - start] = int(xo)
        xo += a
    return idx


def blur_consts(radius):
    """BoxBlur.c: _gaussian_blur_radius(radius, passes=3) and ImagingLineBoxBlur8's weights."""
    f = np.float32
    r = f(radius)
    sigma2 = f(f(r * r) / f(3))
    L = f(math.sqrt(12.0 * float(sigma2) + 1.0))
    l = f(math.floor((float(L) - 1.0) / 2.0))
    a = f(f(f(2) * l + f(1)) * f(f(l * f(l + f(1))) - f(f(3) * sigma2)))
    a = f(a / f(f(6) * f(sigma2 - f(f(l + f(1)) * f(l + f(1))))))
    fr = f(l + a)
    ww = int(f(f(16777216.0) / f(f(fr * f(2)) + f(1))))
    fw = (((1 << 24) - (2 * int(fr) + 1) * ww) & 0xFFFFFFFF) // 2
    return ww, fw, float(fr)


# ---- pipeline -------------------------------------------------------------------------------
def _resample_axis(src, xmin, cnt, kk):
    """One Resample.c pass along axis 1 of src [R, in, C] uint8 -> [R, count, C] uint8."""
    out = np.empty((src.shape[0], len(xmin), src.shape[2]), np.uint8)
    s64 = src.astype(np.int64)
    for j in range(len(xmin)):
        n = int(cnt[j])
        acc = (s64[:, xmin[j]:xmin[j] + n, :] * kk[j, :n].astype(np.int64)[None, :, None]).sum(1)
        out[:, j, :] = np.clip((acc + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS, 0, 255)
    return out


def _box_pass(a, ww, fw):
    """One radius-<1 ImagingLineBoxBlur8 pass along axis 1, edges replicated."""
    v = a.astype(np.uint64)
    left = np.concatenate([v[:, :1], v[:, :-1]], 1)
    right = np.concatenate([v[:, 1:], v[:, -1:]], 1)
    return ((v * np.uint64(ww) + (left + right) * np.uint64(fw) + np.uint64(1 << 23))
            >> np.uint64(24)).astype(np.uint8)


def gaussian_blur(img, radius):
    ww, fw, fr = blur_consts(radius)
    assert int(fr) == 0, "radius >= 1 is out of scope"
    out = img
    for _ in range(3):
        out = _box_pass(out, ww, fw)
    out = out.transpose(1, 0, 2)
    for _ in range(3):
        out = _box_pass(out, ww, fw)
    return np.ascontiguousarray(out.transpose(1, 0, 2))


def crop_pair(img, mask, params, crop):
    """uint8 image [H, W, 3] + label-id mask [H, W] -> (uint8 crop [crop, crop, 3], label-id crop
    [crop, crop] uint8) exactly as PIL produces them for ``params``."""
    flip, ow, oh, padw, padh, x1, y1, blur = params
    H, W = mask.shape
    if flip:
        img, mask = img[:, ::-1], mask[:, ::-1]
    xmin, xcnt, xk = bilinear_tables(W, ow, x1, crop)
    ymin, ycnt, yk = bilinear_tables(H, oh, y1, crop)
    # horizontal pass on the rows the vertical pass reads, then the vertical pass
    r0 = int(ymin.min()) if len(ymin) else 0
    r1 = int((ymin + ycnt).max())
    r0 = min(r0, r1)
    hor = _resample_axis(img[r0:r1], xmin, xcnt, xk)
    ver = _resample_axis(hor.transpose(1, 0, 2), ymin - r0, ycnt, yk).transpose(1, 0, 2)
    out = np.ascontiguousarray(ver)
    if blur is not None:
        out = gaussian_blur(out, blur)
    nx = nearest_table(W, ow, x1, crop)
    ny = nearest_table(H, oh, y1, crop)
    m = mask[np.maximum(ny, 0)][:, np.maximum(nx, 0)].astype(np.uint8)
    m[ny < 0, :] = 0
    m[:, nx < 0] = 0
    return out, m


CITYSCAPES_KEY = np.array([-1, -1, -1, -1, -1, -1, -1, -1, 0, 1, -1, -1, 2, 3, 4, -1, -1, -1, 5,
                           -1, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, -1, -1, 16, 17, 18])


def transform(img, mask, params, crop, key=CITYSCAPES_KEY, offset=1):
    """-> (uint8 crop, int64 target) of one sample."""
    u8, m = crop_pair(img, mask, params, crop)
    return u8, np.asarray(key, np.int64)[m.astype(np.int64) + offset]

