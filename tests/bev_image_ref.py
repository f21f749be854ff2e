"""A numpy restatement of the frame-warp law of include/fastscnn.h (csrc/bev_image.hip): the
coordinates with every operation a separate float64 ufunc (nothing is fused), ``32.0 / W``, the
clamp to the int range, ``rint`` (half to even), the split into integer and 5-bit fraction, four
taps that each count as 0 outside the frame, int64 accumulation and ``(S + 512) >> 10``; plus the
blend of the warped frame with the lane colour, which is the overlay law of tests/overlay_ref.py.

Frames are ``[N, 3, h, w]`` (or ``[N, h, w, 3]`` with ``channels_last``) uint8, bird's-eye masks
``[N, Hb, Wb]`` uint8; everything is host numpy."""
import numpy as np

import overlay_ref

INT_MIN, INT_MAX = float(-2 ** 31), float(2 ** 31 - 1)


def fixed_index(m, hb, wb, bits=5):
    """``(fx, fy, info)``: the source position of every view pixel in ``1 / 2**bits`` pixel, int64
    ``[hb, wb]``, and ``info`` = the number of pixels with ``W == 0`` and of pixels where the clamp
    to the int range was taken (``bits`` other than 5 only serve the law's own checks)."""
    m = np.asarray(m, dtype=np.float64).reshape(9)
    x = np.arange(wb, dtype=np.float64)[None, :]
    y = np.arange(hb, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        X = np.add(np.add(np.multiply(m[0], x), np.multiply(m[1], y)), m[2])
        Y = np.add(np.add(np.multiply(m[3], x), np.multiply(m[4], y)), m[5])
        W = np.add(np.add(np.multiply(m[6], x), np.multiply(m[7], y)), m[8])
        zero = np.broadcast_to(W == 0, (hb, wb))
        W = np.where(W != 0, np.divide(float(2 ** bits), np.where(W != 0, W, 1.0)), 0.0)
        out = []
        clamped = np.zeros((hb, wb), dtype=bool)
        for v in (np.multiply(X, W), np.multiply(Y, W)):
            v = np.broadcast_to(v, (hb, wb))
            clamped |= ~((v < INT_MAX) & (v > INT_MIN))
            v = np.where(v < INT_MAX, v, INT_MAX)
            v = np.where(v > INT_MIN, v, INT_MIN)
            out.append(np.rint(v).astype(np.int64))
    return out[0], out[1], {"w_zero": int(zero.sum()), "clamped": int(clamped.sum())}


def warp(frames, m, hb, wb, channels_last=False, bits=5, info=None):
    """The warped frames, uint8 in the layout of the frames.  ``info`` (a dict) receives
    ``fixed_index``'s counts and ``inside``, the number of view pixels with a tap of non-zero weight in the frame."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 4
    f = frames if channels_last else frames.transpose(0, 2, 3, 1)  # [N, h, w, 3]
    h, w = f.shape[1:3]
    fx, fy, counts = fixed_index(m, hb, wb, bits)
    one = 1 << bits
    sx, sy = fx >> bits, fy >> bits  # arithmetic: floor
    ax, ay = fx & (one - 1), fy & (one - 1)
    acc = np.zeros((f.shape[0], hb, wb, 3), dtype=np.int64)
    any_in = np.zeros((hb, wb), dtype=bool)
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        tx, ty = sx + dx, sy + dy
        wt = (ax if dx else one - ax) * (ay if dy else one - ay)
        ok = (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
        any_in |= ok & (wt != 0)
        tap = np.zeros((f.shape[0], hb, wb, 3), dtype=np.int64)
        tap[:, ok] = f[:, ty[ok], tx[ok]]
        acc += wt[None, :, :, None] * tap
    out = ((acc + (1 << (2 * bits - 1))) >> (2 * bits)).astype(np.uint8)
    if info is not None:
        info.update(counts, inside=int(any_in.sum()))
    return np.ascontiguousarray(out if channels_last else out.transpose(0, 3, 1, 2))


def nearest(frames, m, hb, wb, channels_last=False):
    """The frames warped by the nearest-neighbour law of the mask (for the recorded run's table)."""
    import bev_ref
    frames = np.asarray(frames)
    f = frames if channels_last else frames.transpose(0, 2, 3, 1)
    ok, sx, sy = bev_ref.inside(m, hb, wb, f.shape[1], f.shape[2])
    out = np.zeros((f.shape[0], hb, wb, 3), dtype=np.uint8)
    out[:, ok] = f[:, sy[ok], sx[ok]]
    return out if channels_last else out.transpose(0, 3, 1, 2)


def blend(image, mask, alpha=0.5, color=(0, 255, 0), frame_weight=1.0, gamma=0.0,
          channels_last=False):
    """The segmented picture: the overlay law's lane mode on the warped frames ``image`` and the
    bird's-eye mask ``[N, Hb, Wb]`` of the same size."""
    image, mask = np.asarray(image), np.asarray(mask)
    hb, wb = image.shape[1:3] if channels_last else image.shape[2:4]
    assert mask.shape == (image.shape[0], hb, wb)
    return overlay_ref.overlay(image, mask, alpha=alpha, color=color, frame_weight=frame_weight,
                               gamma=gamma, channels_last=channels_last)[0]


def planted_frames(n, h, w, channels_last=False, seed=0):
    """Random bytes with rows and columns of 0 and 255 planted at the borders."""
    rng = np.random.default_rng(7919 * h + 31 * w + n + seed)
    f = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    f[:, 0] = 255
    f[:, h - 1] = 0
    f[:, :, 0] = 0
    f[:, :, w - 1] = 255
    if h > 4 and w > 4:
        f[:, 1, 1:w - 1] = 0
        f[:, 1:h - 1, w - 2] = 255
    f = np.ascontiguousarray(f if channels_last else f.transpose(0, 3, 1, 2))
    f.setflags(write=False)
    return f
