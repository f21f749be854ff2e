"""A numpy restatement of the overlay law of include/fastscnn.h (csrc/overlay.hip): the nearest
source pixel by exact integer division, the lane / palette colour, and the blend with every fp32
operation as a separate np.float32 ufunc, then np.rint (half to even) and a clip.

Frames are ``[N, 3, h, w]`` (or ``[N, h, w, 3]`` with ``channels_last``), masks ``[N, Hm, Wm]``
uint8; everything is host numpy."""
import numpy as np


def nearest_index(size, src):
    """Source index of every output index of a ``src -> size`` nearest resize: ``(x * src) // size``."""
    return (np.arange(size, dtype=np.int64) * int(src)) // int(size)


def resize_nearest(mask, h, w):
    """``[N, Hm, Wm]`` -> ``[N, h, w]`` by the law's source map (the identity at equal sizes)."""
    sy = nearest_index(h, mask.shape[1])
    sx = nearest_index(w, mask.shape[2])
    return mask[:, sy[:, None], sx[None, :]]


def colors(labels, color=(0, 255, 0), palette=None):
    """``[N, h, w]`` label bytes (lane mode) or class ids (palette mode) -> uint8 ``[N, h, w, 3]``."""
    if palette is None:
        c = np.asarray(color, dtype=np.uint8).reshape(1, 1, 1, 3)
        return np.where((labels != 0)[..., None], c, np.uint8(0)).astype(np.uint8)
    pal = np.asarray(palette, dtype=np.uint8).reshape(-1, 3)
    full = np.zeros((256, 3), dtype=np.uint8)
    full[:pal.shape[0]] = pal
    return full[labels.astype(np.int64)]


def blend(a, o, frame_weight=1.0, alpha=0.5, gamma=0.0):
    """``uint8(clip(rint(((a * fw) + (o * alpha)) + gamma), 0, 255))``, NaN -> 0; ``a`` and ``o``
    of one shape, any dtype that converts to fp32 exactly."""
    a = np.asarray(a).astype(np.float32)
    o = np.asarray(o).astype(np.float32)
    fw, al, ga = np.float32(frame_weight), np.float32(alpha), np.float32(gamma)
    with np.errstate(all="ignore"):
        p = np.multiply(a, fw, dtype=np.float32)
        q = np.multiply(o, al, dtype=np.float32)
        s = np.add(p, q, dtype=np.float32)
        t = np.add(s, ga, dtype=np.float32)
        r = np.clip(np.rint(t), np.float32(0), np.float32(255))
    return np.where(np.isnan(r), np.float32(0), r).astype(np.uint8)


def overlay(frames, mask, alpha=0.5, color=(0, 255, 0), palette=None, frame_weight=1.0, gamma=0.0,
            channels_last=False, ids=None):
    """The law on host arrays.  ``mask`` holds the label bytes; in palette mode the class ids are
    ``ids`` (default: the mask bytes themselves, as in the stand-alone form).  Returns
    ``(overlay in the layout of the frames, the mask resized to the frames)``."""
    frames = np.asarray(frames)
    h, w = frames.shape[1:3] if channels_last else frames.shape[2:4]
    labels = resize_nearest(np.asarray(mask), h, w)
    src = labels if palette is None or ids is None else resize_nearest(np.asarray(ids), h, w)
    o = colors(src, color, palette)  # [N, h, w, 3]
    if not channels_last:
        o = o.transpose(0, 3, 1, 2)
    return blend(frames, o, frame_weight, alpha, gamma), labels
