"""The lane overlay: the picture a person looks at, blended on the device.

Every consumer of the exported model in the reference builds the same image on the host from the
frame and the mask -- ``create_visualization`` (``kuruma/core/preprocessing.py:85-104``: green where
``mask > 0``, then ``cv2.addWeighted(frame, 1.0, green, alpha, 0)``), the evaluation scripts with a
per-class colour image at 0.7 / 0.3 or 0.6 / 0.4 -- after ``postprocess_matched_resolution``
(``:53-79``) brought the mask back to the camera frame's size with a nearest-neighbour resize.

``overlay_mask`` does that in one launch for a mask that is already in device memory (ground truth,
a ``bird_eye`` mask over a warped image, ``predict``'s output); ``EndToEndFastSCNN.overlay`` is the
same blend fused behind the backbone (``csrc/overlay.hip``).  The law -- nearest source pixel by
exact integer division, ``((a * frame_weight) + (colour * alpha)) + gamma`` with every operation
rounded to fp32 on its own, round half to even, saturate -- is stated in ``include/fastscnn.h``.
Colours are given in the frames' own channel order.
"""
import ctypes

import numpy as np

__all__ = ["overlay_mask", "MAX_CLASSES"]

MAX_CLASSES = 32  # rows of the fused tail's colour table (include/fastscnn.h)

_FRAME_CODES = {"torch.uint8": 3, "torch.float32": 0, "torch.float16": 2, "torch.bfloat16": 1}


def _color3(color):
    c = [int(v) for v in color] if hasattr(color, "__len__") else None
    if c is None or len(c) != 3 or min(c) < 0 or max(c) > 255:
        raise RuntimeError("overlay: color is three values 0 .. 255 in the frames' channel order, "
                           "got %s" % (color,))
    return c


def _palette_host(palette):
    """A palette (tensor or sequence) as a contiguous host uint8 ``[P, 3]`` array, 1 <= P <= 256."""
    import torch
    if isinstance(palette, torch.Tensor):
        if palette.dtype != torch.uint8:
            raise RuntimeError("overlay: the palette is uint8 [P, 3], not %s" % (palette.dtype,))
        p = palette.detach().cpu().numpy()
    else:
        p = np.asarray(palette)
        if p.dtype.kind not in "iu" or (p.size and (p.min() < 0 or p.max() > 255)):
            raise RuntimeError("overlay: the palette holds integers 0 .. 255")
        p = p.astype(np.uint8)
    if p.ndim != 2 or p.shape[1] != 3 or not 1 <= p.shape[0] <= 256:
        raise RuntimeError("overlay: the palette is uint8 [P, 3] with 1 <= P <= 256 rows, got %s"
                           % (tuple(p.shape),))
    return np.ascontiguousarray(p)


def class_table(num_classes, scale, color, palette):
    """The fused tail's one form for both modes: ``(uint8 [32][3] colour of class id, 32-bit mask
    whose bit id tells whether class id gets its colour)``.  Lane mode: the colour in every row,
    bit id = ``(id * scale) mod 256 != 0``; palette mode: the palette's rows, bit id = ``id < P``."""
    n = min(int(num_classes), MAX_CLASSES)
    table = np.zeros((MAX_CLASSES, 3), dtype=np.uint8)
    bits = 0
    if palette is None:
        table[:n] = np.asarray(_color3(color), dtype=np.uint8)
        for c in range(n):
            if (c * int(scale)) & 255:
                bits |= 1 << c
    else:
        p = _palette_host(palette)
        rows = min(n, p.shape[0])
        table[:rows] = p[:rows]
        bits = (1 << rows) - 1
    return (ctypes.c_ubyte * (MAX_CLASSES * 3))(*table.reshape(-1).tolist()), bits


def check_frames(frames, channels_last, who):
    """Frames as the deployment front end takes them: ``(contiguous frames, N, h, w)``."""
    import torch
    if not isinstance(frames, torch.Tensor) or frames.dim() != 4:
        raise RuntimeError("%s: expected 4-d frames" % who)
    if not frames.is_cuda:
        raise RuntimeError("%s: the HIP path needs a ROCm device tensor (got %s); move the frames "
                           "to 'cuda'" % (who, frames.device))
    if str(frames.dtype) not in _FRAME_CODES:
        raise RuntimeError("%s: frames are uint8 / fp32 / fp16 / bf16, not %s" % (who, frames.dtype))
    if frames.shape[3 if channels_last else 1] != 3:
        raise RuntimeError("%s: expected frames %s, got %s"
                           % (who, "[N, h, w, 3]" if channels_last else "[N, 3, h, w]",
                              tuple(frames.shape)))
    n = int(frames.shape[0])
    h, w = (int(v) for v in (frames.shape[1:3] if channels_last else frames.shape[2:4]))
    if n < 1 or h < 2 or w < 2:
        raise RuntimeError("%s: frames %s need N >= 1 and h, w >= 2" % (who, tuple(frames.shape)))
    return frames.contiguous(), n, h, w


def overlay_mask(frames, mask, alpha=0.5, color=(0, 255, 0), palette=None, frame_weight=1.0,
                 gamma=0.0, return_mask=False, channels_last=False):
    """The overlay of ``frames`` (uint8 / fp32 / fp16 / bf16 holding 0..255, ``[N, 3, h, w]`` or
    ``[N, h, w, 3]`` with ``channels_last``) with a uint8 ``mask`` ``[N, Hm, Wm]`` on the same ROCm
    device (``fscnn_overlay_mask``): uint8 in the layout of the frames, always a fresh buffer.

    The mask is resized to the frame with the nearest-neighbour law of ``cv2.INTER_NEAREST``
    (source index ``x * Wm // w``).  Lane mode (``palette=None``, the reference's
    ``create_visualization``): ``color`` where the mask byte is not 0.  Palette mode: ``palette`` is
    a uint8 ``[P, 3]`` tensor or sequence (1 <= P <= 256) and the mask byte a class id; ids from
    ``P`` on get no colour.  Every pixel is ``frame * frame_weight + colour * alpha + gamma`` in
    fp32, rounded half to even and saturated (``cv2.addWeighted``).  ``return_mask=True`` returns
    ``(overlay, mask resized to the frames)``."""
    import torch

    from . import _lib
    frames, n, h, w = check_frames(frames, channels_last, "overlay_mask")
    if not isinstance(mask, torch.Tensor) or mask.dim() != 3 or mask.dtype != torch.uint8:
        raise RuntimeError("overlay_mask: expected a uint8 mask [N, H, W]")
    if mask.device != frames.device:
        raise RuntimeError("overlay_mask: the HIP path needs the mask on the frames' ROCm device "
                           "(got %s and %s)" % (mask.device, frames.device))
    if int(mask.shape[0]) != n or min(mask.shape[1:]) < 1:
        raise RuntimeError("overlay_mask: %d frames but a mask of shape %s"
                           % (n, tuple(mask.shape)))
    mask = mask.contiguous()
    dev = frames.device
    c3 = pal = None
    rows = 0
    if palette is None:
        c3 = (ctypes.c_ubyte * 3)(*_color3(color))
    else:
        pal = torch.from_numpy(_palette_host(palette)).to(dev)
        rows = int(pal.shape[0])
    out = torch.empty(frames.shape, dtype=torch.uint8, device=dev)
    resized = torch.empty((n, h, w), dtype=torch.uint8, device=dev) if return_mask else None
    with torch.cuda.device(dev):
        _lib.call("fscnn_overlay_mask", _lib.ptr(frames), _FRAME_CODES[str(frames.dtype)],
                  int(bool(channels_last)), n, h, w, _lib.ptr(mask), int(mask.shape[1]),
                  int(mask.shape[2]), c3, _lib.ptr(pal), rows, float(frame_weight), float(alpha),
                  float(gamma), _lib.ptr(out), _lib.ptr(resized), _lib.stream_ptr(dev))
    return (out, resized) if return_mask else out
