"""GPU input path: what the reference's DataLoader does per image on the
CPU, done for a whole batch on the device.

* ``normalize_images``: ``transforms.ToTensor()`` + ``transforms.Normalize(mean, std)``
  (train.py:104-107, eval.py:22-25, demo.py:37-40) of uint8 HWC RGB images -> NCHW fp32/bf16
  network input, bit-identical to torchvision's fp32 result.
* ``CityscapesLabelMap``: ``CitySegmentation._class_to_index`` (data_loader/cityscapes.py:56-71),
  dataset label ids -> train ids (ignored ids -> -1) through a device lookup table.
* ``SyncTransform``: the train / val augmentation in front of those two,
  ``CitySegmentation._sync_transform`` / ``_val_sync_transform`` (data_loader/cityscapes.py:93-150),
  fused with them into one launch per batch; the same pixels as PIL.
"""
import collections
import ctypes
import random

import numpy as np
import torch

from . import _lib

IMAGENET_MEAN = (.485, .456, .406)
IMAGENET_STD = (.229, .224, .225)

# data_loader/cityscapes.py:58-64 (label id v -> _key[v + 1], v in [-1, 33])
CITYSCAPES_KEY = (-1, -1, -1, -1, -1, -1, -1, -1, 0, 1, -1, -1, 2, 3, 4, -1, -1, -1, 5, -1, 6, 7,
                  8, 9, 10, 11, 12, 13, 14, 15, -1, -1, 16, 17, 18)


def normalize_images(images, mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype=torch.float32):
    """uint8 [N, H, W, 3] (or [H, W, 3]) device tensor -> normalised [N, 3, H, W] ``dtype``."""
    if images.dim() == 3:
        images = images.unsqueeze(0)
    if images.dim() != 4 or images.shape[3] != 3 or images.dtype != torch.uint8:
        raise RuntimeError("normalize_images: expected uint8 [N, H, W, 3], got %s %s"
                           % (images.dtype, tuple(images.shape)))
    if not images.is_cuda:
        raise RuntimeError("normalize_images: the HIP path needs a ROCm device tensor")
    if dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("normalize_images: dtype must be float32 or bfloat16")
    images = images.contiguous()
    N, H, W, _ = images.shape
    out = torch.empty((N, 3, H, W), dtype=dtype, device=images.device)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    _lib.call("fscnn_normalize_u8", _lib.ptr(images), N, H, W, ctypes.cast(m, ctypes.c_void_p),
              ctypes.cast(s, ctypes.c_void_p), _lib.ptr(out), _lib.dtype_code(dtype),
              _lib.stream_ptr(images.device))
    return out


class CityscapesLabelMap:
    """``CitySegmentation._class_to_index`` on the device.

    Like the reference (data_loader/cityscapes.py:66-68 ``assert value in self._mapping``), a
    label id outside the table raises ``AssertionError`` (one device reduction + host read per
    call: this is the data-loading path, where the reference inspects every mask on the CPU).
    ``strict=False`` maps such ids to -1 (ignored) without the check."""

    def __init__(self, key=CITYSCAPES_KEY, offset=1, device="cuda", strict=True):
        self.lut = torch.tensor(key, dtype=torch.int64, device=device)
        self.offset = int(offset)
        self.strict = bool(strict)

    def __call__(self, mask):
        if mask.dtype != torch.uint8 or not mask.is_cuda:
            raise RuntimeError("CityscapesLabelMap: expected a uint8 ROCm device tensor")
        mask = mask.contiguous()
        if self.strict and mask.numel():
            hi = int(mask.max())  # uint8 ids are >= 0 > -offset; valid ids are < len - offset
            assert hi < self.lut.numel() - self.offset, \
                "label id %d is not in the Cityscapes mapping" % hi
        out = torch.empty(mask.shape, dtype=torch.int64, device=mask.device)
        _lib.call("fscnn_remap_labels", _lib.ptr(mask), mask.numel(), _lib.ptr(self.lut),
                  self.lut.numel(), self.offset, -1, _lib.ptr(out), _lib.stream_ptr(mask.device))
        return out


# One sample's augmentation parameters: mirror, resized size (before the pad), zero pad on the
# right / bottom, the crop's origin in the resized + padded image, blur radius or None.
SyncParams = collections.namedtuple("SyncParams", "flip ow oh padw padh x1 y1 blur")

# include/fastscnn.h fscnn_sync_desc
_SYNC_DESC = np.dtype([("image", "<u8"), ("mask", "<u8")] + [(k, "<i4") for k in (
    "H", "W", "flip", "ow", "oh", "x1", "y1", "blur")] + [("ww", "<u4"), ("fw", "<u4")] + [
        (k, "<i4") for k in ("kx", "ky", "off_xb", "off_xk", "off_yb", "off_yk", "off_nx",
                             "off_ny")])
assert _SYNC_DESC.itemsize == 88


class SyncTransform:
    """``CitySegmentation._sync_transform`` / ``_val_sync_transform`` (data_loader/
    cityscapes.py:93-150; the same code in tusimple.py:168-208) for a batch on the device, in one
    launch, with PIL's integer resize and blur arithmetic: random mirror, random short-edge
    rescale (bilinear image / nearest mask), zero pad, random crop, optional Gaussian blur,
    ToTensor + Normalize and the label remap.  Full-resolution uint8 images and label-id masks go
    in, the network input ``[N, 3, crop, crop]`` and the targets ``[N, crop, crop]`` come out,
    pixel for pixel what the reference's DataLoader produces for the same parameters.

    ``sample`` draws like the reference does from ``random`` (same order, so ``seed=s`` gives
    the reference's values after ``random.seed(s)``).  Labels go through ``label_lut[id +
    lut_offset]`` (Cityscapes: ``_key``, offset 1; TuSimple's ``mask > 0`` is ``(0,) + (1,) *
    255`` with offset 0); ids outside the table become -1.  No host synchronisation: tables are
    built on the host into a ring of pinned staging buffers, copied asynchronously and consumed
    by the launch on the current stream."""

    RING = 4

    def __init__(self, base_size, crop_size, label_lut=CITYSCAPES_KEY, lut_offset=1,
                 mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype=torch.float32, seed=None):
        if dtype not in (torch.float32, torch.bfloat16):
            raise RuntimeError("SyncTransform: dtype must be float32 or bfloat16")
        if crop_size < 1 or base_size < 1:
            raise RuntimeError("SyncTransform: base_size and crop_size must be positive")
        self.base_size, self.crop_size = int(base_size), int(crop_size)
        self.label_lut = tuple(int(v) for v in label_lut)
        self.lut_offset = int(lut_offset)
        self.dtype = dtype
        self.rng = random.Random(seed)
        self._mean = (ctypes.c_float * 3)(*[float(v) for v in mean])
        self._std = (ctypes.c_float * 3)(*[float(v) for v in std])
        self._luts = {}    # device -> int64 table
        self._ring = []    # [pinned uint8 tensor, event of its last copy]
        self._slot = 0

    # ---- parameters ------------------------------------------------------------------------
    def sample(self, w, h):
        """The draws of ``_sync_transform`` (cityscapes.py:115-147) for a w x h image."""
        rng, base, crop = self.rng, self.base_size, self.crop_size
        flip = rng.random() < 0.5
        short = rng.randint(int(base * 0.5), int(base * 2.0))
        if h > w:
            ow = short
            oh = int(1.0 * h * ow / w)
        else:
            oh = short
            ow = int(1.0 * w * oh / h)
        padw = padh = 0
        if short < crop:
            padh = crop - oh if oh < crop else 0
            padw = crop - ow if ow < crop else 0
        x1 = rng.randint(0, ow + padw - crop)
        y1 = rng.randint(0, oh + padh - crop)
        blur = rng.random() if rng.random() < 0.5 else None
        return SyncParams(flip, ow, oh, padw, padh, x1, y1, blur)

    def val_params(self, w, h):
        """``_val_sync_transform`` (cityscapes.py:93-110): short edge -> crop, centre crop."""
        crop = self.crop_size
        if w > h:
            oh = crop
            ow = int(1.0 * w * oh / h)
        else:
            ow = crop
            oh = int(1.0 * h * ow / w)
        return SyncParams(False, ow, oh, 0, 0, int(round((ow - crop) / 2.)),
                          int(round((oh - crop) / 2.)), None)

    # ---- launch ----------------------------------------------------------------------------
    @staticmethod
    def _samples(images, masks):
        if isinstance(images, torch.Tensor):
            if images.dim() != 4 or masks.dim() != 3:
                raise RuntimeError("SyncTransform: expected images [N, H, W, 3] and masks [N, H, W]")
            images, masks = images.contiguous(), masks.contiguous()
        if len(images) != len(masks) or len(images) == 0:
            raise RuntimeError("SyncTransform: need as many masks as images (at least one)")
        out = []
        for im, mk in zip(images, masks):
            if im.dtype != torch.uint8 or mk.dtype != torch.uint8 or im.dim() != 3 or \
                    im.shape[2] != 3 or tuple(mk.shape) != tuple(im.shape[:2]):
                raise RuntimeError("SyncTransform: expected uint8 [H, W, 3] images with uint8 "
                                   "[H, W] masks, got %s %s / %s %s" % (
                                       im.dtype, tuple(im.shape), mk.dtype, tuple(mk.shape)))
            if not im.is_cuda or not mk.is_cuda or mk.device != im.device:
                raise RuntimeError("SyncTransform: the HIP path needs ROCm device tensors")
            out.append((im.contiguous(), mk.contiguous()))
        if any(im.device != out[0][0].device for im, _ in out):
            raise RuntimeError("SyncTransform: all samples must be on one device")
        return out

    def _staging(self, nbytes):
        """The next pinned slot of the ring, once the copy that last read it has completed."""
        if len(self._ring) < self.RING:
            self._ring.append([None, None])
        slot = self._ring[self._slot % len(self._ring)]
        self._slot += 1
        if slot[1] is not None:
            slot[1].synchronize()  # (RING steps old: complete unless the host runs far ahead)
        if slot[0] is None or slot[0].numel() < nbytes:
            slot[0] = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, pin_memory=True)
        return slot

    def __call__(self, images, masks, params=None, return_u8=False):
        """-> (x [N, 3, crop, crop] ``dtype``, target [N, crop, crop] int64) and, with
        ``return_u8``, the uint8 crop [N, crop, crop, 3] before normalisation.  ``images`` /
        ``masks``: uint8 device tensors [N, H, W, 3] / [N, H, W], or lists of per-image tensors
        of any sizes.  ``params``: one ``SyncParams`` per sample (default: ``sample``)."""
        samples = self._samples(images, masks)
        N, crop = len(samples), self.crop_size
        if params is None:
            params = [self.sample(im.shape[1], im.shape[0]) for im, _ in samples]
        if len(params) != N:
            raise RuntimeError("SyncTransform: %d parameter sets for %d samples" % (len(params), N))
        dev = samples[0][0].device
        lib = _lib.load()

        # table sizes first (taps per position of each resize), then one blob: descriptors + tables
        ks = ctypes.c_int()
        layout = []
        nint = (N * _SYNC_DESC.itemsize + 15) // 16 * 4
        for (im, _), p in zip(samples, params):
            p = SyncParams(*p)
            H, W = im.shape[0], im.shape[1]
            if p.x1 < 0 or p.y1 < 0 or p.x1 + crop > p.ow + p.padw or p.y1 + crop > p.oh + p.padh:
                raise RuntimeError("SyncTransform: crop window outside the image: %s" % (p,))
            k = []
            for insz, outsz in ((W, p.ow), (H, p.oh)):
                _lib.check(lib.fscnn_sync_tables(insz, outsz, 0, 1, 0, None, None, None,
                                                 ctypes.byref(ks)), "fscnn_sync_tables")
                k.append(ks.value)
            offs = {}
            for name, n in (("off_xb", 2 * crop), ("off_xk", crop * k[0]), ("off_yb", 2 * crop),
                            ("off_yk", crop * k[1]), ("off_nx", crop), ("off_ny", crop)):
                offs[name] = nint
                nint += n
            layout.append((p, H, W, k, offs))
        nbytes = nint * 4
        slot = self._staging(nbytes)
        host = slot[0].numpy()
        base = host.ctypes.data
        desc = host[:N * _SYNC_DESC.itemsize].view(_SYNC_DESC)
        ww, fw = ctypes.c_uint(), ctypes.c_uint()
        for n, ((im, mk), (p, H, W, k, offs)) in enumerate(zip(samples, layout)):
            _lib.check(lib.fscnn_sync_tables(W, p.ow, p.x1, crop, k[0], base + 4 * offs["off_xb"],
                                             base + 4 * offs["off_xk"], base + 4 * offs["off_nx"],
                                             None), "fscnn_sync_tables")
            _lib.check(lib.fscnn_sync_tables(H, p.oh, p.y1, crop, k[1], base + 4 * offs["off_yb"],
                                             base + 4 * offs["off_yk"], base + 4 * offs["off_ny"],
                                             None), "fscnn_sync_tables")
            ww.value = fw.value = 0
            if p.blur is not None:
                _lib.check(lib.fscnn_sync_blur_weights(float(p.blur), ctypes.byref(ww),
                                                       ctypes.byref(fw)), "fscnn_sync_blur_weights")
            desc[n] = (im.data_ptr(), mk.data_ptr(), H, W, int(bool(p.flip)), p.ow, p.oh, p.x1,
                       p.y1, int(p.blur is not None), ww.value, fw.value, k[0], k[1],
                       offs["off_xb"], offs["off_xk"], offs["off_yb"], offs["off_yk"],
                       offs["off_nx"], offs["off_ny"])

        lut = self._luts.get(dev)
        if lut is None:
            lut = self._luts[dev] = torch.tensor(self.label_lut, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            blob = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            blob.copy_(slot[0][:nbytes], non_blocking=True)
            if slot[1] is None:
                slot[1] = torch.cuda.Event()
            slot[1].record()
            x = torch.empty((N, 3, crop, crop), dtype=self.dtype, device=dev)
            target = torch.empty((N, crop, crop), dtype=torch.int64, device=dev)
            u8 = torch.empty((N, crop, crop, 3), dtype=torch.uint8, device=dev) if return_u8 else None
            _lib.call("fscnn_sync_transform", base, _lib.ptr(blob), nbytes, N, crop, _lib.ptr(lut),
                      lut.numel(), self.lut_offset, ctypes.cast(self._mean, ctypes.c_void_p),
                      ctypes.cast(self._std, ctypes.c_void_p), _lib.ptr(x),
                      _lib.dtype_code(self.dtype), _lib.ptr(target), _lib.ptr(u8),
                      _lib.stream_ptr(dev))
        return (x, target, u8) if return_u8 else (x, target)

    def val(self, images, masks, return_u8=False):
        """The validation path: ``_val_sync_transform``'s deterministic resize + centre crop."""
        samples = self._samples(images, masks)
        params = [self.val_params(im.shape[1], im.shape[0]) for im, _ in samples]
        return self([im for im, _ in samples], [mk for _, mk in samples], params, return_u8)
