"""The deployment model: raw camera frames in, class probabilities (or the lane mask) out.

Drop-in for ``EndToEndFastSCNN`` of the reference's ``export_onnx_fixed.py:34-98``, the model that
is exported for the car and that ``kuruma/core/inference.py``, ``onnx_single_image_inference.py``
and ``lane_dashboard_e2e.py`` run:

* resize the 0..255 frame to ``base_size x base_size`` (bilinear, ``align_corners=False``),
  ``/ 255`` and optionally ``(x - mean) / std``            (``EndToEndPreprocessing``, :62-98);
* the backbone;
* resize the full-resolution logits back to ``input_size`` (bilinear, ``align_corners=False``) and
  softmax over the classes (:53-58); the host then takes ``argmax * 255`` as the lane mask
  (``kuruma/core/preprocessing.py:53-79``) -- here ``predict(frames, scale=255)``.

Same constructor arguments in the same order, same sub-module names (``backbone``,
``preprocessor`` with ``mean`` / ``std`` buffers only when both are given), hence the same
``state_dict()`` keys.  The call is two launches around the backbone's inference plan
(``csrc/e2e.hip``): the front end writes the backbone's input straight from the frame, and the
tail reads the 1/8-resolution logits and writes only the ``input_size`` output -- neither the
full-resolution logits nor, for ``predict``, any probability is ever formed.

``bird_eye`` is a second tail (``csrc/bev.hip``) for what the car's code does next with the lane
mask (``kuruma/vision/transform.py:130-201``, ``path_planning.py:188-293``): from the same
1/8-resolution logits straight to the bird's-eye mask and the per-row table the centreline is
read from (``bev.centerline``), without writing the frame-size mask.  ``bird_eye_view`` adds the
other half of ``transform_image_and_mask``, the camera frame warped bilinearly to the same view,
and the segmented bird's-eye picture, in one more launch (``csrc/bev_image.hip``).

``overlay`` is a third tail (``csrc/overlay.hip``) for the picture a person looks at
(``create_visualization``, ``kuruma/core/preprocessing.py:85-104``): the frame blended with the
lane colour or a class palette, from the same 1/8-resolution logits and the frame that is already
in device memory, in one launch.
"""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from . import bev as _bev
from . import path as _path
from .fast_scnn import E_UNSUPPORTED

__all__ = ["EndToEndFastSCNN", "EndToEndPreprocessing"]

_BEV_FUSED_MAX_PIXELS = 8 * 208 * 108  # bird_eye: largest measured total the fused tail won or tied

_FRAME_DTYPES = {torch.uint8: _lib.DT_U8, torch.float32: _lib.DT_F32, torch.float16: _lib.DT_F16,
                 torch.bfloat16: _lib.DT_BF16}


class EndToEndPreprocessing(nn.Module):
    """export_onnx_fixed.py:62-98: holds the normalisation constants; the arithmetic runs in the
    wrapper's front-end kernel."""

    def __init__(self, input_size=(640, 360), base_size=1024, mean=None, std=None):
        super().__init__()
        self.input_size = input_size
        self.base_size = base_size
        if mean is not None and std is not None:
            self.register_buffer("mean", torch.tensor(mean).view(1, 3, 1, 1))
            self.register_buffer("std", torch.tensor(std).view(1, 3, 1, 1))
        else:
            self.mean = None
            self.std = None

    def forward(self, *args, **kwargs):  # pragma: no cover - guard
        raise RuntimeError("EndToEndPreprocessing is a buffer container; call the "
                           "EndToEndFastSCNN module")


class EndToEndFastSCNN(nn.Module):
    """``EndToEndFastSCNN(backbone_model, input_size=(W, H), base_size, mean, std, apply_softmax)``
    of the reference, plus three trailing keywords:

    ``dtype``          arithmetic of the backbone and dtype of the output: fp32, fp16 (the Atlas
                       deployment's) or bf16; an active ``torch.autocast("cuda")`` overrides it
    ``channels_last``  frames are ``[N, h, w, 3]`` (a camera / OpenCV frame) instead of
                       ``[N, 3, h, w]``
    ``bgr``            frames carry their channels as B, G, R

    Frames hold 0..255 values as uint8, fp32, fp16 or bf16; any ``h, w >= 2`` is taken, and the
    output size is always ``input_size``, as in the reference.  The backbone must be in eval mode
    and everything on a ROCm device.  ``_last_fused`` tells whether the last call ran the fused
    tail or the unfused route (geometries the tail does not take, ``FSCNN_E2E_FUSED=0``)."""

    def __init__(self, backbone_model, input_size=(640, 360), base_size=1024, mean=None, std=None,
                 apply_softmax=True, dtype=torch.float32, channels_last=False, bgr=False):
        super().__init__()
        if base_size < 32:
            raise RuntimeError("EndToEndFastSCNN: base_size %d too small (the backbone needs "
                               ">= 32)" % base_size)
        if dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise RuntimeError("EndToEndFastSCNN: dtype %s (fp32 / fp16 / bf16)" % (dtype,))
        if len(input_size) != 2 or min(input_size) < 1:
            raise RuntimeError("EndToEndFastSCNN: input_size is (W, H), got %s" % (input_size,))
        self.backbone = backbone_model
        self.preprocessor = EndToEndPreprocessing(input_size, base_size, mean, std)
        self.apply_softmax = apply_softmax
        self.input_size = input_size  # (W, H) of the output
        self.base_size = base_size
        self.dtype = dtype
        self.channels_last = channels_last
        self.bgr = bgr
        object.__setattr__(self, "_last_fused", None)
        object.__setattr__(self, "_norm", None)  # (key, host mean[3], host std[3])

    # ---- pieces ---------------------------------------------------------------------------------
    def _compute_dtype(self):
        if torch.is_autocast_enabled("cuda"):
            dt = torch.get_autocast_dtype("cuda")
            if dt in (torch.float16, torch.bfloat16):
                return dt
            raise RuntimeError("EndToEndFastSCNN: unsupported autocast dtype %s" % (dt,))
        return self.dtype

    def _norm_host(self):
        """The mean / std buffers as host float[3] arrays (what the library takes), refreshed when
        the buffers were written (load_state_dict) or moved."""
        m, s = self.preprocessor.mean, self.preprocessor.std
        if m is None or s is None:
            return None, None
        key = (m.data_ptr(), m._version, s.data_ptr(), s._version)
        if self._norm is None or self._norm[0] != key:
            hm = (ctypes.c_float * 3)(*[float(v) for v in m.detach().float().reshape(3).cpu()])
            hs = (ctypes.c_float * 3)(*[float(v) for v in s.detach().float().reshape(3).cpu()])
            object.__setattr__(self, "_norm", (key, hm, hs))
        return self._norm[1], self._norm[2]

    def _check(self, frames):
        if self.backbone.training:
            raise RuntimeError("EndToEndFastSCNN is the inference pipeline; call model.eval() first")
        if not isinstance(frames, torch.Tensor) or frames.dim() != 4:
            raise RuntimeError("EndToEndFastSCNN: expected 4-d frames")
        if not frames.is_cuda:
            raise RuntimeError("EndToEndFastSCNN: the HIP path needs a ROCm device tensor (got %s); "
                               "move the model and the frames to 'cuda'" % (frames.device,))
        if frames.dtype not in _FRAME_DTYPES:
            raise RuntimeError("EndToEndFastSCNN: frames are uint8 / fp32 / fp16 / bf16, not %s"
                               % (frames.dtype,))
        cdim = 3 if self.channels_last else 1
        if frames.shape[cdim] != 3:
            raise RuntimeError("EndToEndFastSCNN: expected frames %s, got %s"
                               % ("[N, h, w, 3]" if self.channels_last else "[N, 3, h, w]",
                                  tuple(frames.shape)))
        N = frames.shape[0]
        h, w = (frames.shape[1:3] if self.channels_last else frames.shape[2:4])
        if N < 1 or h < 2 or w < 2:
            raise RuntimeError("EndToEndFastSCNN: frames %s need N >= 1 and h, w >= 2"
                               % (tuple(frames.shape),))
        return frames.contiguous(), int(N), int(h), int(w)

    def preprocess(self, frames, dtype=None):
        """The front end alone: the backbone's input ``[N, 3, base, base]`` in ``dtype``."""
        frames, N, h, w = self._check(frames)
        dt = self._compute_dtype() if dtype is None else dtype
        return self._pre(frames, N, h, w, dt)

    def _pre(self, frames, N, h, w, dt):
        base = self.base_size
        x = torch.empty((N, 3, base, base), dtype=dt, device=frames.device)
        hm, hs = self._norm_host()
        with torch.cuda.device(frames.device):
            _lib.call("fscnn_e2e_pre", _lib.ptr(frames), _FRAME_DTYPES[frames.dtype],
                      int(self.channels_last), int(self.bgr), N, h, w, base, hm, hs, _lib.ptr(x),
                      _lib.dtype_code(dt), _lib.stream_ptr(frames.device))
        return x

    def _run(self, frames, probs, scale):
        """One pipeline call: probabilities / logits (``probs``) or the scaled labels."""
        frames, N, h, w = self._check(frames)
        bb, dev = self.backbone, frames.device
        dt = self._compute_dtype()
        wo, ho = int(self.input_size[0]), int(self.input_size[1])
        base, C = self.base_size, bb.num_classes
        with torch.no_grad():
            nat = bb.native()
            ar = bb._exec_arena(dev)
            if ar["P"].device != dev:
                raise RuntimeError("EndToEndFastSCNN: frames on %s but parameters on %s"
                                   % (dev, ar["P"].device))
            plan, _, _ = nat.plan(N, base, base, _lib.dtype_code(dt), False, dev)
            lib = _lib.load()
            need = int(lib.fscnn_e2e_ws_bytes(plan))
            if need < 0:
                _lib.check(need, "fscnn_e2e_ws_bytes")
            ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
            out = torch.empty((N, C, ho, wo), dtype=dt, device=dev) if probs else None
            labels = None if probs else torch.empty((N, ho, wo), dtype=torch.uint8, device=dev)
            hm, hs = self._norm_host()
            with torch.cuda.device(dev):
                rc = lib.fscnn_forward_e2e(
                    plan, _lib.ptr(frames), _FRAME_DTYPES[frames.dtype], int(self.channels_last),
                    int(self.bgr), h, w, hm, hs, ho, wo, int(bool(self.apply_softmax)),
                    _lib.ptr(out), _lib.dtype_code(dt), _lib.ptr(labels), int(scale) & 255,
                    _lib.ptr(ar["P"]), _lib.ptr(ar["R"]), _lib.ptr(ar["NBT"]), _lib.ptr(ws),
                    _lib.stream_ptr(dev))
            fused = rc != E_UNSUPPORTED  # nothing was launched: the geometry check comes first
            if fused:
                _lib.check(rc, "fscnn_forward_e2e")
            else:
                out, labels = self._unfused(frames, N, h, w, dt, probs, scale)
        object.__setattr__(self, "_last_fused", fused)
        return out if probs else labels

    def _unfused(self, frames, N, h, w, dt, probs, scale):
        """The same results from full-resolution logits: the front-end kernel, ``backbone(x)[0]``
        and torch's resize plus softmax or argmax (export_onnx_fixed.py:47-58)."""
        wo, ho = int(self.input_size[0]), int(self.input_size[1])
        x = self._pre(frames, N, h, w, dt)
        y = self.backbone._run_forward(x, 0, dt=dt)[0][0]
        if y.shape[2] != ho or y.shape[3] != wo:
            y = F.interpolate(y, size=(ho, wo), mode="bilinear", align_corners=False)
        if probs:
            return (F.softmax(y, dim=1) if self.apply_softmax else y), None
        return None, (torch.argmax(y, 1) * (int(scale) & 255)).to(torch.uint8)

    # ---- the reference interface -----------------------------------------------------------------
    def forward(self, frames):
        """``[N, C, H, W]`` with ``(W, H) = input_size``: probabilities, or the resampled logits
        when ``apply_softmax`` is false."""
        return self._run(frames, True, 1)

    def predict(self, frames, scale=1):
        """uint8 ``[N, H, W]`` = ``(argmax over classes * scale)`` as uint8, wrapping the way
        numpy's ``astype(uint8)`` does; ``scale=255`` is the deployment's lane mask
        (kuruma/core/preprocessing.py:53-79).  Ties resolve to the lowest class, like
        ``torch.argmax``.  No probability tensor is written."""
        return self._run(frames, False, scale)

    # ---- the bird's-eye tail ----------------------------------------------------------------------
    @staticmethod
    def _fused_view(n, hb, wb):
        """Whether ``bird_eye`` takes the fused tail for a batch of ``n`` views of ``hb x wb``.
        The fused tail evaluates the class scores once per view pixel, the two-launch route once
        per frame pixel plus a byte gather per view pixel, so the fused tail pays while the views
        are small.  Measured (profiles/bev_time.md, 640 x 360 frames): not slower up to
        8 x 208 x 108 view pixels in all, slower from 1 x 1043 x 542 on; the rule keeps to what was
        measured."""
        return n * hb * wb <= _BEV_FUSED_MAX_PIXELS

    def bird_eye(self, frames, view_params, scale=255, min_width=10, return_mask=True,
                 fused=None):
        """``(bev_mask, rows)``: the lane mask ``predict(frames, scale)`` warped to the bird's-eye
        view of ``view_params`` (``BirdEyeView.params(..., source_size=input_size)[3]``: nearest
        neighbour, border 0, like the reference's ``cv2.warpPerspective`` of the mask) as uint8
        ``[N, Hb, Wb]`` (``None`` with ``return_mask=False``), and the int32 row table
        ``[N, Hb, 4]`` = per row (run_start, run_end, count, index_sum) of the non-zero pixels:
        the longest run of at least ``min_width`` (leftmost on ties, ``0, 0`` for none), and the
        count and the sum of the column indices; ``bev.centerline`` turns it into either
        centreline of the reference.  One launch after the backbone; the frame-size mask is not
        written.  Views wider than 8192 or taller than 65535 pixels are refused.

        ``fused``: ``None`` picks the route (``_fused_view``: the fused tail for small views,
        ``predict`` followed by ``fscnn_bev_mask`` for large ones, as measured), ``True`` /
        ``False`` force one; both give the same bits.  ``_last_fused`` tells which one ran."""
        wb, hb = (int(v) for v in view_params["output_size"])
        min_width = int(min_width)
        if not (1 <= wb <= _bev.MAX_WIDTH and 1 <= hb <= _bev.MAX_HEIGHT) or min_width < 1:
            raise RuntimeError("EndToEndFastSCNN.bird_eye: view %d x %d, min_width %d: the "
                               "bird's-eye tail takes widths 1 .. %d, heights 1 .. %d and "
                               "min_width >= 1" % (wb, hb, min_width, _bev.MAX_WIDTH,
                                                   _bev.MAX_HEIGHT))
        frames, N, h, w = self._check(frames)
        if N > 65535:
            raise RuntimeError("EndToEndFastSCNN.bird_eye: batch %d above 65535" % N)
        m = _bev.inverse_map(view_params)
        bb, dev = self.backbone, frames.device
        dt = self._compute_dtype()
        wo, ho = int(self.input_size[0]), int(self.input_size[1])
        base = self.base_size
        with torch.no_grad():
            nat = bb.native()
            ar = bb._exec_arena(dev)
            if ar["P"].device != dev:
                raise RuntimeError("EndToEndFastSCNN: frames on %s but parameters on %s"
                                   % (dev, ar["P"].device))
            plan, _, _ = nat.plan(N, base, base, _lib.dtype_code(dt), False, dev)
            lib = _lib.load()
            need = int(lib.fscnn_e2e_ws_bytes(plan))
            if need < 0:
                _lib.check(need, "fscnn_e2e_ws_bytes")
            ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
            mask = torch.empty((N, hb, wb), dtype=torch.uint8, device=dev) if return_mask else None
            rows = torch.empty((N, hb, 4), dtype=torch.int32, device=dev)
            m9 = (ctypes.c_double * 9)(*[float(v) for v in m])
            hm, hs = self._norm_host()
            if fused is None:
                fused = self._fused_view(N, hb, wb)
            rc = E_UNSUPPORTED
            with torch.cuda.device(dev):
                if fused:
                    rc = lib.fscnn_forward_e2e_bev(
                        plan, _lib.ptr(frames), _FRAME_DTYPES[frames.dtype],
                        int(self.channels_last), int(self.bgr), h, w, hm, hs, ho, wo,
                        int(scale) & 255, m9, hb, wb, min_width, _lib.ptr(mask), _lib.ptr(rows),
                        _lib.ptr(ar["P"]), _lib.ptr(ar["R"]), _lib.ptr(ar["NBT"]), _lib.ptr(ws),
                        _lib.stream_ptr(dev))
            fused = rc != E_UNSUPPORTED  # nothing was launched: the geometry check comes first
            if fused:
                _lib.check(rc, "fscnn_forward_e2e_bev")
        if not fused:  # by choice, FSCNN_E2E_FUSED=0, more than 32 classes: the mask, then the warp
            mask, rows = _bev.warp_mask(self.predict(frames, scale), m, (wb, hb), min_width,
                                        return_mask)
        object.__setattr__(self, "_last_fused", fused)
        return mask, rows

    def bird_eye_view(self, frames, view_params, frame_view_params=None, scale=255, min_width=10,
                      segmented=False, alpha=0.5, color=(0, 255, 0)):
        """The colour bird's-eye view next to the mask: ``(bev_image, bev_mask, rows)``, plus the
        segmented picture with ``segmented=True`` -- what ``transform_image_and_mask`` and
        ``create_visualization(bird_eye_image, bird_eye_mask)`` give the reference
        (``kuruma/core/inference.py:275-287``).

        ``bev_mask`` and ``rows`` are ``bird_eye(frames, view_params, scale, min_width)``, same
        bits and same routing.  ``bev_image`` is the uint8 frames warped bilinearly to the same view
        (``bev.warp_image``, border 0, the layout and channel order of the frames), the segmented
        picture that image with ``color`` (in the frames' channel order) blended at ``alpha`` where
        the mask is set.  Both come from one more launch on the same stream (``csrc/bev_image.hip``);
        nothing is read back.

        ``view_params`` describes the mask's source, ``input_size``, as for ``bird_eye``.  Frames of
        another size need their own matrix: pass ``frame_view_params`` = the same view built with
        ``BirdEyeView.params(..., source_size=(w, h))``.  Float frames are refused by this method
        only: the law is OpenCV's fixed-point remap of 8-bit images."""
        who = "EndToEndFastSCNN.bird_eye_view"
        if isinstance(frames, torch.Tensor) and frames.dtype != torch.uint8:
            raise RuntimeError("%s: frames are uint8, not %s: a float frame would take OpenCV's "
                               "float bilinear law, which this is not" % (who, frames.dtype))
        if not isinstance(frames, torch.Tensor) or frames.dim() != 4:
            raise RuntimeError("%s: expected 4-d frames" % who)
        wb, hb = (int(v) for v in view_params["output_size"])
        h, w = (int(v) for v in (frames.shape[1:3] if self.channels_last else frames.shape[2:4]))
        wo, ho = int(self.input_size[0]), int(self.input_size[1])
        if frame_view_params is None:
            if (w, h) != (wo, ho):
                raise RuntimeError(
                    "%s: the frames are %d x %d but view_params maps input_size %d x %d; pass "
                    "frame_view_params=BirdEyeView.params(pixels_per_unit, margin_ratio, "
                    "full_image, source_size=(%d, %d))[3] for the same view"
                    % (who, w, h, wo, ho, w, h))
            frame_view_params = view_params
        elif tuple(int(v) for v in frame_view_params["output_size"]) != (wb, hb):
            raise RuntimeError("%s: frame_view_params has output_size %s but view_params %s; both "
                               "describe one view" % (who, tuple(frame_view_params["output_size"]),
                                                      (wb, hb)))
        mask, rows = self.bird_eye(frames, view_params, scale=scale, min_width=min_width)
        res = _bev.warp_image(frames, _bev.inverse_map(frame_view_params), (wb, hb),
                              channels_last=bool(self.channels_last),
                              mask=mask if segmented else None, alpha=alpha, color=color)
        return (res[0], mask, rows, res[1]) if segmented else (res, mask, rows)

    # ---- the steering tail ------------------------------------------------------------------------
    def steer(self, frames, view_params, controller=None, smooth_method="polynomial", degree=3,
              num_waypoints=20, min_width=10, fast_mode=True, force_bottom_center=True, scale=255,
              anchor=None, car_position=None, return_rows=False):
        """Raw frames -> the wheel commands: ``bird_eye(frames, view_params, scale, min_width,
        return_mask=False)`` and then ``path.plan`` on its row table, on the same stream, with
        nothing read back in between (two launches after the backbone on ``bird_eye``'s fused
        route, three on its ``predict`` + ``fscnn_bev_mask`` route for large views).  Returns the float64
        record ``[N, path.REC + 2 * num_waypoints]`` on the device (``path.PWM_LEFT`` /
        ``path.PWM_RIGHT`` and the other offsets of ``path``; ``controller.control_result(i)``
        gives the reference's dictionary), and the row table too with ``return_rows``.  The
        planner arguments are ``plan_complete_path``'s, ``controller`` a
        ``path.VisualLateralErrorController`` whose EMA state stays on the device, one slot per
        batch index."""
        _, rows = self.bird_eye(frames, view_params, scale=scale, min_width=max(int(min_width), 1),
                                return_mask=False)
        rec = _path.plan(rows, view_params, controller, smooth_method, degree, num_waypoints,
                         min_width, fast_mode, force_bottom_center, anchor, car_position)
        return (rec, rows) if return_rows else rec

    # ---- the overlay tail -------------------------------------------------------------------------
    def _fused_overlay(self, h, w):
        """Whether ``overlay`` takes the fused tail for ``h x w`` frames.  The fused tail evaluates
        the class scores once per frame pixel, the two-launch route once per mask pixel, so the
        fused tail is taken exactly when the frame has no more pixels than the mask: a rule read
        off the work counts, to be widened only to what profiles/overlay_time.md shows."""
        return h * w <= int(self.input_size[0]) * int(self.input_size[1])

    def overlay(self, frames, alpha=0.5, color=(0, 255, 0), palette=None, frame_weight=1.0,
                gamma=0.0, return_mask=False, scale=255, fused=None):
        """The picture a person looks at: ``frames`` blended with the lane colour, uint8 in the
        layout of the frames (a fresh buffer), or ``(overlay, mask)`` with ``return_mask=True``.

        The label of a frame pixel is ``predict(frames, scale)`` at the nearest output pixel
        (``x * W // w``, the ``cv2.INTER_NEAREST`` resize of ``postprocess_matched_resolution``; the
        identity when the frames have the output's size).  Lane mode (the reference's
        ``create_visualization``): ``color``, in the frames' own channel order, where the label is
        not 0.  Palette mode: ``palette`` is a uint8 ``[P, 3]`` tensor or sequence and the class
        (the argmax itself, whatever ``scale``) picks its row; classes from ``P`` on get no colour.
        Every pixel is ``frame * frame_weight + colour * alpha + gamma`` in fp32, rounded half to
        even and saturated (``cv2.addWeighted``; include/fastscnn.h states the law).  ``mask`` is
        the uint8 ``[N, h, w]`` label of every frame pixel.  One launch after the backbone
        (``csrc/overlay.hip``): the frame is read once, the overlay written once, and neither a
        mask nor a probability is formed unless asked for.

        ``fused``: ``None`` picks the route (``_fused_overlay``: the fused tail when the frame has
        no more pixels than ``input_size``, else ``predict`` followed by ``fscnn_overlay_mask``),
        ``True`` / ``False`` force one; both give the same bits.  ``_last_fused`` tells which one
        ran."""
        from . import vis as _vis
        frames, N, h, w = self._check(frames)
        bb, dev = self.backbone, frames.device
        dt = self._compute_dtype()
        wo, ho = int(self.input_size[0]), int(self.input_size[1])
        base = self.base_size
        table, bits = _vis.class_table(bb.num_classes, scale, color, palette)
        if fused is None:
            fused = self._fused_overlay(h, w)
        rc = E_UNSUPPORTED
        out = mask = None
        if fused:
            with torch.no_grad():
                nat = bb.native()
                ar = bb._exec_arena(dev)
                if ar["P"].device != dev:
                    raise RuntimeError("EndToEndFastSCNN: frames on %s but parameters on %s"
                                       % (dev, ar["P"].device))
                plan, _, _ = nat.plan(N, base, base, _lib.dtype_code(dt), False, dev)
                lib = _lib.load()
                need = int(lib.fscnn_e2e_ws_bytes(plan))
                if need < 0:
                    _lib.check(need, "fscnn_e2e_ws_bytes")
                ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
                out = torch.empty(frames.shape, dtype=torch.uint8, device=dev)
                mask = torch.empty((N, h, w), dtype=torch.uint8, device=dev) if return_mask else None
                hm, hs = self._norm_host()
                with torch.cuda.device(dev):
                    rc = lib.fscnn_forward_e2e_overlay(
                        plan, _lib.ptr(frames), _FRAME_DTYPES[frames.dtype],
                        int(self.channels_last), int(self.bgr), h, w, hm, hs, ho, wo,
                        int(scale) & 255, table, bits, float(frame_weight), float(alpha),
                        float(gamma), _lib.ptr(out), _lib.ptr(mask), _lib.ptr(ar["P"]),
                        _lib.ptr(ar["R"]), _lib.ptr(ar["NBT"]), _lib.ptr(ws), _lib.stream_ptr(dev))
            fused = rc != E_UNSUPPORTED  # nothing was launched: the geometry check comes first
            if fused:
                _lib.check(rc, "fscnn_forward_e2e_overlay")
        if not fused:
            # by choice, a window too large for LDS, FSCNN_E2E_FUSED=0, more than 32 classes: the
            # mask, then the blend.  Palette mode blends by class id, so it predicts with scale 1
            # and scales the returned mask afterwards (uint8 products wrap mod 256, as the label
            # byte does)
            by_id = palette is not None
            labels = self.predict(frames, 1 if by_id else scale)
            res = _vis.overlay_mask(frames, labels, alpha=alpha, color=color, palette=palette,
                                    frame_weight=frame_weight, gamma=gamma,
                                    return_mask=return_mask, channels_last=self.channels_last)
            out, mask = res if return_mask else (res, None)
            if by_id and return_mask and (int(scale) & 255) != 1:
                mask = mask * (int(scale) & 255)
        object.__setattr__(self, "_last_fused", fused)
        return (out, mask) if return_mask else out
