"""The bird's-eye view of the deployment pipeline: calibration, view parameters and the centreline.

Restates, without OpenCV, what the reference's consumers do around the lane mask
(``kuruma/core/inference.py:190-240``, ``kuruma/interfaces/realtime.py:196-218``):

* ``kuruma/core/calibration.py``: ``get_builtin_calibration`` (the A4-paper four-point
  calibration of a 640 x 360 camera) and ``get_corrected_calibration`` (top and bottom image edges
  forced parallel in the world), float32 casts included;
* ``PerspectiveTransformer.calculate_bird_eye_params`` and the size adjustment of
  ``transform_image_and_mask`` (``kuruma/vision/transform.py:49-201``) -> ``BirdEyeView.params``;
* ``PathPlanner.extract_centerline`` / ``extract_centerline_fast`` and ``_pixels_to_world``
  (``kuruma/vision/path_planning.py:188-314``) -> ``centerline``, read from the row table that
  ``EndToEndFastSCNN.bird_eye`` (``csrc/bev.hip``) leaves, instead of a Python loop over pixels.

The warps and the row scan run on the device -- the mask by the nearest neighbour
(``warp_mask``, ``csrc/bev.hip``), the camera frame bilinearly with the segmented picture in the
same launch (``warp_image``, ``csrc/bev_image.hip``) -- and this module is otherwise host arithmetic
on 3 x 3 matrices and on ``Hb x 4`` integers.  Path smoothing, waypoints and the wheel PWM follow in
``path`` (``csrc/path.hip``), which reads the same row table on the device;
``EndToEndFastSCNN.steer`` runs both behind the backbone.
"""
import numpy as np

__all__ = ["BirdEyeView", "centerline", "warp_mask", "warp_image", "get_builtin_calibration",
           "get_corrected_calibration", "perspective_transform", "inverse_map", "MAX_WIDTH",
           "MAX_HEIGHT"]

MAX_WIDTH, MAX_HEIGHT = 8192, 65535  # of a bird's-eye view the kernel takes (include/fastscnn.h)


def perspective_transform(src, dst):
    """The 3 x 3 float64 homography taking four ``src`` points to four ``dst`` points, as
    ``cv2.getPerspectiveTransform`` sets it up: points cast to float32, the 8 x 8 system
    ``[x y 1 0 0 0 -xu -yu; 0 0 0 x y 1 -xv -yv]`` solved in float64, ``h33 = 1``."""
    s = np.asarray(src, dtype=np.float32).astype(np.float64).reshape(4, 2)
    d = np.asarray(dst, dtype=np.float32).astype(np.float64).reshape(4, 2)
    a = np.zeros((8, 8), dtype=np.float64)
    b = np.zeros(8, dtype=np.float64)
    for i in range(4):
        x, y = s[i]
        u, v = d[i]
        a[i] = [x, y, 1, 0, 0, 0, -x * u, -y * u]
        a[i + 4] = [0, 0, 0, x, y, 1, -x * v, -y * v]
        b[i], b[i + 4] = u, v
    h = np.linalg.solve(a, b)
    return np.append(h, 1.0).reshape(3, 3)


def _project(matrix_f32, points):
    """Image points through a float32 matrix the way the reference does it: float32 throughout."""
    out = []
    for p in np.asarray(points, dtype=np.float32):
        w = matrix_f32 @ p
        out.append([w[0] / w[2], w[1] / w[2]])
    return np.array(out)


def get_builtin_calibration():
    """calibration.py:16-49: an A4 sheet (21.0 x 29.7 cm) seen by the 640 x 360 camera."""
    image_points = [(260, 87), (378, 87), (410, 217), (231, 221)]
    world_points = [(0, 0), (21, 0), (21, 29.7), (0, 29.7)]
    return {
        "image_size": [640, 360],
        "image_points": image_points,
        "world_points": world_points,
        "transform_matrix": perspective_transform(image_points, world_points).tolist(),
        "inverse_transform_matrix": perspective_transform(world_points, image_points).tolist(),
        "units": "centimeters",
    }


def get_corrected_calibration():
    """calibration.py:51-124: the image corners projected with the built-in matrix (in float32),
    the y of the top pair and of the bottom pair averaged, and the homography solved again from
    the corners to the corrected world points."""
    cal = get_builtin_calibration()
    t32 = np.array(cal["transform_matrix"], dtype=np.float32)
    wc = _project(t32, [[0, 0, 1], [639, 0, 1], [639, 359, 1], [0, 359, 1]])
    top_y = (wc[0][1] + wc[1][1]) / 2
    bottom_y = (wc[2][1] + wc[3][1]) / 2
    corrected = [[wc[0][0], top_y], [wc[1][0], top_y], [wc[2][0], bottom_y], [wc[3][0], bottom_y]]
    src = [[0, 0], [639, 0], [639, 359], [0, 359]]
    return {
        "image_size": [640, 360],
        "image_points": cal["image_points"],
        "world_points": cal["world_points"],
        "transform_matrix": perspective_transform(src, corrected).tolist(),
        "inverse_transform_matrix": perspective_transform(corrected, src).tolist(),
        "corrected_world_corners": [[float(a), float(b)] for a, b in corrected],
        "original_world_corners": wc.tolist(),
        "units": "centimeters",
    }


class BirdEyeView:
    """``PerspectiveTransformer(calibration_data=None, use_corrected=True)`` of the reference: it
    produces the view parameters ``EndToEndFastSCNN.bird_eye`` takes, and
    ``transform_image_and_mask`` warps a frame and its mask on the device."""

    def __init__(self, calibration=None, use_corrected=True):
        if calibration is None:
            calibration = get_corrected_calibration() if use_corrected else get_builtin_calibration()
        self.calibration_data = calibration
        self.transform_matrix = np.array(calibration["transform_matrix"], dtype=np.float32)
        self.inverse_transform_matrix = np.array(calibration["inverse_transform_matrix"],
                                                 dtype=np.float32)
        self.image_points = calibration["image_points"]
        self.world_points = calibration["world_points"]
        self.original_image_size = calibration["image_size"]

    def calculate_bird_eye_params(self, pixels_per_unit=20, margin_ratio=0.1, full_image=True):
        """transform.py:49-128: ``(output_width, output_height, combined_transform, view_bounds)``,
        in the reference's float32 arithmetic."""
        if full_image:
            w, h = self.original_image_size
            wc = _project(self.transform_matrix,
                          [[0, 0, 1], [w - 1, 0, 1], [w - 1, h - 1, 1], [0, h - 1, 1]])
            min_x, min_y = wc.min(axis=0)
            max_x, max_y = wc.max(axis=0)
            # (a float32 scalar times a Python float stays float32, as under numpy >= 2)
            margin_x = (max_x - min_x) * np.float32(margin_ratio)
            margin_y = (max_y - min_y) * np.float32(margin_ratio)
            min_x, min_y, max_x, max_y = min_x - margin_x, min_y - margin_y, max_x + margin_x, \
                max_y + margin_y
        else:
            wp = np.array(self.world_points)
            min_x, min_y = wp.min(axis=0)
            max_x, max_y = wp.max(axis=0)
            margin = max(max_x - min_x, max_y - min_y) * margin_ratio
            min_x, min_y, max_x, max_y = min_x - margin, min_y - margin, max_x + margin, \
                max_y + margin
        out_w = int((max_x - min_x) * pixels_per_unit)
        out_h = int((max_y - min_y) * pixels_per_unit)
        world_to_pixel = np.array([[pixels_per_unit, 0, -min_x * pixels_per_unit],
                                   [0, pixels_per_unit, -min_y * pixels_per_unit],
                                   [0, 0, 1]], dtype=np.float32)
        return out_w, out_h, world_to_pixel @ self.transform_matrix, (min_x, min_y, max_x, max_y)

    def params(self, pixels_per_unit=20, margin_ratio=0.1, full_image=True, source_size=None):
        """``(output_size (Wb, Hb), combined matrix, view_bounds, view_params)`` for a source mask
        of ``source_size`` = (W, H) (default: the calibration size).  ``combined`` maps source
        pixels to view pixels (what ``cv2.warpPerspective`` is given), rescaled as
        transform.py:150-171 does when the source is not the calibration size; ``view_params``
        carries the reference's keys."""
        out_w, out_h, combined, bounds = self.calculate_bird_eye_params(pixels_per_unit,
                                                                        margin_ratio, full_image)
        ow, oh = self.original_image_size
        if source_size is not None and (int(source_size[0]) != ow or int(source_size[1]) != oh):
            scale = np.array([[int(source_size[0]) / ow, 0, 0], [0, int(source_size[1]) / oh, 0],
                              [0, 0, 1]], dtype=np.float32)
            combined = combined @ np.linalg.inv(scale)
        view_params = {
            "output_size": (out_w, out_h),
            "view_bounds": bounds,
            "pixels_per_unit": pixels_per_unit,
            "margin_ratio": margin_ratio,
            "transform_matrix": combined.tolist(),
            "image_to_world_matrix": self.transform_matrix.tolist(),
        }
        return (out_w, out_h), combined, bounds, view_params

    def transform_image_and_mask(self, image, mask, pixels_per_unit=20, margin_ratio=0.1,
                                 full_image=True):
        """transform.py:130-201 on the device: ``(bird_eye_image, bird_eye_mask, view_params)``.

        ``image`` is a uint8 camera frame ``[H, W, 3]`` and ``mask`` its uint8 lane mask ``[H, W]``
        on a ROCm device, or batches ``[N, H, W, 3]`` / ``[N, H, W]``; the results have the same
        batching.  The image is warped bilinearly (``warp_image``), the mask by the nearest
        neighbour (``warp_mask``), both with border 0 and with the matrix rescaled when the source
        is not the calibration size, as ``params(source_size=...)`` does.  Two launches:
        ``fscnn_bev_image`` and ``fscnn_bev_mask``."""
        import torch
        who = "transform_image_and_mask"
        if not isinstance(image, torch.Tensor) or not isinstance(mask, torch.Tensor):
            raise RuntimeError("%s: image and mask are torch tensors on a ROCm device" % who)
        if image.dtype != torch.uint8 or mask.dtype != torch.uint8:
            raise RuntimeError("%s: image and mask are uint8, not %s / %s: a float image would "
                               "take OpenCV's float bilinear law, which this is not"
                               % (who, image.dtype, mask.dtype))
        batched = image.dim() == 4
        if image.dim() not in (3, 4) or image.shape[-1] != 3 or mask.dim() != image.dim() - 1:
            raise RuntimeError("%s: expected an image [H, W, 3] with a mask [H, W], or batches "
                               "[N, H, W, 3] / [N, H, W]; got %s and %s"
                               % (who, tuple(image.shape), tuple(mask.shape)))
        if not batched:
            image, mask = image[None], mask[None]
        if tuple(mask.shape) != tuple(image.shape[:3]):
            raise RuntimeError("%s: the mask %s does not match the image %s"
                               % (who, tuple(mask.shape), tuple(image.shape)))
        h, w = int(image.shape[1]), int(image.shape[2])
        size, _, _, view_params = self.params(pixels_per_unit, margin_ratio, full_image,
                                              source_size=(w, h))
        _view_size(size, who)
        m = inverse_map(view_params)
        bird = warp_image(image, m, size, channels_last=True)
        bird_mask, _ = warp_mask(mask, m, size)
        if not batched:
            bird, bird_mask = bird[0], bird_mask[0]
        return bird, bird_mask, view_params


def inverse_map(view_params):
    """The destination -> source matrix of a view as 9 float64 values: the inverse of
    ``view_params['transform_matrix']``, taken in float64 as ``cv2.warpPerspective`` does."""
    m = np.asarray(view_params["transform_matrix"], dtype=np.float64).reshape(3, 3)
    inv = np.linalg.inv(m)
    if not np.isfinite(inv).all():
        raise RuntimeError("bird's-eye view: the transform matrix is singular")
    return inv.reshape(9)


def warp_mask(mask, m, size, min_width=10, return_mask=True):
    """The bird's-eye tail on a mask that is already in device memory (``fscnn_bev_mask``):
    ``mask`` uint8 ``[N, H, W]`` on a ROCm device, ``m`` the 9 destination -> source values
    (``inverse_map(view_params)``), ``size`` = (Wb, Hb).  Returns ``(bev_mask or None, rows)`` as
    ``EndToEndFastSCNN.bird_eye`` does; that method is this warp fused behind the backbone."""
    import ctypes

    import torch

    from . import _lib
    if not isinstance(mask, torch.Tensor) or mask.dim() != 3 or mask.dtype != torch.uint8:
        raise RuntimeError("warp_mask: expected a uint8 mask [N, H, W]")
    if not mask.is_cuda:
        raise RuntimeError("warp_mask: the HIP path needs a ROCm device tensor (got %s)"
                           % (mask.device,))
    mask = mask.contiguous()
    n, wb, hb = int(mask.shape[0]), int(size[0]), int(size[1])
    bev = torch.empty((n, hb, wb), dtype=torch.uint8, device=mask.device) if return_mask else None
    rows = torch.empty((n, hb, 4), dtype=torch.int32, device=mask.device)
    cm = (ctypes.c_double * 9)(*[float(v) for v in np.asarray(m, dtype=np.float64).reshape(9)])
    with torch.cuda.device(mask.device):
        _lib.call("fscnn_bev_mask", _lib.ptr(mask), n, int(mask.shape[1]), int(mask.shape[2]), cm,
                  hb, wb, int(min_width), _lib.ptr(bev), _lib.ptr(rows),
                  _lib.stream_ptr(mask.device))
    return bev, rows


def _view_size(size, who):
    wb, hb = int(size[0]), int(size[1])
    if not (1 <= wb <= MAX_WIDTH and 1 <= hb <= MAX_HEIGHT):
        raise RuntimeError("%s: view %d x %d: the bird's-eye kernels take widths 1 .. %d and "
                           "heights 1 .. %d" % (who, wb, hb, MAX_WIDTH, MAX_HEIGHT))
    return wb, hb


def warp_image(frames, m, size, channels_last=None, mask=None, alpha=0.5, color=(0, 255, 0),
               frame_weight=1.0, gamma=0.0):
    """The colour bird's-eye view (``fscnn_bev_image``, ``csrc/bev_image.hip``): uint8 ``frames``
    ``[N, 3, h, w]`` or ``[N, h, w, 3]`` on a ROCm device warped to ``size`` = (Wb, Hb) with the
    fixed-point bilinear law of ``include/fastscnn.h`` (``cv2.warpPerspective`` with
    ``INTER_LINEAR`` and border 0), ``m`` the 9 destination -> source values
    (``inverse_map(view_params)``).  Returns ``image``, uint8 in the layout of the frames.

    ``channels_last=None`` reads the layout off the shape: ``[N, h, w, 3]`` when only the last
    dimension is 3, ``[N, 3, h, w]`` otherwise (so pass it when both are 3); ``True`` / ``False``
    are checked as ``vis.overlay_mask`` checks them.  Channels are never swapped.

    With ``mask`` (uint8 ``[N, Hb, Wb]``, a bird's-eye mask such as ``warp_mask``'s) the same launch
    also writes the segmented picture, the reference's ``create_visualization(bird_eye_image,
    bird_eye_mask)``: ``color`` (in the frames' channel order) where the mask is not 0, blended as
    ``image * frame_weight + colour * alpha + gamma`` by the overlay law; the result is then
    ``(image, blended)``.  Float frames are refused: OpenCV warps them by a different law."""
    import ctypes

    import torch

    from . import _lib
    from . import vis as _vis
    who = "warp_image"
    if isinstance(frames, torch.Tensor) and frames.dtype != torch.uint8:
        raise RuntimeError("%s: frames are uint8, not %s: the law is OpenCV's fixed-point remap of "
                           "8-bit images, and a float frame would take another law"
                           % (who, frames.dtype))
    if not isinstance(frames, torch.Tensor) or frames.dim() != 4:
        raise RuntimeError("%s: expected 4-d frames" % who)
    if channels_last is None:
        channels_last = frames.shape[3] == 3 and frames.shape[1] != 3
    if frames.shape[3 if channels_last else 1] != 3:
        raise RuntimeError("%s: expected frames %s, got %s"
                           % (who, "[N, h, w, 3]" if channels_last else "[N, 3, h, w]",
                              tuple(frames.shape)))
    wb, hb = _view_size(size, who)
    frames, n, h, w = _vis.check_frames(frames, bool(channels_last), who)
    if n > 65535 or h > 16384 or w > 16384:
        raise RuntimeError("%s: frames %s: at most 65535 frames with sides up to 16384"
                           % (who, tuple(frames.shape)))
    m9 = np.asarray(m, dtype=np.float64).reshape(-1)
    if m9.size != 9 or not np.isfinite(m9).all():
        raise RuntimeError("%s: m is 9 finite destination -> source values" % who)
    dev = frames.device
    c3 = None
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or \
                tuple(mask.shape) != (n, hb, wb):
            raise RuntimeError("%s: the mask is the uint8 bird's-eye mask [%d, %d, %d], got %s"
                               % (who, n, hb, wb, getattr(mask, "shape", type(mask))))
        if mask.device != dev:
            raise RuntimeError("%s: the HIP path needs the mask on the frames' ROCm device (got %s "
                               "and %s)" % (who, mask.device, dev))
        mask = mask.contiguous()
        c3 = (ctypes.c_ubyte * 3)(*_vis._color3(color))
    shape = (n, hb, wb, 3) if channels_last else (n, 3, hb, wb)
    image = torch.empty(shape, dtype=torch.uint8, device=dev)
    blended = torch.empty(shape, dtype=torch.uint8, device=dev) if mask is not None else None
    cm = (ctypes.c_double * 9)(*[float(v) for v in m9])
    with torch.cuda.device(dev):
        _lib.call("fscnn_bev_image", _lib.ptr(frames), int(bool(channels_last)), n, h, w, cm, hb,
                  wb, _lib.ptr(image), _lib.ptr(mask), c3, float(frame_weight), float(alpha),
                  float(gamma), _lib.ptr(blended), _lib.stream_ptr(dev))
    return image if mask is None else (image, blended)


def centerline(rows, view_params, fast=False, min_width=None, skip_rows=None,
               scan_from_bottom=True):
    """``(centerline_points, centerline_world)`` of the reference from one image's row table
    ``rows`` (``[Hb, 4]`` int32: run_start, run_end, count, index_sum).

    ``fast=False``: ``PathPlanner.extract_centerline`` -- every row with a run, the point
    ``((run_start + run_end) // 2, y)``; the table's runs already honour the ``min_width`` the
    table was made with, and a larger ``min_width`` here drops the rows whose longest run is
    shorter (default: keep all).  ``fast=True``: ``extract_centerline_fast`` -- every
    ``skip_rows``-th row (default 5) with ``count >= min_width`` (default 5), the point
    ``(index_sum // count, y)``.  World coordinates are ``min + pixel / pixels_per_unit``."""
    r = np.asarray(rows.cpu() if hasattr(rows, "cpu") else rows).astype(np.int64)
    if r.ndim != 2 or r.shape[1] != 4:
        raise RuntimeError("centerline: rows of one image, [Hb, 4], got %s" % (r.shape,))
    height = r.shape[0]
    step = (5 if skip_rows is None else int(skip_rows)) if fast else 1
    if step < 1:
        raise RuntimeError("centerline: skip_rows must be >= 1")
    ys = range(height - 1, -1, -step) if scan_from_bottom else range(0, height, step)
    points = []
    if fast:
        need = 5 if min_width is None else int(min_width)
        for y in ys:
            if r[y, 2] >= need and r[y, 2] > 0:
                points.append((int(r[y, 3] // r[y, 2]), y))
    else:
        need = 1 if min_width is None else int(min_width)
        for y in ys:
            if r[y, 1] > r[y, 0] and r[y, 1] - r[y, 0] >= need:
                points.append((int((r[y, 0] + r[y, 1]) // 2), y))
    min_x, min_y = view_params["view_bounds"][:2]
    ppu = view_params["pixels_per_unit"]
    world = [(min_x + px / ppu, min_y + py / ppu) for px, py in points]
    return points, world
