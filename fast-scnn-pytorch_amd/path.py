"""The steering tail of the deployment pipeline: row table -> path -> wheel PWM, on the device.

What the reference does on the host after the bird's-eye view
(``PathPlanner.smooth_path`` / ``generate_waypoints`` / ``plan_complete_path``,
``kuruma/vision/path_planning.py:316-525``; ``VisualLateralErrorController.compute_wheel_pwm``,
``kuruma/control/visual_controller.py:72-207, 236-308``) is one launch here (``csrc/path.hip``,
the law: ``include/fastscnn.h``): the centreline is read from the row table that
``EndToEndFastSCNN.bird_eye`` leaves on the device, fitted by a QR factorisation (never the normal
equations), and turned into waypoints, the preview point, the smoothed lateral error and
``(pwm_left, pwm_right)``.  The result is one float64 record per frame, ``[N, REC + 2 * K]``, at the
offsets below; nothing is read back in between, and the EMA state lives on the device, one slot
per batch index (each batch slot is its own camera stream).

``plan`` is the call; ``PathPlanner`` and ``VisualLateralErrorController`` carry the reference's
names, arguments and result dictionaries (``path_data(i)`` / ``control_result(i)`` read one copy of
the record).  The control-map drawing, the JSON export and the spline option (which the reference
itself replaces by the polynomial) are not here.

Where numpy would warn of a rank-deficient fit and return a truncated-SVD answer, this law gives
no path and sets ``RANK_DEFICIENT`` in the status.
"""
import ctypes
import math

import numpy as np

from . import _lib

__all__ = ["plan", "run", "PathPlanner", "VisualLateralErrorController", "bottom_center_world",
           "REC", "MAX_WAYPOINTS"]

# offsets of the record (FSCNN_PATH_* of include/fastscnn.h)
COEF, NPOINTS, STATUS, LENGTH, CONTROL_X, CONTROL_Y, RAW_ERROR, ERROR, STEERING, DYNAMIC, \
    PWM_LEFT, PWM_RIGHT, NWAY, REC = 0, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16
NO_CENTERLINE, TOO_FEW, RANK_DEFICIENT, NONE_AHEAD = 1, 2, 4, 8
MAX_WAYPOINTS = 256
BOTTOM_CENTER_PIXEL = (320, 359)  # hard-coded in the reference whatever the frame size


def bottom_center_world(view_params, pixel=BOTTOM_CENTER_PIXEL):
    """The reference's bottom-centre point, which is both the fit's anchor and the car position:
    image pixel ``(320, 359, 1)`` through ``view_params['image_to_world_matrix']`` in float32
    (``_get_bottom_center_world_coord``, ``_get_car_position_world``)."""
    t = np.array(view_params["image_to_world_matrix"], dtype=np.float32)
    w = t @ np.array([pixel[0], pixel[1], 1], dtype=np.float32)
    return float(w[0] / w[2]), float(w[1] / w[2])


def run(rows, params, ema_state=None):
    """``fscnn_path_plan`` on a row table in device memory: ``rows`` int32 ``[N, Hb, 4]``,
    ``params`` the fields of ``fscnn_path_params`` as a dict, ``ema_state`` float64 ``[N, 2]`` on
    the same device or ``None`` (smoothing off).  Returns the float64 record ``[N, REC + 2 * K]``."""
    import torch
    if not isinstance(rows, torch.Tensor) or rows.dim() != 3 or rows.shape[2] != 4 \
            or rows.dtype != torch.int32:
        raise RuntimeError("path.run: expected an int32 row table [N, Hb, 4]")
    if not rows.is_cuda:
        raise RuntimeError("path.run: the HIP path needs a ROCm device tensor (got %s)"
                           % (rows.device,))
    rows = rows.contiguous()
    n, hb = int(rows.shape[0]), int(rows.shape[1])
    k = int(params["num_waypoints"])
    if ema_state is not None and (ema_state.dtype != torch.float64 or ema_state.device != rows.device
                                  or tuple(ema_state.shape) != (n, 2)
                                  or not ema_state.is_contiguous()):
        raise RuntimeError("path.run: ema_state is a contiguous float64 [N, 2] on the rows' device")
    p = _lib.PathParams()
    for name, ctype in _lib.PathParams._fields_:
        if name != "reserved":
            setattr(p, name, (int if ctype is _lib.c_int else float)(params[name]))
    out = torch.empty((n, REC + 2 * max(k, 0)), dtype=torch.float64, device=rows.device)
    with torch.cuda.device(rows.device):
        _lib.call("fscnn_path_plan", _lib.ptr(rows), n, hb, ctypes.byref(p), _lib.ptr(ema_state),
                  _lib.ptr(out), _lib.stream_ptr(rows.device))
    return out


class VisualLateralErrorController:
    """The reference's controller (same constructor arguments, no prints) with its EMA state on the
    device: one (state, flag) pair per batch slot, read and updated by the kernel, so successive
    calls need no host read."""

    def __init__(self, steering_gain=50.0, base_pwm=300, curvature_damping=0.1,
                 preview_distance=30.0, max_pwm=1000, min_pwm=100, ema_alpha=0.5,
                 enable_smoothing=True):
        self.steering_gain = steering_gain
        self.base_pwm = base_pwm
        self.curvature_damping = curvature_damping
        self.preview_distance = preview_distance
        self.max_pwm = max_pwm
        self.min_pwm = min_pwm
        self.ema_alpha = ema_alpha
        self.enable_smoothing = enable_smoothing
        self.ema_state = None  # float64 [N, 2] on the device, made by the first call
        self._last = None      # (record, car position) of the last call

    def params(self):
        return dict(steering_gain=self.steering_gain, base_pwm=self.base_pwm,
                    curvature_damping=self.curvature_damping,
                    preview_distance=self.preview_distance, max_pwm=self.max_pwm,
                    min_pwm=self.min_pwm, ema_alpha=self.ema_alpha)

    def state_for(self, n, device):
        """The EMA state of a batch of ``n`` on ``device`` (``None`` with smoothing off); a batch
        of another size or device starts afresh."""
        import torch
        if not self.enable_smoothing:
            return None
        if self.ema_state is None or self.ema_state.shape[0] != n or self.ema_state.device != device:
            self.ema_state = torch.zeros((n, 2), dtype=torch.float64, device=device)
        return self.ema_state

    def reset_ema_state(self):
        """The next call of every slot takes its raw error (a device-side fill, no host read)."""
        if self.ema_state is not None:
            self.ema_state.zero_()

    def update_smoothing_params(self, ema_alpha=None, enable_smoothing=None):
        if ema_alpha is not None:
            self.ema_alpha = max(0.1, min(1.0, ema_alpha))
        if enable_smoothing is not None:
            old = self.enable_smoothing
            self.enable_smoothing = enable_smoothing
            if not enable_smoothing and old:
                self.reset_ema_state()

    def control_result(self, i=0, record=None):
        """The reference's ``compute_wheel_pwm`` dictionary for frame ``i`` of the last call (or of
        ``record``): host arithmetic on one copy of the frame's record."""
        if record is None and self._last is None:
            raise RuntimeError("control_result: no call has been made with this controller")
        rec = self._last[0] if record is None else record
        r = rec[i, :REC].cpu().numpy()
        e, raw, dyn = float(r[ERROR]), float(r[RAW_ERROR]), float(r[DYNAMIC])
        factor = self.base_pwm / dyn if dyn > 0 else 1.0
        return {
            "lateral_error": e,
            "car_position": None if self._last is None else self._last[1],
            "control_point": None if math.isnan(r[CONTROL_X]) else (float(r[CONTROL_X]),
                                                                     float(r[CONTROL_Y])),
            "steering_adjustment": float(r[STEERING]),
            "dynamic_pwm": dyn,
            "pwm_right": float(r[PWM_RIGHT]),
            "pwm_left": float(r[PWM_LEFT]),
            "turn_direction": "left" if e < 0 else "right" if e > 0 else "straight",
            "curvature_level": abs(e) / self.preview_distance,
            "pwm_reduction_factor": factor,
            "dynamic_speed": dyn,
            "speed_right": float(r[PWM_RIGHT]),
            "speed_left": float(r[PWM_LEFT]),
            "speed_reduction_factor": factor,
            "smoothing_enabled": self.enable_smoothing,
            "ema_alpha": self.ema_alpha,
            "raw_lateral_error": raw,
            "smoothed_lateral_error": e,
            "smoothing_effect": abs(raw - e) if self.enable_smoothing else 0.0,
            "status": int(r[STATUS]),
        }


def plan_params(view_params, controller, degree=3, num_waypoints=20, min_width=10, fast_mode=True,
                force_bottom_center=True, anchor=None, car_position=None):
    """``fscnn_path_params`` as a dict with ``plan_complete_path``'s defaults applied: fast mode
    scans every third row from the bottom for ``count >= min_width // 2`` and caps the degree at
    2; the exact mode takes every row with a run of at least ``min_width``."""
    bottom = None
    if anchor is None or car_position is None:
        bottom = bottom_center_world(view_params)
    anchor = bottom if anchor is None else anchor
    car = bottom if car_position is None else car_position
    min_x, min_y, _, max_y = (float(v) for v in view_params["view_bounds"])
    p = dict(degree=min(2, int(degree)) if fast_mode else int(degree),
             num_waypoints=int(num_waypoints), fast=int(bool(fast_mode)),
             min_width=int(min_width) // 2 if fast_mode else int(min_width), skip_rows=3,
             scan_from_bottom=1, force_bottom_center=int(bool(force_bottom_center)),
             min_x=min_x, min_y=min_y, max_y=max_y,
             pixels_per_unit=float(view_params["pixels_per_unit"]),
             anchor_x=float(anchor[0]), anchor_y=float(anchor[1]), car_x=float(car[0]),
             car_y=float(car[1]))
    p.update(controller.params())
    return p


def plan(rows, view_params, controller=None, smooth_method="polynomial", degree=3,
         num_waypoints=20, min_width=10, fast_mode=True, force_bottom_center=True, anchor=None,
         car_position=None):
    """Row table ``[N, Hb, 4]`` on the device -> the float64 record ``[N, REC + 2 * K]``:
    ``plan_complete_path`` followed by ``compute_wheel_pwm`` for every frame, one launch.
    ``controller``: a ``VisualLateralErrorController`` (its EMA state is read and updated on the
    device; default: the reference's default controller with smoothing off).  ``anchor`` /
    ``car_position`` override the reference's bottom-centre point, in world centimetres."""
    if smooth_method not in ("polynomial", "spline"):
        raise RuntimeError("path.plan: smooth_method is 'polynomial' (or 'spline', which the "
                           "reference replaces by the polynomial), not %r" % (smooth_method,))
    if controller is None:
        controller = VisualLateralErrorController(enable_smoothing=False)
    if int(rows.shape[1]) != int(view_params["output_size"][1]):
        raise RuntimeError("path.plan: rows of %d-row views, view_params of %d rows"
                           % (rows.shape[1], view_params["output_size"][1]))
    p = plan_params(view_params, controller, degree, num_waypoints, min_width, fast_mode,
                    force_bottom_center, anchor, car_position)
    rec = run(rows, p, controller.state_for(int(rows.shape[0]), rows.device))
    controller._last = (rec, (p["car_x"], p["car_y"]))
    return rec


class PathPlanner:
    """``PathPlanner(view_params)`` of the reference on a row table instead of a mask."""

    def __init__(self, view_params):
        self.view_params = view_params
        self.pixels_per_unit = view_params["pixels_per_unit"]
        self.view_bounds = view_params["view_bounds"]
        self._last = None

    def plan_complete_path(self, rows, smooth_method="polynomial", degree=3, num_waypoints=20,
                           min_width=10, fast_mode=True, force_bottom_center=True,
                           controller=None):
        """The record of the whole batch, on the device (``path_data(i)`` reads one frame)."""
        rec = plan(rows, self.view_params, controller, smooth_method, degree, num_waypoints,
                   min_width, fast_mode, force_bottom_center)
        self._last = (rec, bool(fast_mode), bool(force_bottom_center), int(num_waypoints),
                      min(2, int(degree)) if fast_mode else int(degree))
        return rec

    def path_data(self, i=0):
        """The reference's ``path_data`` dictionary of frame ``i`` of the last call, from one copy
        of its record.  The centreline lists are not part of the record: ``bev.centerline`` reads
        them from the row table."""
        if self._last is None:
            raise RuntimeError("path_data: plan_complete_path has not been called")
        rec, fast, force, k, degree = self._last
        r = rec[i].cpu().numpy()
        status = int(r[STATUS])
        if status & NO_CENTERLINE:  # the reference's early return
            return {"centerline_pixels": [], "centerline_world": [], "smooth_path_func": None,
                    "fit_params": None, "waypoints": [], "path_length": 0, "status": status}
        has = int(r[NWAY]) > 0
        fit = r[COEF:COEF + degree + 1].copy() if has else None
        way = [(float(x), float(y)) for x, y in r[REC:REC + 2 * k].reshape(k, 2)] if has else []
        return {"smooth_path_func": np.poly1d(fit) if has else None, "fit_params": fit,
                "waypoints": way, "path_length": float(r[LENGTH]) if has else 0,
                "num_centerline_points": int(r[NPOINTS]), "num_waypoints": len(way),
                "fast_mode": fast, "force_bottom_center": force, "status": status}
