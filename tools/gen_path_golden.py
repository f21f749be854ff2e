"""Writes the two fixtures of the steering tail's tests from the reference (run on the CPU):

    python tools/gen_path_golden.py REFERENCE_DIR

tests/golden/path_recorded_run.npz: the run the reference recorded itself,
  REFERENCE_DIR/kuruma/test/output/raw_20250702_024355_405_{path,control}_data.json: centreline,
  fit_params, waypoints, path_length, the controller's parameters and its outputs.
tests/golden/path_cases.npz: the reference's own PathPlanner and VisualLateralErrorController,
  imported from REFERENCE_DIR/kuruma, run on small planted bird's-eye masks; their inputs (masks,
  view parameters, arguments) and their outputs (centreline, fit_params, waypoints, path length,
  every numeric key of the control result over three successive calls).

Nothing of the reference is restated here: the two classes are imported and called.  They import
cv2 at module level without calling it in the methods used, and OpenCV is not a dependency of this
project, so an empty stand-in module is registered under that name first.  ``view_bounds`` is
handed over as Python floats (what a JSON round trip of the view parameters gives), so that the
reference's world coordinates are float64 under every numpy version.
"""
import contextlib
import io
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEM = "raw_20250702_024355_405"
CONTROL_KEYS = ["lateral_error", "raw_lateral_error", "smoothed_lateral_error", "smoothing_effect",
                "steering_adjustment", "dynamic_pwm", "pwm_left", "pwm_right", "curvature_level",
                "pwm_reduction_factor", "dynamic_speed", "speed_left", "speed_right",
                "speed_reduction_factor"]


def recorded_run(ref):
    out = os.path.join(ref, "kuruma", "test", "output")
    with open(os.path.join(out, STEM + "_path_data.json")) as f:
        path = json.load(f)
    with open(os.path.join(out, STEM + "_control_data.json")) as f:
        ctl = json.load(f)
    cur = ctl["current_control"]
    np.savez(os.path.join(ROOT, "tests", "golden", "path_recorded_run.npz"),
             centerline_world=np.array(path["centerline_world"], dtype=np.float64),
             fit_params=np.array(path["fit_params"], dtype=np.float64),
             waypoints=np.array(path["waypoints"], dtype=np.float64),
             path_length=np.float64(path["path_length"]),
             num_centerline_points=np.int64(path["num_centerline_points"]),
             car_position=np.array(cur["car_position"], dtype=np.float64),
             control_point=np.array(cur["control_point"], dtype=np.float64),
             **{"param_" + k: np.float64(v) for k, v in ctl["parameters"].items()},
             **{k: np.float64(cur[k]) for k in ("lateral_error", "steering_adjustment",
                                                "dynamic_pwm", "pwm_left", "pwm_right",
                                                "curvature_level", "pwm_reduction_factor")},
             source=np.array(STEM))


def lane_mask(h, w, ppu, origin, car, kind, seed, rows=None):
    """A planted bird's-eye mask: a 12 cm lane around a straight or bent centre, every third
    frame with a 3-pixel speck beside it (shorter than any min_width used)."""
    m = np.zeros((h, w), dtype=np.uint8)
    if kind == "empty":
        return m
    rng = np.random.RandomState(seed)
    for y in (range(h) if rows is None else rows):
        t = (car[1] - (origin[1] + y / ppu)) / 100.0
        wx = car[0] - 7.3 if kind == "straight" else \
            car[0] - 3.1 - 55.0 * t * t + 18.0 * t * t * t + (seed % 5) * 2.2
        c = int(round((wx - origin[0]) * ppu)) + int(rng.randint(-1, 2))
        a, b = max(c - int(6 * ppu), 0), min(c + int(6 * ppu), w)
        m[y, a:b] = 255
        if seed % 3 == 0 and b + 8 < w:
            m[y, b + 5:b + 8] = 255
    return m


def cases(ref):
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.path.insert(0, os.path.join(ref, "kuruma"))
    import _fscnn_boot
    _fscnn_boot.load()
    from fast_scnn_pytorch_amd.bev import BirdEyeView
    with contextlib.redirect_stdout(io.StringIO()):
        from control.visual_controller import VisualLateralErrorController
        from vision.path_planning import PathPlanner

    (w, h), _, bounds, vp = BirdEyeView().params(pixels_per_unit=1, margin_ratio=0.1)
    vp = dict(vp, view_bounds=tuple(float(v) for v in bounds))
    origin = vp["view_bounds"][:2]
    store = {"view_bounds": np.array(vp["view_bounds"], dtype=np.float64),
             "pixels_per_unit": np.float64(vp["pixels_per_unit"]),
             "output_size": np.array(vp["output_size"], dtype=np.int64),
             "image_to_world_matrix": np.array(vp["image_to_world_matrix"], dtype=np.float64),
             "control_keys": np.array(CONTROL_KEYS)}
    # name: (three (kind, seed, rows) frames, plan_complete_path arguments, controller arguments)
    table = {
        "fast_default": ([("curved", 1, None), ("curved", 2, None), ("straight", 3, None)],
                         dict(), dict()),
        "exact_cubic": ([("curved", 4, None), ("curved", 6, None), ("curved", 7, None)],
                        dict(degree=3, fast_mode=False), dict(steering_gain=10.0, base_pwm=500,
                                                              min_pwm=100, max_pwm=800)),
        "exact_line_free": ([("straight", 1, None), ("curved", 8, range(50, 108)),
                             ("curved", 9, range(30, 90))],
                            dict(degree=1, fast_mode=False, force_bottom_center=False,
                                 num_waypoints=7), dict(ema_alpha=0.3)),
        "empty_then_lane": ([("empty", 0, None), ("curved", 11, None), ("empty", 0, None)],
                            dict(degree=2), dict()),
        "short_lane_too_few": ([("curved", 1, [100]), ("curved", 2, [40, 100]),
                                ("curved", 3, [10, 40, 100])],
                               dict(degree=2, fast_mode=False, force_bottom_center=False),
                               dict(enable_smoothing=False)),
        "clipped": ([("curved", 13, None), ("curved", 14, None), ("curved", 16, None)],
                    dict(degree=2, num_waypoints=50), dict(steering_gain=400.0, base_pwm=900,
                                                           curvature_damping=0.02)),
    }
    store["case_names"] = np.array(list(table))
    for name, (frames, pargs, cargs) in table.items():
        with contextlib.redirect_stdout(io.StringIO()):
            planner = PathPlanner(vp)
            ctl = VisualLateralErrorController(**cargs)
            car = ctl._get_car_position_world(vp)
        car = (float(car[0]), float(car[1]))
        masks, control = [], []
        for f, (kind, seed, rows) in enumerate(frames):
            mask = lane_mask(h, w, 1, origin, car, kind, seed, rows)
            with contextlib.redirect_stdout(io.StringIO()):
                pd = planner.plan_complete_path(mask, **pargs)
                cr = ctl.compute_wheel_pwm(pd, vp)
            masks.append(mask)
            pre = "%s.%d." % (name, f)
            store[pre + "centerline_world"] = np.array(pd["centerline_world"],
                                                       dtype=np.float64).reshape(-1, 2)
            has = pd["fit_params"] is not None
            store[pre + "fit_params"] = np.array(pd["fit_params"] if has else [], dtype=np.float64)
            store[pre + "waypoints"] = np.array(pd["waypoints"], dtype=np.float64).reshape(-1, 2)
            store[pre + "path_length"] = np.float64(pd["path_length"])
            cp = cr["control_point"]
            store[pre + "control_point"] = np.array([] if cp is None else cp, dtype=np.float64)
            control.append([float(cr[k]) for k in CONTROL_KEYS])
        store[name + ".masks"] = np.stack(masks)
        store[name + ".control"] = np.array(control, dtype=np.float64)
        store[name + ".car_position"] = np.array(car, dtype=np.float64)
        store[name + ".planner_args"] = np.array(json.dumps(pargs))
        store[name + ".controller_args"] = np.array(json.dumps(cargs))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "path_cases.npz"), **store)


if __name__ == "__main__":
    recorded_run(sys.argv[1])
    cases(sys.argv[1])
