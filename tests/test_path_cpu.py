"""CPU-side checks of the steering tail: the numpy yardstick (tests/path_ref.py) against what the
reference itself produced (tests/golden/path_recorded_run.npz, path_cases.npz;
tools/gen_path_golden.py), the derivation of the GPU tolerance, the selection margins of every GPU
case, and the host-side interface (ABI table, defaults, guards)."""
import json
import os
import re

import numpy as np
import pytest

import helpers
import path_ref as R
from fast_scnn_pytorch_amd import _lib, bev
from fast_scnn_pytorch_amd import path as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-12  # "a few ulp": the same float64 arithmetic as the recorded run


def close(a, b, what):
    """Relative 1e-12 of the recorded value; a recorded 0.0 is met exactly."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    zero = b == 0
    assert (a[zero] == 0).all(), what
    if (~zero).any():
        err = float((np.abs(a - b)[~zero] / np.abs(b[~zero])).max())
        print("%s: relative distance %.3g" % (what, err))
        assert err <= RTOL, what


# ---- 1. the run the reference recorded -------------------------------------------------------------
def recorded_params(g):
    return dict(degree=2, num_waypoints=20, force_bottom_center=1, min_y=float(g["waypoints"][0, 1]),
                max_y=float(g["waypoints"][-1, 1]), anchor_x=float(g["car_position"][0]),
                anchor_y=float(g["car_position"][1]), car_x=float(g["car_position"][0]),
                car_y=float(g["car_position"][1]), steering_gain=float(g["param_steering_gain"]),
                base_pwm=float(g["param_base_pwm"]),
                curvature_damping=float(g["param_curvature_damping"]),
                preview_distance=float(g["param_preview_distance"]),
                max_pwm=float(g["param_max_pwm"]), min_pwm=float(g["param_min_pwm"]), ema_alpha=0.5)


def test_yardstick_matches_the_recorded_run():
    """Degree 2, 20 centreline points, 20 waypoints, gain 10, base 500, min 100, max 800, fed with
    the recorded centreline: fit_params, waypoints, path length, control point, lateral error,
    dynamic_pwm and both wheel values within relative 1e-12 (absolute below magnitude 1)."""
    g = helpers.load_golden("path_recorded_run")
    assert g["centerline_world"].shape == (20, 2) and g["waypoints"].shape == (20, 2)
    rec, _ = R.plan_world([tuple(q) for q in g["centerline_world"]], recorded_params(g),
                          smoothing=True)
    assert rec["status"] == 0 and rec["num_centerline_points"] == int(g["num_centerline_points"])
    close(rec["coef"], g["fit_params"], "fit_params")
    close(rec["waypoints"], g["waypoints"], "waypoints")
    close(rec["path_length"], g["path_length"], "path_length")
    close(rec["control_point"], g["control_point"], "control_point")
    for k in ("lateral_error", "steering_adjustment", "dynamic_pwm", "pwm_left", "pwm_right"):
        close(rec[k], g[k], k)


# ---- 2. the reference's classes on planted masks -----------------------------------------------------
def golden_cases():
    """[(name, frame, rows [Hb, 4], params, enable_smoothing, golden dict)] of path_cases.npz; the
    row table is read off the stored mask the way csrc/bev.hip defines it (bev_ref.row_table)."""
    import bev_ref
    g = helpers.load_golden("path_cases")
    vp = {"view_bounds": tuple(float(v) for v in g["view_bounds"]),
          "pixels_per_unit": float(g["pixels_per_unit"]),
          "output_size": tuple(int(v) for v in g["output_size"]),
          "image_to_world_matrix": g["image_to_world_matrix"].tolist()}
    out = []
    for name in (str(n) for n in g["case_names"]):
        pargs = json.loads(str(g[name + ".planner_args"]))
        cargs = json.loads(str(g[name + ".controller_args"]))
        ctl = P.VisualLateralErrorController(**cargs)
        min_width = pargs.get("min_width", 10)
        p = P.plan_params(vp, ctl, pargs.get("degree", 3), pargs.get("num_waypoints", 20),
                          min_width, pargs.get("fast_mode", True),
                          pargs.get("force_bottom_center", True))
        tables = bev_ref.row_table(g[name + ".masks"], min_width)
        for f in range(3):
            out.append((name, f, tables[f], p, ctl.enable_smoothing, g))
    return out, vp


def test_yardstick_matches_the_reference_classes():
    """Every frame of every case: centreline, fit_params, waypoints, path length, control point and
    every numeric key of the control result over the three successive calls, within 1e-12."""
    cases, vp = golden_cases()
    assert len(cases) == 18
    keys = [str(k) for k in cases[0][5]["control_keys"]]
    state = None
    for name, f, rows, p, smoothing, g in cases:
        if f == 0:
            state = None
        pre = "%s.%d." % (name, f)
        car = g[name + ".car_position"]
        assert (p["car_x"], p["car_y"]) == (float(car[0]), float(car[1])) == R.bottom_center(vp)
        pts = R.world(R.select(rows, p["fast"], p["min_width"], p["skip_rows"], 1), p["min_x"],
                      p["min_y"], p["pixels_per_unit"])
        close(np.array(pts).reshape(-1, 2), g[pre + "centerline_world"], pre + "centerline")
        _, want_world = bev.centerline(rows, vp, fast=bool(p["fast"]), min_width=p["min_width"],
                                       skip_rows=p["skip_rows"])
        assert [tuple(map(float, q)) for q in want_world] == pts
        rec, state = R.plan(rows, p, state, smoothing)
        has = g[pre + "fit_params"].size > 0
        assert (rec["coef"] is not None) == has, pre
        if has:
            close(rec["coef"], g[pre + "fit_params"], pre + "fit_params")
            close(rec["waypoints"], g[pre + "waypoints"], pre + "waypoints")
            close(rec["control_point"], g[pre + "control_point"], pre + "control_point")
        else:
            assert g[pre + "waypoints"].size == 0 and g[pre + "control_point"].size == 0
            assert rec["control_point"] is None and rec["raw_lateral_error"] == 0.0
        close(rec["path_length"], g[pre + "path_length"], pre + "path_length")
        e, raw = rec["lateral_error"], rec["raw_lateral_error"]
        dyn = rec["dynamic_pwm"]
        mine = {"lateral_error": e, "raw_lateral_error": raw, "smoothed_lateral_error": e,
                "smoothing_effect": abs(raw - e) if smoothing else 0.0,
                "steering_adjustment": rec["steering_adjustment"], "dynamic_pwm": dyn,
                "pwm_left": rec["pwm_left"], "pwm_right": rec["pwm_right"],
                "curvature_level": abs(e) / p["preview_distance"],
                "pwm_reduction_factor": p["base_pwm"] / dyn, "dynamic_speed": dyn,
                "speed_left": rec["pwm_left"], "speed_right": rec["pwm_right"],
                "speed_reduction_factor": p["base_pwm"] / dyn}
        close([mine[k] for k in keys], g[name + ".control"][f], pre + "control")


# ---- 3. where the GPU tolerance comes from ------------------------------------------------------------
def all_gpu_frames():
    """Every frame the GPU tests put through the kernel, in call order:
    [(id, rows [Hb, 4], params, stream, smoothing)].  Frames with the same ``stream`` are
    successive calls of one EMA slot; ``None``: a call without EMA state."""
    out = []
    for name, rows, p in R.gpu_cases():
        out += [("%s/%d" % (name, f), rows[f], p, None, False) for f in range(rows.shape[0])]
    cases, _ = golden_cases()
    out += [("golden-%s/%d" % (name, f), rows, p, "golden-" + name if smoothing else None, smoothing)
            for name, f, rows, p, smoothing, _ in cases]
    rows, p = R.recorded_case(helpers.load_golden("path_recorded_run"))
    out.append(("recorded-run", rows[0], p, "recorded-run", True))
    for call, (rows, p) in enumerate(R.ema_sequence()):
        out += [("ema-call%d/%d" % (call, f), rows[f], p, "ema-%d" % f, True) for f in range(2)]
    return out


def test_tolerance_derivation():
    """For every GPU case with a path: the waypoints of np.polyfit against those of an
    np.longdouble Householder solve of the same weighted system; U = the largest distance.
    TOL = 16 * U.  The figures measured are with the constants in tests/path_ref.py."""
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is not wider than float64 here"
    u_max, n_max, n_fit = 0.0, 0.0, 0
    for name, rows, p, _, _ in all_gpu_frames():
        rec, _ = R.plan(rows, p)
        if rec["coef"] is None:
            continue
        n_fit += 1
        pts = R.world(R.select(rows, p["fast"], p["min_width"], p["skip_rows"],
                               p["scan_from_bottom"]), p["min_x"], p["min_y"],
                      p["pixels_per_unit"])
        anchor = (p["anchor_x"], p["anchor_y"]) if p["force_bottom_center"] else None
        a, b = R.system(pts, p["degree"], anchor)[:2]
        ys = rec["waypoints"][:, 1].astype(np.longdouble)
        truth = np.polyval(R.solve_longdouble(a, b), ys)
        u = float(np.abs(rec["waypoints"][:, 0] - truth).max())
        nrm = float(np.abs(np.polyval(R.solve_normal(a, b), rec["waypoints"][:, 1]) - truth).max())
        if u > u_max:
            print("U grows to %.3g at %s (normal equations there: %.3g)" % (u, name, nrm))
        u_max, n_max = max(u_max, u), max(n_max, nrm)
    print("frames with a path %d, U = %.4g cm, TOL = %.3g cm, normal equations worst %.3g cm = "
          "%.3g x TOL" % (n_fit, u_max, R.TOL, n_max, n_max / R.TOL))
    assert n_fit >= 200
    assert R.TOL == pytest.approx(16 * R.U_MEASURED, rel=0.02)
    assert 0.5 * R.U_MEASURED <= u_max <= R.U_MEASURED  # the constant is what is measured here
    assert n_max >= 100 * R.TOL  # else the cases are too easy: change the cases, not the factor


# ---- 4. no discrete choice within reach of a TOL-sized difference ------------------------------------
def test_selection_margins():
    """Every GPU case, none excluded, the EMA streams call by call with their state: best and
    second-best |distance - preview_distance| ahead of the car at least 1e-3 cm apart; no lateral
    error, raw or smoothed, within 1e-3 of 0 except where there is no path; no clip input within
    1e-3 of its bound, for the smoothed and for the raw error (the GPU tests run the EMA cases
    with smoothing off too); no waypoint within 1e-3 of the car's y.  The frames of the
    end-to-end test come from the backbone on the GPU and cannot be listed here."""
    seen = {"fallback": 0, "min": 0, "max": 0, "hi": 0, "lo": 0, "none": 0, "smoothed": 0}
    state = {}
    for name, rows, p, stream, smoothing in all_gpu_frames():
        rec, state[stream] = R.plan(rows, p, state.get(stream) if smoothing else None, smoothing)
        if stream is None:
            state.pop(None, None)
        raw = rec["raw_lateral_error"]
        if rec["coef"] is None:
            seen["none"] += 1
            assert raw == 0.0
        else:
            car = (p["car_x"], p["car_y"])
            assert np.abs(rec["waypoints"][:, 1] - car[1]).min() >= 1e-3, name
            d = sorted(R.preview_diffs(rec["waypoints"], car, p["preview_distance"]))
            if len(d) >= 2:
                assert d[1] - d[0] >= 1e-3, (name, d[:2])
            seen["fallback"] += not d
            assert abs(raw) >= 1e-3 and abs(rec["lateral_error"]) >= 1e-3, (name, raw)
        seen["smoothed"] += rec["lateral_error"] != raw
        for e in (rec["lateral_error"], raw):
            w = R.wheels(e, p)
            raw_dyn = p["base_pwm"] / (1 + p["curvature_damping"] * abs(e))
            assert min(abs(raw_dyn - p["min_pwm"]), abs(raw_dyn - p["max_pwm"])) >= 1e-3, name
            left = w["dynamic_pwm"] + w["steering_adjustment"]
            right = w["dynamic_pwm"] - w["steering_adjustment"]
            for v in (left, right):
                assert min(abs(v - 1000), abs(v + 1000)) >= 1e-3, name
        seen["min"] += raw_dyn < p["min_pwm"]
        seen["max"] += raw_dyn > p["max_pwm"]
        seen["hi"] += left > 1000
        seen["lo"] += left < -1000
    print(seen)
    assert all(v > 0 for v in seen.values()), seen  # every branch is met by some case


# ---- 5. the interface ------------------------------------------------------------------------------------
def test_abi_table_and_header_agree():
    src = open(os.path.join(ROOT, "include", "fastscnn.h")).read()
    m = re.search(r"int\s+fscnn_path_plan\s*\(([^;]*?)\)\s*;", src, re.S)
    assert m, "fscnn_path_plan is not declared in include/fastscnn.h"
    assert len(_lib.SIGNATURES["fscnn_path_plan"][1]) == len(m.group(1).split(","))
    for name, value in (("COEF", P.COEF), ("NPOINTS", P.NPOINTS), ("STATUS", P.STATUS),
                        ("LENGTH", P.LENGTH), ("CONTROL_X", P.CONTROL_X),
                        ("CONTROL_Y", P.CONTROL_Y), ("RAW_ERROR", P.RAW_ERROR),
                        ("ERROR", P.ERROR), ("STEERING", P.STEERING), ("DYNAMIC", P.DYNAMIC),
                        ("PWM_LEFT", P.PWM_LEFT), ("PWM_RIGHT", P.PWM_RIGHT), ("NWAY", P.NWAY),
                        ("REC", P.REC), ("NO_CENTERLINE", P.NO_CENTERLINE),
                        ("TOO_FEW", P.TOO_FEW), ("RANK_DEFICIENT", P.RANK_DEFICIENT),
                        ("NONE_AHEAD", P.NONE_AHEAD)):
        d = re.search(r"#define\s+FSCNN_PATH_%s\s+(\d+)" % name, src)
        assert d and int(d.group(1)) == value, name
    # the struct of the header, field for field
    body = re.search(r"typedef struct fscnn_path_params \{(.*?)\} fscnn_path_params;", src, re.S)
    fields = []
    for kind, names in re.findall(r"(int|double)\s+([^;]+);", re.sub(r"/\*.*?\*/", "", body.group(1))):
        fields += [(n.strip(), kind) for n in names.split(",")]
    assert fields == [(n, "int" if t is _lib.c_int else "double")
                      for n, t in _lib.PathParams._fields_]
    assert (R.NO_CENTERLINE, R.TOO_FEW, R.RANK_DEFICIENT, R.NONE_AHEAD) == (
        P.NO_CENTERLINE, P.TOO_FEW, P.RANK_DEFICIENT, P.NONE_AHEAD)


def test_plan_params_apply_the_reference_defaults():
    vp = bev.BirdEyeView().params(1, 0.1, True)[3]
    ctl = P.VisualLateralErrorController()
    p = P.plan_params(vp, ctl)
    assert (p["degree"], p["fast"], p["min_width"], p["skip_rows"], p["scan_from_bottom"]) == (
        2, 1, 5, 3, 1)
    assert (p["anchor_x"], p["anchor_y"]) == (p["car_x"], p["car_y"]) == R.bottom_center(vp)
    assert p["min_y"] == float(vp["view_bounds"][1]) and p["max_y"] == float(vp["view_bounds"][3])
    q = P.plan_params(vp, ctl, degree=3, fast_mode=False, min_width=7, anchor=(1.0, 2.0),
                      car_position=(3.0, 4.0))
    assert (q["degree"], q["fast"], q["min_width"]) == (3, 0, 7)
    assert (q["anchor_x"], q["anchor_y"], q["car_x"], q["car_y"]) == (1.0, 2.0, 3.0, 4.0)
    assert {k: p[k] for k in R.CONTROLLER_DEFAULTS} == R.CONTROLLER_DEFAULTS
    ctl.update_smoothing_params(ema_alpha=0.01, enable_smoothing=False)
    assert ctl.ema_alpha == 0.1 and ctl.enable_smoothing is False


def test_cpu_guards():
    import torch
    vp = bev.BirdEyeView().params(1, 0.1, True)[3]
    rows = torch.zeros((1, 108, 4), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device"):
        P.plan(rows, vp)
    with pytest.raises(RuntimeError, match="int32"):
        P.plan(rows.float(), vp)
    with pytest.raises(RuntimeError, match="smooth_method"):
        P.plan(rows, vp, smooth_method="bezier")
    with pytest.raises(RuntimeError, match="rows"):
        P.plan(torch.zeros((1, 50, 4), dtype=torch.int32), vp)
    with pytest.raises(RuntimeError, match="no call"):
        P.VisualLateralErrorController().control_result(0)
    with pytest.raises(RuntimeError, match="not been called"):
        P.PathPlanner(vp).path_data(0)
