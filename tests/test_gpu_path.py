"""The steering tail on the GPU (csrc/path.hip, fast_scnn_pytorch_amd.path,
EndToEndFastSCNN.steer): fscnn_path_plan on planted row tables against the numpy yardstick
(tests/path_ref.py) within the derived TOL (tests/test_path_cpu.py::test_tolerance_derivation),
status bits, counts and the "no path" outputs exactly; the EMA state on the device; the reference's
own outputs (tests/golden/path_cases.npz, path_recorded_run.npz) through the kernel; steer against
bird_eye + plan, bit for bit; the refusals."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

import bev_ref
import e2e_ref
import helpers
import path_ref as R
from e2e_ref import fixture, geometry
from fast_scnn_pytorch_amd import _lib, bev
from fast_scnn_pytorch_amd import path as P
from fast_scnn_pytorch_amd.deploy import EndToEndFastSCNN
from models.fast_scnn import FastSCNN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = R.TOL


def run(rows, p, state=None):
    return P.run(torch.from_numpy(np.ascontiguousarray(rows)).to(DEV), p, state).cpu().numpy()


def compare(got, want, p, what):
    """One frame's record against the yardstick's.  Exact: status, counts, the absent values, the
    0.0 raw error of a frame without a path.  Within TOL: coefficients evaluated at the waypoints,
    the waypoints, the control point, both lateral errors; TOL times the gain of each control
    quantity (steering_gain * TOL for the wheel values); the path length within the sum of its
    segments' bounds, 2 * K * TOL."""
    k, d = p["num_waypoints"], p["degree"]
    assert got.shape == (P.REC + 2 * k,), what
    assert int(got[P.STATUS]) == want["status"], (what, got[P.STATUS], want["status"])
    assert int(got[P.NPOINTS]) == want["num_centerline_points"], what
    way = got[P.REC:].reshape(k, 2)
    gain = abs(p["steering_gain"])
    dyn_gain = abs(p["base_pwm"] * p["curvature_damping"])
    if want["coef"] is None:
        assert int(got[P.NWAY]) == 0 and got[P.LENGTH] == 0.0, what
        assert np.isnan(got[P.COEF:P.COEF + 4]).all() and np.isnan(way).all(), what
        assert np.isnan(got[P.CONTROL_X]) and np.isnan(got[P.CONTROL_Y]), what
        assert got[P.RAW_ERROR] == 0.0, what
    else:
        assert int(got[P.NWAY]) == k, what
        assert np.isnan(got[P.COEF + d + 1:P.COEF + 4]).all(), what
        coef = got[P.COEF:P.COEF + d + 1]
        ys = want["waypoints"][:, 1]
        err = {"coef@waypoints": np.abs(np.polyval(coef, ys) - want["waypoints"][:, 0]).max(),
               "waypoints": np.abs(way - want["waypoints"]).max(),
               "control": np.abs(got[P.CONTROL_X:P.CONTROL_Y + 1] - want["control_point"]).max(),
               "raw": abs(got[P.RAW_ERROR] - want["raw_lateral_error"])}
        print("%s: %s (TOL %.2g)" % (what, {n: "%.2g" % v for n, v in err.items()}, TOL))
        for n, v in err.items():
            assert v <= TOL, (what, n, v)
        assert abs(got[P.LENGTH] - want["path_length"]) <= 2 * k * TOL, what
    assert abs(got[P.ERROR] - want["lateral_error"]) <= TOL, what
    assert abs(got[P.STEERING] - want["steering_adjustment"]) <= gain * TOL, what
    assert abs(got[P.DYNAMIC] - want["dynamic_pwm"]) <= dyn_gain * TOL, what
    assert abs(got[P.PWM_LEFT] - want["pwm_left"]) <= gain * TOL, what
    assert abs(got[P.PWM_RIGHT] - want["pwm_right"]) <= gain * TOL, what


# ---- 1. the grid and the planted cases ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid():
    return R.grid_cases()


@pytest.mark.parametrize("hb", R.HBS)
def test_grid_matches_the_yardstick(hb):
    """Hb x N in {1, 3} x degree x anchor, with fast / exact, skip_rows, scan direction and K each
    rotated on its own, plus the fast-mode default scanned both ways: fewer rows than threads, one
    row per thread, a second trip."""
    cases = [c for c in grid() if c[0].startswith("hb%d-" % hb)]
    assert len(cases) == 14
    for name, rows, p in cases:
        got = run(rows, p)
        assert got.shape == (rows.shape[0], P.REC + 2 * p["num_waypoints"])
        for f in range(rows.shape[0]):
            compare(got[f], R.plan(rows[f], p)[0], p, "%s/%d" % (name, f))


def test_grid_covers_every_factor():
    """Each value of each factor, and the pairs without which a factor could not be seen: the scan
    direction changes the selection only in fast mode with skip_rows > 1, so top-down must meet
    that, at every Hb, and must select other rows than bottom-up would in some case."""
    ps = [p for _, _, p in grid()]
    assert {p["degree"] for p in ps} == {1, 2, 3}
    assert {p["num_waypoints"] for p in ps} == set(R.KS)
    assert {(p["fast"], p["force_bottom_center"]) for p in ps} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    fast = [p for p in ps if p["fast"]]
    assert {(p["scan_from_bottom"], p["skip_rows"]) for p in fast} == {
        (b, s) for b in (0, 1) for s in R.SKIPS}
    for d in (1, 2, 3):
        assert {p["skip_rows"] for p in fast if p["degree"] == d} == set(R.SKIPS)
        assert {p["num_waypoints"] for p in ps if p["degree"] == d} == set(R.KS)
        assert {(p["fast"], p["force_bottom_center"]) for p in ps if p["degree"] == d} == {
            (0, 0), (0, 1), (1, 0), (1, 1)}
    for hb in R.HBS:
        here = [(rows, p) for name, rows, p in grid() if name.startswith("hb%d-" % hb)]
        assert {rows.shape[0] for rows, _ in here} == {1, 3}
        assert any(p["fast"] and not p["scan_from_bottom"] and p["skip_rows"] > 1 for _, p in here)
        assert any(p["fast"] and p["force_bottom_center"] and p["degree"] == 2
                   and p["skip_rows"] == 3 and p["scan_from_bottom"] for _, p in here)
    differ = sum(sorted(R.select(rows[0], 1, p["min_width"], p["skip_rows"], False))
                 != sorted(R.select(rows[0], 1, p["min_width"], p["skip_rows"], True))
                 for _, rows, p in grid() if p["fast"] and not p["scan_from_bottom"])
    assert differ >= 10, differ
    assert {c[1].shape[1] for c in grid()} == set(R.HBS)


@pytest.mark.parametrize("case", R.planted_cases(), ids=[c[0] for c in R.planted_cases()])
def test_planted_case(case):
    name, rows, p = case
    want = R.plan(rows[0], p)[0]
    got = run(rows, p)[0]
    compare(got, want, p, name)
    status = int(got[P.STATUS])
    if name in ("empty", "anchor-alone-is-not-a-path"):
        assert status == P.NO_CENTERLINE
    if name.startswith("too-few"):
        assert status == P.TOO_FEW and int(got[P.NPOINTS]) == p["degree"]
    if name.startswith("exactly"):
        assert status == 0 and int(got[P.NPOINTS]) == p["degree"] + 1
    if name.startswith("straight-d") and p["degree"] >= 2:
        assert np.abs(got[P.COEF:P.COEF + p["degree"] - 1]).max() < 1e-3  # the upper ones ~ 0
    if name == "all-behind":
        assert status == P.NONE_AHEAD and got[P.CONTROL_Y] == p["min_y"]
    if name == "to-min-pwm":
        assert got[P.DYNAMIC] == p["min_pwm"]
    if name == "to-max-pwm":
        assert got[P.DYNAMIC] == p["max_pwm"]
    if name == "left-clipped-high":
        assert got[P.PWM_LEFT] == 1000.0 and got[P.PWM_RIGHT] == -1000.0
    if name == "left-clipped-low":
        assert got[P.PWM_LEFT] == -1000.0 and got[P.PWM_RIGHT] == 1000.0
    if name == "rank-deficient":
        assert status == P.RANK_DEFICIENT


# ---- 2. the EMA state on the device -------------------------------------------------------------------------
def test_ema_sequence_reset_and_slots():
    """Three successive calls with changing tables, two batch slots: each slot follows its own
    reference sequence; a one-slot run gives slot 0's bits; after a reset the next call's error is
    its raw error exactly; with smoothing off the state is untouched."""
    seq = R.ema_sequence()
    state = torch.zeros((2, 2), dtype=torch.float64, device=DEV)
    solo = torch.zeros((1, 2), dtype=torch.float64, device=DEV)
    ref = [None, None]
    for call, (rows, p) in enumerate(seq):
        got = run(rows, p, state)
        alone = run(rows[:1], p, solo)
        assert np.array_equal(alone[0], got[0], equal_nan=True)
        for f in range(2):
            want, ref[f] = R.plan(rows[f], p, ref[f], True)
            compare(got[f], want, p, "call %d slot %d" % (call, f))
            if call:
                assert got[f][P.ERROR] != got[f][P.RAW_ERROR]
        s = state.cpu().numpy()
        assert np.array_equal(s[:, 0], got[:, P.ERROR]) and (s[:, 1] == 1.0).all()
    assert abs(got[0][P.ERROR] - got[1][P.ERROR]) > 1e-3  # the slots did not share a state
    # reset, through the controller that owns the state
    rows, p = seq[0]
    ctl = P.VisualLateralErrorController(ema_alpha=p["ema_alpha"])
    ctl.ema_state = state
    ctl.reset_ema_state()
    got = run(rows, p, ctl.state_for(2, state.device))
    assert np.array_equal(got[:, P.ERROR], got[:, P.RAW_ERROR])
    # smoothing off: the error is the raw error and the state stays as it is
    before = state.clone()
    ctl.enable_smoothing = False
    assert ctl.state_for(2, state.device) is None
    rows, p = seq[1]
    got = run(rows, p, ctl.state_for(2, state.device))
    assert np.array_equal(got[:, P.ERROR], got[:, P.RAW_ERROR])
    assert torch.equal(state, before)


# ---- 3. what the reference itself produced, through the kernel -------------------------------------------------
def test_reference_cases_through_the_kernel():
    """path_cases.npz: the reference's PathPlanner and controller on planted masks, three
    successive calls per case; the kernel on the masks' row tables, against the recorded outputs."""
    g = helpers.load_golden("path_cases")
    vp = {"view_bounds": tuple(float(v) for v in g["view_bounds"]),
          "pixels_per_unit": float(g["pixels_per_unit"]),
          "output_size": tuple(int(v) for v in g["output_size"]),
          "image_to_world_matrix": g["image_to_world_matrix"].tolist()}
    keys = [str(k) for k in g["control_keys"]]
    for name in (str(n) for n in g["case_names"]):
        pargs = json.loads(str(g[name + ".planner_args"]))
        ctl = P.VisualLateralErrorController(**json.loads(str(g[name + ".controller_args"])))
        planner = P.PathPlanner(vp)
        tables = bev_ref.row_table(g[name + ".masks"], pargs.get("min_width", 10))
        for f in range(3):
            rows = torch.from_numpy(tables[f:f + 1].copy()).to(DEV)
            planner.plan_complete_path(rows, controller=ctl, **pargs)
            pd, cr = planner.path_data(0), ctl.control_result(0)
            pre = "%s.%d." % (name, f)
            want_fit = g[pre + "fit_params"]
            assert (pd["fit_params"] is not None) == (want_fit.size > 0), pre
            if want_fit.size:
                way = np.array(pd["waypoints"])
                assert np.abs(way - g[pre + "waypoints"]).max() <= TOL, pre
                assert np.abs(np.polyval(pd["fit_params"], way[:, 1])
                              - g[pre + "waypoints"][:, 0]).max() <= TOL, pre
                assert pd["num_centerline_points"] == len(g[pre + "centerline_world"])
                assert abs(pd["path_length"] - g[pre + "path_length"]) <= 2 * len(way) * TOL
                assert np.abs(np.array(cr["control_point"]) - g[pre + "control_point"]).max() <= TOL
            else:
                assert pd["waypoints"] == [] and pd["path_length"] == 0
                assert cr["control_point"] is None and cr["raw_lateral_error"] == 0.0
            gain = abs(ctl.steering_gain)
            # base / dynamic moves by base / dynamic^2 per unit of dynamic_pwm, whose own gain is
            # base * damping; dynamic is at least min_pwm
            factor = (ctl.base_pwm / ctl.min_pwm) ** 2 * ctl.curvature_damping * TOL
            bound = {"lateral_error": TOL, "raw_lateral_error": TOL, "smoothed_lateral_error": TOL,
                     "smoothing_effect": 2 * TOL, "steering_adjustment": gain * TOL,
                     "dynamic_pwm": ctl.base_pwm * ctl.curvature_damping * TOL,
                     "dynamic_speed": ctl.base_pwm * ctl.curvature_damping * TOL,
                     "pwm_left": gain * TOL, "pwm_right": gain * TOL, "speed_left": gain * TOL,
                     "speed_right": gain * TOL, "curvature_level": TOL / ctl.preview_distance,
                     "pwm_reduction_factor": factor, "speed_reduction_factor": factor}
            for k, want in zip(keys, g[name + ".control"][f]):
                assert abs(cr[k] - want) <= bound[k], (pre, k, cr[k], want)
            want_dir = "left" if g[name + ".control"][f][0] < 0 else \
                "right" if g[name + ".control"][f][0] > 0 else "straight"
            assert cr["turn_direction"] == want_dir


def test_recorded_run_through_the_kernel():
    """The run the reference recorded: its centreline rebuilt as a row table from its grid
    integers (tests/test_bev_cpu.py), the yardstick confirming the rebuilt world points, then the
    kernel against the recorded fit, waypoints, path length and wheel values."""
    g = helpers.load_golden("path_recorded_run")
    rows, p = R.recorded_case(g)
    assert p["min_y"] == R.VIEW["min_y"]
    world = np.array(R.world(R.select(rows[0], 0, 10), p["min_x"], p["min_y"], 1.0))
    assert np.abs(world - g["centerline_world"]).max() <= 1e-12
    state = torch.zeros((1, 2), dtype=torch.float64, device=DEV)
    got = run(rows, p, state)[0]
    want = dict(status=0, num_centerline_points=20, coef=g["fit_params"], waypoints=g["waypoints"],
                path_length=float(g["path_length"]), control_point=g["control_point"],
                raw_lateral_error=float(g["lateral_error"]),
                **{k: float(g[k]) for k in ("lateral_error", "steering_adjustment", "dynamic_pwm",
                                            "pwm_left", "pwm_right")})
    compare(got, want, p, "recorded run")


# ---- 4. end to end ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_steer_is_bird_eye_then_plan(dtype):
    """e2e_200x70_c2 at the 208 x 108 view: steer(frames) is bit-identical to
    plan(bird_eye(frames)[1]) and within TOL of the yardstick on the rows copied back."""
    g = fixture("200x70", 2)
    size, base, mean, std = geometry(g)
    bb = FastSCNN(2)
    bb.load_state_dict(e2e_ref.weights(2))
    e2e = EndToEndFastSCNN(bb.to(DEV).eval(), input_size=size, base_size=base, mean=mean, std=std,
                           dtype=dtype)
    e2e.preprocessor.to(DEV)
    e2e.eval()
    frames = g["frames"][:3].to(DEV)
    vp = bev.BirdEyeView().params(1, 0.1, True, source_size=size)[3]
    for kw in (dict(), dict(degree=3, fast_mode=False, min_width=4, num_waypoints=33)):
        c1, c2 = P.VisualLateralErrorController(), P.VisualLateralErrorController()
        for call in range(2):  # the second call runs the EMA on the device state
            rec, rows = e2e.steer(frames, vp, c1, return_rows=True, **kw)
            _, rows2 = e2e.bird_eye(frames, vp, min_width=max(kw.get("min_width", 10), 1),
                                    return_mask=False)
            assert torch.equal(rows, rows2)
            rec2 = P.plan(rows2, vp, c2, **kw)
            assert rec.dtype == torch.float64 and rec.shape == (3, P.REC + 2 * kw.get(
                "num_waypoints", 20))
            assert torch.equal(rec.view(torch.int64), rec2.view(torch.int64))  # bits, NaNs too
        p = P.plan_params(vp, c1, **kw)
        fresh = P.run(rows, p).cpu().numpy()
        for f in range(3):
            want = R.plan(rows[f].cpu().numpy(), p)[0]
            print("%s frame %d: %d centreline points, status %d" % (
                dtype, f, want["num_centerline_points"], want["status"]))
            compare(fresh[f], want, p, "steer %s/%d" % (dtype, f))
        assert c1.control_result(1)["pwm_left"] == float(rec[1, P.PWM_LEFT])


# ---- 5. refusals ----------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    lib = _lib.load()
    rows = torch.zeros((1, 8, 4), dtype=torch.int32, device=DEV)
    out = torch.full((1, P.REC + 2 * 257), -7.0, dtype=torch.float64, device=DEV)
    st = _lib.stream_ptr(torch.device(DEV))

    def call(n=1, hb=8, **kw):
        p = _lib.PathParams()
        for k, v in R.params(8, **kw).items():
            setattr(p, k, v if isinstance(v, int) else float(v))
        return lib.fscnn_path_plan(_lib.ptr(rows), n, hb, ctypes.byref(p), None, _lib.ptr(out), st)
    assert call(num_waypoints=257) == -2 and call(num_waypoints=0) == -2
    assert call(degree=4) == -2 and call(degree=0) == -2
    assert call(hb=65536) == -2 and call(hb=0) == -2
    assert call(n=65536) == -2 and call(n=0) == -2
    assert call(steering_gain=float("nan")) == -1
    assert b"steering_gain" in lib.fscnn_last_error()
    assert call(max_y=float("inf")) == -1 and call(pixels_per_unit=0.0) == -1
    assert call(skip_rows=0) == -1
    assert lib.fscnn_path_plan(_lib.ptr(rows), 1, 8, None, None, _lib.ptr(out), st) == -1
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())  # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert float(out[0, P.STATUS]) == P.NO_CENTERLINE and bool((out[0, P.REC + 40:] == -7.0).all())
