"""The steering tail's law (include/fastscnn.h) restated in numpy: the yardstick of the GPU tests.

Selection, world points, the weighted fit (``np.polyfit`` itself, as the reference calls it),
``np.linspace`` waypoints, ``np.poly1d`` evaluation, path length, preview search, EMA and the wheel
law, written after ``PathPlanner`` (kuruma/vision/path_planning.py:188-525) and
``VisualLateralErrorController`` (kuruma/control/visual_controller.py:72-207, 236-308); checked
against what those two classes themselves produced (tests/golden/path_cases.npz,
path_recorded_run.npz) by tests/test_path_cpu.py.

``TOL``: the bound of the GPU comparison on coefficients evaluated at the waypoints, in cm.
tests/test_path_cpu.py::test_tolerance_derivation measures U, the largest distance over every
GPU case between the waypoints of ``np.polyfit`` and of an ``np.longdouble`` Householder solve of
the same weighted system, and asserts ``TOL == 16 * U`` (within rounding of the constant): two
backward-stable fp64 solvers each sit about U from the truth, and the factor covers the other
rotation order across 256 workers and FMA contraction."""
import warnings

import numpy as np

U_MEASURED = 1.02e-8  # cm, measured 2026-10-21 (numpy 2.2.6); test_tolerance_derivation prints it
TOL = 1.64e-7  # = 16 * U_MEASURED, rounded up in the third digit; the normal equations' worst
# distance on the same cases, 3.3e-2 cm, is 2.0e5 x TOL

NO_CENTERLINE, TOO_FEW, RANK_DEFICIENT, NONE_AHEAD = 1, 2, 4, 8
ANCHOR_WEIGHT = 1e6

CONTROLLER_DEFAULTS = dict(steering_gain=50.0, base_pwm=300.0, curvature_damping=0.1,
                           preview_distance=30.0, max_pwm=1000.0, min_pwm=100.0, ema_alpha=0.5)


def bottom_center(view_params, pixel=(320, 359)):
    """_get_bottom_center_world_coord / _get_car_position_world: float32 throughout."""
    t = np.array(view_params["image_to_world_matrix"], dtype=np.float32)
    w = t @ np.array([pixel[0], pixel[1], 1], dtype=np.float32)
    return float(w[0] / w[2]), float(w[1] / w[2])


def select(rows, fast, min_width, skip_rows=1, scan_from_bottom=True):
    """Centreline pixels [(px, y), ...] of one row table, in scan order."""
    r = np.asarray(rows).astype(np.int64)
    hb = r.shape[0]
    pts = []
    if fast:
        ys = range(hb - 1, -1, -skip_rows) if scan_from_bottom else range(0, hb, skip_rows)
        for y in ys:
            if r[y, 2] >= min_width and r[y, 2] > 0:
                pts.append((int(r[y, 3] // r[y, 2]), y))
    else:
        for y in (range(hb - 1, -1, -1) if scan_from_bottom else range(hb)):
            if r[y, 1] > r[y, 0] and r[y, 1] - r[y, 0] >= min_width:
                pts.append((int((r[y, 0] + r[y, 1]) // 2), y))
    return pts


def world(points, min_x, min_y, ppu):
    return [(float(min_x) + px / float(ppu), float(min_y) + py / float(ppu)) for px, py in points]


def system(world_pts, degree, anchor=None):
    """(A, b, y, x, w) of the weighted least-squares problem, rows sorted by y as smooth_path
    leaves them."""
    pts = np.array(world_pts, dtype=np.float64).reshape(-1, 2)
    y, x = pts[:, 1], pts[:, 0]
    order = np.argsort(y)
    y, x = y[order], x[order]
    w = np.ones_like(y)
    if anchor is not None:
        y, x, w = np.append(y, anchor[1]), np.append(x, anchor[0]), np.append(w, ANCHOR_WEIGHT)
        order = np.argsort(y)
        y, x, w = y[order], x[order], w[order]
    a = np.vander(y, degree + 1) * w[:, None]
    return a, x * w, y, x, w


def fit(world_pts, degree, anchor=None):
    """(coefficients highest power first or None, status bits)."""
    if len(world_pts) == 0:
        return None, NO_CENTERLINE
    n = len(world_pts) + (anchor is not None)
    if n <= degree:
        return None, TOO_FEW
    a, b, y, x, w = system(world_pts, degree, anchor)
    d = np.abs(np.diag(np.linalg.qr(a, mode="r")))
    if d.min() < n * np.finfo(np.float64).eps * d.max() or d.min() == 0:
        return None, RANK_DEFICIENT
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a RankWarning here would mean the two rank tests part
        return np.polyfit(y, x, degree, w=w), 0


def waypoints(coef, min_y, max_y, k):
    ys = np.linspace(min_y, max_y, k)
    return np.stack([np.poly1d(coef)(ys), ys], axis=1)


def path_length(wps):
    total = 0.0
    for i in range(1, len(wps)):
        dx, dy = wps[i][0] - wps[i - 1][0], wps[i][1] - wps[i - 1][1]
        total += np.sqrt(dx * dx + dy * dy)
    return float(total)


def preview_diffs(wps, car, preview_distance):
    """|distance - preview_distance| of the waypoints ahead of the car, in order."""
    return [abs(np.sqrt((wx - car[0]) ** 2 + (wy - car[1]) ** 2) - preview_distance)
            for wx, wy in wps if wy < car[1]]


def preview(wps, car, preview_distance):
    """(control point or None, none_ahead)."""
    if len(wps) == 0:
        return None, False
    best, best_d = None, float("inf")
    for wx, wy in wps:
        if wy < car[1]:
            d = abs(np.sqrt((wx - car[0]) ** 2 + (wy - car[1]) ** 2) - preview_distance)
            if d < best_d:
                best, best_d = (float(wx), float(wy)), d
    if best is None:
        wx, wy = min(wps, key=lambda q: q[1])
        return (float(wx), float(wy)), True
    return best, False


def wheels(e, c):
    steering = c["steering_gain"] * e
    dynamic = float(np.clip(c["base_pwm"] / (1 + c["curvature_damping"] * abs(e)), c["min_pwm"],
                            c["max_pwm"]))
    return dict(lateral_error=e, steering_adjustment=steering, dynamic_pwm=dynamic,
                pwm_left=float(np.clip(dynamic + steering, -1000, 1000)),
                pwm_right=float(np.clip(dynamic - steering, -1000, 1000)))


def ema_step(raw, state, alpha):
    """(lateral error, new state); ``state`` None = first call."""
    e = raw if state is None else alpha * raw + (1 - alpha) * state
    return e, e


def plan_world(world_pts, p, state=None, smoothing=False):
    """One frame from its centreline world points.  ``p``: the fields of fscnn_path_params as a
    dict.  Returns the record as a dict (``coef``, ``waypoints`` None with no path) and the new EMA
    state."""
    anchor = (p["anchor_x"], p["anchor_y"]) if p["force_bottom_center"] else None
    coef, status = fit(world_pts, p["degree"], anchor)
    car = (p["car_x"], p["car_y"])
    rec = dict(num_centerline_points=len(world_pts), coef=coef, waypoints=None, path_length=0.0,
               control_point=None, raw_lateral_error=0.0)
    if coef is not None:
        wps = waypoints(coef, p["min_y"], p["max_y"], p["num_waypoints"])
        cp, none_ahead = preview(wps, car, p["preview_distance"])
        status |= NONE_AHEAD if none_ahead else 0
        rec.update(waypoints=wps, path_length=path_length(wps), control_point=cp,
                   raw_lateral_error=cp[0] - car[0])
    rec["status"] = status
    e = rec["raw_lateral_error"]
    if smoothing:
        e, state = ema_step(e, state, p["ema_alpha"])
    rec.update(wheels(e, p))
    return rec, state


def plan(rows, p, state=None, smoothing=False):
    """One frame from its row table [Hb, 4]."""
    pts = select(rows, p["fast"], p["min_width"], p["skip_rows"], p["scan_from_bottom"])
    return plan_world(world(pts, p["min_x"], p["min_y"], p["pixels_per_unit"]), p, state,
                      smoothing)


# ---- the other two solvers of the tolerance derivation ---------------------------------------------
def solve_longdouble(a, b):
    """Householder QR least squares in np.longdouble (80-bit here)."""
    a = np.array(a, dtype=np.longdouble)
    b = np.array(b, dtype=np.longdouble)
    m, n = a.shape
    for j in range(n):
        v = a[j:, j].copy()
        alpha = -np.copysign(np.sqrt((v * v).sum()), v[0])
        v[0] -= alpha
        vv = (v * v).sum()
        if vv == 0:
            continue
        a[j:, :] -= np.outer(v, (2 / vv) * (v @ a[j:, :]))
        b[j:] -= v * ((2 / vv) * (v @ b[j:]))
    c = np.zeros(n, dtype=np.longdouble)
    for j in range(n - 1, -1, -1):
        c[j] = (b[j] - a[j, j + 1:n] @ c[j + 1:]) / a[j, j]
    return c


def solve_normal(a, b):
    """The solver this pipeline must not use: fp64 normal equations."""
    return np.linalg.solve(a.T @ a, a.T @ b)


# ---- planted row tables of the GPU tests ---------------------------------------------------------
VIEW = dict(min_x=-86.31710510253906, min_y=-54.44426651000977, max_y=53.79618453979492,
            anchor_x=10.853042602539062, anchor_y=44.964935302734375)  # the recorded 208 x 108 view


def params(hb, ppu=None, **kw):
    """fscnn_path_params as a dict for a view of ``hb`` rows spanning the recorded view's depth:
    ``ppu`` defaults to hb / 108 pixels per cm, so that every Hb sees the same world."""
    ppu = hb / 108.0 if ppu is None else ppu
    p = dict(degree=2, num_waypoints=20, fast=1, min_width=5, skip_rows=1, scan_from_bottom=1,
             force_bottom_center=1, min_x=VIEW["min_x"], min_y=VIEW["min_y"], max_y=VIEW["max_y"],
             pixels_per_unit=ppu, anchor_x=VIEW["anchor_x"], anchor_y=VIEW["anchor_y"],
             car_x=VIEW["anchor_x"], car_y=VIEW["anchor_y"], **CONTROLLER_DEFAULTS)
    p.update(kw)
    return p


def lane_rows(hb, ppu, kind, seed=0, width=None, ys=None):
    """A row table [hb, 4] with a planted lane of ``width`` pixels (default: 12 cm): ``straight``
    (a vertical lane 7.3 cm left of the car), ``curved`` (a cubic bend) or ``empty``; ``ys``
    restricts the lane to those rows.  The centre is rounded to the pixel grid and, at one pixel
    per cm and finer, jittered by a seeded +-1 pixel, as a segmented lane is; the same run serves
    both centreline flavours (run and centroid)."""
    rows = np.zeros((hb, 4), dtype=np.int32)
    if kind == "empty":
        return rows
    width = max(2, int(round(12 * ppu))) if width is None else width
    rng = np.random.RandomState(seed)
    for y in (range(hb) if ys is None else ys):
        wy = VIEW["min_y"] + y / ppu
        t = (VIEW["anchor_y"] - wy) / 100.0
        if kind == "straight":
            wx = VIEW["anchor_x"] - 7.3
        else:
            wx = VIEW["anchor_x"] - 3.1 - 55.0 * t * t + 18.0 * t * t * t + (seed % 5) * 2.2
        c = int(round((wx - VIEW["min_x"]) * ppu)) + (int(rng.randint(-1, 2)) if ppu >= 1 else 0)
        a = max(c - width // 2, 0)
        b = a + width
        rows[y] = (a, b, b - a, sum(range(a, b)))
    return rows


HBS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 600]
KS = [1, 2, 20, 256]
SKIPS = [1, 3, 5]


def grid_cases():
    """[(id, rows [N, Hb, 4], params)]: every Hb x N x degree x anchor, with fast / exact,
    skip_rows, scan direction and K each rotated on its own (from the indices of N, degree, anchor
    and Hb, so that no two factors move together; test_grid_covers_every_factor asserts the pairs
    that matter), plus at every Hb plan_complete_path's fast-mode default (anchor, degree 2, every
    third row) scanned bottom-up and top-down."""
    out = []

    def add(hb, n, seed, **kw):
        p = params(hb, min_width=2, **kw)
        kinds = ["curved", "straight", "curved"]
        rows = np.stack([lane_rows(hb, p["pixels_per_unit"], kinds[(f + seed) % 3], seed=seed + f)
                         for f in range(n)])
        out.append(("hb%d-n%d-d%d-%s-%s%d-%s-k%d" % (
            hb, n, p["degree"], "anchor" if p["force_bottom_center"] else "free",
            "fast" if p["fast"] else "exact", p["skip_rows"],
            "up" if p["scan_from_bottom"] else "down", p["num_waypoints"]), rows, p))
    for h, hb in enumerate(HBS):
        for ni, n in enumerate((1, 3)):
            for di, degree in enumerate((1, 2, 3)):
                for ai, anchor in enumerate((1, 0)):
                    j = 6 * ni + 2 * di + ai
                    add(hb, n, 12 * h + j, degree=degree, force_bottom_center=anchor,
                        fast=(ni + di + h) % 2, skip_rows=SKIPS[(ni + ai + h) % 3],
                        scan_from_bottom=(di + ai + h // 2) % 2, num_waypoints=KS[(j + h) % 4])
        for bottom in (1, 0):
            add(hb, 1, 12 * h + 100 + bottom, degree=2, force_bottom_center=1, fast=1,
                skip_rows=3, scan_from_bottom=bottom, num_waypoints=20)
    return out


def planted_cases():
    """The named cases of the issue, one frame each, on the 108-row view at 1 pixel per cm."""
    hb, out = 108, []

    def add(name, rows, **kw):
        out.append((name, rows[None], params(hb, **kw)))
    add("empty", lane_rows(hb, 1.0, "empty"))
    for d in (1, 2, 3):
        ys = [10 + 25 * j for j in range(d + 1)]
        add("too-few-d%d" % d, lane_rows(hb, 1.0, "curved", 1, ys=ys[:d]), degree=d,
            force_bottom_center=0)
        add("exactly-d%d" % d, lane_rows(hb, 1.0, "curved", 1, ys=ys), degree=d,
            force_bottom_center=0)
        add("straight-d%d" % d, lane_rows(hb, 1.0, "straight"), degree=d,
            anchor_x=VIEW["anchor_x"] - 7.3)  # the anchor on the lane's line
        add("curved-d%d" % d, lane_rows(hb, 1.0, "curved", 3), degree=d)
    add("all-behind", lane_rows(hb, 1.0, "curved", 2), car_y=VIEW["min_y"] - 5.0)
    add("to-min-pwm", lane_rows(hb, 1.0, "straight"), curvature_damping=2.0, base_pwm=500.0,
        min_pwm=100.0)
    add("to-max-pwm", lane_rows(hb, 1.0, "straight"), base_pwm=2000.0, max_pwm=800.0)
    add("left-clipped-high", lane_rows(hb, 1.0, "straight"), steering_gain=-500.0)
    add("left-clipped-low", lane_rows(hb, 1.0, "straight"), steering_gain=500.0)
    add("rank-deficient", lane_rows(hb, 1.0, "straight", ys=[40]), degree=1,
        anchor_y=VIEW["min_y"] + 40.0)
    add("anchor-alone-is-not-a-path", lane_rows(hb, 1.0, "empty"), degree=1)
    return out


def gpu_cases():
    return grid_cases() + planted_cases()


def ema_sequence():
    """Three successive calls of two batch slots with changing tables: [(rows [2, Hb, 4], params)]."""
    hb = 108
    p = params(hb, degree=2, skip_rows=3, ema_alpha=0.3)
    return [(np.stack([lane_rows(hb, 1.0, "curved", seed=s),
                       lane_rows(hb, 1.0, "curved" if s % 2 else "straight", seed=s + 10)]), p)
            for s in (21, 22, 23)]


def recorded_case(g):
    """The run the reference recorded (path_recorded_run.npz) as a GPU case: its centreline rebuilt
    as a row table [1, 108, 4] from its grid integers (tests/test_bev_cpu.py) -- a 10-pixel run
    centred on x, which the exact centreline reads back as x -- and its parameters."""
    origin = (VIEW["min_x"], VIEW["min_y"])
    pts = np.rint(g["centerline_world"] - np.array(origin)).astype(int)
    rows = np.zeros((1, 108, 4), dtype=np.int32)
    for x, y in pts:
        rows[0, y] = (x - 5, x + 5, 10, sum(range(x - 5, x + 5)))
    car = g["car_position"]
    p = params(108, ppu=1.0, degree=2, num_waypoints=20, fast=0, min_width=10,
               min_y=float(g["waypoints"][0, 1]), max_y=float(g["waypoints"][-1, 1]),
               anchor_x=float(car[0]), anchor_y=float(car[1]), car_x=float(car[0]),
               car_y=float(car[1]), steering_gain=float(g["param_steering_gain"]),
               base_pwm=float(g["param_base_pwm"]),
               curvature_damping=float(g["param_curvature_damping"]),
               preview_distance=float(g["param_preview_distance"]),
               max_pwm=float(g["param_max_pwm"]), min_pwm=float(g["param_min_pwm"]))
    return rows, p
