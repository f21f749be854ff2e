"""CPU-side checks of the bird's-eye tail: the calibration / view restatement of
fast_scnn_pytorch_amd.bev against a run the reference recorded itself
(tests/golden/bev_recorded_run.npz, tools/gen_bev_golden.py), the self-checks of the GPU tests'
numpy yardstick (tests/bev_ref.py), ``centerline`` on hand-written row tables, and the interface
guards of ``EndToEndFastSCNN.bird_eye``."""
import numpy as np
import pytest
import torch

import bev_ref
import helpers
from fast_scnn_pytorch_amd import BirdEyeView, centerline
from fast_scnn_pytorch_amd import bev
from fast_scnn_pytorch_amd.deploy import EndToEndFastSCNN
from models.fast_scnn import FastSCNN


# ---- the recorded reference run -------------------------------------------------------------------------
def recorded_view():
    return BirdEyeView().params(pixels_per_unit=1, margin_ratio=0.1, full_image=True)


def test_view_matches_the_recorded_run():
    """Corrected calibration, 1 pixel per cm, 10 % margin, full image: the output size exactly,
    the view origin and the car position (image point (320, 359) through image_to_world_matrix)
    within 1e-4 cm of what the reference recorded (float32 at magnitude 100 resolves 8e-6)."""
    g = helpers.load_golden("bev_recorded_run")
    size, combined, bounds, vp = recorded_view()
    assert size == (208, 108) and vp["output_size"] == (208, 108)
    assert set(vp) == {"output_size", "view_bounds", "pixels_per_unit", "margin_ratio",
                       "transform_matrix", "image_to_world_matrix"}
    print("min_x %.8f min_y %.8f" % (bounds[0], bounds[1]))
    assert abs(float(bounds[0]) - -86.31710510253906) <= 1e-4
    assert abs(float(bounds[1]) - -54.44426651000977) <= 1e-4
    t = np.array(vp["image_to_world_matrix"], dtype=np.float32)
    p = t @ np.array([320, 359, 1], dtype=np.float32)
    car = np.array([p[0] / p[2], p[1] / p[2]], dtype=np.float64)
    print("car position", car, "recorded", g["car_position"])
    assert np.abs(car - g["car_position"]).max() <= 1e-4
    assert np.allclose(np.array(vp["transform_matrix"]), combined)


def test_recorded_centreline_lies_on_the_view_grid():
    """Each recorded centreline point is (min + integer / 1) of this view within 1e-3, and
    ``centerline`` reproduces the points from a row table holding those integers."""
    g = helpers.load_golden("bev_recorded_run")
    _, _, bounds, vp = recorded_view()
    origin = np.array([float(bounds[0]), float(bounds[1])])
    px = g["centerline_world"] - origin
    assert g["centerline_world"].shape == (20, 2)
    assert np.abs(px - np.rint(px)).max() <= 1e-3
    pts = np.rint(px).astype(int)
    assert (pts[:, 0] >= 0).all() and (pts[:, 0] < 208).all()
    assert (pts[:, 1] >= 0).all() and (pts[:, 1] < 108).all()
    assert (np.diff(pts[:, 1]) < 0).all()  # scanned from the bottom
    rows = np.zeros((108, 4), dtype=np.int32)
    for x, y in pts:  # a 10-pixel run centred on x, as both a run and a centroid
        rows[y] = (x - 5, x + 5, 10, sum(range(x - 5, x + 5)))
    for fast in (False, True):
        got_px, got_w = centerline(rows, vp, fast=fast, min_width=10, skip_rows=1)
        want = [(int(x) - (1 if fast else 0), int(y)) for x, y in pts]  # centroid of x-5 .. x+4
        assert got_px == want
        assert np.abs(np.array(got_w) - (origin + np.array(want))).max() <= 1e-3
    assert np.abs(np.array(centerline(rows, vp)[1]) - g["centerline_world"]).max() <= 1e-3


def test_homography_solves_its_four_points():
    src = [(260, 87), (378, 87), (410, 217), (231, 221)]
    dst = [(0, 0), (21, 0), (21, 29.7), (0, 29.7)]
    h = bev.perspective_transform(src, dst)
    assert h.dtype == np.float64 and h[2, 2] == 1.0
    for (x, y), (u, v) in zip(src, dst):
        p = h @ np.array([x, y, 1.0])
        assert abs(p[0] / p[2] - np.float32(u)) <= 1e-9 and abs(p[1] / p[2] - np.float32(v)) <= 1e-9
    cal = bev.get_corrected_calibration()
    top = np.array(cal["corrected_world_corners"])
    assert top[0, 1] == top[1, 1] and top[2, 1] == top[3, 1]
    assert BirdEyeView(use_corrected=False).transform_matrix.dtype == np.float32


def test_source_size_rescales_the_matrix():
    """transform.py:150-171: a source that is not the calibration size gets combined @ inv(scale)."""
    v = BirdEyeView()
    size, full, _, _ = v.params(1, 0.1, True)
    size2, half, _, vp = v.params(1, 0.1, True, source_size=(320, 180))
    assert size2 == size and half.dtype == np.float32
    assert np.allclose(half @ np.diag([0.5, 0.5, 1.0]).astype(np.float32), full, rtol=1e-6)
    assert np.allclose(bev.inverse_map(vp).reshape(3, 3) @ np.array(vp["transform_matrix"]),
                       np.eye(3), atol=1e-9)
    assert v.params(1, 0.1, True, source_size=(640, 360))[1] is not None
    assert v.params(20, 0.1, True)[0] == (4173, 2168) and v.params(5, 0.1, True)[0] == (1043, 542)


# ---- the yardstick's self-checks --------------------------------------------------------------------------
def test_identity_returns_the_mask():
    m = bev_ref.planted_mask(2, 33, 37)
    assert np.array_equal(bev_ref.warp(m, np.eye(3).ravel(), 33, 37), m)
    big = bev_ref.warp(m, np.eye(3).ravel(), 40, 50)
    assert np.array_equal(big[:, :33, :37], m) and not big[:, 33:].any() and not big[:, :, 37:].any()


def test_integer_translation_shifts_with_zero_border():
    m = bev_ref.planted_mask(1, 33, 37)
    t = np.array([1, 0, 3, 0, 1, -2, 0, 0, 1], dtype=np.float64)  # source = (x + 3, y - 2)
    out = bev_ref.warp(m, t, 33, 37)
    assert np.array_equal(out[:, 2:, :34], m[:, :31, 3:])
    assert not out[:, :2].any() and not out[:, :, 34:].any()


def test_rounding_is_half_to_even_and_w_zero_gives_zero():
    m = np.arange(1, 9, dtype=np.uint8).reshape(1, 1, 8)
    half = np.array([0.5, 0, 0, 0, 1, 0, 0, 0, 1], dtype=np.float64)  # sx = rint(x / 2)
    assert bev_ref.warp(m, half, 1, 8)[0, 0].tolist() == [1, 1, 2, 3, 3, 3, 4, 5]  # 0.5->0, 1.5->2, 2.5->2
    wz = np.array([1, 0, 0, 0, 0, 0, 1, 0, -5, ], dtype=np.float64)  # W = x - 5
    sx, sy = bev_ref.source_index(wz, 1, 8)
    assert sx[0, 5] == 0 and sx[0, 4] == -4 and sx[0, 6] == 6


ROWS = {
    "empty": [0] * 12,
    "full": [255] * 12,
    "two equal runs": [0, 1, 1, 1, 0, 0, 9, 9, 9, 0, 0, 0],
    "right edge": [0, 0, 1, 0, 0, 0, 0, 0, 255, 255, 255, 255],
    "exactly min_width": [0, 5, 5, 5, 0, 0, 0, 0, 0, 0, 0, 0],
    "min_width - 1": [0, 5, 5, 0, 0, 5, 5, 0, 0, 0, 5, 0],
    "longer run later": [1, 1, 1, 0, 1, 1, 1, 1, 0, 1, 1, 1],
}


@pytest.mark.parametrize("min_width", [1, 3, 4])
@pytest.mark.parametrize("name", list(ROWS))
def test_row_table_against_the_pixel_scans(name, min_width):
    row = np.array(ROWS[name], dtype=np.uint8)
    s, e, cnt, isum = bev_ref.row_entry(row, min_width)
    segs = bev_ref.segments_by_pixel(row, min_width)
    if segs:
        assert (s, e) == max(segs, key=lambda t: t[1] - t[0]) and e - s >= min_width
    else:
        assert (s, e) == (0, 0)
    assert cnt == int((row > 0).sum()) and isum == int(np.flatnonzero(row > 0).sum())
    # and through the public centerline, against the per-pixel centres
    vp = {"view_bounds": (-10.0, -20.0, 0, 0), "pixels_per_unit": 2}
    rows = np.array([[s, e, cnt, isum]], dtype=np.int32)
    exact = bev_ref.exact_center_by_pixel(row, min_width)
    pts, world = centerline(rows, vp, fast=False)
    assert pts == ([] if exact is None else [(exact, 0)])
    fast = bev_ref.fast_center_by_pixel(row, min_width)
    pts, world = centerline(rows, vp, fast=True, min_width=min_width, skip_rows=1)
    assert pts == ([] if fast is None else [(fast, 0)])
    if fast is not None:
        assert world == [(-10.0 + fast / 2, -20.0)]


def test_hand_written_rows_literal_values():
    assert bev_ref.row_entry(ROWS["two equal runs"], 3) == (1, 4, 6, 1 + 2 + 3 + 6 + 7 + 8)
    assert bev_ref.row_entry(ROWS["right edge"], 2) == (8, 12, 5, 2 + 8 + 9 + 10 + 11)
    assert bev_ref.row_entry(ROWS["exactly min_width"], 3) == (1, 4, 3, 6)
    assert bev_ref.row_entry(ROWS["min_width - 1"], 3) == (0, 0, 5, 1 + 2 + 5 + 6 + 10)
    assert bev_ref.row_entry(ROWS["min_width - 1"], 1) == (1, 3, 5, 24)
    assert bev_ref.row_entry(ROWS["full"], 1) == (0, 12, 12, 66)
    assert bev_ref.row_entry(ROWS["empty"], 1) == (0, 0, 0, 0)
    assert bev_ref.row_entry(ROWS["longer run later"], 1) == (4, 8, 10, 66 - 3 - 8)


def test_centerline_scan_order_and_skips():
    vp = {"view_bounds": (0.0, 0.0, 0, 0), "pixels_per_unit": 1}
    rows = np.array([[y, y + 6, 6, sum(range(y, y + 6))] for y in range(12)], dtype=np.int32)
    rows[4] = 0
    pts, _ = centerline(rows, vp)
    assert [p[1] for p in pts] == [11, 10, 9, 8, 7, 6, 5, 3, 2, 1, 0] and pts[0] == (14, 11)
    pts, _ = centerline(rows, vp, scan_from_bottom=False, min_width=7)
    assert pts == []
    pts, _ = centerline(rows, vp, fast=True)  # every 5th row from the bottom, count >= 5
    assert pts == [(13, 11), (8, 6), (3, 1)]
    pts, _ = centerline(rows, vp, fast=True, scan_from_bottom=False, skip_rows=4, min_width=7)
    assert pts == []
    pts, _ = centerline(torch.from_numpy(rows), vp, fast=True, scan_from_bottom=False, skip_rows=4)
    assert pts == [(2, 0), (10, 8)]  # row 4 is empty


# ---- interface guards --------------------------------------------------------------------------------------
def test_bird_eye_guards():
    bb = FastSCNN(2)
    m = EndToEndFastSCNN(bb, input_size=(48, 32), base_size=64)
    frames = torch.zeros(1, 3, 32, 48, dtype=torch.uint8)
    vp = BirdEyeView().params(1, 0.1, True, source_size=(48, 32))[3]
    with pytest.raises(RuntimeError, match="eval"):  # a fresh module is in train mode
        m.bird_eye(frames, vp)
    m.eval()
    with pytest.raises(RuntimeError, match="device"):  # CPU tensors: there is no fallback
        m.bird_eye(frames, vp)
    with pytest.raises(RuntimeError, match="device"):
        bev.warp_mask(torch.zeros(1, 32, 48, dtype=torch.uint8), np.eye(3), (8, 8))
    for size in ((8193, 10), (10, 65536), (0, 10)):
        wide = dict(vp, output_size=size)
        with pytest.raises(RuntimeError, match="8192"):
            m.bird_eye(frames, wide)
    with pytest.raises(RuntimeError, match="min_width"):
        m.bird_eye(frames, vp, min_width=0)
