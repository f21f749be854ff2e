"""Shared by the bird's-eye tests: a float64 numpy restatement of the coordinate law of
include/fastscnn.h (nearest-neighbour perspective warp, border 0), the row table by run-length
arithmetic, and a per-pixel restatement of the reference's two row scans
(kuruma/vision/path_planning.py:188-293) that the table is checked against on the CPU."""
import functools
import itertools

import numpy as np

INT_MIN, INT_MAX = float(-2 ** 31), float(2 ** 31 - 1)


def source_index(m, hb, wb):
    """(sx, sy) int64 [hb, wb] of the law: every operation a separate float64 ufunc, so nothing
    is fused; X*W clamped to the int range (NaN -> INT_MAX), rounded half to even."""
    m = np.asarray(m, dtype=np.float64).reshape(9)
    x = np.arange(wb, dtype=np.float64)[None, :]
    y = np.arange(hb, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        X = (m[0] * x + m[1] * y) + m[2]
        Y = (m[3] * x + m[4] * y) + m[5]
        W = (m[6] * x + m[7] * y) + m[8]
        W = np.where(W != 0, 1.0 / np.where(W != 0, W, 1.0), 0.0)
        out = []
        for v in (X * W, Y * W):
            v = np.where(v < INT_MAX, v, INT_MAX)
            v = np.where(v > INT_MIN, v, INT_MIN)
            out.append(np.rint(v).astype(np.int64))
    return out[0], out[1]


def inside(m, hb, wb, ho, wo):
    sx, sy = source_index(m, hb, wb)
    return (sx >= 0) & (sx < wo) & (sy >= 0) & (sy < ho), sx, sy


def warp(mask, m, hb, wb):
    """uint8 [N, hb, wb]: mask[n, sy, sx] where (sx, sy) is inside the source, else 0."""
    mask = np.asarray(mask)
    ok, sx, sy = inside(m, hb, wb, mask.shape[1], mask.shape[2])
    out = np.zeros((mask.shape[0], hb, wb), dtype=np.uint8)
    out[:, ok] = mask[:, sy[ok], sx[ok]]
    return out


def row_entry(row, min_width):
    """(run_start, run_end, count, index_sum) of one row."""
    nz = np.flatnonzero(np.asarray(row) != 0)
    d = np.diff(np.concatenate(([0], (np.asarray(row) != 0).astype(np.int8), [0])))
    starts, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    lens = ends - starts
    keep = lens >= min_width
    s = e = 0
    if keep.any():
        i = int(np.argmax(np.where(keep, lens, -1)))  # first of the longest
        s, e = int(starts[i]), int(ends[i])
    return s, e, int(nz.size), int(nz.sum())


def row_table(bev, min_width):
    """int32 [N, hb, 4] of a warped mask."""
    bev = np.asarray(bev)
    out = np.zeros(bev.shape[:2] + (4,), dtype=np.int32)
    for n, y in itertools.product(range(bev.shape[0]), range(bev.shape[1])):
        out[n, y] = row_entry(bev[n, y], min_width)
    return out


# ---- the reference's scans, pixel by pixel ----------------------------------------------------------
def segments_by_pixel(row, min_width):
    """Every maximal run of pixels > 0 of length >= min_width as (start, end), end exclusive, in
    row order: what PathPlanner._find_drivable_segments returns."""
    segs, x = [], 0
    for on, grp in itertools.groupby(int(p) > 0 for p in row):
        n = sum(1 for _ in grp)
        if on and n >= min_width:
            segs.append((x, x + n))
        x += n
    return segs


def exact_center_by_pixel(row, min_width):
    """extract_centerline's centre of one row, or None: Python's max keeps the first of the
    longest segments."""
    segs = segments_by_pixel(row, min_width)
    if not segs:
        return None
    s = max(segs, key=lambda t: t[1] - t[0])
    return (s[0] + s[1]) // 2


def fast_center_by_pixel(row, min_width):
    """extract_centerline_fast's centre of one row, or None: int(mean of the indices > 0)."""
    idx = np.where(np.asarray(row) > 0)[0]
    return int(np.mean(idx)) if len(idx) >= min_width else None


# ---- inputs of the GPU tests ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted_mask(n, ho, wo):
    """Random 0 / 255 / other non-zero values with planted rows: full rows, rows with two equal
    runs, a run touching the right edge, an empty row."""
    rng = np.random.default_rng(1000 * ho + wo)
    m = np.where(rng.random((n, ho, wo)) < 0.55, 255, 0).astype(np.uint8)
    m[rng.random((n, ho, wo)) < 0.05] = 7
    for i in range(n):
        m[i, 1 % ho] = 255
        m[i, 3 % ho] = 0
        m[i, 5 % ho] = 0
        m[i, 5 % ho, 2:2 + wo // 3] = 255
        m[i, 5 % ho, wo - wo // 3:] = 255
        m[i, 7 % ho, :wo // 2] = 0
        m[i, 7 % ho, wo // 2:] = 1
        m[i, ho - 1] = 255
        m[i, ho - 1, wo // 2] = 0
    m.setflags(write=False)
    return m
