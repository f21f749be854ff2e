"""The bird's-eye tail on the GPU (csrc/bev.hip, EndToEndFastSCNN.bird_eye): the warp and the row
table of a mask in memory against the numpy yardstick (tests/bev_ref.py), exactly; the fused
tail against predict + fscnn_bev_mask, bit for bit; the pipeline against the reference's stored
probabilities; the switch; the neighbours."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bev_ref
import e2e_ref
from e2e_ref import CASES, CLASSES, fixture, geometry
from fast_scnn_pytorch_amd import bev
from fast_scnn_pytorch_amd.deploy import EndToEndFastSCNN
from models.fast_scnn import FastSCNN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
DT_IDS = ["fp32", "fp16", "bf16"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. fscnn_bev_mask against the yardstick --------------------------------------------------------------
SOURCES = [(33, 37), (48, 80)]  # (Ho, Wo)
WIDTHS = [1, 63, 64, 65, 257, 1100, 8192]
MATRICES = ["identity", "calibration", "outside", "w_zero", "stretch"]


def matrix(kind, ho, wo, hb, wb):
    """Destination -> source.  ``calibration``: the corrected calibration rescaled to the source
    size at 1 pixel per cm, its view moved down 40 rows so that the first rows see the road;
    ``outside`` maps every pixel off the source; ``w_zero``: W = x - 5 is exactly 0 at column 5 and
    changes sign across the row; ``stretch`` maps the whole view onto the whole source, so that
    planted full rows become runs of the full view width."""
    if kind == "identity":
        return np.eye(3).ravel()
    if kind == "calibration":
        vp = bev.BirdEyeView().params(1, 0.1, True, source_size=(wo, ho))[3]
        shift = np.array([[1, 0, 0], [0, 1, 40], [0, 0, 1]], dtype=np.float64)
        return (bev.inverse_map(vp).reshape(3, 3) @ shift).ravel()
    if kind == "outside":
        return np.array([1, 0, 1e6, 0, 1, 0, 0, 0, 1], dtype=np.float64)
    if kind == "w_zero":
        return np.array([10, 1, -30, 2, 8, -10, 1, 0, -5], dtype=np.float64)
    return np.array([(wo - 1) / max(wb - 1, 1), 0, 0, 0, (ho - 1) / max(hb - 1, 1), 0, 0, 0, 1],
                    dtype=np.float64)


@functools.lru_cache(maxsize=None)
def dev_mask(n, ho, wo):
    return torch.from_numpy(bev_ref.planted_mask(n, ho, wo).copy()).to(DEV)


@pytest.mark.parametrize("wb", WIDTHS)
@pytest.mark.parametrize("kind", MATRICES)
@pytest.mark.parametrize("src", SOURCES, ids=["33x37", "48x80"])
def test_bev_mask_matches_the_yardstick(src, kind, wb):
    """Mask and rows exactly equal to the float64 numpy restatement, no exclusions; N in {1, 3},
    Hb in {1, 5, 50} (2 at the widest view); also with a null mask output (rows only)."""
    ho, wo = src
    min_width = 10 if wb > 64 else 3 if wb > 1 else 1
    for n in (1, 3):
        for hb in ((2,) if wb == 8192 else (1, 5, 50)):
            m = matrix(kind, ho, wo, hb, wb)
            want = bev_ref.warp(bev_ref.planted_mask(n, ho, wo), m, hb, wb)
            want_rows = bev_ref.row_table(want, min_width)
            got, rows = bev.warp_mask(dev_mask(n, ho, wo), m, (wb, hb), min_width)
            assert got.shape == (n, hb, wb) and got.dtype == torch.uint8
            assert rows.shape == (n, hb, 4) and rows.dtype == torch.int32
            bad = int((got.cpu().numpy() != want).sum())
            assert bad == 0, "%d mask pixels differ (N=%d Hb=%d)" % (bad, n, hb)
            assert np.array_equal(rows.cpu().numpy(), want_rows), (n, hb)
            none, rows_only = bev.warp_mask(dev_mask(n, ho, wo), m, (wb, hb), min_width,
                                            return_mask=False)
            assert none is None and torch.equal(rows_only, rows)
            if kind == "outside":
                assert not want.any() and not want_rows.any()
            if kind == "stretch" and hb == 50:
                assert (want_rows[:, :, 1] - want_rows[:, :, 0]).max() == wb  # a full-width run
    print("%dx%d %s Wb=%d: non-zero share of the last view %.3f" % (ho, wo, kind, wb,
                                                                   (want != 0).mean()))


def test_min_width_one_and_ties():
    """min_width = 1 takes single pixels; equal runs resolve to the left one, across the 64-bit
    words of the row bitmask too."""
    row = np.zeros((1, 1, 300), dtype=np.uint8)
    row[0, 0, 60:70] = 255   # crosses the first word boundary
    row[0, 0, 120:130] = 9   # crosses the second, same length
    row[0, 0, 299] = 1
    for mw, want in ((1, (60, 70)), (10, (60, 70)), (11, (0, 0))):
        _, rows = bev.warp_mask(torch.from_numpy(row).to(DEV), np.eye(3), (300, 1), mw)
        assert tuple(rows[0, 0, :2].tolist()) == want
        assert rows[0, 0, 2:].tolist() == [21, sum(range(60, 70)) + sum(range(120, 130)) + 299]
        assert np.array_equal(rows.cpu().numpy(), bev_ref.row_table(row, mw))
    row[0, 0, 130:200] = 3
    _, rows = bev.warp_mask(torch.from_numpy(row).to(DEV), np.eye(3), (300, 1), 1)
    assert rows[0, 0, :2].tolist() == [120, 200]


def test_c_abi_limits_and_errors():
    """-2 before any launch outside the limits, -1 for a matrix that is not finite."""
    from fast_scnn_pytorch_amd import _lib
    import ctypes
    lib = _lib.load()
    mask = dev_mask(1, 33, 37)
    rows = torch.full((1, 4, 4), -7, dtype=torch.int32, device=DEV)
    eye = (ctypes.c_double * 9)(*np.eye(3).ravel())

    def call(m=eye, hb=1, wb=4, mw=1, n=1):
        return lib.fscnn_bev_mask(_lib.ptr(mask), n, 33, 37, m, hb, wb, mw, None, _lib.ptr(rows),
                                  _lib.stream_ptr(torch.device(DEV)))
    assert call(wb=8193) == -2 and call(wb=0) == -2 and call(hb=65536) == -2 and call(hb=0) == -2
    assert call(mw=0) == -2 and call(n=65536) == -2
    nan = (ctypes.c_double * 9)(*([1, 0, 0, 0, 1, 0, 0, 0, float("nan")]))
    inf = (ctypes.c_double * 9)(*([float("inf"), 0, 0, 0, 1, 0, 0, 0, 1]))
    assert call(m=nan) == -1 and call(m=inf) == -1
    assert b"finite" in lib.fscnn_last_error()
    torch.cuda.synchronize()
    assert bool((rows == -7).all())  # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert rows[0, 0].tolist() == list(bev_ref.row_entry(bev_ref.planted_mask(1, 33, 37)[0, 0, :4], 1))


# ---- 2. fused against unfused ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def backbone(nc):
    m = FastSCNN(nc)
    m.load_state_dict(e2e_ref.weights(nc))
    return m.to(DEV).eval()


def wrapper(case, nc, dtype=torch.float32):
    size, base, mean, std = geometry(fixture(case, nc))
    m = EndToEndFastSCNN(backbone(nc), input_size=size, base_size=base, mean=mean, std=std,
                         dtype=dtype)
    m.preprocessor.to(DEV)
    return m.eval()


def frames_of(case, nc, batch=3):
    return fixture(case, nc)["frames"][:batch].to(DEV)


def view_of(case, nc):
    """The corrected calibration's full-image view at 1 pixel per cm (208 x 108), rescaled to the
    case's frame size."""
    size = geometry(fixture(case, nc))[0]
    return bev.BirdEyeView().params(1, 0.1, True, source_size=size)[3]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("nc", CLASSES)
@pytest.mark.parametrize("case", CASES)
def test_fused_equals_predict_then_warp(case, nc, dtype):
    """bird_eye(frames) == fscnn_bev_mask(predict(frames, scale)) bit for bit, mask and rows,
    batch 3, scale 1 and 255: both tails evaluate a frame pixel with the same ee_pixel."""
    e2e = wrapper(case, nc, dtype)
    frames = frames_of(case, nc)
    vp = view_of(case, nc)
    m = bev.inverse_map(vp)
    for scale in (1, 255):
        mask, rows = e2e.bird_eye(frames, vp, scale=scale, min_width=10)
        assert e2e._last_fused is True
        assert mask.shape == (3, 108, 208) and rows.shape == (3, 108, 4)
        want_mask, want_rows = bev.warp_mask(e2e.predict(frames, scale=scale), m, (208, 108), 10)
        bad = int((mask != want_mask).sum())
        print("%s C=%d %s scale %d: %d differing pixels, non-zero share %.3f"
              % (case, nc, dtype, scale, bad, float((mask != 0).float().mean())))
        assert bad == 0
        assert torch.equal(rows, want_rows)
        none, rows_only = e2e.bird_eye(frames, vp, scale=scale, min_width=10, return_mask=False)
        assert none is None and torch.equal(rows_only, rows)


@pytest.mark.parametrize("nc", CLASSES)
def test_switch_takes_the_unfused_route(nc, tmp_path):
    """FSCNN_E2E_FUSED=0 in a fresh process: bird_eye reports the unfused route and returns the
    warp of that process's own predict (checked here against the numpy yardstick)."""
    out = str(tmp_path / "bev.npz")
    env = dict(os.environ, FSCNN_E2E_FUSED="0")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_bev_worker.py"), out, "200x70",
                    str(nc)], check=True, env=env, timeout=300)
    r = np.load(out)
    assert not bool(r["fused"]) and not bool(r["predict_fused"])
    vp = view_of("200x70", nc)
    want = bev_ref.warp(r["labels"], bev.inverse_map(vp), 108, 208)
    assert np.array_equal(r["mask"], want)
    assert np.array_equal(r["rows"], bev_ref.row_table(want, 10))
    # and the fused route of this process agrees wherever the two predicts do
    e2e = wrapper("200x70", nc)
    frames = frames_of("200x70", nc)
    mask, rows = e2e.bird_eye(frames, vp, scale=255, min_width=10)
    assert e2e._last_fused is True
    same = e2e.predict(frames, scale=255).cpu().numpy() == r["labels"]
    print("C=%d: predicts agree on %.4f of the frame" % (nc, same.mean()))
    if same.all():
        assert np.array_equal(mask.cpu().numpy(), r["mask"])
        assert np.array_equal(rows.cpu().numpy(), r["rows"])


@pytest.mark.parametrize("nc", CLASSES)
def test_large_views_take_two_launches_with_the_same_bits(nc):
    """Past the measured break-even (profiles/bev_time.md) bird_eye runs predict + fscnn_bev_mask
    by itself; forcing either route gives the same mask and rows (1043 x 542 view, batch 3)."""
    e2e = wrapper("80x48", nc, torch.float16)
    frames = frames_of("80x48", nc)
    vp = bev.BirdEyeView().params(5, 0.1, True, source_size=(80, 48))[3]
    assert vp["output_size"] == (1043, 542)
    mask, rows = e2e.bird_eye(frames, vp)
    assert e2e._last_fused is False and mask.shape == (3, 542, 1043)
    fmask, frows = e2e.bird_eye(frames, vp, fused=True)
    assert e2e._last_fused is True
    assert torch.equal(fmask, mask) and torch.equal(frows, rows)
    tmask, trows = e2e.bird_eye(frames[:1], view_of("80x48", nc), fused=False)
    assert e2e._last_fused is False
    small = e2e.bird_eye(frames[:1], view_of("80x48", nc))
    assert e2e._last_fused is True
    assert torch.equal(small[0], tmask) and torch.equal(small[1], trows)


def test_more_than_32_classes_take_the_unfused_route():
    torch.manual_seed(0)
    bb = FastSCNN(40).to(DEV).eval()
    frames = frames_of("80x48", 2, 1)
    e2e = EndToEndFastSCNN(bb, input_size=(80, 48), base_size=64).to(DEV).eval()
    vp = bev.BirdEyeView().params(1, 0.1, True, source_size=(80, 48))[3]
    mask, rows = e2e.bird_eye(frames, vp, scale=1)
    assert e2e._last_fused is False
    want = bev_ref.warp(e2e.predict(frames).cpu().numpy(), bev.inverse_map(vp), 108, 208)
    assert np.array_equal(mask.cpu().numpy(), want)
    assert np.array_equal(rows.cpu().numpy(), bev_ref.row_table(want, 10))


# ---- 3. pipeline against the reference ----------------------------------------------------------------------------
FULL_PROBS = [c for c in CASES if "probs_idx" not in fixture(c, 2)]


@pytest.mark.parametrize("case", FULL_PROBS)
def test_pipeline_matches_the_reference(case):
    """The fp32 bird's-eye mask against warp(argmax(reference probabilities) * 255), leaving out
    only the view pixels whose source pixel has a reference top-2 probability margin <= 2e-4:
    twice the 1e-4 budget of test_pipeline_matches_reference_fp32, the only way two outputs each
    within that budget of the truth can disagree.  The left-out share, computed from the fixtures
    alone, is 0.006 % .. 0.11 % of the in-bounds pixels on these five cases (cap: 5 %)."""
    assert len(FULL_PROBS) == 5
    g = fixture(case, 2)
    size = geometry(g)[0]
    vp = view_of(case, 2)
    m = bev.inverse_map(vp)
    p = g["probs"]
    top = np.sort(p, axis=1)
    close = (top[:, -1] - top[:, -2]) <= 2e-4
    ok, sx, sy = bev_ref.inside(m, 108, 208, size[1], size[0])
    left_out = np.zeros((3, 108, 208), dtype=bool)
    left_out[:, ok] = close[:, sy[ok], sx[ok]]
    share = left_out[:, ok].mean()
    want = bev_ref.warp((p.argmax(1) * 255).astype(np.uint8), m, 108, 208)
    e2e = wrapper(case, 2)
    mask, rows = e2e.bird_eye(frames_of(case, 2), vp, scale=255, min_width=10)
    assert e2e._last_fused is True
    got = mask.cpu().numpy()
    wrong = int(((got != want) & ~left_out).sum())
    print("%s: %d wrong view pixels outside the left-out %.4f %% (of %d in-bounds pixels), "
          "non-zero share %.3f" % (case, wrong, 100 * share, 3 * ok.sum(), (want != 0).mean()))
    assert share <= 0.05
    assert wrong == 0
    assert not got[:, ~ok].any()
    assert np.array_equal(rows.cpu().numpy(), bev_ref.row_table(got, 10))
    # the centreline of the table is the per-pixel centreline of the mask
    pts, world = bev.centerline(rows[0], vp)
    want_pts = [(c, y) for y in range(107, -1, -1)
                for c in [bev_ref.exact_center_by_pixel(got[0, y], 10)] if c is not None]
    assert pts == want_pts and len(world) == len(pts)
    pts, _ = bev.centerline(rows[0], vp, fast=True, min_width=5, skip_rows=5)
    want_pts = [(c, y) for y in range(107, -1, -5)
                for c in [bev_ref.fast_center_by_pixel(got[0, y], 5)] if c is not None]
    assert pts == want_pts


# ---- 4. neighbours ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", CLASSES)
def test_neighbours_unchanged(nc):
    """e2e(frames) and e2e.predict(frames) return after bird_eye calls what they returned before
    (same plans, arenas and workspace layout), and the backbone's state is untouched."""
    bb = backbone(nc)
    e2e = wrapper("200x70", nc)
    frames = frames_of("200x70", nc)
    vp = view_of("200x70", nc)
    p0, l0 = e2e(frames).clone(), e2e.predict(frames, scale=255).clone()
    sd0 = {k: v.clone() for k, v in bb.state_dict().items()}
    first = e2e.bird_eye(frames, vp)
    e2e.bird_eye(frames, vp, scale=1, return_mask=False)
    wrapper("200x70", nc, torch.float16).bird_eye(frames, vp)
    assert torch.equal(e2e(frames), p0) and torch.equal(e2e.predict(frames, scale=255), l0)
    again = e2e.bird_eye(frames, vp)
    assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    for k, v in bb.state_dict().items():
        assert torch.equal(v, sd0[k]), k


def test_gpu_guards():
    e2e = wrapper("80x48", 2)
    frames = frames_of("80x48", 2)
    vp = view_of("80x48", 2)
    with pytest.raises(RuntimeError, match="device"):
        e2e.bird_eye(frames.cpu(), vp)
    with pytest.raises(RuntimeError, match="8192"):
        e2e.bird_eye(frames, dict(vp, output_size=(8193, 108)))
    e2e.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            e2e.bird_eye(frames, vp)
    finally:
        e2e.eval()  # the backbone is shared between the tests
    assert e2e.bird_eye(frames, vp)[1].shape == (3, 108, 4)
