"""The colour bird's-eye view on the GPU (csrc/bev_image.hip: bev.warp_image,
BirdEyeView.transform_image_and_mask, EndToEndFastSCNN.bird_eye_view) against the numpy yardstick
(tests/bev_image_ref.py).  Every comparison is exact."""
import ctypes
import functools
import io

import numpy as np
import pytest
import torch

import bev_image_ref
import bev_ref
import helpers
from fast_scnn_pytorch_amd import _lib, bev
from fast_scnn_pytorch_amd.deploy import EndToEndFastSCNN
from models.fast_scnn import FastSCNN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FRAMES = [(2, 2), (3, 5), (29, 37), (360, 640)]  # (h, w)
VIEWS = [(1, 1), (63, 2), (64, 3), (257, 5), (300, 7), (208, 108)]  # (Wb, Hb)
MATRICES = ["identity", "shift_1", "shift_16", "shift_31", "shift_-17", "rot90", "calibration_1",
            "calibration_2", "horizon"]


def matrix(kind, h, w, hb):
    """Destination -> source.  ``shift_k``: source = view + k / 32 in both directions, so every tap
    at a border mixes with 0; ``rot90``: source = (y, h - 1 - x); ``calibration_p``: the corrected
    calibration rescaled to the frame at p pixels per cm, moved down 40 p rows in the low views so
    that their rows see the road; ``horizon``: W = x - 5 is exactly 0 in column 5 and changes sign
    there, and Y = 2^27 y makes 32 Y / W leave the int range next to that column from row 1 on,
    while row 0 (Y = 0) stays in the frame."""
    if kind == "identity":
        return np.eye(3).ravel()
    if kind.startswith("shift_"):
        k = int(kind[6:]) / 32
        return np.array([1, 0, k, 0, 1, k, 0, 0, 1], dtype=np.float64)
    if kind == "rot90":
        return np.array([0, 1, 0, -1, 0, h - 1, 0, 0, 1], dtype=np.float64)
    if kind.startswith("calibration_"):
        ppu = int(kind[12:])
        vp = bev.BirdEyeView().params(ppu, 0.1, True, source_size=(w, h))[3]
        shift = np.array([[1, 0, 0], [0, 1, 40 * ppu if hb < 50 else 0], [0, 0, 1]], dtype=np.float64)
        return (bev.inverse_map(vp).reshape(3, 3) @ shift).ravel()
    assert kind == "horizon"
    return np.array([10, 1, -30, 0, 2.0 ** 27, 0, 1, 0, -5], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def dev_frames(n, h, w, channels_last):
    return torch.from_numpy(bev_image_ref.planted_frames(n, h, w, channels_last).copy()).to(DEV)


@functools.lru_cache(maxsize=None)
def dev_mask(n, hb, wb):
    return torch.from_numpy(bev_ref.planted_mask(n, hb, wb).copy()).to(DEV)


# ---- 1. fscnn_bev_image against the yardstick ---------------------------------------------------------------
@pytest.mark.parametrize("kind", MATRICES)
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("frame", FRAMES, ids=["%dx%d" % (w, h) for h, w in FRAMES])
def test_warp_matches_the_yardstick(frame, channels_last, kind):
    """Every byte equal to the numpy restatement: N in {1, 3}, the six views."""
    h, w = frame
    inside = 0
    for n in (1, 3):
        f = bev_image_ref.planted_frames(n, h, w, channels_last)
        for wb, hb in VIEWS:
            m = matrix(kind, h, w, hb)
            info = {}
            want = bev_image_ref.warp(f, m, hb, wb, channels_last, info=info)
            got = bev.warp_image(dev_frames(n, h, w, channels_last), m, (wb, hb),
                                 channels_last=channels_last)
            assert got.dtype == torch.uint8 and got.is_contiguous()
            assert tuple(got.shape) == ((n, hb, wb, 3) if channels_last else (n, 3, hb, wb))
            bad = int((got.cpu().numpy() != want).sum())
            assert bad == 0, "%d bytes differ (N=%d view %dx%d)" % (bad, n, wb, hb)
            inside += info["inside"]
            if kind == "identity":
                g = got.cpu().numpy()
                g = g if channels_last else g.transpose(0, 2, 3, 1)
                ff = f if channels_last else f.transpose(0, 2, 3, 1)
                hh, ww = min(h, hb), min(w, wb)
                assert np.array_equal(g[:, :hh, :ww], ff[:, :hh, :ww])
                assert not g[:, hh:].any() and not g[:, :, ww:].any()
            if kind == "horizon" and (wb, hb) != (1, 1):
                assert info["w_zero"] == hb and info["clamped"] > 0, info
    assert inside > 0
    print("%dx%d %s %s: %d view pixels with a tap in the frame" % (w, h, kind, channels_last, inside))


# ---- 2. the blend ---------------------------------------------------------------------------------------------------
BLENDS = [(0.5, 1.0, 0.0), (0.3, 1.0, 0.0), (0.5, 0.7, 3.0)]  # alpha, frame_weight, gamma


@pytest.mark.parametrize("blend", BLENDS, ids=["a0.5", "a0.3", "a0.5_fw0.7_g3"])
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
def test_blend_matches_the_yardstick(channels_last, blend):
    """image and the segmented picture of one launch, with a planted 0 / 255 / 7 mask."""
    alpha, fw, gamma = blend
    h, w = 29, 37
    color = (10, 255, 77)
    for n in (1, 3):
        f = bev_image_ref.planted_frames(n, h, w, channels_last)
        for wb, hb in VIEWS:
            for kind in ("shift_16", "calibration_1"):
                m = matrix(kind, h, w, hb)
                mask = bev_ref.planted_mask(n, hb, wb)
                want = bev_image_ref.warp(f, m, hb, wb, channels_last)
                want_b = bev_image_ref.blend(want, mask, alpha, color, fw, gamma, channels_last)
                got, got_b = bev.warp_image(dev_frames(n, h, w, channels_last), m, (wb, hb),
                                            channels_last=channels_last, mask=dev_mask(n, hb, wb),
                                            alpha=alpha, color=color, frame_weight=fw, gamma=gamma)
                assert np.array_equal(got.cpu().numpy(), want), (n, wb, hb, kind)
                assert np.array_equal(got_b.cpu().numpy(), want_b), (n, wb, hb, kind)
    assert (want_b != want).any()


# ---- 3. the C ABI: null outputs, unaligned outputs, refusals -------------------------------------------------------
def abi(frames, channels_last, n, h, w, m, hb, wb, image, mask, color, blended, fw=1.0, alpha=0.5,
        gamma=0.0):
    """fscnn_bev_image with raw pointers (ints or None); returns the status."""
    cm = (ctypes.c_double * 9)(*[float(v) for v in np.asarray(m).reshape(9)])
    c3 = None if color is None else (ctypes.c_ubyte * 3)(*color)
    vp = lambda p: None if p is None else ctypes.c_void_p(p)  # noqa: E731
    with torch.cuda.device(torch.device(DEV)):
        return _lib.load().fscnn_bev_image(vp(frames), channels_last, n, h, w, cm, hb, wb, vp(image),
                                           vp(mask), c3, fw, alpha, gamma, vp(blended),
                                           _lib.stream_ptr(torch.device(DEV)))


@pytest.mark.parametrize("channels_last", [0, 1], ids=["nchw", "nhwc"])
def test_either_output_alone_and_unaligned_outputs(channels_last):
    """image null with blended set and the reverse; outputs that start 1, 2 and 3 bytes past a
    dword boundary, with the bytes around them left alone."""
    n, h, w, wb, hb = 2, 29, 37, 257, 5
    f = bev_image_ref.planted_frames(n, h, w, bool(channels_last))
    m = matrix("shift_-17", h, w, hb)
    mask = bev_ref.planted_mask(n, hb, wb)
    want = bev_image_ref.warp(f, m, hb, wb, bool(channels_last))
    want_b = bev_image_ref.blend(want, mask, 0.5, (0, 255, 0), channels_last=bool(channels_last))
    size = want.size
    df, dm = dev_frames(n, h, w, bool(channels_last)), dev_mask(n, hb, wb)
    for lead_i, lead_b in ((0, 0), (1, 2), (3, 1), (2, 3)):
        for which in ("image", "blended", "both"):
            bi = torch.full((size + 16,), 0xA5, dtype=torch.uint8, device=DEV)
            bb = torch.full((size + 16,), 0x5A, dtype=torch.uint8, device=DEV)
            pi = bi.data_ptr() + 4 + lead_i if which != "blended" else None
            pb = bb.data_ptr() + 4 + lead_b if which != "image" else None
            rc = abi(df.data_ptr(), channels_last, n, h, w, m, hb, wb, pi, dm.data_ptr(),
                     (0, 255, 0), pb)
            assert rc == 0, _lib.load().fscnn_last_error()
            torch.cuda.synchronize()
            hi, hbl = bi.cpu().numpy(), bb.cpu().numpy()
            if pi is not None:
                o = 4 + lead_i
                assert np.array_equal(hi[o:o + size], want.reshape(-1)), (lead_i, which)
                assert (hi[:o] == 0xA5).all() and (hi[o + size:] == 0xA5).all()
            else:
                assert (hi == 0xA5).all()
            if pb is not None:
                o = 4 + lead_b
                assert np.array_equal(hbl[o:o + size], want_b.reshape(-1)), (lead_b, which)
                assert (hbl[:o] == 0x5A).all() and (hbl[o + size:] == 0x5A).all()
            else:
                assert (hbl == 0x5A).all()


def test_c_abi_refusals_launch_nothing():
    """-1 for a matrix that is not finite, missing arguments and aliasing; -2 outside the limits;
    the outputs keep their bytes."""
    n, h, w, wb, hb = 1, 29, 37, 64, 3
    df, dm = dev_frames(n, h, w, True), dev_mask(n, hb, wb)
    out = torch.full((n * hb * wb * 3,), 0xA5, dtype=torch.uint8, device=DEV)
    out2 = torch.full((n * hb * wb * 3,), 0xA5, dtype=torch.uint8, device=DEV)
    eye = np.eye(3)
    F, M, O, O2 = df.data_ptr(), dm.data_ptr(), out.data_ptr(), out2.data_ptr()

    def call(frames=F, n=n, h=h, w=w, m=eye, hb=hb, wb=wb, image=O, mask=M, color=(0, 255, 0),
             blended=O2):
        return abi(frames, 1, n, h, w, m, hb, wb, image, mask, color, blended)
    nan = np.array([1, 0, 0, 0, 1, 0, 0, 0, float("nan")])
    inf = np.array([float("inf"), 0, 0, 0, 1, 0, 0, 0, 1])
    assert call(m=nan) == -1 and call(m=inf) == -1
    assert b"finite" in _lib.load().fscnn_last_error()
    assert call(frames=None) == -1
    assert call(image=None, blended=None) == -1            # neither output
    assert call(mask=None) == -1 and call(color=None) == -1  # blended needs both
    assert call(image=F) == -1 and call(blended=F) == -1   # aliasing the frames
    assert b"aliasing" in _lib.load().fscnn_last_error()
    assert call(image=O, blended=O) == -1 and call(blended=M) == -1
    for kw in (dict(n=0), dict(n=65536), dict(wb=0), dict(wb=8193), dict(hb=0), dict(hb=65536),
               dict(h=1), dict(w=1), dict(h=16385), dict(w=16385)):
        assert call(**kw) == -2, kw
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and bool((out2 == 0xA5).all())  # nothing was launched
    assert call(mask=None, color=None, blended=None) == 0           # the image alone needs neither
    assert call() == 0
    torch.cuda.synchronize()
    f = bev_image_ref.planted_frames(n, h, w, True)
    want = bev_image_ref.warp(f, eye, hb, wb, True)
    assert np.array_equal(out.cpu().numpy(), want.reshape(-1))
    assert np.array_equal(out2.cpu().numpy(),
                          bev_image_ref.blend(want, bev_ref.planted_mask(n, hb, wb),
                                              channels_last=True).reshape(-1))


def test_python_guards_on_the_device():
    f = dev_frames(1, 29, 37, False)
    with pytest.raises(RuntimeError, match="h, w >= 2"):
        bev.warp_image(torch.zeros(1, 3, 1, 8, dtype=torch.uint8, device=DEV), np.eye(3), (4, 4))
    with pytest.raises(RuntimeError, match="finite"):
        bev.warp_image(f, np.full(9, np.nan), (4, 4))
    with pytest.raises(RuntimeError, match="mask"):
        bev.warp_image(f, np.eye(3), (4, 4), mask=dev_mask(1, 5, 4))
    with pytest.raises(RuntimeError, match="device"):
        bev.warp_image(f, np.eye(3), (4, 4), mask=torch.zeros(1, 4, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="uint8"):
        bev.warp_image(f.half(), np.eye(3), (4, 4))
    # the layout is read off the shape
    a = bev.warp_image(dev_frames(1, 29, 37, True), np.eye(3), (4, 4))
    assert tuple(a.shape) == (1, 4, 4, 3)
    assert tuple(bev.warp_image(f, np.eye(3), (4, 4)).shape) == (1, 3, 4, 4)


# ---- 4. transform_image_and_mask ---------------------------------------------------------------------------------
def test_transform_image_and_mask_on_the_recorded_frame():
    """The reference's signature on the frame its recorded run read: the image equals the
    yardstick, the mask bev_ref.warp, single and batched, and at a source that is not the
    calibration size."""
    Image = pytest.importorskip("PIL.Image")
    g = helpers.load_golden("bev_image_recorded_run")
    src = np.array(Image.open(io.BytesIO(g["source_jpeg"].tobytes())).convert("RGB"))  # writable
    mask = bev_ref.planted_mask(1, 360, 640)[0]
    view = bev.BirdEyeView()
    img_d, mask_d = torch.from_numpy(src).to(DEV), torch.from_numpy(mask.copy()).to(DEV)
    for ppu, size in ((1, (208, 108)), (2, (417, 216))):
        bird, bird_mask, vp = view.transform_image_and_mask(img_d, mask_d, pixels_per_unit=ppu)
        want_vp = view.params(ppu, 0.1, True)[3]
        assert vp == want_vp and tuple(vp["output_size"]) == size
        wb, hb = size
        m = bev.inverse_map(vp)
        assert tuple(bird.shape) == (hb, wb, 3) and tuple(bird_mask.shape) == (hb, wb)
        assert np.array_equal(bird.cpu().numpy(), bev_image_ref.warp(src[None], m, hb, wb, True)[0])
        assert np.array_equal(bird_mask.cpu().numpy(), bev_ref.warp(mask[None], m, hb, wb)[0])
    # batched, half size: the matrix is rescaled as params(source_size=...) does
    small = np.ascontiguousarray(np.stack([src[::2, ::2], src[1::2, 1::2]]))
    small_mask = np.ascontiguousarray(np.stack([mask[::2, ::2], mask[1::2, 1::2]]))
    bird, bird_mask, vp = view.transform_image_and_mask(torch.from_numpy(small).to(DEV),
                                                        torch.from_numpy(small_mask).to(DEV), 1)
    assert vp == view.params(1, 0.1, True, source_size=(320, 180))[3]
    m = bev.inverse_map(vp)
    assert np.array_equal(bird.cpu().numpy(), bev_image_ref.warp(small, m, 108, 208, True))
    assert np.array_equal(bird_mask.cpu().numpy(), bev_ref.warp(small_mask, m, 108, 208))
    assert bird.cpu().numpy().any() and bird_mask.cpu().numpy().any()


# ---- 5. bird_eye_view ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_backbone():
    """Two classes, the random weights the other deployment tests load."""
    import e2e_ref
    m = FastSCNN(2)
    m.load_state_dict(e2e_ref.weights(2))
    return m.to(DEV).eval()


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("frame", [(32, 64), (48, 80)], ids=["input_size", "80x48"])
def test_bird_eye_view(frame, channels_last):
    """Mask and rows bit-equal to bird_eye on the same frames; the image equals the yardstick; the
    segmented picture equals the yardstick blend of that image and mask."""
    h, w = frame
    e2e = EndToEndFastSCNN(small_backbone(), input_size=(64, 32), base_size=64,
                           channels_last=channels_last).eval()
    view = bev.BirdEyeView()
    vp = view.params(1, 0.1, True, source_size=(64, 32))[3]
    fvp = None if (w, h) == (64, 32) else view.params(1, 0.1, True, source_size=(w, h))[3]
    f = bev_image_ref.planted_frames(2, h, w, channels_last)
    frames = dev_frames(2, h, w, channels_last)
    want_mask, want_rows = e2e.bird_eye(frames, vp, scale=255, min_width=10)
    fused = e2e._last_fused
    want = bev_image_ref.warp(f, bev.inverse_map(fvp or vp), 108, 208, channels_last)
    img, mask, rows = e2e.bird_eye_view(frames, vp, frame_view_params=fvp)
    assert e2e._last_fused == fused
    assert torch.equal(mask, want_mask) and torch.equal(rows, want_rows)
    assert np.array_equal(img.cpu().numpy(), want) and want.any()
    color = (0, 200, 255)
    img2, mask2, rows2, seg = e2e.bird_eye_view(frames, vp, frame_view_params=fvp, segmented=True,
                                                alpha=0.3, color=color)
    assert torch.equal(img2, img) and torch.equal(mask2, want_mask) and torch.equal(rows2, want_rows)
    want_seg = bev_image_ref.blend(want, want_mask.cpu().numpy(), 0.3, color,
                                   channels_last=channels_last)
    assert np.array_equal(seg.cpu().numpy(), want_seg)
    print("%dx%d: lane share of the view %.3f, fused %s"
          % (w, h, float((want_mask != 0).float().mean()), fused))
    if fvp is not None:
        with pytest.raises(RuntimeError, match="source_size"):
            e2e.bird_eye_view(frames, vp)
    with pytest.raises(RuntimeError, match="uint8"):
        e2e.bird_eye_view(frames.float(), vp, frame_view_params=fvp)
