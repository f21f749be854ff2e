"""CPU-side checks of the colour bird's-eye view: the self-checks of the GPU tests' numpy yardstick
(tests/bev_image_ref.py), the yardstick's law against a run the reference recorded itself
(tests/golden/bev_image_recorded_run.npz, tools/gen_bev_image_golden.py), and the interface guards
of ``bev.warp_image``, ``BirdEyeView.transform_image_and_mask`` and
``EndToEndFastSCNN.bird_eye_view`` on host tensors."""
import io

import numpy as np
import pytest
import torch

import bev_image_ref
import helpers
from fast_scnn_pytorch_amd import BirdEyeView, bev, warp_image
from fast_scnn_pytorch_amd.deploy import EndToEndFastSCNN
from models.fast_scnn import FastSCNN


# ---- the yardstick's self-checks --------------------------------------------------------------------------
@pytest.mark.parametrize("channels_last", [False, True])
def test_identity_returns_the_frame(channels_last):
    f = bev_image_ref.planted_frames(2, 29, 37, channels_last)
    info = {}
    out = bev_image_ref.warp(f, np.eye(3).ravel(), 29, 37, channels_last, info=info)
    assert np.array_equal(out, f)
    assert info == {"w_zero": 0, "clamped": 0, "inside": 29 * 37}
    big = bev_image_ref.warp(f, np.eye(3).ravel(), 33, 40, channels_last)
    big = big if channels_last else big.transpose(0, 2, 3, 1)
    ff = f if channels_last else f.transpose(0, 2, 3, 1)
    assert np.array_equal(big[:, :29, :37], ff) and not big[:, 29:].any() and not big[:, :, 37:].any()


@pytest.mark.parametrize("k", [1, 16, 31, -17])
def test_translation_by_k_32nds_gives_the_hand_computed_weights(k):
    """Source = (x + k / 32, y): the weights are (32 - a) * 32 and a * 32 of 1024 with
    a = k mod 32, on the taps floor(x + k / 32) and the next one; a tap outside the row is 0."""
    row = np.array([10, 200, 0, 255, 37, 91, 255, 3], dtype=np.int64)
    f = np.repeat(row[None, None, None, :], 3, axis=1).astype(np.uint8)  # [1, 3, 1, 8]
    f = np.concatenate([f, f], axis=2)                                  # two equal rows: h = 2
    m = np.array([1, 0, k / 32, 0, 1, 0, 0, 0, 1], dtype=np.float64)
    out = bev_image_ref.warp(f, m, 1, 8)
    a, s = k % 32, k // 32
    padded = np.concatenate([[0], row, [0]])  # index i + 1 holds tap i, border 0
    want = [((32 - a) * 32 * padded[x + s + 1] + a * 32 * padded[x + s + 2] + 512) >> 10
            for x in range(8)]
    assert out[0, 0, 0].tolist() == want and np.array_equal(out[0, 1], out[0, 0])
    if k == 16:  # halves: (p0 + p1 + 1) >> 1, the last pixel mixes with the border
        assert want == [(int(padded[x + 1]) + int(padded[x + 2]) + 1) >> 1 for x in range(8)]
        assert want[7] == 2
    if k == -17:  # the first pixel mixes the border (weight 17 / 32) with row[0]
        assert want[0] == (15 * 32 * 10 + 512) >> 10


def test_vertical_fraction_and_product_weights():
    f = np.zeros((1, 3, 2, 2), dtype=np.uint8)
    f[0, :, 0, 0], f[0, :, 0, 1], f[0, :, 1, 0], f[0, :, 1, 1] = 255, 0, 0, 255
    m = np.array([1, 0, 8 / 32, 0, 1, 24 / 32, 0, 0, 1], dtype=np.float64)  # ax = 8, ay = 24
    out = bev_image_ref.warp(f, m, 1, 1)
    assert out[0, :, 0, 0].tolist() == [(24 * 8 * 255 + 8 * 24 * 255 + 512) >> 10] * 3


def test_a_view_wholly_outside_the_frame_is_zero():
    f = bev_image_ref.planted_frames(1, 29, 37) | np.uint8(1)
    info = {}
    for m in ([1, 0, 1e6, 0, 1, 0, 0, 0, 1], [1, 0, -2, 0, 1, 0, 0, 0, 1], [1, 0, 0, 0, 1, 29, 0, 0, 1]):
        out = bev_image_ref.warp(f, np.array(m, dtype=np.float64), 5, 2, info=info)
        assert not out.any() and info["inside"] == 0
    white = np.full((1, 3, 29, 37), 255, dtype=np.uint8)
    edge = bev_image_ref.warp(white, np.array([1, 0, -1 + 1 / 32, 0, 1, 0, 0, 0, 1.0]), 5, 1, info=info)
    assert info["inside"] == 5 and (edge == (32 * 255 + 512) >> 10).all()  # 1 / 32 of column 0: 8


def test_w_zero_and_the_clamp_are_reported():
    m = np.array([10, 1, -30, 0, 2.0 ** 27, 0, 1, 0, -5], dtype=np.float64)
    fx, fy, info = bev_image_ref.fixed_index(m, 4, 12)
    assert info["w_zero"] == 4 and info["clamped"] > 0
    assert (fx[:, 5] == 0).all() and (fy[:, 5] == 0).all()  # W == 0 -> the source is (0, 0)
    assert fy[1, 6] == 2 ** 31 - 1 and fy[1, 4] == -2 ** 31


def test_blend_is_the_overlay_law():
    img = np.array([[[[0, 100, 255]], [[1, 2, 3]], [[255, 255, 255]]]], dtype=np.uint8)  # [1, 3, 1, 3]
    mask = np.array([[[0, 255, 7]]], dtype=np.uint8)
    out = bev_image_ref.blend(img, mask, alpha=0.5, color=(0, 255, 9))
    assert out[0, :, 0, 0].tolist() == [0, 1, 255]          # mask 0: the image
    assert out[0, :, 0, 1].tolist() == [100, 130, 255]      # 2 + 127.5 -> 129.5 -> 130 (even)
    assert out[0, :, 0, 2].tolist() == [255, 130, 255]      # mask 7 counts; 130.5 -> 130 (even)


# ---- the recorded run ---------------------------------------------------------------------------------------
def recorded_view():
    return BirdEyeView().params(pixels_per_unit=1, margin_ratio=0.1, full_image=True)


def _jpeg_round_trip(arr, Image):
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="JPEG", quality=95)
    return np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))


def test_the_law_reproduces_the_recorded_bird_eye_picture():
    """The reference's own input frame warped by the yardstick, written as a JPEG of quality 95
    (cv2.imwrite's default) and read back, against the picture the reference wrote: at most 1 % of
    the 67,392 bytes differ.  Measured with PIL 12.2.0: 141 bytes (0.21 %, largest difference 3)
    for this law; 10,654 with 6 fraction bits, 13,994 with 4, 17,753 with 3, 10,796 with 8 and
    24,084 for the nearest neighbour -- so the cap passes only this law."""
    Image = pytest.importorskip("PIL.Image")
    g = helpers.load_golden("bev_image_recorded_run")
    src = np.asarray(Image.open(io.BytesIO(g["source_jpeg"].tobytes())).convert("RGB"))
    rec = np.asarray(Image.open(io.BytesIO(g["bird_eye_jpeg"].tobytes())).convert("RGB"))
    assert src.shape == (360, 640, 3) and rec.shape == (108, 208, 3) and rec.size == 67392
    size, _, _, vp = recorded_view()
    assert size == (208, 108)
    m = bev.inverse_map(vp)
    got = _jpeg_round_trip(bev_image_ref.warp(src[None], m, 108, 208, channels_last=True)[0], Image)
    diff = np.abs(got.astype(np.int64) - rec.astype(np.int64))
    count = int((diff != 0).sum())
    print("bytes that differ from the recorded picture: %d of %d (%.2f %%), largest difference %d"
          % (count, rec.size, 100.0 * count / rec.size, int(diff.max())))
    for bits in (6, 4, 3, 8):
        other = _jpeg_round_trip(bev_image_ref.warp(src[None], m, 108, 208, True, bits=bits)[0], Image)
        print("  %d fraction bits: %d" % (bits, int((other != rec).sum())))
    near = _jpeg_round_trip(bev_image_ref.nearest(src[None], m, 108, 208, True)[0], Image)
    print("  nearest neighbour: %d" % int((near != rec).sum()))
    assert count <= rec.size // 100


# ---- interface guards ------------------------------------------------------------------------------------------
def test_warp_image_guards():
    eye = np.eye(3)
    u8 = torch.zeros(1, 3, 8, 8, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="uint8"):
        warp_image(u8.float(), eye, (4, 4))
    with pytest.raises(RuntimeError, match="4-d"):
        warp_image(u8[0], eye, (4, 4))
    with pytest.raises(RuntimeError, match="expected frames"):
        warp_image(torch.zeros(1, 4, 8, 8, dtype=torch.uint8), eye, (4, 4))
    with pytest.raises(RuntimeError, match="expected frames"):
        warp_image(u8, eye, (4, 4), channels_last=True)
    for size in ((8193, 4), (4, 65536), (0, 4), (4, 0)):
        with pytest.raises(RuntimeError, match="8192"):
            warp_image(u8, eye, size)
    with pytest.raises(RuntimeError, match="device"):  # host tensors: there is no fallback
        warp_image(u8, eye, (4, 4))
    with pytest.raises(RuntimeError, match="device"):  # the layout is read off the shape
        warp_image(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), eye, (4, 4))


def test_transform_image_and_mask_guards():
    v = BirdEyeView()
    img = torch.zeros(360, 640, 3, dtype=torch.uint8)
    mask = torch.zeros(360, 640, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="uint8"):
        v.transform_image_and_mask(img.float(), mask, 1)
    with pytest.raises(RuntimeError, match="uint8"):
        v.transform_image_and_mask(img, mask.float(), 1)
    with pytest.raises(RuntimeError, match=r"\[H, W, 3\]"):
        v.transform_image_and_mask(img[0], mask, 1)                 # rank 2
    with pytest.raises(RuntimeError, match=r"\[H, W, 3\]"):
        v.transform_image_and_mask(img.permute(2, 0, 1), mask, 1)   # channels first
    with pytest.raises(RuntimeError, match=r"\[H, W, 3\]"):
        v.transform_image_and_mask(img[None], mask, 1)              # a batch with a single mask
    with pytest.raises(RuntimeError, match="does not match"):
        v.transform_image_and_mask(img, mask[:180], 1)
    with pytest.raises(RuntimeError, match="8192"):
        v.transform_image_and_mask(img, mask, 40)                   # 8346 x 4337
    with pytest.raises(RuntimeError, match="tensors"):
        v.transform_image_and_mask(img.numpy(), mask.numpy(), 1)
    with pytest.raises(RuntimeError, match="device"):               # host tensors: no fallback
        v.transform_image_and_mask(img, mask, 1)
    with pytest.raises(RuntimeError, match="device"):
        v.transform_image_and_mask(img[None, :180, :320], mask[None, :180, :320], 1)


def test_bird_eye_view_guards():
    m = EndToEndFastSCNN(FastSCNN(2), input_size=(48, 32), base_size=64).eval()
    frames = torch.zeros(1, 3, 32, 48, dtype=torch.uint8)
    view = BirdEyeView()
    vp = view.params(1, 0.1, True, source_size=(48, 32))[3]
    with pytest.raises(RuntimeError, match="uint8"):
        m.bird_eye_view(frames.float(), vp)
    with pytest.raises(RuntimeError, match="4-d"):
        m.bird_eye_view(frames[0], vp)
    big = torch.zeros(1, 3, 48, 80, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match=r"source_size=\(80, 48\)"):   # names the call to make
        m.bird_eye_view(big, vp)
    other = view.params(2, 0.1, True, source_size=(80, 48))[3]
    with pytest.raises(RuntimeError, match="output_size"):
        m.bird_eye_view(big, vp, frame_view_params=other)
    for size in ((8193, 10), (10, 65536), (0, 10)):
        with pytest.raises(RuntimeError, match="8192"):
            m.bird_eye_view(frames, dict(vp, output_size=size))
    with pytest.raises(RuntimeError, match="min_width"):
        m.bird_eye_view(frames, vp, min_width=0)
    with pytest.raises(RuntimeError, match="device"):  # host tensors: there is no fallback
        m.bird_eye_view(frames, vp)
    with pytest.raises(RuntimeError, match="device"):
        m.bird_eye_view(big, vp, frame_view_params=view.params(1, 0.1, True, source_size=(80, 48))[3])
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        m.bird_eye_view(frames, vp)
