"""Host side of the GPU augmentation (SyncTransform, fscnn_sync_tables, fscnn_sync_blur_weights)
against the goldens recorded from the reference's own ``_sync_transform`` /
``_val_sync_transform`` (tools/gen_sync_golden.py) and the numpy restatement of PIL
(tests/sync_transform_ref.py).  Needs the built library, no GPU.  Everything is exact."""
import ctypes
import os

import numpy as np
import pytest

import sync_transform_ref as R
from fast_scnn_pytorch_amd import _lib
from fast_scnn_pytorch_amd.data import SyncParams, SyncTransform

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONFIGS = ("A", "B", "C")
E_INVALID = -1


def load(name):
    g = np.load(os.path.join(GOLDEN, "sync_%s.npz" % name))
    return {k: g[k] for k in g.files}


def golden_params(g, i):
    p = [int(v) for v in g["params"][i]]
    b = float(g["blur"][i])
    return (bool(p[0]),) + tuple(p[1:]) + (b if b >= 0 else None,)


def lib_tables(insize, outsize, start, count):
    lib = _lib.load()
    ks = ctypes.c_int()
    _lib.check(lib.fscnn_sync_tables(insize, outsize, 0, 1, 0, None, None, None, ctypes.byref(ks)))
    k = ks.value
    bounds = np.zeros((count, 2), np.int32)
    coef = np.full((count, k), -7, np.int32)
    near = np.zeros(count, np.int32)
    _lib.check(lib.fscnn_sync_tables(insize, outsize, start, count, k, bounds.ctypes.data,
                                     coef.ctypes.data, near.ctypes.data, None))
    return bounds[:, 0].copy(), bounds[:, 1].copy(), coef, near


@pytest.mark.parametrize("name", CONFIGS)
def test_sampler_matches_recorded_draws(name):
    g = load(name)
    H, W = g["mask"].shape
    for i, s in enumerate(g["seeds"]):
        st = SyncTransform(int(g["base"]), int(g["crop"]), seed=int(s))
        assert tuple(st.sample(W, H)) == golden_params(g, i), int(s)
    # val: the resize size and crop origin the reference's _val_sync_transform used
    vp = SyncTransform(int(g["base"]), int(g["crop"])).val_params(W, H)
    assert (vp.ow, vp.oh, vp.x1, vp.y1) == tuple(int(v) for v in g["val_params"])
    assert tuple(vp) == R.val_params(W, H, int(g["crop"]))
    assert vp.blur is None and not vp.flip and vp.padw == 0 and vp.padh == 0


@pytest.mark.parametrize("name", CONFIGS)
def test_restatement_reproduces_goldens(name):
    g = load(name)
    crop = int(g["crop"])
    for i in range(len(g["seeds"])):
        u8, t = R.transform(g["image"], g["mask"], golden_params(g, i), crop)
        assert np.array_equal(u8, g["crop_u8"][i]), i
        assert np.array_equal(t, g["target"][i]), i
    H, W = g["mask"].shape
    u8, t = R.transform(g["image"], g["mask"], R.val_params(W, H, crop), crop)
    assert np.array_equal(u8, g["val_u8"]) and np.array_equal(t, g["val_target"])


@pytest.mark.parametrize("name", CONFIGS)
def test_library_tables_reproduce_unblurred_goldens(name):
    g = load(name)
    crop = int(g["crop"])
    img, mask = g["image"], g["mask"]
    H, W = mask.shape
    cases = [(golden_params(g, i), g["crop_u8"][i], g["target"][i])
             for i in range(len(g["seeds"])) if g["blur"][i] < 0]
    cases.append((R.val_params(W, H, crop), g["val_u8"], g["val_target"]))
    assert len(cases) >= 5
    for p, want_u8, want_t in cases:
        flip, ow, oh, padw, padh, x1, y1, _ = p
        src, m = (img[:, ::-1], mask[:, ::-1]) if flip else (img, mask)
        xmin, xcnt, xk, nx = lib_tables(W, ow, x1, crop)
        ymin, ycnt, yk, ny = lib_tables(H, oh, y1, crop)
        # identical to the restatement's tables ...
        rx, ry = R.bilinear_tables(W, ow, x1, crop), R.bilinear_tables(H, oh, y1, crop)
        for got, want in zip((xmin, xcnt, xk, ymin, ycnt, yk), rx + ry):
            assert np.array_equal(got, want)
        assert np.array_equal(nx, R.nearest_table(W, ow, x1, crop))
        assert np.array_equal(ny, R.nearest_table(H, oh, y1, crop))
        # ... and, applied in numpy, to the reference's pixels
        r1 = int((ymin + ycnt).max())
        r0 = min(int(ymin.min()), r1)
        hor = R._resample_axis(src[r0:r1], xmin, xcnt, xk)
        ver = R._resample_axis(hor.transpose(1, 0, 2), ymin - r0, ycnt, yk).transpose(1, 0, 2)
        assert np.array_equal(ver, want_u8)
        ids = m[np.maximum(ny, 0)][:, np.maximum(nx, 0)].astype(np.int64)
        ids[ny < 0, :] = 0
        ids[:, nx < 0] = 0
        assert np.array_equal(R.CITYSCAPES_KEY[ids + 1], want_t)


def test_blur_weights_match_restatement():
    lib = _lib.load()
    ww, fw = ctypes.c_uint(), ctypes.c_uint()
    radii = np.random.default_rng(5).random(998).tolist() + [
        0.0, float(np.nextafter(np.float32(1), np.float32(0)))]
    for r in radii:
        _lib.check(lib.fscnn_sync_blur_weights(r, ctypes.byref(ww), ctypes.byref(fw)))
        want = R.blur_consts(r)
        assert (ww.value, fw.value) == want[:2], r
        assert ww.value + 2 * fw.value <= 1 << 24


def test_unsupported_parameters_are_invalid():
    lib = _lib.load()
    ww, fw = ctypes.c_uint(), ctypes.c_uint()
    for r in (1.0, 1.5, 7.0, -0.1, float("nan")):
        assert lib.fscnn_sync_blur_weights(r, ctypes.byref(ww), ctypes.byref(fw)) == E_INVALID
    ks = ctypes.c_int()
    assert lib.fscnn_sync_tables(1024, 128, 0, 1, 0, None, None, None, ctypes.byref(ks)) == 0
    assert ks.value == 17
    assert lib.fscnn_sync_tables(1025, 128, 0, 1, 0, None, None, None,
                                 ctypes.byref(ks)) == E_INVALID
    assert b"shrinks" in lib.fscnn_last_error()
    # a coefficient row shorter than the resize needs
    b, c, n = (np.zeros(8, np.int32) for _ in range(3))
    assert lib.fscnn_sync_tables(64, 16, 0, 2, 3, b.ctypes.data, c.ctypes.data, n.ctypes.data,
                                 None) == E_INVALID


def test_cpu_tensors_raise():
    import torch
    st = SyncTransform(64, 48, seed=0)
    with pytest.raises(RuntimeError):
        st(torch.zeros(1, 96, 192, 3, dtype=torch.uint8), torch.zeros(1, 96, 192, dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        st.val([torch.zeros(96, 192, 3, dtype=torch.uint8)], [torch.zeros(96, 192, dtype=torch.uint8)])
    assert SyncParams(*R.val_params(192, 96, 48)).blur is None
