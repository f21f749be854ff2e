"""SyncTransform on the GPU (csrc/augment.hip) against the goldens recorded from the reference's
own ``_sync_transform`` / ``_val_sync_transform`` (tests/golden/sync_*.npz) and, where no golden
exists, the numpy restatement of PIL (tests/sync_transform_ref.py).  The contract is equality.
Neither PIL nor the reference is needed here."""
import functools
import os

import numpy as np
import pytest
import torch

import sync_transform_ref as R
from oracle import fast_scnn_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONFIGS = ("A", "B", "C")


@functools.lru_cache(maxsize=None)
def load(name):
    g = np.load(os.path.join(GOLDEN, "sync_%s.npz" % name))
    g = {k: g[k] for k in g.files}
    g["image_dev"] = torch.from_numpy(g["image"]).to(DEV)
    g["mask_dev"] = torch.from_numpy(g["mask"]).to(DEV)
    return g


def golden_params(g, i):
    p = [int(v) for v in g["params"][i]]
    b = float(g["blur"][i])
    return (bool(p[0]),) + tuple(p[1:]) + (b if b >= 0 else None,)


def normalized(u8):
    from fast_scnn_pytorch_amd.data import IMAGENET_MEAN, IMAGENET_STD
    return torch.stack([ref.to_tensor_normalize(v, IMAGENET_MEAN, IMAGENET_STD) for v in u8])


@pytest.mark.parametrize("name", CONFIGS)
def test_golden_cases_with_recorded_parameters(name):
    from fast_scnn_pytorch_amd.data import SyncTransform
    g = load(name)
    n = len(g["seeds"])
    params = [golden_params(g, i) for i in range(n)]
    imgs = g["image_dev"].unsqueeze(0).expand(n, -1, -1, -1)
    masks = g["mask_dev"].unsqueeze(0).expand(n, -1, -1)
    st = SyncTransform(int(g["base"]), int(g["crop"]))
    x, t, u8 = st(imgs, masks, params, return_u8=True)
    assert x.dtype == torch.float32 and t.dtype == torch.int64 and u8.dtype == torch.uint8
    got_u8 = u8.cpu().numpy()
    for i in range(n):
        assert np.array_equal(got_u8[i], g["crop_u8"][i]), (i, params[i])
    assert np.array_equal(t.cpu().numpy(), g["target"].astype(np.int64))
    want = normalized(g["crop_u8"])
    assert torch.equal(x.cpu(), want)
    sb = SyncTransform(int(g["base"]), int(g["crop"]), dtype=torch.bfloat16)
    xb, tb = sb(imgs, masks, params)
    assert xb.dtype == torch.bfloat16 and torch.equal(xb.cpu(), want.to(torch.bfloat16))
    assert torch.equal(tb, t)


@pytest.mark.parametrize("name", CONFIGS)
def test_golden_cases_through_the_sampler(name):
    """seed= and no explicit parameters: the sampler's draws reach the launch."""
    from fast_scnn_pytorch_amd.data import SyncTransform
    g = load(name)
    for i, s in enumerate(g["seeds"]):
        st = SyncTransform(int(g["base"]), int(g["crop"]), seed=int(s))
        _, t, u8 = st(g["image_dev"][None], g["mask_dev"][None], return_u8=True)
        assert np.array_equal(u8[0].cpu().numpy(), g["crop_u8"][i]), int(s)
        assert np.array_equal(t[0].cpu().numpy(), g["target"][i].astype(np.int64)), int(s)


def test_ragged_list_equals_each_alone():
    from fast_scnn_pytorch_amd.data import SyncTransform
    a, b = load("A"), load("B")
    assert int(a["crop"]) == int(b["crop"]) and a["mask"].shape != b["mask"].shape
    st = SyncTransform(int(a["base"]), int(a["crop"]))
    for ia, ib in ((0, 0), (5, 3), (17, 11)):
        pa, pb = golden_params(a, ia), golden_params(b, ib)
        x, t, u8 = st([a["image_dev"], b["image_dev"]], [a["mask_dev"], b["mask_dev"]], [pa, pb],
                      return_u8=True)
        xa, ta, ua = st([a["image_dev"]], [a["mask_dev"]], [pa], return_u8=True)
        xb, tb, ub = st([b["image_dev"]], [b["mask_dev"]], [pb], return_u8=True)
        assert torch.equal(x, torch.cat([xa, xb])) and torch.equal(t, torch.cat([ta, tb]))
        assert torch.equal(u8, torch.cat([ua, ub]))
        assert np.array_equal(u8[0].cpu().numpy(), a["crop_u8"][ia])
        assert np.array_equal(u8[1].cpu().numpy(), b["crop_u8"][ib])


@pytest.mark.parametrize("name", CONFIGS)
def test_val_path(name):
    from fast_scnn_pytorch_amd.data import SyncTransform
    g = load(name)
    st = SyncTransform(int(g["base"]), int(g["crop"]))
    x, t, u8 = st.val(g["image_dev"][None], g["mask_dev"][None], return_u8=True)
    assert np.array_equal(u8[0].cpu().numpy(), g["val_u8"])
    assert np.array_equal(t[0].cpu().numpy(), g["val_target"].astype(np.int64))
    assert torch.equal(x.cpu(), normalized(g["val_u8"][None]))


def test_tusimple_lookup_table():
    """tusimple.py's ``mask > 0 -> 1`` as a 256-entry table with offset 0."""
    from fast_scnn_pytorch_amd.data import SyncTransform
    g = load("C")
    crop = int(g["crop"])
    mask = (g["mask"].astype(np.int32) * 7 % 256).astype(np.uint8)  # ids beyond 33 as well
    assert mask.max() > 33 and (mask == 0).any()
    st = SyncTransform(int(g["base"]), crop, label_lut=(0,) + (1,) * 255, lut_offset=0)
    idx = (0, 3, 7, 12)
    params = [golden_params(g, i) for i in idx]
    md = torch.from_numpy(mask).to(DEV)
    _, t = st([g["image_dev"]] * len(idx), [md] * len(idx), params)
    for k, p in enumerate(params):
        _, m = R.crop_pair(g["image"], mask, p, crop)
        assert np.array_equal(t[k].cpu().numpy(), np.where(m > 0, 1, 0))


def test_full_size_extremes():
    """1024 x 2048 sources, base 1024, crop 768, hand-picked parameters at the extremes of what
    the sampler draws, against the restatement: exactly equal."""
    from fast_scnn_pytorch_amd.data import SyncTransform
    H, W, crop = 1024, 2048, 768
    rng = np.random.default_rng(21)
    yy, xx = np.mgrid[0:H, 0:W]
    srcs = []
    for k in range(2):
        img = np.stack([xx * (255.0 / (W - 1)), yy * (255.0 / (H - 1)),
                        (xx + yy) * (255.0 / (H + W - 2))], -1)
        img = np.clip(img + rng.normal(0, 24, img.shape), 0, 255).astype(np.uint8)
        mask = np.kron(rng.integers(0, 34, (H // 32, W // 32)).astype(np.uint8),
                       np.ones((32, 32), np.uint8))
        srcs.append((img, mask))
    cases = [
        # short 512: padded, flipped, blurred at the largest radius, x1 at its maximum (y1: 0 = max)
        (0, (True, 1024, 512, 0, 256, 256, 0, 0.999)),
        # short 2048: x1 = 0, y1 at its maximum
        (1, (False, 4096, 2048, 0, 0, 0, 1280, None)),
        # short 2048: flipped and blurred, x1 at its maximum, y1 = 0
        (0, (True, 4096, 2048, 0, 0, 3328, 0, 0.999)),
    ]
    dev = [(torch.from_numpy(i).to(DEV), torch.from_numpy(m).to(DEV)) for i, m in srcs]
    st = SyncTransform(1024, crop)
    x, t, u8 = st([dev[s][0] for s, _ in cases], [dev[s][1] for s, _ in cases],
                  [p for _, p in cases], return_u8=True)
    got_u8, got_t = u8.cpu().numpy(), t.cpu().numpy()
    for k, (s, p) in enumerate(cases):
        want_u8, want_t = R.transform(srcs[s][0], srcs[s][1], p, crop)
        assert np.array_equal(got_u8[k], want_u8), p
        assert np.array_equal(got_t[k], want_t), p
    assert torch.equal(x[0].cpu(), normalized(got_u8[:1])[0])


def test_output_feeds_the_model():
    from fast_scnn_pytorch_amd.data import SyncTransform
    from models.fast_scnn import FastSCNN
    g = load("C")
    m = FastSCNN(19).to(DEV).train()
    st = SyncTransform(128, 96, seed=3)
    imgs = g["image_dev"].unsqueeze(0).expand(2, -1, -1, -1)
    masks = g["mask_dev"].unsqueeze(0).expand(2, -1, -1)
    x, t = st(imgs, masks)
    assert x.shape == (2, 3, 96, 96) and t.shape == (2, 96, 96)
    assert int(t.min()) >= -1 and int(t.max()) <= 18
    loss = m.forward_loss(x, t)
    loss.backward()
    assert torch.isfinite(loss).all()
