"""The overlay tail on the GPU (csrc/overlay.hip, EndToEndFastSCNN.overlay, vis.overlay_mask)
against the numpy restatement of the law (tests/overlay_ref.py), bit for bit: no tolerances and no
excluded pixels.  The expected overlay is the law applied to this project's own
``e2e.predict(frames, scale)`` copied to the host, so near-tie labels cannot make a test flaky."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import e2e_ref
import overlay_ref
from e2e_ref import CLASSES, fixture, geometry
from fast_scnn_pytorch_amd import bev
from fast_scnn_pytorch_amd.deploy import EndToEndFastSCNN
from fast_scnn_pytorch_amd.vis import overlay_mask
from models.fast_scnn import FastSCNN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
DT_IDS = ["fp32", "fp16", "bf16"]
SAME_SIZE = ["200x70", "61x45", "128x128"]  # frames of the output's size; 200 = 3 tiles + 8


@functools.lru_cache(maxsize=None)
def backbone(nc):
    m = FastSCNN(nc)
    m.load_state_dict(e2e_ref.weights(nc))
    return m.to(DEV).eval()


def wrapper(case, nc, dtype=torch.float32, channels_last=False, input_size=None):
    size, base, mean, std = geometry(fixture(case, nc))
    m = EndToEndFastSCNN(backbone(nc), input_size=input_size or size, base_size=base, mean=mean,
                         std=std, dtype=dtype, channels_last=channels_last)
    m.preprocessor.to(DEV)
    return m.eval()


def frames_of(case, nc, batch=3, channels_last=False):
    f = fixture(case, nc)["frames"][:batch]
    assert f.dtype == torch.uint8
    if channels_last:
        f = f.permute(0, 2, 3, 1).contiguous()
    return f.to(DEV)


@functools.lru_cache(maxsize=None)
def palette19():
    return np.random.default_rng(19).integers(0, 256, (19, 3), dtype=np.uint8)


def host(t):
    return t.float().cpu().numpy() if t.is_floating_point() else t.cpu().numpy()


def check(e2e, frames, route=None, **kw):
    """One ``overlay`` call with ``return_mask`` against the law on ``e2e``'s own predict; returns
    ``(overlay, mask)``."""
    scale = kw.get("scale", 255)
    labels = e2e.predict(frames, scale).cpu().numpy()
    ids = e2e.predict(frames, 1).cpu().numpy() if kw.get("palette") is not None else None
    out, mask = e2e.overlay(frames, return_mask=True, **kw)
    if route is not None:
        assert e2e._last_fused is route
    ref = {k: v for k, v in kw.items() if k not in ("scale", "fused")}
    want, want_mask = overlay_ref.overlay(host(frames), labels, channels_last=e2e.channels_last,
                                          ids=ids, **ref)
    assert out.dtype == torch.uint8 and out.shape == frames.shape
    assert out.data_ptr() != frames.data_ptr()
    assert np.array_equal(mask.cpu().numpy(), want_mask)
    bad = int((out.cpu().numpy() != want).sum())
    assert bad == 0, "%d overlay bytes differ" % bad
    return out, mask


# ---- 1. the fused tail -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("nc", CLASSES)
@pytest.mark.parametrize("case", SAME_SIZE)
def test_fused_tail(case, nc, dtype):
    """Batch 1 and 3, both layouts; the default weights (the a + 127.5 ties), weights that are
    no dyadic fractions, and a negative gamma; the returned mask is predict's."""
    for cl in (False, True):
        e2e = wrapper(case, nc, dtype, cl)
        for batch in (1, 3):
            frames = frames_of(case, nc, batch, cl)
            out, mask = check(e2e, frames, True)
            assert torch.equal(mask, e2e.predict(frames, 255))
            assert torch.equal(e2e.overlay(frames), out) and e2e._last_fused is True
        check(e2e, frames, True, alpha=0.3, frame_weight=0.7, gamma=-20.0, color=(255, 0, 7),
              scale=1)
    print("%s C=%d %s: coloured share %.3f" % (case, nc, dtype, float((mask != 0).float().mean())))


# ---- 2. frames of another size than the output ---------------------------------------------------------------
@pytest.mark.parametrize("nc", CLASSES)
def test_larger_frames_take_two_launches(nc):
    """50 x 40 frames, 37 x 33 output: more frame pixels than mask pixels, so the default route is
    predict + fscnn_overlay_mask; the forced fused tail gives the same bits."""
    for cl in (False, True):
        e2e = wrapper("50x40_to_37x33", nc, channels_last=cl)
        frames = frames_of("50x40_to_37x33", nc, 3, cl)
        assert frames.shape[2 if cl else 3] == 50
        out, mask = check(e2e, frames, False)
        assert mask.shape == (3, 40, 50)
        fout, fmask = check(e2e, frames, True, fused=True)
        assert torch.equal(fout, out) and torch.equal(fmask, mask)
        check(e2e, frames, False, fused=False)


@pytest.mark.parametrize("nc", CLASSES)
def test_smaller_frames_take_the_fused_tail(nc):
    """61 x 45 frames, 80 x 48 output: the fused tail by default, the two-launch route on demand,
    equal bits."""
    for cl in (False, True):
        e2e = wrapper("61x45", nc, torch.float16, cl, input_size=(80, 48))
        frames = frames_of("61x45", nc, 3, cl)
        out, mask = check(e2e, frames, True)
        tout, tmask = check(e2e, frames, False, fused=False)
        assert torch.equal(tout, out) and torch.equal(tmask, mask)


# ---- 3. palette mode ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", CLASSES)
@pytest.mark.parametrize("case", ["200x70", "50x40_to_37x33"])
def test_palette_mode(case, nc):
    """A 19-row palette at 0.7 / 0.3 on both routes (the returned mask keeps its scale); with
    frame_weight 0 and alpha 1 the overlay is palette[argmax]; a 5-row palette leaves the classes
    from 5 on uncoloured."""
    pal = palette19()
    e2e = wrapper(case, nc)
    frames = frames_of(case, nc)
    outs = [check(e2e, frames, fused, fused=fused, palette=torch.from_numpy(pal),
                  frame_weight=0.7, alpha=0.3) for fused in (True, False)]
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    ids = overlay_ref.resize_nearest(e2e.predict(frames).cpu().numpy(), *frames.shape[2:])
    for fused in (True, False):
        pure = e2e.overlay(frames, palette=pal.tolist(), frame_weight=0.0, alpha=1.0, fused=fused)
        assert np.array_equal(pure.cpu().numpy(), pal[ids].transpose(0, 3, 1, 2))
        check(e2e, frames, fused, fused=fused, palette=pal[:5], scale=3)


# ---- 4. float frames ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", CLASSES)
def test_float_frames_match_uint8(nc):
    for cl in (False, True):
        e2e = wrapper("61x45", nc, channels_last=cl)
        frames = frames_of("61x45", nc, 3, cl)
        want = e2e.overlay(frames, alpha=0.3)
        for fdt in (torch.float32, torch.bfloat16, torch.float16):
            assert torch.equal(e2e.overlay(frames.to(fdt), alpha=0.3), want), fdt
            assert torch.equal(e2e.overlay(frames.to(fdt), alpha=0.3, fused=False), want), fdt


# ---- 5. overlay_mask alone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("size", [(5, 3), (67, 9), (130, 2)], ids=["5x3", "67x9", "130x2"])
def test_overlay_mask_alone(size, cl):
    """Random frames and masks, batch 3: rows at odd byte offsets (w = 5, 67), the ragged last
    group (67 = 16 x 4 + 3, 130 = 32 x 4 + 2); masks of the frame's size, larger and smaller; lane
    and palette mode; uint8 and fp16 frames; with and without the resized mask."""
    w, h = size
    rng = np.random.default_rng(w * 100 + h)
    f = rng.integers(0, 256, (3, h, w, 3) if cl else (3, 3, h, w), dtype=np.uint8)
    frames = torch.from_numpy(f).to(DEV)
    pal = palette19()
    for wm, hm in ((w, h), (2 * w + 3, 3 * h + 1), (max(w // 3, 1), max(h // 2, 1))):
        m = rng.integers(0, 24, (3, hm, wm), dtype=np.uint8)
        m[rng.random(m.shape) < 0.4] = 0
        mask = torch.from_numpy(m).to(DEV)
        for kw in (dict(), dict(alpha=0.3, frame_weight=0.7, gamma=2.5, color=(1, 2, 255)),
                   dict(palette=pal, alpha=0.4, frame_weight=0.6), dict(palette=pal[:1])):
            want, want_mask = overlay_ref.overlay(f, m, channels_last=cl, **kw)
            out, resized = overlay_mask(frames, mask, return_mask=True, channels_last=cl, **kw)
            assert np.array_equal(out.cpu().numpy(), want), (wm, hm, kw)
            assert np.array_equal(resized.cpu().numpy(), want_mask)
            assert torch.equal(overlay_mask(frames, mask, channels_last=cl, **kw), out)
            assert torch.equal(overlay_mask(frames.half(), mask, channels_last=cl, **kw), out)


def test_overlay_mask_edges_of_the_blend():
    """Half to even, saturation at both ends, the two pure weights -- on the device."""
    a = torch.arange(256, dtype=torch.uint8, device=DEV).view(1, 1, 2, 128).expand(1, 3, 2, 128)
    a = a.contiguous()
    ones = torch.ones((1, 2, 128), dtype=torch.uint8, device=DEV)
    an = a.cpu().numpy()
    for kw in (dict(alpha=0.5, color=(255, 255, 255)), dict(alpha=1.0, color=(200, 1, 0)),
               dict(alpha=0.5, gamma=-130.0, color=(5, 5, 5)), dict(alpha=0.0),
               dict(frame_weight=0.0, alpha=1.0, color=(3, 2, 1)),
               dict(alpha=0.5, gamma=float("nan")), dict(alpha=0.1, frame_weight=0.9, gamma=0.5)):
        want, _ = overlay_ref.overlay(an, ones.cpu().numpy(), **kw)
        assert np.array_equal(overlay_mask(a, ones, **kw).cpu().numpy(), want), kw
    got = overlay_mask(a, ones, alpha=0.5, color=(255, 255, 255))
    assert got[0, 0, 0, :4].tolist() == [128, 128, 130, 130]
    assert torch.equal(overlay_mask(a, ones, alpha=0.0), a)


# ---- 6. the unfused routes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", CLASSES)
def test_switch_takes_the_unfused_route(nc, monkeypatch):
    """FSCNN_E2E_FUSED=0: overlay reports the unfused route, forced or not, and equals the law on
    that route's own predict."""
    e2e = wrapper("200x70", nc)
    frames = frames_of("200x70", nc)
    monkeypatch.setenv("FSCNN_E2E_FUSED", "0")
    check(e2e, frames, False)
    check(e2e, frames, False, fused=True, palette=palette19(), alpha=0.3, frame_weight=0.7)
    e2e.predict(frames)
    assert e2e._last_fused is False


def test_more_than_32_classes_take_the_unfused_route():
    torch.manual_seed(0)
    bb = FastSCNN(40).to(DEV).eval()
    frames = frames_of("80x48", 2, 1)
    e2e = EndToEndFastSCNN(bb, input_size=(80, 48), base_size=64).to(DEV).eval()
    check(e2e, frames, False, scale=1)
    pal = np.random.default_rng(40).integers(0, 256, (40, 3), dtype=np.uint8)
    check(e2e, frames, False, palette=pal, fused=True)


# ---- 7. neighbours -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", CLASSES)
def test_neighbours_unchanged(nc):
    """e2e(frames), predict and bird_eye return after overlay calls what they returned before."""
    bb = backbone(nc)
    e2e = wrapper("200x70", nc)
    frames = frames_of("200x70", nc)
    vp = bev.BirdEyeView().params(1, 0.1, True, source_size=(200, 70))[3]
    p0, l0 = e2e(frames).clone(), e2e.predict(frames, scale=255).clone()
    b0 = [t.clone() for t in e2e.bird_eye(frames, vp)]
    sd0 = {k: v.clone() for k, v in bb.state_dict().items()}
    keep = frames.clone()
    first = e2e.overlay(frames)
    e2e.overlay(frames, palette=palette19(), return_mask=True, fused=False)
    wrapper("200x70", nc, torch.float16).overlay(frames, scale=1)
    assert torch.equal(frames, keep)
    assert torch.equal(e2e(frames), p0) and torch.equal(e2e.predict(frames, scale=255), l0)
    b1 = e2e.bird_eye(frames, vp)
    assert torch.equal(b1[0], b0[0]) and torch.equal(b1[1], b0[1])
    assert torch.equal(e2e.overlay(frames), first)
    for k, v in bb.state_dict().items():
        assert torch.equal(v, sd0[k]), k


# ---- 8. errors ---------------------------------------------------------------------------------------------------
def test_gpu_guards():
    e2e = wrapper("80x48", 2)
    frames = frames_of("80x48", 2)
    mask = e2e.predict(frames, 255)
    with pytest.raises(RuntimeError, match="device"):
        e2e.overlay(frames.cpu())
    with pytest.raises(RuntimeError, match="device"):
        overlay_mask(frames, mask.cpu())
    with pytest.raises(RuntimeError, match="uint8 / fp32"):
        overlay_mask(frames.to(torch.int32), mask)
    with pytest.raises(RuntimeError, match="uint8 mask"):
        overlay_mask(frames, mask.float())
    with pytest.raises(RuntimeError, match="3 frames"):
        overlay_mask(frames, mask[:2])
    with pytest.raises(RuntimeError, match="expected frames"):
        overlay_mask(frames, mask, channels_last=True)
    with pytest.raises(RuntimeError, match="palette"):
        e2e.overlay(frames, palette=np.zeros((257, 3), dtype=np.uint8))
    with pytest.raises(RuntimeError, match="palette"):
        overlay_mask(frames, mask, palette=[])
    e2e.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            e2e.overlay(frames)
    finally:
        e2e.eval()  # the backbone is shared between the tests
    assert e2e.overlay(frames).shape == frames.shape


def test_c_abi_refusals():
    """-1 for aliased or null buffers and bad sizes, -2 before any launch for more than 32 classes
    and for a window that does not fit in LDS; nothing is written."""
    from fast_scnn_pytorch_amd import _lib
    lib = _lib.load()
    st = _lib.stream_ptr(torch.device(DEV))
    frames = torch.full((1, 3, 4, 8), 9, dtype=torch.uint8, device=DEV)
    mask = torch.ones((1, 4, 8), dtype=torch.uint8, device=DEV)
    out = torch.full((1, 3, 4, 8), 77, dtype=torch.uint8, device=DEV)
    green = (ctypes.c_ubyte * 3)(0, 255, 0)

    def by_mask(f=frames, o=out, h=4, w=8, pal=None, rows=0, hm=4, color=green):
        return lib.fscnn_overlay_mask(_lib.ptr(f), 3, 0, 1, h, w, _lib.ptr(mask), hm, 8, color,
                                      _lib.ptr(pal), rows, 1.0, 0.5, 0.0, _lib.ptr(o), None, st)
    assert by_mask(o=frames) == -1 and b"alias" in lib.fscnn_last_error()
    assert by_mask(o=None) == -1 and by_mask(f=None) == -1 and by_mask(h=1) == -1
    assert by_mask(color=None) == -1 and by_mask(hm=0) == -1
    assert by_mask(pal=mask, rows=0) == -1 and by_mask(pal=mask, rows=257) == -1
    assert by_mask(h=16385) == -2
    # 64 x 64 x 19 fp32 logits behind a 4 x 8 frame: the one tile's window is the whole grid
    logits = torch.zeros((1, 64, 64, 19), dtype=torch.float32, device=DEV)
    table = (ctypes.c_ubyte * 96)()

    def by_logits(c=19, ldx=19, o=out):
        return lib.fscnn_e2e_overlay(_lib.ptr(logits), 0, 1, 64, 64, c, ldx, 512, 360, 640, 255,
                                     _lib.ptr(frames), 3, 0, 4, 8, table, 2, 1.0, 0.5, 0.0,
                                     _lib.ptr(o), None, st)
    assert by_logits() == -2 and b"geometry" in lib.fscnn_last_error()
    assert by_logits(c=33, ldx=33) == -2
    assert by_logits(o=frames) == -1
    torch.cuda.synchronize()
    assert bool((out == 77).all()) and bool((frames == 9).all())  # nothing was launched
    assert by_mask() == 0
    torch.cuda.synchronize()
    assert out[0, :, 0, 0].tolist() == [9, 136, 9]
