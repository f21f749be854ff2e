"""The deployment pipeline on the GPU (EndToEndFastSCNN, csrc/e2e.hip): the whole pipeline
against the reference wrapper's fixtures, each of the two kernels against an fp64 evaluation with
torch's own fp32 error as the yardstick, the labels, the unfused route and the neighbours.

Yardsticks are evaluated on the CPU (torch's fp32 ops on the same data); bounds follow the
precision of the formats: a multiple of the yardstick's own distance from fp64 plus half a unit in
the last place of the output dtype at the value's magnitude."""
import functools

import pytest
import torch

import e2e_ref
from e2e_ref import CASES, CLASSES, fixture, geometry, half_ulp, pre_ref, tail_ref
from fast_scnn_pytorch_amd.deploy import EndToEndFastSCNN
from models.fast_scnn import FastSCNN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
DT_IDS = ["fp32", "fp16", "bf16"]


@functools.lru_cache(maxsize=None)
def backbone(nc):
    m = FastSCNN(nc)
    m.load_state_dict(e2e_ref.weights(nc))
    return m.to(DEV).eval()


def wrapper(case, nc, dtype=torch.float32, **kw):
    size, base, mean, std = geometry(fixture(case, nc))
    kw.setdefault("input_size", size)
    m = EndToEndFastSCNN(backbone(nc), base_size=base, mean=mean, std=std, dtype=dtype, **kw)
    m.preprocessor.to(DEV)  # (the shared backbone is on the device already)
    return m.eval()


def frames_of(case, nc, batch=3):
    return fixture(case, nc)["frames"][:batch].to(DEV)


# ---- 1. whole pipeline against the reference ------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("nc", CLASSES)
@pytest.mark.parametrize("case", CASES)
def test_pipeline_matches_reference_fp32(case, nc, batch):
    """fp32 probabilities within 1e-4 of the reference wrapper's: the project's fp32 eval budget
    on logits (test_gpu_model.py) carries over, both resamplings being convex combinations and
    softmax not enlarging a max-norm error."""
    g = fixture(case, nc)
    e2e = wrapper(case, nc)
    out = e2e(frames_of(case, nc, batch))
    size = geometry(g)[0]
    assert out.shape == (batch, nc, size[1], size[0]) and out.dtype == torch.float32
    assert e2e._last_fused is True
    got = out.cpu().numpy().ravel()
    if "probs_idx" in g:
        idx = g["probs_idx"][g["probs_idx"] < got.size]
        want = g["probs"][:idx.size]
        got = got[idx]
    else:
        want = g["probs"][:batch].ravel()
    err = abs(got - want).max()
    print("%s C=%d N=%d: max |p - reference| %.2e" % (case, nc, batch, err))
    assert err <= 1e-4


# ---- 2. front end ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pre_refs(case):
    g = fixture(case, 2)
    _, base, mean, std = geometry(g)
    r64 = pre_ref(g["frames"], base, mean, std, torch.float64)
    yard = (pre_ref(g["frames"], base, mean, std, torch.float32).double() - r64).abs().max().item()
    return r64, yard


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", CASES)
def test_front_end_against_fp64(case, dtype):
    """e2e_pre on the stored frames, uint8 and float input, against the formula in fp64.  Bound:
    2 x the max error of torch's fp32 F.interpolate -> / 255 -> normalise on the same frames (the
    kernel is free to order the lerp and fold the constants differently) + half an ulp of the
    output dtype.  An NHWC + BGR uint8 frame gives the bit-identical tensor to the same pixels fed
    as NCHW RGB float."""
    r64, yard = pre_refs(case)
    frames = frames_of(case, 2)
    e2e = wrapper(case, 2, dtype)
    bound = 2.0 * yard + half_ulp(r64, dtype)
    outs = {}
    for name, fr in (("uint8", frames), ("fp32", frames.float()), ("fp16", frames.half()),
                     ("bf16", frames.bfloat16())):
        x = e2e.preprocess(fr)
        assert x.dtype == dtype and x.shape == r64.shape and x.is_contiguous()
        outs[name] = x
        err = (x.double().cpu() - r64).abs()
        print("%s -> %s, %s frames: max err %.2e (yardstick %.2e), worst err / bound %.3f"
              % (case, dtype, name, err.max(), yard, (err / bound).max()))
        assert bool((err <= bound).all())
    for name in ("fp32", "fp16", "bf16"):
        assert torch.equal(outs[name], outs["uint8"]), name
    cam = wrapper(case, 2, dtype, channels_last=True, bgr=True)
    nhwc_bgr = frames.flip(1).permute(0, 2, 3, 1).contiguous()
    assert torch.equal(cam.preprocess(nhwc_bgr), outs["fp32"])
    # the flags one at a time
    assert torch.equal(wrapper(case, 2, dtype, bgr=True).preprocess(frames.flip(1)), outs["fp32"])
    assert torch.equal(wrapper(case, 2, dtype, channels_last=True).preprocess(
        frames.permute(0, 2, 3, 1).contiguous().float()), outs["fp32"])


# ---- 3 / 5. tail ------------------------------------------------------------------------------------
def tail_case(case, nc, dtype, softmax):
    """(fused output, fp64 reference, bound) of the tail on this implementation's own logits."""
    frames = frames_of(case, nc)
    e2e = wrapper(case, nc, dtype, apply_softmax=softmax)
    size = geometry(fixture(case, nc))[0]
    x = e2e.preprocess(frames)
    with torch.no_grad():
        logits = backbone(nc)(x)[0]
    assert logits.dtype == dtype
    lg = logits.cpu()
    r64 = tail_ref(lg.double(), size, softmax)
    yard = (tail_ref(lg.float(), size, softmax).double() - r64).abs().max().item()
    out = e2e(frames)
    assert out.dtype == dtype and out.shape == r64.shape and e2e._last_fused is True
    return out, r64, 4.0 * yard + half_ulp(r64, dtype), yard


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("nc", CLASSES)
@pytest.mark.parametrize("case", CASES)
def test_tail_against_fp64(case, nc, dtype):
    """Reference: backbone(x)[0].double() -> F.interpolate(align_corners=False) -> softmax with x
    the front end's output.  Bound: 4 x the error of torch's fp32 evaluation of the same two ops on
    those logits (the kernel may not reproduce the x8 upsample's rounding order bit for bit in fp32
    and has its own exponential) + half an output ulp."""
    out, r64, bound, yard = tail_case(case, nc, dtype, True)
    err = (out.double().cpu() - r64).abs()
    print("%s C=%d %s: max err %.2e (yardstick %.2e), worst err / bound %.3f"
          % (case, nc, dtype, err.max(), yard, (err / bound).max()))
    assert bool((err <= bound).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("nc", CLASSES)
@pytest.mark.parametrize("case", ["200x70", "50x40_to_37x33", "128x128"])
def test_apply_softmax_false_returns_resampled_logits(case, nc, dtype):
    out, r64, bound, yard = tail_case(case, nc, dtype, False)
    err = (out.double().cpu() - r64).abs()
    print("%s C=%d %s logits: max err %.2e (yardstick %.2e), worst err / bound %.3f"
          % (case, nc, dtype, err.max(), yard, (err / bound).max()))
    assert bool((err <= bound).all())
    assert float(out.float().sum(1).sub(1).abs().max()) > 1e-3  # not probabilities


# ---- 4. labels --------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", CLASSES)
@pytest.mark.parametrize("case", CASES)
def test_predict_labels(case, nc):
    g = fixture(case, nc)
    frames = frames_of(case, nc)
    e2e = wrapper(case, nc)
    lab = e2e.predict(frames)
    size = geometry(g)[0]
    assert lab.dtype == torch.uint8 and lab.shape == (3, size[1], size[0])
    assert e2e._last_fused is True
    sure = torch.from_numpy(g["margin"] > 1e-4)
    excluded = 1.0 - sure.float().mean().item()
    wrong = int((lab.cpu() != torch.from_numpy(g["argmax"]))[sure].sum())
    print("%s C=%d: %d wrong labels at margin > 1e-4, %.3f %% excluded"
          % (case, nc, wrong, 100 * excluded))
    assert wrong == 0
    assert excluded <= 0.01
    # scale: the lane mask is labels * 255 as uint8 (wrapping like numpy's astype)
    mask = e2e.predict(frames, scale=255)
    assert torch.equal(mask, (lab.to(torch.int64) * 255).to(torch.uint8))
    assert torch.equal(e2e.predict(frames[:1]), lab[:1])
    # predict is the argmax of forward wherever the two largest probabilities differ
    p = e2e(frames)
    top = torch.sort(p, dim=1).values
    clear = top[:, -1] > top[:, -2]
    assert torch.equal(lab[clear], p.argmax(1).to(torch.uint8)[clear])
    assert float(clear.float().mean()) > 0.99


@pytest.mark.parametrize("nc", CLASSES)
def test_predict_identity_case_equals_backbone_predict(nc):
    """128x128 frames, base 128, output 128x128: every resampling is the identity, so the labels
    are exactly those of the backbone's own fused upsample + argmax on the front end's output."""
    frames = frames_of("128x128", nc)
    for dtype in DTYPES:
        e2e = wrapper("128x128", nc, dtype)
        want = backbone(nc).predict(e2e.preprocess(frames), dtype=torch.uint8)
        assert torch.equal(e2e.predict(frames), want), dtype
        assert torch.equal(e2e.predict(frames, scale=7), want * 7), dtype


# ---- 6. the unfused route ---------------------------------------------------------------------------
@pytest.mark.parametrize("nc", CLASSES)
@pytest.mark.parametrize("case", ["200x70", "61x45", "50x40_to_37x33"])
def test_forced_unfused_route_agrees(case, nc, monkeypatch):
    """FSCNN_E2E_FUSED=0 sends the same call down the unfused route (front-end kernel,
    backbone(x)[0], torch's F.interpolate + softmax / argmax); it agrees with the fused one within
    the tail's bound.  fp32: in 16 bits the unfused route rounds the resampled logits before the
    softmax (torch's ops each return 16 bits), which the fused tail does not."""
    frames = frames_of(case, nc)
    fused, r64, bound, _ = tail_case(case, nc, torch.float32, True)
    lab = wrapper(case, nc).predict(frames, scale=255)
    e2e = wrapper(case, nc)
    monkeypatch.setenv("FSCNN_E2E_FUSED", "0")
    unfused = e2e(frames)
    assert e2e._last_fused is False
    lab_u = e2e.predict(frames, scale=255)
    assert e2e._last_fused is False
    monkeypatch.delenv("FSCNN_E2E_FUSED")
    err = (unfused.double() - fused.double()).abs().cpu()
    print("%s C=%d: max |unfused - fused| %.2e, worst / bound %.3f"
          % (case, nc, err.max(), (err / bound).max()))
    assert bool((err <= bound).all())
    top = torch.sort(fused, dim=1).values
    clear = (top[:, -1] - top[:, -2]) > 1e-5
    assert torch.equal(lab_u[clear], lab[clear])
    assert torch.equal(e2e(frames), fused) and e2e._last_fused is True


def test_more_than_32_classes_take_the_unfused_route():
    """The tail keeps the classes in registers, 32 at the most; a 40-class model runs unfused."""
    torch.manual_seed(0)
    bb = FastSCNN(40).to(DEV).eval()
    frames = frames_of("80x48", 2, 1)
    e2e = EndToEndFastSCNN(bb, input_size=(80, 48), base_size=64).to(DEV).eval()
    p = e2e(frames)
    assert e2e._last_fused is False and p.shape == (1, 40, 48, 80)
    with torch.no_grad():
        want = tail_ref(bb(e2e.preprocess(frames))[0], (80, 48))
    assert torch.allclose(p, want, atol=1e-6)
    assert torch.equal(e2e.predict(frames), want.argmax(1).to(torch.uint8))


# ---- 7. errors --------------------------------------------------------------------------------------
def test_train_mode_and_cpu_tensors_raise():
    e2e = wrapper("80x48", 2)
    frames = frames_of("80x48", 2)
    with pytest.raises(RuntimeError, match="device"):
        e2e(frames.cpu())
    with pytest.raises(RuntimeError, match="device"):
        e2e.predict(frames.cpu())
    with pytest.raises(RuntimeError):
        e2e(frames[:, :2])
    with pytest.raises(RuntimeError):
        e2e(frames.to(torch.int32))
    e2e.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            e2e(frames)
        with pytest.raises(RuntimeError, match="eval"):
            e2e.predict(frames)
    finally:
        e2e.eval()  # the backbone is shared between the tests
    assert e2e(frames).shape == (3, 2, 48, 80)


def test_autocast_overrides_dtype():
    e2e = wrapper("80x48", 2)
    frames = frames_of("80x48", 2)
    with torch.autocast("cuda", dtype=torch.float16):
        p = e2e(frames)
    assert p.dtype == torch.float16
    assert torch.equal(p, wrapper("80x48", 2, torch.float16)(frames))


# ---- 8. neighbours ----------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", CLASSES)
def test_neighbours_unchanged(nc):
    """backbone(x) and backbone.predict(x) give the same bits after e2e calls as before them (the
    pipeline shares the backbone's plans, arenas and workspace layout)."""
    bb = backbone(nc)
    frames = frames_of("200x70", nc)
    e2e = wrapper("200x70", nc)
    x = e2e.preprocess(frames)
    with torch.no_grad():
        y0, l0 = bb(x)[0].clone(), bb.predict(x).clone()
    sd0 = {k: v.clone() for k, v in bb.state_dict().items()}
    e2e(frames)
    e2e.predict(frames, scale=255)
    wrapper("200x70", nc, torch.float16)(frames)
    with torch.no_grad():
        assert torch.equal(bb(x)[0], y0) and torch.equal(bb.predict(x), l0)
    for k, v in bb.state_dict().items():
        assert torch.equal(v, sd0[k]), k
