"""``FastSCNN.validate`` (csrc/evalhead.hip): the fused validation head against the code it
replaces.  Counters: integer equality with ``SegmentationMetric`` fed ``predict(x)``.  Loss:
within 1e-5 relative of the criterion evaluated by torch in fp64 on ``model(x)``'s own outputs
(the bound of the fused training heads, tests/test_gpu_dice_head.py / test_gpu_literal.py; the
head works from the same stored, rounded logits, so it holds for fp32 / bf16 / fp16 alike;
measured on the MI355X: at most 1.2e-7 over every case of this file).
No full-resolution tensor, determinism, no side effects, the unfused fallbacks, the refusals."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fast_scnn_pytorch_amd import portable_init
from fast_scnn_pytorch_amd.loss import (DiceLoss, FocalDiceLoss, MixDiceLoss,
                                        MixSoftmaxCrossEntropyLoss,
                                        MixSoftmaxCrossEntropyOHEMLoss)
from fast_scnn_pytorch_amd.metric import SegmentationMetric
from helpers import portable_sd

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SHAPES = [(2, 3, 128, 256),   # two images, several workgroups per image
          (1, 3, 67, 93),     # ragged, N = 1 (the predict test's shape)
          (1, 3, 64, 2112),   # W above a 2048-wide chunk: three column chunks, the last partial
          (3, 3, 40, 72)]     # H not a multiple of the row group at the low-res row boundaries


@functools.lru_cache(maxsize=None)
def _model(nc, aux=False):
    from models.fast_scnn import FastSCNN
    m = FastSCNN(nc, aux=aux)
    m.load_state_dict(portable_sd(nc, aux, seed=0, variant="bnrand"))
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _input(shape, dt, seed=1):
    return torch.from_numpy(portable_init.input_tensor(seed, shape)).to(DEV).to(dt)


def _ce_target(shape, nc, seed=2, stray=False):
    """About 10 % ignored (-1) pixels and one fully ignored row; ``stray``: a few labels >= C
    (255: labeled for the metric, outside the loss)."""
    N, _, H, W = shape
    t = torch.from_numpy(portable_init.target_tensor(seed, (N, H, W), nc, ignore_frac=0.1))
    t[:, 5, :] = -1
    if stray:
        t[:, 9, 3:W // 2] = 255
    return t.to(DEV)


def _lanes(N, H, W, seed):
    """The dice tests' lane pattern: about 10 % ones as thin slanted bands plus speckle."""
    hh = torch.arange(H).view(1, H, 1)
    ww = torch.arange(W).view(1, 1, W)
    band = ((ww + 2 * hh) % 40) < 3
    g = torch.Generator(device="cpu").manual_seed(seed)
    t = (band | (torch.rand(N, H, W, generator=g) < 0.03)).long()
    t[:, : H // 8, :] = 0
    return t


def _dice_target(shape, nc, seed=3):
    N, _, H, W = shape
    if nc == 2:
        return _lanes(N, H, W, seed).to(DEV)
    return torch.from_numpy(portable_init.target_tensor(seed, (N, H, W), nc)).to(DEV)


def _ref_counts(m, x, t):
    ref = SegmentationMetric(m.num_classes)
    ref.update(m.predict(x), t)
    return ref.counts()


def _ce64(out, t, ignore=-1):
    return F.cross_entropy(out.double(), t, ignore_index=ignore)


def _dice64(out, t, crit):
    """utils/loss.py:12-100 in fp64 on full-resolution logits."""
    o = out.double()
    p1 = F.softmax(o, dim=1)[:, 1].contiguous().view(-1)
    tf = t.contiguous().view(-1).double()
    inner = getattr(crit, "dice_loss", crit)
    smooth = inner.smooth
    dice = (2.0 * (p1 * tf).sum() + smooth) / (p1.sum() + tf.sum() + smooth)
    if not isinstance(crit, FocalDiceLoss):
        return 1 - dice
    ce = F.cross_entropy(o, t, reduction="none")
    pt = torch.exp(-ce)
    focal = (crit.alpha * (1 - pt) ** crit.gamma * ce).mean()
    return (1 - crit.dice_weight) * focal + crit.dice_weight * (1 - dice)


def _check_loss(tag, loss, ref):
    rel = abs(loss.item() - ref.item()) / abs(ref.item())
    print("%s: loss %.8f fp64 %.8f rel %.2e" % (tag, loss.item(), ref.item(), rel))
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda
    assert np.isfinite(loss.item())
    assert rel <= 1e-5, (tag, loss.item(), ref.item())


# ---- 1. counters ------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [19, 2])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dt", DTYPES)
def test_counters_equal_predict_metric(dt, shape, nc):
    m = _model(nc)
    x1, x2 = _input(shape, dt, 1), _input(shape, dt, 4)
    t1, t2 = _ce_target(shape, nc, 2, stray=True), _ce_target(shape, nc, 5)
    M1 = SegmentationMetric(nc)
    m.validate(x1, t1, metric=M1)
    assert m._last_validate_fused is True
    c1 = _ref_counts(m, x1, t1)
    assert c1[1] > 0 and c1[0] > 0  # something labeled, something correct
    assert np.array_equal(M1.counts(), c1), (M1.counts(), c1)
    m.validate(x2, t2, metric=M1)  # a second batch accumulates
    assert np.array_equal(M1.counts(), c1 + _ref_counts(m, x2, t2))
    assert M1.get()[0] == pytest.approx(float(M1.counts()[0]) / float(M1.counts()[1]))


# ---- 2. loss ----------------------------------------------------------------------------------
@pytest.mark.parametrize("crit", ["none", "mix_ce"])
@pytest.mark.parametrize("nc,shape", [(19, SHAPES[0]), (19, SHAPES[1]), (2, SHAPES[2]),
                                      (19, SHAPES[3])])
@pytest.mark.parametrize("dt", DTYPES)
def test_ce_loss_vs_fp64(dt, nc, shape, crit):
    m = _model(nc)
    x, t = _input(shape, dt), _ce_target(shape, nc)
    criterion = None if crit == "none" else MixSoftmaxCrossEntropyLoss(aux=False)
    loss = m.validate(x, t, criterion=criterion)
    assert m._last_validate_fused is True
    with torch.no_grad():
        ref = _ce64(m(x)[0], t)
    _check_loss("%s nc=%d %s %s" % (dt, nc, shape, crit), loss, ref)


def test_ce_loss_other_ignore_index():
    """``ignore_index`` of the argument and of the criterion: 255 ignored, -1 out of range
    (left out by the kernels like any target outside [0, C))."""
    m = _model(19)
    x, t = _input(SHAPES[0], torch.float32), _ce_target(SHAPES[0], 19).clone()
    t[t < 0] = 255
    with torch.no_grad():
        ref = _ce64(m(x)[0], t, 255)
    _check_loss("ignore_index=255", m.validate(x, t, ignore_index=255), ref)
    _check_loss("criterion ignore 255",
                m.validate(x, t, criterion=MixSoftmaxCrossEntropyLoss(aux=False, ignore_label=255)),
                ref)


def _dice_criterion(kind):
    return {"dice": DiceLoss(), "mix_dice": MixDiceLoss(aux=False),
            "focal_dice": FocalDiceLoss(alpha=.25, gamma=1.5)}[kind]


@pytest.mark.parametrize("kind", ["dice", "mix_dice", "focal_dice"])
@pytest.mark.parametrize("nc,shape", [(2, SHAPES[0]), (3, SHAPES[0]), (19, SHAPES[0]),
                                      (2, SHAPES[1]), (2, SHAPES[2])])
@pytest.mark.parametrize("dt", DTYPES)
def test_dice_loss_vs_fp64(dt, nc, shape, kind):
    m = _model(nc)
    x, t = _input(shape, dt), _dice_target(shape, nc)
    crit = _dice_criterion(kind)
    loss = m.validate(x, t, criterion=crit)
    assert m._last_validate_fused is True
    with torch.no_grad():
        ref = _dice64(m(x)[0], t, crit)
    _check_loss("%s nc=%d %s %s" % (dt, nc, shape, kind), loss, ref)


@pytest.mark.parametrize("kind", ["dice", "focal_dice"])
@pytest.mark.parametrize("dt", DTYPES)
def test_dice_loss_no_lane_frame(dt, kind):
    """An all-zero Dice target (T = 0, I = 0: a frame without lanes)."""
    m = _model(2)
    x = _input(SHAPES[0], dt)
    t = torch.zeros(2, 128, 256, dtype=torch.long, device=DEV)
    crit = _dice_criterion(kind)
    loss = m.validate(x, t, criterion=crit)
    assert m._last_validate_fused is True
    with torch.no_grad():
        ref = _dice64(m(x)[0], t, crit)
    _check_loss("%s no lanes %s" % (dt, kind), loss, ref)


def test_wide_logit_spread():
    """Classifier weights x 8000 (x 300 moves the class maximum by 3.9 between neighbouring
    low-res cells of this input): the maxima of neighbouring cells lie more than 60 apart, where
    the head sums a pixel against its own maximum instead of the cells' bound (evalhead.hip
    EH_SPREAD).  Same loss bound, same exact counters."""
    from models.fast_scnn import FastSCNN
    m = FastSCNN(19)
    m.load_state_dict(portable_sd(19, False, seed=0, variant="bnrand"))
    with torch.no_grad():
        m.classifier.conv[1].weight.mul_(8000.0)
    m = m.to(DEV).eval()
    shape = SHAPES[0]
    x, t = _input(shape, torch.float32), _ce_target(shape, 19)
    m._keep_ws = True
    M1 = SegmentationMetric(19)
    loss = m.validate(x, t, metric=M1)
    assert m._last_validate_fused is True
    low = m.debug_buffer("logits").float().view(2, 16, 32, 19).amax(-1)
    spread = max((low[:, 1:] - low[:, :-1]).abs().max().item(),
                 (low[:, :, 1:] - low[:, :, :-1]).abs().max().item())
    print("largest step of the class maximum between neighbouring cells: %.1f" % spread)
    assert spread > 60.0
    with torch.no_grad():
        ref = _ce64(m(x)[0], t)
    _check_loss("wide spread", loss, ref)
    assert np.array_equal(M1.counts(), _ref_counts(m, x, t))


# ---- 3. aux -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nc", [2, 19])
def test_aux_loss_and_counters(dt, nc):
    m = _model(nc, aux=True)
    shape = SHAPES[0]
    x = _input(shape, dt)
    if nc == 2:
        t, w = _dice_target(shape, 2), 0.4
        crit, crit_main = MixDiceLoss(aux=True, aux_weight=w), MixDiceLoss(aux=False)
        ref_fn = lambda o: _dice64(o, t, crit)  # noqa: E731
    else:
        t, w = _ce_target(shape, 19), 0.2
        crit = MixSoftmaxCrossEntropyLoss(aux=True, aux_weight=w)
        crit_main = MixSoftmaxCrossEntropyLoss(aux=False)
        ref_fn = lambda o: _ce64(o, t)  # noqa: E731
    with torch.no_grad():
        outs = m(x)
    main, aux = ref_fn(outs[0]), ref_fn(outs[1])
    M1 = SegmentationMetric(nc)
    loss = m.validate(x, t, criterion=crit, metric=M1)
    assert m._last_validate_fused is True
    _check_loss("%s aux nc=%d" % (dt, nc), loss, main + w * aux)
    assert np.array_equal(M1.counts(), _ref_counts(m, x, t))  # output 0's argmax
    loss0 = m.validate(x, t, criterion=crit_main)  # the criterion's aux=False: main only
    assert m._last_validate_fused is True
    _check_loss("%s aux net, criterion aux=False nc=%d" % (dt, nc), loss0, main)
    assert abs(aux.item()) > 1e-3  # the two results above really differ


# ---- 4. no full-resolution tensor -------------------------------------------------------------
def test_no_full_resolution_tensor():
    m = _model(19)
    shape = (2, 3, 256, 512)
    x, t = _input(shape, torch.float32), _ce_target(shape, 19)
    M1 = SegmentationMetric(19)
    M1.device_counts(x.device)
    m.predict(x)
    m.validate(x, t, metric=M1)  # plans and arenas exist from here on
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    m.predict(x)
    torch.cuda.synchronize()
    peak_predict = torch.cuda.max_memory_allocated() - base
    torch.cuda.reset_peak_memory_stats()
    m.validate(x, t, metric=M1)
    torch.cuda.synchronize()
    peak_validate = torch.cuda.max_memory_allocated() - base
    print("peak over predict %d B, over validate %d B" % (peak_predict, peak_validate))
    assert m._last_validate_fused is True
    assert peak_validate <= peak_predict + (1 << 20)


# ---- 5. determinism and side effects ----------------------------------------------------------
@pytest.mark.parametrize("kind", ["ce", "focal_dice"])
def test_deterministic_and_no_side_effects(kind):
    nc = 19 if kind == "ce" else 2
    m = _model(nc)
    shape = SHAPES[0]
    x = _input(shape, torch.bfloat16)
    t = _ce_target(shape, nc) if kind == "ce" else _dice_target(shape, nc)
    crit = None if kind == "ce" else FocalDiceLoss()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    a = m.validate(x, t, criterion=crit)  # grad enabled outside
    with torch.no_grad():
        b = m.validate(x, t, criterion=crit)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert a.requires_grad is False and a.grad_fn is None and b.requires_grad is False
    after = m.state_dict()
    assert sorted(before) == sorted(after)
    for k in before:
        assert torch.equal(before[k], after[k]), k


# ---- 6. fallbacks -----------------------------------------------------------------------------
def test_ohem_takes_the_unfused_route():
    m = _model(19)
    shape = SHAPES[0]
    x, t = _input(shape, torch.float32), _ce_target(shape, 19)
    crit = MixSoftmaxCrossEntropyOHEMLoss(aux=False, use_weight=False)
    M1 = SegmentationMetric(19)
    loss = m.validate(x, t, criterion=crit, metric=M1)
    assert m._last_validate_fused is False
    with torch.no_grad():
        ref = crit(m(x), t)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and not loss.requires_grad
    assert torch.equal(loss, ref)
    assert np.array_equal(M1.counts(), _ref_counts(m, x, t))


def test_dice_outside_class_range_takes_the_unfused_route():
    """C = 40 is above the head's 32 classes (the library answers E_UNSUPPORTED)."""
    m = _model(40)
    shape = SHAPES[1]
    x, t = _input(shape, torch.float32), _dice_target(shape, 40)
    M1 = SegmentationMetric(40)
    loss = m.validate(x, t, criterion=DiceLoss(), metric=M1)
    assert m._last_validate_fused is False
    with torch.no_grad():
        ref = DiceLoss()(m(x)[0], t)
    assert torch.equal(loss, ref.reshape(()))
    assert np.array_equal(M1.counts(), _ref_counts(m, x, t))


def test_switch_off_takes_the_unfused_route(tmp_path):
    """FSCNN_VAL_FUSED=0 in a child process (tests/_validate_worker.py): the unfused route, the
    loss of ``cross_entropy(model(x)[0], t)`` bit for bit, exact counters; the default child
    takes the fused route and agrees to the loss bound."""
    res = {}
    for switch in ("0", None):
        out = str(tmp_path / ("val_%s.npz" % switch))
        env = dict(os.environ)
        env.pop("FSCNN_VAL_FUSED", None)
        if switch is not None:
            env["FSCNN_VAL_FUSED"] = switch
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_validate_worker.py"),
                            out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        res[switch] = dict(np.load(out))
    off, on = res["0"], res[None]
    assert int(off["fused"]) == 0 and int(on["fused"]) == 1
    assert off["loss"] == off["unfused_loss"]  # bit for bit
    assert np.array_equal(off["counts"], off["ref_counts"])
    assert np.array_equal(on["counts"], on["ref_counts"])
    assert abs(float(on["loss"]) - float(on["loss64"])) <= 1e-5 * abs(float(on["loss64"]))


# ---- 7. refusals ------------------------------------------------------------------------------
def test_refusals():
    from models.fast_scnn import FastSCNN
    m = FastSCNN(19).to(DEV)
    x = _input((2, 3, 64, 128), torch.float32)
    t = _ce_target((2, 3, 64, 128), 19)
    with pytest.raises(RuntimeError, match="eval"):
        m.train().validate(x, t)
    m.eval()
    with pytest.raises(RuntimeError):
        m.validate(x, t[:, :32])
    with pytest.raises(RuntimeError):
        m.validate(x, t[:1])
    with pytest.raises(RuntimeError):
        m.validate(x, t.cpu())
    with pytest.raises(RuntimeError):
        m.validate(x, t, metric=SegmentationMetric(2))
    assert torch.isfinite(m.validate(x, t))  # and the model still works afterwards
