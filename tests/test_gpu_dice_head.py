"""The fused Dice / Focal+Dice loss head (head.hip dice_head_kernel, FastSCNN.forward_loss with
``criterion=``): the head against fp64 autograd on the stored low-res logits, the fused step
against the unfused one through the whole model, determinism and the Python interface."""
import pytest
import torch
import torch.nn.functional as F

from fast_scnn_pytorch_amd import portable_init
from fast_scnn_pytorch_amd.loss import (DiceLoss, FocalDiceLoss, MixDiceLoss,
                                        MixSoftmaxCrossEntropyLoss)
from helpers import golden_input, golden_sd, load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _rnd(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def _low_res(n):
    """Spatial size of the 1/8-resolution logits (conv0 k3 s2 p0, then two stride-2 3x3 p1)."""
    n = (n - 3) // 2 + 1
    n = (n - 1) // 2 + 1
    return (n - 1) // 2 + 1


def _make_model(g, nc):
    from models.fast_scnn import FastSCNN
    m = FastSCNN(nc)
    m.load_state_dict(golden_sd(g))
    return m.to(DEV)


def _criterion(kind):
    return DiceLoss() if kind == "dice" else FocalDiceLoss(alpha=.25, gamma=1.5)


def _ref64(L, t, H, W, crit):
    """utils/loss.py:12-100 in fp64 on the upsampled low-res logits L [N, C, Hl, Wl]."""
    up = F.interpolate(L, (H, W), mode="bilinear", align_corners=True)
    p1 = F.softmax(up, dim=1)[:, 1].contiguous().view(-1)
    tf = t.contiguous().view(-1).double()
    smooth = crit.smooth
    dice = (2.0 * (p1 * tf).sum() + smooth) / (p1.sum() + tf.sum() + smooth)
    if isinstance(crit, DiceLoss):
        return 1 - dice
    ce = F.cross_entropy(up, t, reduction="none")
    pt = torch.exp(-ce)
    focal = (crit.alpha * (1 - pt) ** crit.gamma * ce).mean()
    return (1 - crit.dice_weight) * focal + crit.dice_weight * (1 - dice)


def _lanes(N, H, W, seed):
    """Lane-like binary targets: about 10 % ones, as thin slanted bands plus speckle."""
    hh = torch.arange(H).view(1, H, 1)
    ww = torch.arange(W).view(1, 1, W)
    band = ((ww + 2 * hh) % 40) < 3
    t = (band | (_rnd((N, H, W), seed) < 0.03)).long()
    t[:, : H // 8, :] = 0  # no lanes above the horizon
    return t


def _head_vs_fp64(dt, nc, N, H, W, kind, zero_target=False):
    from models.fast_scnn import FastSCNN
    torch.manual_seed(7)
    m = FastSCNN(nc).to(DEV).train()
    m._dropout_seed = 3
    m._keep_ws = True
    crit = _criterion(kind)
    x = _rnd((N, 3, H, W), 11, -1.0, 1.0).to(DEV).to(dt)
    if zero_target:
        t = torch.zeros(N, H, W, dtype=torch.long)
    elif nc == 2:
        t = _lanes(N, H, W, 12)
    else:
        t = _rnd((N, H, W), 12, 0, nc).floor().long().clamp_(0, nc - 1)
    t = t.to(DEV)
    scale = 1024.0 if dt == torch.float16 else 1.0  # f16: unscaled Dice gradients are subnormal
    loss = m.forward_loss(x, t, criterion=crit)
    (loss * scale).backward()
    torch.cuda.synchronize()
    Hl, Wl = _low_res(H), _low_res(W)
    L = m.debug_buffer("logits").double().view(N, Hl, Wl, nc).permute(0, 3, 1, 2).clone()
    G = m.debug_buffer("g_logits").double().view(N, Hl, Wl, nc).permute(0, 3, 1, 2)
    L.requires_grad_(True)
    lref = _ref64(L, t, H, W, crit)
    (lref * scale).backward()
    gref = L.grad
    err = (G - gref).abs()
    print("%s nc=%d %dx%d %s: loss %.8f ref %.8f rel %.2e; grad max err %.3e / max|g| %.3e = %.2e"
          % (dt, nc, H, W, kind, loss.item(), lref.item(),
             abs(loss.item() - lref.item()) / abs(lref.item()), err.max().item(),
             gref.abs().max().item(), err.max().item() / gref.abs().max().item()))
    assert torch.isfinite(loss).all() and torch.isfinite(G).all()
    assert abs(loss.item() - lref.item()) <= 1e-5 * abs(lref.item()), (loss.item(), lref.item())
    ulp = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dt]
    sub = 2.0 ** -24 if dt == torch.float16 else 0.0
    bound = ulp * gref.abs() + 2e-5 * gref.abs().max() + sub
    assert bool((err <= bound).all()), "dlogits: max err %.3e (max |g| %.3e)" % (
        err.max().item(), gref.abs().max().item())


@pytest.mark.parametrize("kind", ["dice", "focal_dice"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("nc,N,H,W", [
    (2, 2, 128, 256),     # the binary lane case: one pass, int8 targets on 16-bit plans
    (2, 2, 64, 2112),     # Wl = 264: two column chunks (carry), W > 2048: int64 targets per pixel
    (2, 2, 64, 260),      # W % 8 != 0: int64 target rows staged in LDS; odd low-res width
    (19, 2, 128, 256),    # general C (two passes); targets 0 .. 18 used as floats
    (3, 2, 64, 256),      # general C below the 8-class instance's width
])
def test_dice_head_vs_fp64(dt, nc, N, H, W, kind):
    """The head against autograd in fp64 on the SAME low-res logits the forward stored: bilinear
    align_corners upsample (models/fast_scnn.py:40) + DiceLoss / FocalDiceLoss (utils/loss.py:
    12-100).  Loss to 1e-5 relative; dlogits to one rounding of the plan dtype plus 2e-5 of the
    largest gradient (the CE head's bounds, tests/test_gpu_literal.py); fp16 through a x1024
    loss scale.  Measured on the MI355X: loss within 6e-8 relative; fp32 gradient error at most
    4.9e-6 of the largest gradient (64 x 2112), so the 2e-5 bound holds as stated."""
    _head_vs_fp64(dt, nc, N, H, W, kind)


@pytest.mark.parametrize("kind", ["dice", "focal_dice"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16])
def test_dice_head_no_lane_frame(dt, kind):
    """An all-zero target batch (T = 0, I = 0: a frame without lanes): finite, same bounds."""
    _head_vs_fp64(dt, 2, 2, 128, 256, kind, zero_target=True)


def _c2_batch(dt):
    """The train_c2 golden input; its golden target carries ignored (-1) pixels, which the Dice
    criteria do not define (they would enter the sums as t = -1), so the target is drawn with
    portable_init.target_tensor (both classes, nothing ignored)."""
    g = load_golden("train_c2")
    x = golden_input(g).to(DEV).to(dt)
    t = torch.from_numpy(portable_init.target_tensor(5, tuple(x.shape[:1] + x.shape[2:]), 2))
    assert t.min().item() == 0 and t.max().item() == 1
    return g, x, t.to(DEV)


@pytest.mark.parametrize("kind", ["mix_dice", "focal_dice"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_fused_dice_head_matches_unfused(dt, kind):
    g, x, t = _c2_batch(dt)
    crit = MixDiceLoss(aux=False) if kind == "mix_dice" else FocalDiceLoss()
    m1 = _make_model(g, 2).train()
    m1._dropout_seed = 5
    l1 = crit(m1(x), t) if kind == "mix_dice" else crit(m1(x)[0], t)
    l1.backward()
    m2 = _make_model(g, 2).train()
    m2._dropout_seed = 5
    l2 = m2.forward_loss(x, t, criterion=crit)
    l2.backward()
    torch.cuda.synchronize()
    # bf16: the unfused path rounds full-res logits to bf16 before the loss, the fused one does not
    tol = 1e-6 if dt == torch.float32 else 2e-3
    print(dt, kind, l1.item(), l2.item())
    assert abs(l1.item() - l2.item()) <= tol * abs(l1.item()), (l1.item(), l2.item())
    n1, n2 = dict(m1.named_parameters()), dict(m2.named_parameters())
    a = torch.cat([n1[k].grad.flatten() for k in n1]).double()
    b = torch.cat([n2[k].grad.flatten() for k in n2]).double()
    cos = (a @ b / (a.norm() * b.norm())).item()
    assert cos > (0.99999 if dt == torch.float32 else 0.9), cos
    for k in ("classifier.conv.1.weight", "classifier.conv.1.bias"):
        ga, gb = n1[k].grad.double(), n2[k].grad.double()
        assert (ga - gb).norm().item() <= (1e-5 if dt == torch.float32 else 2e-2) * ga.norm().item(), k
    s1, s2 = m1.state_dict(), m2.state_dict()
    for k in s1:
        if "running" in k:
            assert torch.equal(s1[k], s2[k]), k


@pytest.mark.parametrize("nc", [2, 19])
def test_fused_dice_step_is_deterministic(nc):
    from models.fast_scnn import FastSCNN
    torch.manual_seed(3)
    sd = FastSCNN(nc).state_dict()
    x = _rnd((2, 3, 128, 256), 21, -1.0, 1.0).to(DEV).to(torch.bfloat16)
    t = (_lanes(2, 128, 256, 22) if nc == 2 else
         _rnd((2, 128, 256), 22, 0, nc).floor().long().clamp_(0, nc - 1)).to(DEV)
    runs = []
    for _ in range(2):
        m = FastSCNN(nc)
        m.load_state_dict(sd)
        m = m.to(DEV).train()
        m._dropout_seed = 9
        loss = m.forward_loss(x, t, criterion=FocalDiceLoss())
        loss.backward()
        torch.cuda.synchronize()
        runs.append((loss.detach().clone(), [p.grad.clone() for p in m.parameters()]))
    assert torch.equal(runs[0][0], runs[1][0])
    for ga, gb in zip(runs[0][1], runs[1][1]):
        assert torch.equal(ga, gb)


def test_fused_dice_step_per_stage_backward():
    """The grad_stage_hook form (one native backward call per stage, what DistributedFastSCNN
    uses) carries the Dice head's planes and sums to stage 0 and gives the one-call gradients."""
    g, x, t = _c2_batch(torch.float32)
    grads, calls = [], []
    for hook in (None, lambda s, G, b, e: calls.append(s)):
        m = _make_model(g, 2).train()
        m._dropout_seed = 5
        m.grad_stage_hook = hook
        loss = m.forward_loss(x, t, criterion=FocalDiceLoss())
        loss.backward()
        torch.cuda.synchronize()
        grads.append(torch.cat([p.grad.flatten() for p in m.parameters()]))
    assert calls == [0, 1, 2, 3]
    # the same launches; only where the weight-gradient slabs are reduced differs
    torch.testing.assert_close(grads[1], grads[0], rtol=1e-6, atol=1e-6 * grads[0].abs().max().item())


def _ce_step(g, x, t, **kw):
    m = _make_model(g, 2).train()
    m._dropout_seed = 5
    loss = m.forward_loss(x, t, **kw)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), torch.cat([p.grad.flatten() for p in m.parameters()])


def test_criterion_none_and_ce_criterion_are_the_ce_head():
    g, x, t = _c2_batch(torch.float32)
    l0, g0 = _ce_step(g, x, t)
    l1, g1 = _ce_step(g, x, t, criterion=None)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    t = t.clone()
    t[:, :5, :] = 255
    l2, g2 = _ce_step(g, x, t, ignore_index=255)
    l3, g3 = _ce_step(g, x, t, criterion=MixSoftmaxCrossEntropyLoss(ignore_label=255))
    assert torch.equal(l2, l3) and torch.equal(g2, g3)
    assert not torch.equal(l0, l2)


def test_dice_head_refusals():
    from fast_scnn_pytorch_amd.loss import MixSoftmaxCrossEntropyOHEMLoss
    from models.fast_scnn import FastSCNN
    x = _rnd((2, 3, 64, 128), 1).to(DEV)
    t = _lanes(2, 64, 128, 2).to(DEV)
    aux = FastSCNN(2, aux=True).to(DEV).train()
    with pytest.raises(RuntimeError, match="main output only"):
        aux.forward_loss(x, t, criterion=MixDiceLoss(aux=True))
    m = FastSCNN(2).to(DEV)
    with pytest.raises(RuntimeError, match="train"):
        m.eval().forward_loss(x, t, criterion=DiceLoss())
    m.train()
    with pytest.raises(RuntimeError, match="unfused"):
        m.forward_loss(x, t, criterion=MixSoftmaxCrossEntropyOHEMLoss(use_weight=False))
