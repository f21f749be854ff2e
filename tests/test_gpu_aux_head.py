"""The fused aux loss heads (FastSCNN.forward_loss_aux, fscnn_forward_loss_aux /
fscnn_backward_loss_aux): the reference anchor (the train_c19_aux golden), the fused step against
the unfused one through the whole model for the three two-output criteria, the two unweighted
terms and the aux_weight law (Dice with 2 classes and with 19: the one-pass and the two-pass
head), the OHEM k-th branch and kept sets of both heads against fp64, CHECK_TARGETS, determinism, no
host synchronisation, the per-stage backward, the input gradient, the refusals, graph replay in a
fresh child process and the DistributedFastSCNN delegation."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fast_scnn_pytorch_amd import portable_init
from fast_scnn_pytorch_amd.loss import (OHEM_CLASS_WEIGHT, DiceLoss, FocalDiceLoss, MixDiceLoss,
                                        MixSoftmaxCrossEntropyLoss,
                                        MixSoftmaxCrossEntropyOHEMLoss,
                                        SoftmaxCrossEntropyOHEMLoss)
from helpers import golden_input, golden_sd, golden_target, load_golden, portable_sd

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# dice: the 2-class one-pass Dice head; dice19: the general-C two-pass head (train.py's C = 19)
KINDS = ["ce", "dice", "dice19", "ohem"]
AUX4 = ("auxlayer.4.weight", "auxlayer.4.bias")
CLS = ("classifier.conv.1.weight", "classifier.conv.1.bias")


def _criterion(kind, aux_weight=0.4):
    if kind == "ce":
        return MixSoftmaxCrossEntropyLoss(aux=True, aux_weight=aux_weight, ignore_label=-1)
    if kind.startswith("dice"):
        return MixDiceLoss(aux=True, aux_weight=aux_weight)
    return MixSoftmaxCrossEntropyOHEMLoss(aux=True, aux_weight=aux_weight)  # (0.7, 256), weights


def _single(kind):
    """The criterion's single-output law."""
    if kind == "ce":
        return MixSoftmaxCrossEntropyLoss(aux=False, ignore_label=-1)
    if kind.startswith("dice"):
        return DiceLoss()
    return SoftmaxCrossEntropyOHEMLoss()


_SD = {}


def _sd(kind):
    """19-class aux weights of the golden (calibrated BN statistics) / 2-class aux for Dice."""
    if kind not in _SD:
        _SD[kind] = (portable_sd(2, aux=True, seed=0, variant="bnrand") if kind == "dice"
                     else golden_sd(load_golden("train_c19_aux")))
    return _SD[kind]


def _model(kind, seed=5):
    from models.fast_scnn import FastSCNN
    m = FastSCNN(2 if kind == "dice" else 19, aux=True)
    m.load_state_dict(_sd(kind))
    m = m.to(DEV).train()
    m._dropout_seed = seed
    return m


def _batch(kind, shape, dt=torch.float32):
    """Input and target of a shape: the golden's own at its shape; Dice has no ignored pixel."""
    N, _, H, W = shape
    g = load_golden("train_c19_aux")
    dice = kind.startswith("dice")
    if not dice and tuple(int(s) for s in g["shape"]) == tuple(shape):
        return golden_input(g).to(DEV).to(dt), golden_target(g).to(DEV)
    x = torch.from_numpy(portable_init.input_tensor(31, tuple(shape))).to(DEV).to(dt)
    nc = 2 if kind == "dice" else 19
    t = torch.from_numpy(portable_init.target_tensor(32, (N, H, W), nc,
                                                     ignore_frac=0.0 if dice else 0.05)).to(DEV)
    if dice:
        assert int(((t < 0) | (t >= nc)).sum()) == 0
        assert kind == "dice" or int(t.max()) > 1   # dice19: labels beyond class 1 do occur
    return x, t


def _grads(m):
    return {k: p.grad.detach().double() for k, p in m.named_parameters()}


def _flat(g):
    return torch.cat([v.flatten() for v in g.values()])


def _compare(dt, l1, g1, s1, l2, g2, s2, what=""):
    """The fused-vs-unfused bounds of test_fused_ohem_head_matches_unfused /
    test_fused_dice_head_matches_unfused, auxlayer.4.* held to the classifier conv's bound."""
    f32 = dt == torch.float32
    a, b = _flat(g1), _flat(g2)
    cos = (a @ b / (a.norm() * b.norm())).item()
    rel = {k: ((g1[k] - g2[k]).norm() / g1[k].norm()).item() for k in CLS + AUX4}
    print(what, dt, "loss %.8f / %.8f rel %.2e; cos %.8f; %s"
          % (l1, l2, abs(l1 - l2) / abs(l1), cos,
             " ".join("%s %.2e" % (k.split(".", 1)[0][:3] + k[-6:], v) for k, v in rel.items())))
    assert abs(l1 - l2) <= (1e-6 if f32 else 2e-3) * abs(l1), (l1, l2)
    assert cos > (0.99999 if f32 else 0.9), cos
    for k, v in rel.items():
        assert v <= (1e-5 if f32 else 2e-2), (k, v)
    for k in s1:
        if "running" in k:
            assert torch.equal(s1[k], s2[k]), k


def _assert_no_prob_near_thresh(outs, t, thresh=0.7, band=1e-3):
    """Precondition of the OHEM comparisons: no label probability of either full-resolution output
    within `band` of the threshold, so both routes keep the same pixels."""
    lab = t >= 0
    for o in outs:
        p = F.softmax(o.detach().float(), 1).gather(1, t.clamp(min=0).unsqueeze(1))[:, 0]
        assert not bool((lab & ((p - thresh).abs() <= band)).any())


def _steps(kind, shape, dt, aux_weight=0.4):
    """(unfused, fused) steps of two equal models: loss, gradients, state_dict, model."""
    x, t = _batch(kind, shape, dt)
    crit = _criterion(kind, aux_weight)
    m1 = _model(kind)
    outs = m1(x)
    if kind == "ohem":
        _assert_no_prob_near_thresh(outs, t)
    l1 = crit(outs, t)
    l1.backward()
    m2 = _model(kind)
    l2 = m2.forward_loss_aux(x, t, crit)
    assert l2.dim() == 0 and l2.dtype == torch.float32
    l2.backward()
    torch.cuda.synchronize()
    return (l1.item(), _grads(m1), m1.state_dict(), m1), (l2.item(), _grads(m2), m2.state_dict(), m2)


GOLDEN_SHAPE = (2, 3, 96, 160)


def test_reference_anchor_ce():
    """train_c19_aux (MixSoftmaxCrossEntropyLoss(aux=True, 0.4), both Dropouts active): the
    reference's loss, its sampled auxlayer.4 gradients, and every gradient of the unfused step."""
    g = load_golden("train_c19_aux")
    assert tuple(int(s) for s in g["shape"]) == GOLDEN_SHAPE
    x, t = golden_input(g).to(DEV), golden_target(g).to(DEV)
    crit = _criterion("ce", 0.4)
    runs = []
    for fused in (False, True):
        m = _model("ce", seed=int(g["drop_seed"]))
        loss = m.forward_loss_aux(x, t, crit) if fused else crit(m(x), t)
        loss.backward()
        torch.cuda.synchronize()
        runs.append((loss.item(), _grads(m), m.state_dict()))
    (l1, g1, s1), (l2, g2, s2) = runs
    ref = float(g["loss"])
    print("loss fused %.8f golden %.8f" % (l2, ref))
    assert abs(l2 - ref) < 1e-5 * max(1.0, abs(ref))
    assert sorted(g1) == sorted(k for k, _ in m.named_parameters())  # every parameter's gradient
    _compare(torch.float32, l1, g1, s1, l2, g2, s2, "anchor")
    for k in AUX4:
        gr = g2[k].cpu().numpy().ravel()[g["grad_idx." + k]]
        rv = g["grad_val." + k].astype(np.float64)
        err = np.linalg.norm(gr - rv) / np.linalg.norm(rv)
        print(k, "vs golden samples: rel %.2e" % err)
        assert err <= 1e-4, (k, err)


@pytest.mark.parametrize("shape,dt", [
    (GOLDEN_SHAPE, torch.float32), (GOLDEN_SHAPE, torch.bfloat16),
    ((3, 3, 64, 96), torch.float32), ((3, 3, 64, 96), torch.bfloat16),   # odd batch
    ((2, 3, 256, 512), torch.bfloat16),  # 4,096 low-res pixels: streaming classifier dgrad + Dropout
], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).split(".")[-1])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_aux_step_matches_unfused(kind, shape, dt):
    (l1, g1, s1, _), (l2, g2, s2, _) = _steps(kind, shape, dt)
    _compare(dt, l1, g1, s1, l2, g2, s2, "%s %s" % (kind, shape))


@pytest.mark.parametrize("kind", KINDS)
def test_loss_terms_and_aux_weight(kind):
    """_last_loss_terms = the single-output criterion on each unfused output (same seed); the
    returned loss is their weighted sum; doubling aux_weight doubles the auxlayer.4 gradients and
    leaves the classifier conv's alone."""
    dt = torch.float32
    x, t = _batch(kind, GOLDEN_SHAPE, dt)
    m1 = _model(kind)
    outs = m1(x)
    one = _single(kind)
    want = [one(outs[0], t).item(), one(outs[1], t).item()]
    res = {}
    for w in (0.4, 0.8):
        m = _model(kind)
        loss = m.forward_loss_aux(x, t, _criterion(kind, w))
        terms = m._last_loss_terms
        assert terms.is_cuda and terms.dtype == torch.float32 and tuple(terms.shape) == (2,)
        loss.backward()
        torch.cuda.synchronize()
        res[w] = (loss.item(), terms.cpu().double(), _grads(m))
    loss, terms, _ = res[0.4]
    print(kind, "terms", terms.tolist(), "unfused", want, "loss", loss)
    for i in range(2):
        assert abs(terms[i].item() - want[i]) <= 1e-6 * abs(want[i]), (i, terms[i].item(), want[i])
    for w in (0.4, 0.8):
        loss, terms, _ = res[w]
        total = terms[0].item() + float(np.float32(w)) * terms[1].item()
        assert abs(loss - total) <= 1e-6 * abs(total), (w, loss, total)
    assert torch.equal(res[0.4][1], res[0.8][1])
    for k in AUX4:
        torch.testing.assert_close(res[0.8][2][k], 2.0 * res[0.4][2][k], rtol=1e-6, atol=0.0)
    for k in CLS:
        torch.testing.assert_close(res[0.8][2][k], res[0.4][2][k], rtol=1e-6, atol=0.0)


def _rnd(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def _low_res(n):
    n = (n - 3) // 2 + 1
    n = (n - 1) // 2 + 1
    return (n - 1) // 2 + 1


def _kth_batch():
    """As tests/test_gpu_ohem_head.py _kth_batch / _targets: 2 x 3 x 128 x 256 bf16, uniform
    classes, 10 % ignored plus one fully ignored 8-row band."""
    N, H, W = 2, 128, 256
    x = _rnd((N, 3, H, W), 21, -1.0, 1.0).to(DEV).to(torch.bfloat16)
    t = _rnd((N, H, W), 12, 0, 19).floor().long().clamp_(0, 18)
    t[_rnd((N, H, W), 13) < 0.1] = -1
    t[:, 16:24, :] = -1
    return x, t.to(DEV)


def _kth_criterion(aux_weight=0.4):
    return MixSoftmaxCrossEntropyOHEMLoss(aux=True, aux_weight=aux_weight, thresh=0.01,
                                          min_kept=5000)


def _kth_model(seed=9):
    from models.fast_scnn import FastSCNN
    torch.manual_seed(3)
    m = FastSCNN(19, aux=True).to(DEV).train()
    m._dropout_seed = seed
    return m


def test_ohem_kth_branch_on_both_heads():
    """Criterion (0.01, 5000): each head selects its own k-th smallest label probability, keeps
    its own set, and the total is the criterion law in fp64 (upsample, then weighted CE over each
    head's kept set) on the stored low-res logits of both outputs."""
    N, H, W, nc = 2, 128, 256, 19
    x, t = _kth_batch()
    m = _kth_model()
    m._keep_ws = True
    loss = m.forward_loss_aux(x, t, _kth_criterion())
    torch.cuda.synchronize()
    heads = m._debug["ohem"]
    Hl, Wl = _low_res(H), _low_res(W)
    tc = t.cpu()
    lab = (tc >= 0).numpy()
    w64 = torch.tensor(OHEM_CLASS_WEIGHT, dtype=torch.float64)
    thr, terms = [], []
    for i, name in enumerate(("logits", "aux_logits")):
        prob = heads[i]["prob"].cpu().numpy()
        th = heads[i]["thr"].cpu().numpy()[0]
        counts = heads[i]["counts"].cpu().numpy()
        assert th > np.float32(0.01) and np.isfinite(th)      # the k-th branch
        assert counts[0] == lab.sum() and (prob[~lab] == 2.0).all()
        kept = lab & (prob <= th)
        pl = np.sort(prob[lab])
        assert th == pl[5000 - 1] and kept.sum() >= 5000
        # the head's own kept set: the weight sum it stored is that of #(plane <= thr)
        assert counts[1] == (lab & (prob <= np.float32(0.01))).sum()
        wsum = w64[tc[torch.from_numpy(kept)]].sum().item()
        got_w = heads[i]["pair"].cpu().double()[1].item()
        print(name, "kept weight sum %.6f head %.6f" % (wsum, got_w))
        assert abs(got_w - wsum) <= 1e-6 * wsum, (got_w, wsum)
        L = m.debug_buffer(name).double().view(N, Hl, Wl, nc).permute(0, 3, 1, 2).cpu()
        up = F.interpolate(L, (H, W), mode="bilinear", align_corners=True)
        tm = torch.where(torch.from_numpy(kept), tc, torch.full_like(tc, -1))
        terms.append(F.cross_entropy(up, tm, weight=w64, ignore_index=-1).item())
        thr.append(float(th))
        print(name, "thr %.6f kept %d term %.8f" % (th, kept.sum(), terms[-1]))
    assert thr[0] != thr[1]
    got = m._last_loss_terms.cpu().double()
    for i in range(2):
        assert abs(got[i].item() - terms[i]) <= 1e-5 * abs(terms[i]), (i, got[i].item(), terms[i])
    total = terms[0] + float(np.float32(0.4)) * terms[1]
    assert abs(loss.item() - total) <= 1e-5 * abs(total), (loss.item(), total)
    # and as a count: without class weights each head's stored sum is its kept count, exactly
    # #(plane <= thr) of its own plane (train-mode logits do not depend on the running statistics,
    # so the planes are those of the run above)
    planes = [(h["prob"].cpu().numpy(), h["thr"].cpu().numpy()[0]) for h in heads]
    crit = MixSoftmaxCrossEntropyOHEMLoss(aux=True, aux_weight=0.4, thresh=0.01, min_kept=5000,
                                          use_weight=False)
    m.forward_loss_aux(x, t, crit)
    torch.cuda.synchronize()
    for i, (prob0, th0) in enumerate(planes):
        h = m._debug["ohem"][i]
        prob, th = h["prob"].cpu().numpy(), h["thr"].cpu().numpy()[0]
        assert np.array_equal(prob, prob0) and th == th0
        assert h["pair"].cpu()[1].item() == float((lab & (prob <= th)).sum())


def test_fused_aux_step_is_deterministic():
    from models.fast_scnn import FastSCNN
    torch.manual_seed(3)
    sd = FastSCNN(19, aux=True).state_dict()
    x, t = _kth_batch()
    runs = []
    for _ in range(2):
        m = FastSCNN(19, aux=True)
        m.load_state_dict(sd)
        m = m.to(DEV).train()
        m._dropout_seed = 9
        loss = m.forward_loss_aux(x, t, _kth_criterion())
        loss.backward()
        torch.cuda.synchronize()
        runs.append((loss.detach().clone(), m._last_loss_terms.clone(),
                     [p.grad.clone() for p in m.parameters()]))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for ga, gb in zip(runs[0][2], runs[1][2]):
        assert torch.equal(ga, gb)


@pytest.mark.parametrize("kind", ["ce", "ohem"])
def test_fused_aux_step_has_no_host_sync(kind):
    m = _kth_model()
    x, t = _kth_batch()
    crit = _kth_criterion() if kind == "ohem" else _criterion("ce")
    m.forward_loss_aux(x, t, crit).backward()  # warm: plans, arenas, the weights' one copy
    m.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = m.forward_loss_aux(x, t, crit)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())


@pytest.mark.parametrize("kind", KINDS)
def test_fused_aux_step_per_stage_backward(kind):
    """The grad_stage_hook form (one native backward call per stage, what DistributedFastSCNN
    uses) gives the one-call gradients; the loss may be scaled in place before the backward."""
    x, t = _batch(kind, GOLDEN_SHAPE)
    grads, calls = [], []
    for hook in (None, lambda s, G, b, e: calls.append(s)):
        m = _model(kind)
        m.grad_stage_hook = hook
        loss = m.forward_loss_aux(x, t, _criterion(kind))
        if hook is not None:
            loss /= 2  # the backward reads the heads' own state, never the returned loss
        loss.backward()
        torch.cuda.synchronize()
        grads.append(torch.cat([p.grad.flatten() for p in m.parameters()]))
    assert calls == [0, 1, 2, 3]
    torch.testing.assert_close(2 * grads[1], grads[0], rtol=1e-6,
                               atol=1e-6 * grads[0].abs().max().item())


@pytest.mark.parametrize("kind", ["ce", "ohem"])
def test_fused_aux_input_gradient(kind):
    xg, t = _batch(kind, GOLDEN_SHAPE)
    crit = _criterion(kind)
    dx = []
    for fused in (False, True):
        x = xg.clone().requires_grad_()
        m = _model(kind)
        loss = m.forward_loss_aux(x, t, crit) if fused else crit(m(x), t)
        loss.backward()
        torch.cuda.synchronize()
        assert x.grad is not None and torch.isfinite(x.grad).all()
        dx.append(x.grad.double())
    assert dx[0].norm().item() > 0
    rel = (dx[1] - dx[0]).norm().item() / dx[0].norm().item()
    print(kind, "dx rel", rel)
    assert rel <= 1e-5


def test_aux_head_refusals():
    from models.fast_scnn import FastSCNN
    x, t = _batch("dice", (2, 3, 64, 128))
    ok = MixDiceLoss(aux=True)
    m = _model("dice")
    plain = FastSCNN(2).to(DEV).train()
    for crit in (FocalDiceLoss(), DiceLoss(), SoftmaxCrossEntropyOHEMLoss(use_weight=False),
                 torch.nn.CrossEntropyLoss(), MixDiceLoss(aux=False),
                 MixSoftmaxCrossEntropyLoss(aux=False)):
        with pytest.raises(RuntimeError, match="unfused"):
            m.forward_loss_aux(x, t, crit)
    with pytest.raises(RuntimeError, match="unfused"):
        plain.forward_loss_aux(x, t, ok)                       # no aux head
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m.forward_loss_aux(x[:1], t[:1], ok)                   # N < 2
    with pytest.raises(RuntimeError, match="ROCm device tensors"):
        m.forward_loss_aux(x.cpu(), t.cpu(), ok)
    with pytest.raises(RuntimeError, match="train"):
        m.eval().forward_loss_aux(x, t, ok)
    m.train()
    with pytest.raises(RuntimeError, match="input image's gradient"):
        m.forward_loss_aux(x.clone().requires_grad_(), t, ok)  # Dice forms no dx
    with pytest.raises(RuntimeError, match="weight tensor should be defined either for all 2 "
                                           "classes"):
        m.forward_loss_aux(x, t, MixSoftmaxCrossEntropyOHEMLoss(aux=True))  # 19 weights
    big = FastSCNN(40, aux=True).to(DEV).train()
    with pytest.raises(RuntimeError, match="1 .. 32 classes"):
        big.forward_loss_aux(x, t, MixSoftmaxCrossEntropyLoss(aux=True))
    one = FastSCNN(1, aux=True).to(DEV).train()
    with pytest.raises(RuntimeError, match="2 .. 32"):
        one.forward_loss_aux(x, torch.zeros_like(t), ok)
    # the existing entries keep refusing an aux model
    with pytest.raises(RuntimeError, match="main output only"):
        m.forward_loss(x, t)
    with pytest.raises(RuntimeError, match="main output only"):
        m.forward_loss_ohem(x, t, MixSoftmaxCrossEntropyOHEMLoss(use_weight=False))
    # and the same call without a defect runs
    loss = m.forward_loss_aux(x, t, ok)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())


def test_check_targets_behaves_as_in_the_single_output_entries(monkeypatch):
    """loss.CHECK_TARGETS: a target that is neither ignore_index nor a class raises IndexError
    (Dice has no ignore_index: any target outside [0, C)); valid targets run."""
    from fast_scnn_pytorch_amd import loss as L
    monkeypatch.setattr(L, "CHECK_TARGETS", True)
    for kind, bad in (("ce", 25), ("ohem", -2), ("dice", -1), ("dice19", 19)):
        x, t = _batch(kind, (2, 3, 64, 96))
        m = _model(kind)
        crit = _criterion(kind)
        tb = t.clone()
        tb[1, 5, 7] = bad
        with pytest.raises(IndexError, match="Target %d is out of bounds" % bad):
            m.forward_loss_aux(x, tb, crit)
        loss = m.forward_loss_aux(x, t, crit)  # (CE / OHEM: t holds ignored pixels, -1)
        loss.backward()
        torch.cuda.synchronize()
        assert torch.isfinite(loss).all()


def _graph_worker(tmp_path, graphs):
    out = str(tmp_path / ("aux_%d.npz" % graphs))
    env = dict(os.environ)
    env.pop("FSCNN_GRAPHS", None)
    if graphs:
        env["FSCNN_GRAPHS"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_aux_head_worker.py"), out],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return dict(np.load(out))


def test_graph_replay_bit_identical(tmp_path):
    """Four CE and four OHEM steps (dropout seeds a, b, a, b; the last with another aux_weight)
    in a fresh process with and without FSCNN_GRAPHS=1 (tests/_aux_head_worker.py)."""
    ref = _graph_worker(tmp_path, 0)
    got = _graph_worker(tmp_path, 1)
    assert sorted(ref) == sorted(got)
    for k in ref:
        assert np.array_equal(ref[k], got[k]), k
    for kind in ("ce", "ohem"):
        g = [ref["%s_grad%d" % (kind, i)] for i in range(4)]
        ls = [ref["%s_loss%d" % (kind, i)] for i in range(4)]
        assert all(np.isfinite(v).all() for v in g)
        assert np.array_equal(g[0], g[2]) and ls[0] == ls[2]     # same seed, same step
        assert not np.array_equal(g[0], g[1])                    # the seed matters
        assert not np.array_equal(g[3], g[1]) and ls[3] != ls[1]  # and so does aux_weight


def test_ddp_delegation(tmp_path):
    """DistributedFastSCNN.forward_loss_aux: the wrapped model's loss and gradients, through the
    per-stage hook (one rank)."""
    import torch.distributed as dist
    from fast_scnn_pytorch_amd.ddp import DistributedFastSCNN
    x, t = _batch("ohem", GOLDEN_SHAPE)
    crit = _criterion("ohem")
    m0 = _model("ohem")
    l0 = m0.forward_loss_aux(x, t, crit)
    l0.backward()
    dist.init_process_group("gloo", init_method="file://%s" % (tmp_path / "store"), rank=0,
                            world_size=1)
    try:
        m = _model("ohem")
        ddp = DistributedFastSCNN(m)
        loss = ddp.forward_loss_aux(x, t, crit)
        loss.backward()
        torch.cuda.synchronize()
        assert [b[0] for b in ddp.bucket_log] == [0, 1, 2, 3]
    finally:
        dist.destroy_process_group()
    assert torch.equal(loss, l0)
    a = torch.cat([p.grad.flatten() for p in m0.parameters()])
    b = torch.cat([p.grad.flatten() for p in m.parameters()])
    torch.testing.assert_close(b, a, rtol=1e-6, atol=1e-6 * a.abs().max().item())
