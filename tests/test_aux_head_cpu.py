"""CPU-side checks of the fused aux loss heads' boundary (FastSCNN.forward_loss_aux,
fscnn_forward_loss_aux / fscnn_backward_loss_aux): ``_aux_head_spec`` resolves this package's
two-output criteria and objects with the reference's attribute layout (utils/loss.py:42-68,
103-124, 179-206) alike and refuses everything else, the head buffer's size query answers for
plans (host-side tables), and both run entries refuse null arguments before any HIP call.  No
compute call is made (there is no GPU here)."""
import ctypes
import inspect

import pytest
import torch

from fast_scnn_pytorch_amd import _lib
from fast_scnn_pytorch_amd import loss as L
from fast_scnn_pytorch_amd.fast_scnn import _aux_head_spec

F32, BF16, F16 = _lib.DT_F32, _lib.DT_BF16, _lib.DT_F16
X = _lib.c_vp(0x1000)   # a non-null pointer no refused call may touch
E_INVALID = -1


class _Obj:
    pass


def _named(name, bases=(), **attrs):
    """A plain stand-in object whose class carries a utils/loss.py class name."""
    o = type(name, bases or (_Obj,), {})()
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def test_aux_head_spec_package_criteria():
    assert _aux_head_spec(L.MixSoftmaxCrossEntropyLoss(aux=True, aux_weight=0.4,
                                                       ignore_label=255)) == ("ce", 0.4, 255)
    assert _aux_head_spec(L.MixSoftmaxCrossEntropyLoss()) == ("ce", 0.2, -1)
    assert _aux_head_spec(L.MixDiceLoss(aux=True, aux_weight=0.4, smooth=1e-3)) == \
        ("dice", 0.4, 1e-3)
    c = L.MixSoftmaxCrossEntropyOHEMLoss(aux=True, aux_weight=0.3, ignore_index=7, thresh=0.6,
                                         min_kept=1000)
    spec = _aux_head_spec(c)
    assert spec[:5] == ("ohem", 0.3, 7, 0.6, 1000)
    assert spec[5] is c.weight and tuple(spec[5].shape) == (19,)
    assert _aux_head_spec(L.MixSoftmaxCrossEntropyOHEMLoss(aux=True, use_weight=False)) == \
        ("ohem", 0.2, -1, 0.7, 256, None)


def test_aux_head_spec_reference_layout():
    """utils/loss.py: MixSoftmaxCrossEntropyLoss is an nn.CrossEntropyLoss (ignore_index),
    MixDiceLoss keeps smooth in .dice_loss, the OHEM criterion its class weights in the inner
    nn.CrossEntropyLoss (.criterion)."""
    ce = _named("MixSoftmaxCrossEntropyLoss", (torch.nn.CrossEntropyLoss,), aux=True,
                aux_weight=0.4)
    ce.ignore_index = 3
    assert _aux_head_spec(ce) == ("ce", 0.4, 3)
    dice = _named("MixDiceLoss", aux=True, aux_weight=0.4,
                  dice_loss=_named("DiceLoss", smooth=1e-6))
    assert _aux_head_spec(dice) == ("dice", 0.4, 1e-6)
    w = torch.arange(19, dtype=torch.float32)
    inner = torch.nn.CrossEntropyLoss(weight=w, ignore_index=-1)
    base = type("SoftmaxCrossEntropyOHEMLoss", (_Obj,), {})
    ohem = _named("MixSoftmaxCrossEntropyOHEMLoss", (base,), ignore_label=-1, thresh=0.7,
                  min_kept=256, criterion=inner, aux=True, aux_weight=0.4)
    spec = _aux_head_spec(ohem)
    assert spec[:5] == ("ohem", 0.4, -1, 0.7, 256) and torch.equal(spec[5], w)


def test_aux_head_spec_refusals():
    refused = [L.MixSoftmaxCrossEntropyLoss(aux=False), L.MixDiceLoss(aux=False),
               L.MixSoftmaxCrossEntropyOHEMLoss(aux=False, use_weight=False),
               L.FocalDiceLoss(), L.DiceLoss(), L.SoftmaxCrossEntropyOHEMLoss(use_weight=False),
               object(), None, torch.nn.CrossEntropyLoss()]
    for c in refused:
        with pytest.raises(RuntimeError, match="unfused"):
            _aux_head_spec(c)
    with pytest.raises(RuntimeError, match="aux=False"):
        _aux_head_spec(L.MixDiceLoss(aux=False))
    with pytest.raises(RuntimeError, match="attributes"):
        _aux_head_spec(_named("MixDiceLoss", aux=True))  # the name alone


def test_python_entry_points():
    from fast_scnn_pytorch_amd.ddp import DistributedFastSCNN
    from models.fast_scnn import FastSCNN
    for f in (FastSCNN.forward_loss_aux, DistributedFastSCNN.forward_loss_aux):
        assert list(inspect.signature(f).parameters) == ["self", "x", "target", "criterion"]

    class Probe:  # DistributedFastSCNN.forward_loss_aux hands everything to its module
        def forward_loss_aux(self, x, target, criterion):
            return (x, target, criterion)

    d = DistributedFastSCNN.__new__(DistributedFastSCNN)
    object.__setattr__(d, "module", Probe())
    c = L.MixDiceLoss()
    assert d.forward_loss_aux(1, 2, c) == (1, 2, c)


def test_cpu_tensors_and_wrong_models_refused():
    from models.fast_scnn import FastSCNN
    x = torch.zeros(2, 3, 64, 64)
    t = torch.zeros(2, 64, 64, dtype=torch.long)
    m = FastSCNN(2, aux=True).train()
    with pytest.raises(RuntimeError, match="ROCm device tensors"):
        m.forward_loss_aux(x, t, L.MixDiceLoss())
    with pytest.raises(RuntimeError, match="unfused"):
        m.forward_loss_aux(x, t, L.FocalDiceLoss())
    with pytest.raises(RuntimeError, match="train"):
        m.eval().forward_loss_aux(x, t, L.MixDiceLoss())
    with pytest.raises(RuntimeError, match="unfused"):
        FastSCNN(2).train().forward_loss_aux(x, t, L.MixDiceLoss())  # no aux head


@pytest.fixture(scope="module")
def nets():
    lib = _lib.load()
    hs = {}
    for nc, aux in ((19, 1), (19, 0)):
        h = _lib.c_vp()
        _lib.check(lib.fscnn_net_create(nc, aux, ctypes.byref(h)), "fscnn_net_create")
        hs[(nc, aux)] = h
    yield hs
    for h in hs.values():
        lib.fscnn_net_destroy(h)


def _plan(net, N, H, W, dt, train):
    p = _lib.c_vp()
    _lib.check(_lib.load().fscnn_plan_create(net, N, H, W, dt, train, ctypes.byref(p)),
               "fscnn_plan_create")
    return p


@pytest.mark.parametrize("dt", [F32, BF16, F16])
@pytest.mark.parametrize("N,H,W", [(2, 96, 160), (3, 64, 96)])
def test_aux_head_ws_bytes(nets, N, H, W, dt):
    lib = _lib.load()
    plan = _plan(nets[(19, 1)], N, H, W, dt, 1)
    try:
        ce, dice, ohem = (lib.fscnn_aux_head_ws_bytes(plan, h) for h in (0, 1, 2))
        assert ce > 0 and dice > 0 and ohem > 0
        assert ce % 256 == 0 and dice % 256 == 0 and ohem % 256 == 0
        # OHEM: the CE head's buffers plus two fp32 planes at the input resolution
        assert ohem >= ce + 2 * N * H * W * 4
        assert lib.fscnn_aux_head_ws_bytes(plan, 7) < 0
        assert b"head 7" in lib.fscnn_last_error()
        assert lib.fscnn_aux_head_ws_bytes(plan, -1) < 0
    finally:
        lib.fscnn_plan_destroy(plan)


def test_aux_head_ws_bytes_refuses_other_plans(nets):
    lib = _lib.load()
    for net, train in ((nets[(19, 0)], 1), (nets[(19, 1)], 0), (nets[(19, 1)], 2)):
        plan = _plan(net, 2, 96, 160, F32, train)
        try:
            assert lib.fscnn_aux_head_ws_bytes(plan, 0) < 0
            assert b"fscnn_aux_head_ws_bytes" in lib.fscnn_last_error()
        finally:
            lib.fscnn_plan_destroy(plan)
    assert lib.fscnn_aux_head_ws_bytes(None, 0) < 0


def _fwd(plan, h, x=X, target=X, loss_out=X, head_ws=X):
    hp = ctypes.byref(h) if h is not None else None
    return ("fscnn_forward_loss_aux",
            (plan, x, F32, target, hp, loss_out, X, X, X, X, head_ws, 0, 0.1, 0.1, None))


def _bwd(plan, h, x=X, grad_loss=X, head_ws=X):
    hp = ctypes.byref(h) if h is not None else None
    return ("fscnn_backward_loss_aux",
            (plan, grad_loss, hp, x, F32, None, F32, X, X, X, X, head_ws, 0, 0.1, 0, 3, None))


def test_run_entries_refuse_before_any_launch(nets):
    lib = _lib.load()
    plan = _plan(nets[(19, 1)], 2, 96, 160, F32, 1)
    plain = _plan(nets[(19, 0)], 2, 96, 160, F32, 1)
    h = _lib.AuxHead(head=0, aux_weight=0.4, ignore_index=-1)
    bad_head = _lib.AuxHead(head=7, aux_weight=0.4, ignore_index=-1)
    bad_kept = _lib.AuxHead(head=2, aux_weight=0.4, ignore_index=-1, thresh=0.7, min_kept=-1)
    cases = [_fwd(plan, h, x=None), _fwd(plan, h, target=None), _fwd(plan, h, loss_out=None),
             _fwd(plan, h, head_ws=None), _fwd(plan, None), _fwd(None, h),
             _fwd(plan, bad_head), _fwd(plan, bad_kept), _fwd(plain, h),
             _bwd(plan, h, x=None), _bwd(plan, h, grad_loss=None), _bwd(plan, h, head_ws=None),
             _bwd(plan, None), _bwd(None, h), _bwd(plan, bad_head), _bwd(plain, h)]
    try:
        for name, args in cases:
            rc = getattr(lib, name)(*args)
            assert rc == E_INVALID, (name, args, rc)
            assert name.encode() in lib.fscnn_last_error(), lib.fscnn_last_error()
    finally:
        lib.fscnn_plan_destroy(plan)
        lib.fscnn_plan_destroy(plain)


def test_aux_dice_head_is_plain_dice(nets):
    """fscnn_aux_head.focal_weight != 0 (a two-output Focal+Dice, which the reference does not
    have) is refused with E_UNSUPPORTED before any launch, by both run entries."""
    lib = _lib.load()
    plan = _plan(nets[(19, 1)], 2, 96, 160, F32, 1)
    h = _lib.AuxHead(head=1, aux_weight=0.4, ignore_index=-1, smooth=1e-6, dice_weight=0.5,
                     focal_weight=0.5, alpha=0.5, gamma=2.0)
    try:
        for name, args in (_fwd(plan, h), _bwd(plan, h)):
            assert getattr(lib, name)(*args) == -2
            assert b"focal_weight" in lib.fscnn_last_error()
    finally:
        lib.fscnn_plan_destroy(plan)


def test_existing_entries_keep_refusing_aux_plans(nets):
    """fscnn_forward_loss on an aux plan: still "main output only", E_UNSUPPORTED, no launch."""
    lib = _lib.load()
    plan = _plan(nets[(19, 1)], 2, 96, 160, F32, 1)
    try:
        rc = lib.fscnn_forward_loss(plan, X, F32, X, -1, X, X, X, X, X, 0, 0.1, 0.1, None)
        assert rc == -2
        assert b"main output only" in lib.fscnn_last_error()
    finally:
        lib.fscnn_plan_destroy(plan)
