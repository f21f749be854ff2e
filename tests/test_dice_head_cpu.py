"""CPU-side checks of the fused Dice / Focal+Dice loss head's boundary: the three C-ABI entry
points are declared, exported and bound; the head workspace query answers for training plans
only; and ``_head_spec`` resolves this package's criteria and objects with the reference's
attribute layout (utils/loss.py:12-124) alike.  No compute call is made (there is no GPU here)."""
import inspect
import os
import re
import subprocess

import pytest

from fast_scnn_pytorch_amd import _lib
from fast_scnn_pytorch_amd import loss as L
from fast_scnn_pytorch_amd.fast_scnn import _head_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fscnn_dice_head_ws_bytes", "fscnn_forward_loss_dice", "fscnn_backward_loss_dice")


def test_symbols_declared_exported_bound():
    src = open(os.path.join(ROOT, "include", "fastscnn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (fscnn_\w+)", out))
    for s in NEW:
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % s, src)
        assert m, "%s is not declared in include/fastscnn.h" % s
        assert s in exported, s
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s)
        # one ctypes argument per declared parameter
        assert len(_lib.SIGNATURES[s][1]) == len(m.group(1).split(",")), s
    assert _lib.SIGNATURES["fscnn_dice_head_ws_bytes"][0] is _lib.c_ll


def test_head_ws_bytes():
    from fast_scnn_pytorch_amd.fast_scnn import _Native
    lib = _lib.load()
    nat = _Native(2, False)
    sizes = {}
    for dt in (_lib.DT_F32, _lib.DT_BF16):
        p, fw, bw = nat.plan(2, 128, 256, dt, True)
        n = int(lib.fscnn_dice_head_ws_bytes(p))
        # two classes: (Ga, Gb, Gf) x (own row, spill) fp32 planes at 16 x 32 cells x 2 images,
        # and 4 partial sums per (low-res row, image); the plan's own sizes are unchanged by it
        assert n >= 2 * 3 * 4 * (2 * 16 * 32) + 4 * 4 * (2 * 16)
        assert n < fw
        sizes[dt] = n
        assert nat.plan(2, 128, 256, dt, True)[1:] == (fw, bw)
    assert sizes[_lib.DT_F32] == sizes[_lib.DT_BF16]  # the planes are fp32 for every plan dtype
    nat19 = _Native(19, False)
    p19, _, _ = nat19.plan(2, 128, 256, _lib.DT_BF16, True)
    assert int(lib.fscnn_dice_head_ws_bytes(p19)) >= 2 * 19 * 4 * (2 * 16 * 32)
    pe, _, _ = nat.plan(2, 128, 256, _lib.DT_F32, False)
    assert int(lib.fscnn_dice_head_ws_bytes(pe)) < 0
    assert b"train" in lib.fscnn_last_error()


class _Obj:
    pass


def _named(name, bases=(), **attrs):
    """A plain stand-in object whose class carries a utils/loss.py class name."""
    o = type(name, bases or (_Obj,), {})()
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def test_head_spec_package_criteria():
    assert _head_spec(None, 7) == ("ce", 7)
    assert _head_spec(L.DiceLoss(smooth=1e-3)) == ("dice", 1e-3, 1.0, 0.0, 0.5, 2.0)
    assert _head_spec(L.MixDiceLoss()) == ("dice", 1e-6, 1.0, 0.0, 0.5, 2.0)
    assert _head_spec(L.MixDiceLoss(aux=False, smooth=0.5)) == ("dice", 0.5, 1.0, 0.0, 0.5, 2.0)
    assert _head_spec(L.FocalDiceLoss(alpha=.25, gamma=1.5, dice_weight=.3)) == \
        ("dice", 1e-6, 0.3, 0.7, 0.25, 1.5)
    # the criterion's own ignore_index wins over the argument
    assert _head_spec(L.MixSoftmaxCrossEntropyLoss(ignore_label=255), -1) == ("ce", 255)
    with pytest.raises(RuntimeError, match="unfused"):
        _head_spec(L.MixSoftmaxCrossEntropyOHEMLoss(use_weight=False))
    with pytest.raises(RuntimeError, match="unfused"):
        _head_spec(object())


def test_head_spec_reference_layout():
    """utils/loss.py keeps FocalDiceLoss's smooth in .dice_loss and derives
    MixSoftmaxCrossEntropyLoss from nn.CrossEntropyLoss (.ignore_index)."""
    dice = _named("DiceLoss", smooth=2e-6)
    assert _head_spec(dice) == ("dice", 2e-6, 1.0, 0.0, 0.5, 2.0)
    mix = _named("MixDiceLoss", aux=True, aux_weight=0.4, dice_loss=dice)
    assert _head_spec(mix) == ("dice", 2e-6, 1.0, 0.0, 0.5, 2.0)
    fd = _named("FocalDiceLoss", alpha=0.5, gamma=2.0, dice_weight=0.5, dice_loss=dice)
    assert _head_spec(fd) == ("dice", 2e-6, 0.5, 0.5, 0.5, 2.0)
    ce = _named("MixSoftmaxCrossEntropyLoss", aux=False, aux_weight=0.2, ignore_index=-1)
    assert _head_spec(ce, 255) == ("ce", -1)
    base = type("SoftmaxCrossEntropyOHEMLoss", (_Obj,), {})
    with pytest.raises(RuntimeError, match="unfused"):
        _head_spec(_named("MixSoftmaxCrossEntropyOHEMLoss", (base,)))


def test_python_entry_points_take_criterion():
    from fast_scnn_pytorch_amd.ddp import DistributedFastSCNN
    from models.fast_scnn import FastSCNN
    for f in (FastSCNN.forward_loss, DistributedFastSCNN.forward_loss):
        ps = inspect.signature(f).parameters
        assert list(ps)[:4] == ["self", "x", "target", "ignore_index"]
        assert ps["ignore_index"].default == -1 and ps["criterion"].default is None

    class Probe:  # DistributedFastSCNN.forward_loss hands the criterion to its module
        def forward_loss(self, x, target, **kw):
            return kw

    d = DistributedFastSCNN.__new__(DistributedFastSCNN)
    object.__setattr__(d, "module", Probe())
    c = L.DiceLoss()
    assert d.forward_loss(1, 2, criterion=c) == {"ignore_index": -1, "criterion": c}
    assert d.forward_loss(1, 2, ignore_index=5) == {"ignore_index": 5, "criterion": None}
