"""CPU-side checks of the fused OHEM loss head's boundary: ``_ohem_spec`` resolves this package's
criteria and objects with the reference's attribute layout (utils/loss.py:127-206) alike, the
Python entry points exist with the documented signatures and refuse CPU tensors, and the C-ABI
entry point is declared, exported and bound.  No compute call is made (there is no GPU here)."""
import inspect
import os
import re
import subprocess

import pytest
import torch

from fast_scnn_pytorch_amd import _lib
from fast_scnn_pytorch_amd import loss as L
from fast_scnn_pytorch_amd.fast_scnn import _head_spec, _ohem_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = "fscnn_forward_loss_ohem"


class _Obj:
    pass


def _named(name, bases=(), **attrs):
    """A plain stand-in object whose class carries a utils/loss.py class name."""
    o = type(name, bases or (_Obj,), {})()
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def test_ohem_spec_package_criteria():
    c = L.SoftmaxCrossEntropyOHEMLoss(ignore_label=255, thresh=0.6, min_kept=1000)
    kind, ign, thresh, min_kept, w = _ohem_spec(c)
    assert (kind, ign, thresh, min_kept) == ("ohem", 255, 0.6, 1000)
    assert w is c.weight and tuple(w.shape) == (19,)
    m = L.MixSoftmaxCrossEntropyOHEMLoss(use_weight=False)
    assert _ohem_spec(m) == ("ohem", -1, 0.7, 256, None)
    assert _ohem_spec(L.MixSoftmaxCrossEntropyOHEMLoss(aux=True, ignore_index=7))[1] == 7


def test_ohem_spec_reference_layout():
    """utils/loss.py keeps the class weights in the inner nn.CrossEntropyLoss (.criterion)."""
    w = torch.arange(19, dtype=torch.float32)
    inner = torch.nn.CrossEntropyLoss(weight=w, ignore_index=-1)
    base = type("SoftmaxCrossEntropyOHEMLoss", (_Obj,), {})
    mix = _named("MixSoftmaxCrossEntropyOHEMLoss", (base,), ignore_label=-1, thresh=0.7,
                 min_kept=256, criterion=inner, aux=False, aux_weight=0.2)
    spec = _ohem_spec(mix)
    assert spec[:4] == ("ohem", -1, 0.7, 256) and torch.equal(spec[4], w)
    plain = _named("SoftmaxCrossEntropyOHEMLoss", ignore_label=3, thresh=0.5, min_kept=0,
                   criterion=torch.nn.CrossEntropyLoss(ignore_index=3))
    assert _ohem_spec(plain) == ("ohem", 3, 0.5, 0, None)


def test_ohem_spec_refuses_everything_else():
    for c in (object(), L.DiceLoss(), L.MixSoftmaxCrossEntropyLoss(), None):
        with pytest.raises(RuntimeError, match="OHEM"):
            _ohem_spec(c)
    with pytest.raises(RuntimeError, match="attributes"):
        _ohem_spec(_named("SoftmaxCrossEntropyOHEMLoss", thresh=0.7))  # the name alone
    # forward_loss keeps refusing the criterion, and may now name the new entry
    with pytest.raises(RuntimeError, match="unfused"):
        _head_spec(L.MixSoftmaxCrossEntropyOHEMLoss(use_weight=False))


def test_python_entry_points():
    from fast_scnn_pytorch_amd.ddp import DistributedFastSCNN
    from models.fast_scnn import FastSCNN
    for f in (FastSCNN.forward_loss_ohem, DistributedFastSCNN.forward_loss_ohem):
        assert list(inspect.signature(f).parameters) == ["self", "x", "target", "criterion"]

    class Probe:  # DistributedFastSCNN.forward_loss_ohem hands everything to its module
        def forward_loss_ohem(self, x, target, criterion):
            return (x, target, criterion)

    d = DistributedFastSCNN.__new__(DistributedFastSCNN)
    object.__setattr__(d, "module", Probe())
    c = L.MixSoftmaxCrossEntropyOHEMLoss(use_weight=False)
    assert d.forward_loss_ohem(1, 2, c) == (1, 2, c)


def test_cpu_tensors_and_foreign_criteria_refused():
    from models.fast_scnn import FastSCNN
    m = FastSCNN(2).train()
    x = torch.zeros(2, 3, 64, 64)
    t = torch.zeros(2, 64, 64, dtype=torch.long)
    with pytest.raises(RuntimeError, match="ROCm device tensors"):
        m.forward_loss_ohem(x, t, L.MixSoftmaxCrossEntropyOHEMLoss(use_weight=False))
    with pytest.raises(RuntimeError, match="OHEM"):
        m.forward_loss_ohem(x, t, L.DiceLoss())
    with pytest.raises(RuntimeError, match="train"):
        m.eval().forward_loss_ohem(x, t, L.MixSoftmaxCrossEntropyOHEMLoss(use_weight=False))


def test_symbol_declared_exported_bound():
    src = open(os.path.join(ROOT, "include", "fastscnn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (fscnn_\w+)", out))
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % SYM, src)
    assert m, "%s is not declared in include/fastscnn.h" % SYM
    assert SYM in exported
    assert SYM in _lib.SIGNATURES
    assert hasattr(lib, SYM)
    # one ctypes argument per declared parameter
    assert len(_lib.SIGNATURES[SYM][1]) == len(m.group(1).split(","))
