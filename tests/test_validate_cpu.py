"""CPU-side checks of ``FastSCNN.validate``'s boundary: the two C-ABI entry points are declared,
exported and bound with matching argument counts; the workspace query answers for inference
plans only; the method refuses CPU tensors; ``_head_spec`` still refuses the OHEM criterion
(validate catches that and takes the unfused route); ``SegmentationMetric.device_counts`` is
additive.  No compute call is made (there is no GPU here)."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from fast_scnn_pytorch_amd import _lib
from fast_scnn_pytorch_amd import loss as L
from fast_scnn_pytorch_amd.fast_scnn import _head_spec
from fast_scnn_pytorch_amd.metric import SegmentationMetric

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fscnn_validate", "fscnn_validate_ws_bytes")


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
    assert _lib.SIGNATURES["fscnn_validate_ws_bytes"][0] is _lib.c_ll


def test_validate_ws_bytes():
    from fast_scnn_pytorch_amd.fast_scnn import _Native
    lib = _lib.load()
    nat = _Native(19, False)
    pe, fw, bw = nat.plan(2, 128, 256, _lib.DT_F32, False)
    n = int(lib.fscnn_validate_ws_bytes(pe))
    # four fp32 partial sums per workgroup, at least one workgroup per image; far below 1 MiB
    assert 4 * 4 * 2 <= n < (1 << 20)
    assert nat.plan(2, 128, 256, _lib.DT_F32, False)[1:] == (fw, bw)  # the plan is unchanged
    p16, _, _ = nat.plan(2, 128, 256, _lib.DT_BF16, False)
    assert int(lib.fscnn_validate_ws_bytes(p16)) == n  # fp32 records for every plan dtype
    pt, _, _ = nat.plan(2, 128, 256, _lib.DT_F32, True)
    assert int(lib.fscnn_validate_ws_bytes(pt)) < 0
    assert b"inference" in lib.fscnn_last_error()


def test_validate_refuses_cpu_tensors():
    from models.fast_scnn import FastSCNN
    m = FastSCNN(19).eval()
    with pytest.raises(RuntimeError):
        m.validate(torch.zeros(1, 3, 64, 64), torch.zeros(1, 64, 64, dtype=torch.long))
    with pytest.raises(RuntimeError, match="eval"):
        m.train().validate(torch.zeros(2, 3, 64, 64), torch.zeros(2, 64, 64, dtype=torch.long))


def test_validate_signature():
    from models.fast_scnn import FastSCNN
    ps = inspect.signature(FastSCNN.validate).parameters
    assert list(ps) == ["self", "x", "target", "criterion", "metric", "ignore_index"]
    assert ps["criterion"].default is None and ps["metric"].default is None
    assert ps["ignore_index"].default == -1
    assert FastSCNN(2)._last_validate_fused is None


def test_head_spec_still_refuses_ohem():
    with pytest.raises(RuntimeError, match="unfused"):
        _head_spec(L.MixSoftmaxCrossEntropyOHEMLoss(use_weight=False))
    assert _head_spec(None, 255) == ("ce", 255)
    assert _head_spec(L.MixDiceLoss(aux=True, aux_weight=0.4))[0] == "dice"


def test_metric_device_counts_is_additive():
    m = SegmentationMetric(3)
    assert np.array_equal(m.counts(), np.zeros(11, dtype=np.int64))
    c = m.device_counts("cpu")
    assert c.dtype == torch.int64 and tuple(c.shape) == (11,) and int(c.sum()) == 0
    assert m.device_counts("cpu") is c  # allocated once
    c[0] += 5
    c[1] += 7
    assert m.counts()[0] == 5 and abs(m.get()[0] - 5.0 / 7.0) < 1e-12
    m.reset()
    assert np.array_equal(m.counts(), np.zeros(11, dtype=np.int64))
