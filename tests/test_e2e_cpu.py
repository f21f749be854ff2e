"""CPU-side checks of the deployment pipeline (EndToEndFastSCNN, export_onnx_fixed.py:34-98): the
wrapper's state_dict schema and argument errors, and the pin of the GPU tests' yardstick -- a
short fp64 restatement of the pipeline on the oracle forward -- to the probabilities the
reference wrapper itself produced (tests/golden/e2e_*.npz, tools/gen_e2e_golden.py)."""
import numpy as np
import pytest
import torch

import e2e_ref
import helpers
from fast_scnn_pytorch_amd.deploy import EndToEndFastSCNN
from models.fast_scnn import FastSCNN
from oracle import fast_scnn_ref as ref


@pytest.mark.parametrize("nc", e2e_ref.CLASSES)
def test_state_dict_keys_match_the_reference_wrapper(nc):
    schema = helpers.load_golden("e2e_schema")
    m = EndToEndFastSCNN(FastSCNN(nc), mean=e2e_ref.MEAN, std=e2e_ref.STD)
    assert list(m.state_dict()) == [str(k) for k in schema["c%d_norm" % nc]]
    assert m.preprocessor.mean.shape == (1, 3, 1, 1) and m.preprocessor.std.shape == (1, 3, 1, 1)
    plain = EndToEndFastSCNN(FastSCNN(nc))
    assert list(plain.state_dict()) == [str(k) for k in schema["c%d_plain" % nc]]
    assert plain.preprocessor.mean is None and plain.preprocessor.std is None
    # mean without std registers nothing, as in the reference
    assert list(EndToEndFastSCNN(FastSCNN(nc), mean=e2e_ref.MEAN).state_dict()) == \
        list(plain.state_dict())
    # loads from and into a state dict with the reference's keys
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    sd["preprocessor.mean"] += 0.25
    m.load_state_dict(sd)
    assert torch.equal(m.preprocessor.mean, sd["preprocessor.mean"])


def test_constructor_follows_the_reference_signature():
    bb = FastSCNN(2)
    m = EndToEndFastSCNN(bb, (320, 180), 512, e2e_ref.MEAN, e2e_ref.STD, False)
    assert m.backbone is bb and m.input_size == (320, 180) and m.base_size == 512
    assert m.apply_softmax is False and m.dtype == torch.float32
    assert m.channels_last is False and m.bgr is False
    d = EndToEndFastSCNN(bb)
    assert d.input_size == (640, 360) and d.base_size == 1024 and d.apply_softmax is True
    h = EndToEndFastSCNN(bb, dtype=torch.float16, channels_last=True, bgr=True)
    assert h.dtype == torch.float16 and h.channels_last and h.bgr


def test_argument_errors():
    bb = FastSCNN(2)
    with pytest.raises(RuntimeError):
        EndToEndFastSCNN(bb, base_size=31)
    with pytest.raises(RuntimeError):
        EndToEndFastSCNN(bb, dtype=torch.float64)
    m = EndToEndFastSCNN(bb, input_size=(48, 32), base_size=64)
    frames = torch.zeros(1, 3, 32, 48, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="eval"):  # a fresh module is in train mode
        m(frames)
    with pytest.raises(RuntimeError, match="eval"):
        m.predict(frames)
    m.eval()
    assert not bb.training
    with pytest.raises(RuntimeError, match="device"):  # CPU tensors: there is no fallback
        m(frames)
    with pytest.raises(RuntimeError, match="device"):
        m.predict(frames, scale=255)


@pytest.mark.parametrize("nc", e2e_ref.CLASSES)
@pytest.mark.parametrize("case", e2e_ref.CASES)
def test_fp64_restatement_reproduces_the_reference(case, nc):
    """The yardstick of tests/test_gpu_e2e.py, F.interpolate / softmax around oracle.forward in
    fp64, gives the reference wrapper's stored fp32 probabilities to 1e-5 (the reference's own fp32
    result is within 8e-6 of fp64 on these cases), the stored fp64 argmax wherever the margin
    exceeds 1e-4, and the stored margins."""
    g = e2e_ref.fixture(case, nc)
    size, base, mean, std = e2e_ref.geometry(g)
    with torch.no_grad():
        x = e2e_ref.pre_ref(g["frames"], base, mean, std, torch.float64)
        lg = ref.forward(e2e_ref.weights(nc, torch.float64), x, nc)[0][0]
        rs = e2e_ref.tail_ref(lg, size, softmax=False)
        probs = torch.softmax(rs, 1)
    assert probs.shape == (3, nc, size[1], size[0])
    got = probs.numpy()
    if "probs_idx" in g:
        got = got.ravel()[g["probs_idx"]]
    err = np.abs(got - g["probs"]).max()
    print("%s C=%d: fp64 restatement vs stored fp32 probabilities %.2e" % (case, nc, err))
    assert err <= 1e-5
    srt = torch.sort(rs, dim=1).values
    margin = (srt[:, -1] - srt[:, -2]).numpy()
    assert np.abs(margin - g["margin"]).max() <= 1e-5
    sure = g["margin"] > 1e-4
    assert (rs.argmax(1).numpy() == g["argmax"])[sure].all()
    assert 1.0 - sure.mean() <= 0.001
