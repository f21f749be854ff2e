"""Shared by the deployment-pipeline tests: the fixture cases and a short restatement of the
reference pipeline (export_onnx_fixed.py:34-98) in torch ops, evaluated in any dtype."""
import functools

import torch
import torch.nn.functional as F

import helpers

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
CASES = ["80x48", "200x70", "61x45", "50x40_to_37x33", "128x128"]
CLASSES = [2, 19]


@functools.lru_cache(maxsize=None)
def fixture(case, nc):
    g = helpers.load_golden("e2e_%s_c%d" % (case, nc))
    g["frames"] = torch.from_numpy(g["frames"])
    return g


def geometry(g):
    """(input_size (W, H), base_size, mean, std) of a fixture."""
    norm = bool(int(g["norm"]))
    return (tuple(int(v) for v in g["input_size"]), int(g["base_size"]),
            MEAN if norm else None, STD if norm else None)


@functools.lru_cache(maxsize=None)
def weights(nc, dtype=torch.float32):
    return helpers.golden_sd(helpers.load_golden(str(fixture(CASES[0], nc)["weights"])), dtype)


def pre_ref(frames, base, mean, std, dtype):
    """EndToEndPreprocessing.forward in ``dtype``; mean / std are the wrapper's fp32 buffers."""
    x = frames.to(dtype)
    if x.shape[2] != base or x.shape[3] != base:
        x = F.interpolate(x, size=(base, base), mode="bilinear", align_corners=False)
    x = x / 255.0
    if mean is not None and std is not None:
        x = (x - torch.tensor(mean).view(1, 3, 1, 1).to(dtype)) / \
            torch.tensor(std).view(1, 3, 1, 1).to(dtype)
    return x


def tail_ref(logits, size, softmax=True):
    """The wrapper's resize back to ``size`` = (W, H) and softmax, in the dtype of ``logits``."""
    y = logits
    if y.shape[2] != size[1] or y.shape[3] != size[0]:
        y = F.interpolate(y, size=(size[1], size[0]), mode="bilinear", align_corners=False)
    return F.softmax(y, dim=1) if softmax else y


def half_ulp(ref, dtype):
    """Half a unit in the last place of ``dtype`` at the magnitude of each element of ``ref``."""
    p, emin = {torch.float32: (24, -126), torch.float16: (11, -14), torch.bfloat16: (8, -126)}[dtype]
    e = torch.frexp(ref.double().abs())[1].double() - 1.0  # floor(log2 |ref|)
    e = torch.clamp(e, min=float(emin))
    return torch.pow(2.0, e - p)
