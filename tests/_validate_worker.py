"""Worker for tests/test_gpu_validate.py (run in a fresh process, so that FSCNN_VAL_FUSED is set
for the whole process and the test process's environment stays as it is).  One
``FastSCNN.validate`` call with the CE criterion and a metric; saves the loss, the route taken,
the counters, and what they are compared with: ``cross_entropy(model(x)[0], t)``, the fp64
cross entropy of the same logits, and the counters of ``predict`` + ``SegmentationMetric``.

    python tests/_validate_worker.py OUT.npz
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(out):
    import numpy as np
    import torch
    import torch.nn.functional as F
    import _fscnn_boot
    _fscnn_boot.load()
    from fast_scnn_pytorch_amd import arch, portable_init
    from fast_scnn_pytorch_amd.loss import cross_entropy
    from fast_scnn_pytorch_amd.metric import SegmentationMetric
    from models.fast_scnn import FastSCNN

    dev = torch.device("cuda", 0)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in
          arch.portable_state_dict(19, seed=0, variant="bnrand").items()}
    m = FastSCNN(19)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    shape = (2, 3, 96, 160)
    x = torch.from_numpy(portable_init.input_tensor(3, shape)).to(dev)
    t = torch.from_numpy(portable_init.target_tensor(4, (2,) + shape[2:], 19, 0.1)).to(dev)
    metric = SegmentationMetric(19)
    loss = m.validate(x, t, metric=metric)
    ref = SegmentationMetric(19)
    ref.update(m.predict(x), t)
    with torch.no_grad():
        logits = m(x)[0]
        unfused = cross_entropy(logits, t)
        loss64 = F.cross_entropy(logits.double(), t, ignore_index=-1)
    torch.cuda.synchronize()
    np.savez(out, loss=np.float32(loss.item()), fused=np.int64(bool(m._last_validate_fused)),
             unfused_loss=np.float32(unfused.item()), loss64=np.float64(loss64.item()),
             counts=metric.counts(), ref_counts=ref.counts())


if __name__ == "__main__":
    main(sys.argv[1])
