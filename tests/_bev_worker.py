"""Worker for tests/test_gpu_bev.py, run in a fresh process with FSCNN_E2E_FUSED set by the
caller: one fp32 ``bird_eye`` call and one ``predict`` call (scale 255, batch 3) on a fixture
case at the corrected calibration's 208 x 108 view, saved with the route each of them took.

    python tests/_bev_worker.py OUT.npz CASE NUM_CLASSES
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(out, case, nc):
    import numpy as np
    import torch
    import _fscnn_boot
    _fscnn_boot.load()
    import e2e_ref
    from fast_scnn_pytorch_amd import bev
    from fast_scnn_pytorch_amd.deploy import EndToEndFastSCNN
    from models.fast_scnn import FastSCNN

    dev = torch.device("cuda", 0)
    g = e2e_ref.fixture(case, nc)
    size, base, mean, std = e2e_ref.geometry(g)
    bb = FastSCNN(nc)
    bb.load_state_dict(e2e_ref.weights(nc))
    e2e = EndToEndFastSCNN(bb, input_size=size, base_size=base, mean=mean, std=std).to(dev).eval()
    frames = g["frames"][:3].to(dev)
    vp = bev.BirdEyeView().params(1, 0.1, True, source_size=size)[3]
    mask, rows = e2e.bird_eye(frames, vp, scale=255, min_width=10)
    fused = e2e._last_fused
    labels = e2e.predict(frames, scale=255)
    torch.cuda.synchronize()
    np.savez(out, mask=mask.cpu().numpy(), rows=rows.cpu().numpy(), labels=labels.cpu().numpy(),
             fused=np.array(bool(fused)), predict_fused=np.array(bool(e2e._last_fused)))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], int(sys.argv[3]))
