"""Worker for tests/test_gpu_aux_head.py::test_graph_replay_bit_identical (run in a fresh process:
the executor reads FSCNN_GRAPHS once per process).  Four fp32 train steps of FastSCNN(19, aux=True)
through ``forward_loss_aux`` with the CE criterion and four with the OHEM criterion (class weights
on), Dropout(0.1) active with dropout seeds 5, 9, 5, 9; the last step of each uses aux_weight 0.7
instead of 0.4.  Saves every step's loss, unweighted terms and flat gradient arena, and the final
running statistics.

    python tests/_aux_head_worker.py OUT.npz
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(out):
    import numpy as np
    import torch
    import _fscnn_boot
    _fscnn_boot.load()
    from fast_scnn_pytorch_amd import arch, portable_init
    from fast_scnn_pytorch_amd.loss import (MixSoftmaxCrossEntropyLoss,
                                            MixSoftmaxCrossEntropyOHEMLoss)
    from models.fast_scnn import FastSCNN

    dev = torch.device("cuda", 0)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in
          arch.portable_state_dict(19, True, 0, "bnrand").items()}
    shape = (2, 3, 96, 160)
    x = torch.from_numpy(portable_init.input_tensor(3, shape)).to(dev)
    t = torch.from_numpy(portable_init.target_tensor(4, (2,) + shape[2:], 19, 0.05)).to(dev)
    res = {}
    for kind in ("ce", "ohem"):
        m = FastSCNN(19, aux=True)
        m.load_state_dict(sd)
        m = m.to(dev).train()
        crits = {}
        for w in (0.4, 0.7):
            crits[w] = (MixSoftmaxCrossEntropyLoss(aux=True, aux_weight=w) if kind == "ce" else
                        MixSoftmaxCrossEntropyOHEMLoss(aux=True, aux_weight=w))
        for i, seed in enumerate((5, 9, 5, 9)):
            m.zero_grad(set_to_none=True)
            m._dropout_seed = seed
            loss = m.forward_loss_aux(x, t, crits[0.7 if i == 3 else 0.4])
            loss.backward()
            torch.cuda.synchronize()
            res["%s_loss%d" % (kind, i)] = np.float32(loss.item())
            res["%s_terms%d" % (kind, i)] = m._last_loss_terms.cpu().numpy()
            res["%s_grad%d" % (kind, i)] = torch.cat(
                [p.grad.reshape(-1) for p in m.parameters()]).cpu().numpy()
        for k, v in m.state_dict().items():
            if "running" in k:
                res["%s_bn.%s" % (kind, k)] = v.cpu().numpy()
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1])
