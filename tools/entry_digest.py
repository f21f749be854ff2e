#!/usr/bin/env python3
"""Digest every FastSCNN entry point's results, to compare two trees bit for bit (needs the GPU).

    python tools/entry_digest.py [--out FILE]

Uses only the public API and the private hooks the tests use (``_dropout_seed``,
``grad_stage_hook``), so the same file runs on any revision.  Prints one line per case: its name
and the SHA-256 of, concatenated, the loss / output bytes, every parameter gradient, the input
gradient where one is requested, and the running-statistics arena and ``num_batches_tracked``
after the call.  Every case starts from ``torch.manual_seed(0)`` with the dropout seed pinned to
1234 at the default p, so the mask path is live; ``*/drawn_seed`` leaves the seed to the global
CPU generator and digests the generator's state as well.

Cases run at N=2, 64x64 with 2 and 19 classes; the train cases also at the ragged N=3, 72x104.
Two runs of one tree in fresh processes are expected to agree on every line (train steps are
byte-stable run to run); a refactor of the host path must reproduce every line.
"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SMALL, RAGGED = (2, 3, 64, 64), (3, 3, 72, 104)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()

    import numpy as np
    import torch
    import _fscnn_boot
    _fscnn_boot.load()
    from fast_scnn_pytorch_amd import arch, portable_init
    from fast_scnn_pytorch_amd.loss import (DiceLoss, FocalDiceLoss, MixDiceLoss,
                                            MixSoftmaxCrossEntropyLoss,
                                            MixSoftmaxCrossEntropyOHEMLoss,
                                            SoftmaxCrossEntropyOHEMLoss)
    from fast_scnn_pytorch_amd.metric import SegmentationMetric
    from models.fast_scnn import FastSCNN

    if not torch.cuda.is_available():
        raise SystemExit("entry_digest: no GPU visible")
    dev = torch.device("cuda", 0)
    f32, bf16 = torch.float32, torch.bfloat16
    lines = []
    sds = {}

    def model(nc, aux, train=True):
        if (nc, aux) not in sds:
            sds[nc, aux] = {k: torch.from_numpy(np.asarray(v)) for k, v in
                            arch.portable_state_dict(nc, aux, 0, "bnrand").items()}
        m = FastSCNN(nc, aux=aux)
        m.load_state_dict(sds[nc, aux])
        m = m.to(dev)
        m.train(train)
        m._dropout_seed = 1234
        return m

    def batch(shape, nc, dt=f32, ignore=0.05):
        N, _, H, W = shape
        x = torch.from_numpy(portable_init.input_tensor(31, tuple(shape))).to(dev).to(dt)
        t = torch.from_numpy(portable_init.target_tensor(32, (N, H, W), nc, ignore_frac=ignore))
        return x, t.to(dev)

    def raw(t):
        if t is None:
            return b"<none>"
        if not isinstance(t, torch.Tensor):
            return repr(t).encode()
        return t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy().tobytes()

    def emit(name, m, results, x=None, extra=()):
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in results:
            h.update(raw(t))
        for p in m.parameters():
            h.update(raw(p.grad))
        if x is not None:
            h.update(raw(x.grad))
        ar = m.arena()
        h.update(raw(ar["R"]))
        h.update(raw(ar["NBT"]))
        for t in extra:
            h.update(raw(t))
        line = "%-44s %s" % (name, h.hexdigest())
        print(line, flush=True)
        lines.append(line)

    def tag(shape, nc, dt=None):
        s = "%dx%dx%d/c%d" % (shape[0], shape[2], shape[3], nc)
        return s if dt is None else s + "/" + str(dt).split(".")[-1]

    def ohem_crit(cls, nc, weights, **kw):
        c = cls(use_weight=weights and nc == 19, **kw)
        if weights and nc != 19:  # a CPU tensor, like the criterion's own: the weight cache runs
            c.weight = torch.linspace(0.8, 1.2, nc, dtype=torch.float32)
        return c

    train_cfgs = [(SMALL, 2, f32), (SMALL, 19, f32), (RAGGED, 2, f32), (RAGGED, 19, f32),
                  (RAGGED, 19, bf16)]

    # 1. train forward + unfused criterion backward
    for shape in (SMALL, RAGGED):
        for nc in (2, 19):
            for aux in (False, True):
                for arith in ("fp32", "bf16", "ac16"):
                    torch.manual_seed(0)
                    m = model(nc, aux)
                    x, t = batch(shape, nc, bf16 if arith == "bf16" else f32)
                    crit = MixSoftmaxCrossEntropyLoss(aux=aux, aux_weight=0.4)
                    with torch.autocast("cuda", dtype=torch.float16, enabled=arith == "ac16"):
                        outs = m(x)
                        loss = crit(outs, t)
                    loss.backward()
                    emit("train/%s/aux%d/%s" % (tag(shape, nc), int(aux), arith), m,
                         tuple(outs) + (loss,))

    # 2. eval-mode forward with an input gradient (the recompute path + dx)
    for nc in (2, 19):
        for aux in (False, True):
            torch.manual_seed(0)
            m = model(nc, aux, train=False)
            x, t = batch(SMALL, nc)
            x.requires_grad_()
            outs = m(x)
            loss = MixSoftmaxCrossEntropyLoss(aux=aux, aux_weight=0.4)(outs, t)
            loss.backward()
            emit("evalgrad/%s/aux%d" % (tag(SMALL, nc, f32), int(aux)), m, tuple(outs) + (loss,), x)

    # 3. forward_loss
    for shape, nc, dt in train_cfgs:
        for kind in ("none", "mixce", "ce_dx", "dice", "focaldice"):
            torch.manual_seed(0)
            m = model(nc, False)
            dice = kind in ("dice", "focaldice")
            x, t = batch(shape, nc, dt, ignore=0.0 if dice else 0.05)
            crit = {"none": None, "ce_dx": None, "dice": DiceLoss(), "focaldice": FocalDiceLoss(),
                    "mixce": MixSoftmaxCrossEntropyLoss(aux=False)}[kind]
            if kind == "ce_dx":
                x.requires_grad_()
            loss = m.forward_loss(x, t, criterion=crit)
            loss.backward()
            emit("forward_loss/%s/%s" % (tag(shape, nc, dt), kind), m, (loss,),
                 x if kind == "ce_dx" else None)

    # the dropout seed left to the global CPU generator: one draw per train-mode forward
    for entry in ("forward", "forward_loss"):
        torch.manual_seed(0)
        m = model(19, False)
        m._dropout_seed = None
        x, t = batch(SMALL, 19)
        if entry == "forward":
            loss = MixSoftmaxCrossEntropyLoss(aux=False)(m(x), t)
        else:
            loss = m.forward_loss(x, t)
        loss.backward()
        emit("%s/%s/drawn_seed" % (entry, tag(SMALL, 19, f32)), m, (loss,),
             extra=(torch.get_rng_state(),))

    # 4. forward_loss_ohem, with and without class weights
    for shape, nc, dt in train_cfgs:
        for weights in (True, False):
            torch.manual_seed(0)
            m = model(nc, False)
            x, t = batch(shape, nc, dt)
            loss = m.forward_loss_ohem(x, t, ohem_crit(SoftmaxCrossEntropyOHEMLoss, nc, weights))
            loss.backward()
            emit("forward_loss_ohem/%s/w%d" % (tag(shape, nc, dt), int(weights)), m, (loss,))

    # 5. forward_loss_aux
    for shape, nc, dt in train_cfgs:
        for kind in ("ce", "dice", "ohem", "ohem_dx"):
            torch.manual_seed(0)
            m = model(nc, True)
            x, t = batch(shape, nc, dt, ignore=0.0 if kind == "dice" else 0.05)
            if kind == "ce":
                crit = MixSoftmaxCrossEntropyLoss(aux=True, aux_weight=0.4)
            elif kind == "dice":
                crit = MixDiceLoss(aux=True, aux_weight=0.4)
            else:
                crit = ohem_crit(MixSoftmaxCrossEntropyOHEMLoss, nc, True, aux=True,
                                 aux_weight=0.4)
            if kind == "ohem_dx":
                x.requires_grad_()
            loss = m.forward_loss_aux(x, t, crit)
            loss.backward()
            emit("forward_loss_aux/%s/%s" % (tag(shape, nc, dt), kind), m,
                 (loss, m._last_loss_terms), x if kind == "ohem_dx" else None)

    # 6. the staged backward (grad_stage_hook: four native calls)
    for aux in (False, True):
        torch.manual_seed(0)
        m = model(19, aux)
        x, t = batch(RAGGED, 19)
        seen = []
        m.grad_stage_hook = lambda s, G, b, e: seen.append((s, b, e))
        if aux:
            loss = m.forward_loss_aux(x, t, MixSoftmaxCrossEntropyLoss(aux=True, aux_weight=0.4))
        else:
            loss = m.forward_loss(x, t)
        loss.backward()
        emit("staged/%s/aux%d" % (tag(RAGGED, 19, f32), int(aux)), m, (loss, seen))

    # 7. predict and validate
    for nc in (2, 19):
        for dt in (f32, bf16):
            for ldt in (torch.int64, torch.uint8):
                torch.manual_seed(0)
                m = model(nc, False, train=False)
                x, _ = batch(SMALL, nc, dt)
                emit("predict/%s/%s" % (tag(SMALL, nc, dt), str(ldt).split(".")[-1]), m,
                     (m.predict(x, ldt),))
            for kind in ("none", "focaldice", "mixce_aux"):
                torch.manual_seed(0)
                aux = kind == "mixce_aux"
                m = model(nc, aux, train=False)
                x, t = batch(SMALL, nc, dt, ignore=0.0 if kind == "focaldice" else 0.05)
                crit = {"none": None, "focaldice": FocalDiceLoss(),
                        "mixce_aux": MixSoftmaxCrossEntropyLoss(aux=True, aux_weight=0.4)}[kind]
                metric = SegmentationMetric(nc) if aux else None
                loss = m.validate(x, t, crit, metric)
                emit("validate/%s/%s" % (tag(SMALL, nc, dt), kind), m,
                     (loss, m._last_validate_fused,
                      metric.device_counts(dev) if metric is not None else None))

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print("entry_digest: %d cases" % len(lines))


if __name__ == "__main__":
    main()
