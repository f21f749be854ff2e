"""FusedAdamW on the MI355X: the two kernels through the C ABI, the optimizer on FastSCNN's arena,
under GradScaler, and state interchange with torch.optim.AdamW.

Reference and tolerance, everywhere below: the reference is torch.optim.AdamW on fp64 CPU copies
of the same inputs; the yardstick is torch.optim.AdamW(foreach=False, fused=False) in fp32 on the
same inputs.  For each of p, exp_avg, exp_avg_sq (and max_exp_avg_sq) our max-abs deviation from
the fp64 result must be <= 2 x the yardstick's (a differently ordered but equally valid fp32
evaluation: fma contraction, the device's bias corrections), with a floor of one fp32 ulp of the
tensor's largest magnitude so that an exact yardstick cannot make the test unsatisfiable.
"""
import functools

import numpy as np
import pytest
import torch

from helpers import golden_input, golden_sd, golden_target, load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda"
KINDS = ("p", "exp_avg", "exp_avg_sq", "max_exp_avg_sq")


def _lib():
    from fast_scnn_pytorch_amd import _lib as lib
    return lib


# ---- reference twins -------------------------------------------------------------------------
def _twin(params0, groups, dtype, state0=None, **defaults):
    """torch.optim.AdamW on CPU copies of params0 (list of tensors) in ``dtype``.  groups: list of
    (indices, hyperparameters).  state0: per parameter, None or a dict step / exp_avg / ...."""
    ps = [p.detach().cpu().to(dtype).clone().requires_grad_(True) for p in params0]
    opt = torch.optim.AdamW([{"params": [ps[i] for i in idx], **hp} for idx, hp in groups],
                            foreach=False, fused=False, **defaults)
    for p, st in zip(ps, state0 or []):
        if st is not None:
            opt.state[p] = {k: (torch.tensor(float(v), dtype=torch.float32) if k == "step" else
                                v.detach().cpu().to(dtype).clone()) for k, v in st.items()}
    return ps, opt


def _twin_step(ps, opt, grads):
    for p, g in zip(ps, grads):
        p.grad = None if g is None else g.detach().cpu().to(p.dtype)
    opt.step()


def _twin_kinds(ps, opt):
    """{kind: flat tensor} over the parameters that have state (p: over all)."""
    out = {"p": torch.cat([p.detach().flatten() for p in ps])}
    for k in KINDS[1:]:
        ts = [opt.state[p][k].flatten() for p in ps if k in opt.state.get(p, {})]
        if ts:
            out[k] = torch.cat(ts)
    return out


def _ulp(x):
    return float(np.spacing(np.float32(x)))


def _check(ours, ref64, yard32, what):
    """ours / ref64 / yard32: {kind: flat tensor}.  Prints the observed ratio, then asserts."""
    assert set(ours) == set(ref64) == set(yard32), (what, set(ours), set(ref64))
    for k in ours:
        r = ref64[k].double()
        ours_k = ours[k].detach().cpu()
        assert ours_k.dtype == torch.float32 and ours_k.shape == r.shape, (what, k)
        assert torch.isfinite(ours_k).all(), (what, k)
        d_ours = float((ours_k.double() - r).abs().max())
        d_yard = float((yard32[k].double() - r).abs().max())
        floor = _ulp(float(r.abs().max()))
        print("%s %-14s ours %.3e yardstick %.3e floor %.3e ratio %.3f" % (
            what, k, d_ours, d_yard, floor, d_ours / max(d_yard, floor)))
        assert d_ours <= max(2.0 * d_yard, floor), (what, k, d_ours, d_yard, floor)


# ---- 1. span kernel through the C ABI --------------------------------------------------------
LRS = [1e-3, 3e-3, 1e-2, 5e-4, 2e-3]


def _span_inputs(n, seed):
    """p ~ N(0,1); per step gradients whose magnitudes span 1e-20 .. 1e2 with exact zeros: some
    elements are zero at every step (m = v = 0), some so small that v underflows (denom = eps)."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    mag = 10.0 ** (torch.rand(n, generator=gen) * 22 - 20)
    cls = torch.arange(n) % 5
    mag[cls == 1] = 0.0          # never any gradient
    mag[cls == 2] = 1e-20        # g*g underflows fp32
    if n == 1:
        mag[:] = 1e-20
    grads = []
    for _ in LRS:
        g = torch.randn(n, generator=gen) * mag
        g[torch.rand(n, generator=gen) < 0.1] = 0.0
        grads.append(g.float())
    return p, grads


def _call_span(p, g, m, v, vmax, step, hp, lr, tick=1, grad_scale=None, found_inf=None, n=None):
    lib = _lib()
    lib.call("fscnn_adamw", lib.ptr(p), lib.ptr(g), lib.ptr(m), lib.ptr(v), lib.ptr(vmax),
             p.numel() if n is None else n, lr, hp["betas"][0], hp["betas"][1], hp["eps"],
             hp["weight_decay"], int(hp["amsgrad"]), int(hp["maximize"]), lib.ptr(step), tick,
             lib.ptr(grad_scale), lib.ptr(found_inf), lib.stream_ptr())


def _hp(weight_decay=0.01, amsgrad=False, maximize=False, betas=(0.9, 0.999), eps=1e-8):
    return dict(betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad,
                maximize=maximize)


def _offset_views(tensors, off):
    """Device copies that start ``off`` floats past a 16-byte boundary."""
    out = []
    for t in tensors:
        buf = torch.zeros(t.numel() + 4, device=DEV)
        assert buf.data_ptr() % 16 == 0
        v = buf[off:off + t.numel()]
        v.copy_(t)
        out.append(v)
    return out


SPAN_CASES = [(n, 0, _hp(), 0) for n in (1, 3, 5, 1023, 1025, 4099)] + [
    (4099, 1, _hp(), 0),                                   # 4-byte aligned pointers only
    (1025, 0, _hp(weight_decay=0.0, amsgrad=True), 0),
    (1025, 1, _hp(amsgrad=True, maximize=True), 0),
    (1023, 0, _hp(weight_decay=0.0, maximize=True), 0),
    (4099, 0, _hp(amsgrad=True), 1000),                    # bias corrections at large t
    (1025, 0, _hp(betas=(0.3, 0.5)), 0),                   # lerp's other form (weight >= 0.5)
]


@pytest.mark.parametrize("n,off,hp,step0", SPAN_CASES, ids=[
    "n%d-off%d-wd%g-ams%d-max%d-b%g-t%d" % (c[0], c[1], c[2]["weight_decay"], c[2]["amsgrad"],
                                           c[2]["maximize"], c[2]["betas"][0], c[3])
    for c in SPAN_CASES])
def test_span_kernel_matches_torch(n, off, hp, step0):
    p0, grads = _span_inputs(n, 1234 + n)
    gen = torch.Generator().manual_seed(n)
    m0 = torch.zeros(n)
    v0 = torch.zeros(n)
    x0 = torch.zeros(n)
    if step0:  # a state that 1000 steps could have left
        m0 = torch.randn(n, generator=gen) * 0.1
        v0 = torch.rand(n, generator=gen) * 0.01
        x0 = v0 * 1.5
    st0 = {"step": step0, "exp_avg": m0, "exp_avg_sq": v0}
    if hp["amsgrad"]:
        st0["max_exp_avg_sq"] = x0
    twins = [_twin([p0], [([0], {})], dt, [st0], lr=LRS[0], **hp)
             for dt in (torch.float64, torch.float32)]
    p, m, v, x = _offset_views([p0, m0, v0, x0], off)
    step = torch.full((), float(step0), device=DEV)
    for lr, g in zip(LRS, grads):
        (gd,) = _offset_views([g], off)
        assert gd.data_ptr() % 16 == 4 * off
        _call_span(p, gd, m, v, x if hp["amsgrad"] else None, step, hp, lr)
        for ps, opt in twins:
            opt.param_groups[0]["lr"] = lr
            _twin_step(ps, opt, [g])
    torch.cuda.synchronize()
    assert float(step) == step0 + len(LRS)  # the device step counts the calls
    ours = {"p": p, "exp_avg": m, "exp_avg_sq": v}
    if hp["amsgrad"]:
        ours["max_exp_avg_sq"] = x
    else:
        assert torch.equal(x.cpu(), x0)  # never written
    (r64, y32) = [_twin_kinds(ps, opt) for ps, opt in twins]
    _check(ours, r64, y32, "span n=%d off=%d" % (n, off))
    # the never-touched elements: zero gradient at every step leaves m = v = 0
    dead = torch.stack([g == 0 for g in grads]).all(0)
    assert n < 5 or dead.any()
    if step0 == 0:
        assert torch.equal(m.cpu()[dead], torch.zeros(int(dead.sum())))
        assert torch.equal(v.cpu()[dead], torch.zeros(int(dead.sum())))


# ---- 2. exact properties ---------------------------------------------------------------------
def _span_state(n=1025, seed=7, amsgrad=True):
    gen = torch.Generator().manual_seed(seed)
    t = [torch.randn(n, generator=gen), torch.randn(n, generator=gen),
         torch.randn(n, generator=gen) * 0.1, torch.rand(n, generator=gen) * 0.01,
         torch.rand(n, generator=gen) * 0.02]
    return [a.to(DEV) for a in t]  # p, g, m, v, vmax


def test_lr_zero_leaves_p_bit_unchanged():
    p, g, m, v, x = _span_state()
    before = [a.clone() for a in (p, m, v, x)]
    step = torch.full((), 3.0, device=DEV)
    _call_span(p, g, m, v, x, step, _hp(weight_decay=0.0, amsgrad=True), 0.0)
    _call_span(p, g, m, v, x, step, _hp(weight_decay=0.3, amsgrad=True), 0.0)
    torch.cuda.synchronize()
    assert torch.equal(p, before[0])
    assert not torch.equal(m, before[1]) and not torch.equal(v, before[2])
    assert float(step) == 5.0


@pytest.mark.parametrize("n", [5, 4099])
def test_found_inf_changes_nothing(n):
    p, g, m, v, x = _span_state(n)
    before = [a.clone() for a in (p, m, v, x)]
    step = torch.full((), 3.0, device=DEV)
    inf = torch.ones(1, device=DEV)
    scale = torch.full((), 8.0, device=DEV)
    _call_span(p, g, m, v, x, step, _hp(amsgrad=True), 1e-2, grad_scale=scale, found_inf=inf)
    torch.cuda.synchronize()
    for a, b in zip((p, m, v, x), before):
        assert torch.equal(a, b)
    assert float(step) == 3.0
    inf.zero_()  # the same call with found_inf = 0 does step
    _call_span(p, g, m, v, x, step, _hp(amsgrad=True), 1e-2, grad_scale=scale, found_inf=inf)
    torch.cuda.synchronize()
    assert float(step) == 4.0
    for a, b in zip((p, m, v, x), before):
        assert not torch.equal(a, b)


def test_grad_scale_power_of_two_is_exact():
    a = _span_state(4099)
    b = [t.clone() for t in a]
    sa = torch.zeros((), device=DEV)
    sb = torch.zeros((), device=DEV)
    scale = torch.full((), 4.0, device=DEV)
    hp = _hp(amsgrad=True)
    for lr in LRS[:2]:
        _call_span(a[0], a[1], a[2], a[3], a[4], sa, hp, lr)
        _call_span(b[0], b[1] * 4.0, b[2], b[3], b[4], sb, hp, lr, grad_scale=scale)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert float(sa) == float(sb) == 2.0


# ---- 3. segment kernel -----------------------------------------------------------------------
SEG_LAYOUT = [(0, 16, 0), (16, 48, 1), (64, 1, 0), (80, 1040, 1), (1136, 2064, 0)]  # off, n, group
SEG_HP = [dict(lr=1e-2, **_hp(weight_decay=0.1, amsgrad=True)),
          dict(lr=3e-4, **_hp(weight_decay=0.0, betas=(0.8, 0.99), maximize=True))]


def _seg_table(layout):
    from fast_scnn_pytorch_amd.optim import _AdamwSeg, _segments
    segs, chunk_seg = _segments([s[0] for s in layout], [s[1] for s in layout],
                                [s[2] for s in layout])
    hsegs = (_AdamwSeg * len(segs))(*segs)
    dsegs = torch.frombuffer(bytearray(hsegs), dtype=torch.uint8).to(DEV)
    dchunk = torch.tensor(chunk_seg, dtype=torch.int32, device=DEV)
    return segs, hsegs, dsegs, dchunk


def _call_segments(arenas, g, table, hps, steps, tick=1, grad_scale=None, found_inf=None):
    from fast_scnn_pytorch_amd.optim import _AdamwGroup
    lib = _lib()
    segs, hsegs, dsegs, dchunk = table
    cg = (_AdamwGroup * len(hps))()
    for k, (c, hp) in enumerate(zip(cg, hps)):
        c.lr, (c.beta1, c.beta2), c.eps = hp["lr"], hp["betas"], hp["eps"]
        c.weight_decay, c.amsgrad, c.maximize = hp["weight_decay"], hp["amsgrad"], hp["maximize"]
        c.step_slot = k
    p, m, v, x = arenas
    lib.call("fscnn_adamw_segments", lib.ptr(p), lib.ptr(g), lib.ptr(m), lib.ptr(v), lib.ptr(x),
             lib.ptr(dsegs), hsegs, len(segs), lib.ptr(dchunk), dchunk.numel(), cg, len(hps),
             lib.ptr(steps), steps.numel(), tick, lib.ptr(grad_scale), lib.ptr(found_inf),
             lib.stream_ptr())


def _seg_arenas():
    gen = torch.Generator().manual_seed(99)
    n = 4096
    # sentinel patterns: distinct, finite, non-trivial values everywhere
    p = (torch.arange(n, dtype=torch.float32) * 0.37 + 1.0).sin() * 2.0
    m = (torch.arange(n, dtype=torch.float32) * 0.11).cos() * 0.1
    v = (torch.arange(n, dtype=torch.float32) * 0.07).sin().abs() * 0.01 + 1e-6
    x = v * 1.25
    grads = [torch.randn(n, generator=gen) for _ in range(2)]
    return [t.to(DEV) for t in (p, m, v, x)], [g.to(DEV) for g in grads]


def test_segment_kernel_equals_span_kernel_per_segment():
    table = _seg_table(SEG_LAYOUT)
    assert [(s[0], s[1], s[2]) for s in table[0]] == [(o, o + n, g) for o, n, g in SEG_LAYOUT]
    assert table[3].numel() == 6  # 1 + 1 + 1 + 1 + 2 chunks
    arenas, grads = _seg_arenas()
    before = [a.clone() for a in arenas]
    ref = [a.clone() for a in arenas]
    steps = torch.tensor([0.0, 7.0], device=DEV)
    rsteps = [torch.full((), 0.0, device=DEV), torch.full((), 7.0, device=DEV)]
    last = {g: max(i for i, s in enumerate(SEG_LAYOUT) if s[2] == g) for g in (0, 1)}
    for it, g in enumerate(grads):
        hps = [dict(hp, lr=hp["lr"] * (1 + it)) for hp in SEG_HP]
        _call_segments(arenas, g, table, hps, steps)
        for i, (o, n, gi) in enumerate(SEG_LAYOUT):
            hp = hps[gi]
            sl = slice(o, o + n)
            _call_span(ref[0][sl], g[sl], ref[1][sl], ref[2][sl],
                       ref[3][sl] if hp["amsgrad"] else None, rsteps[gi], hp, hp["lr"],
                       tick=int(i == last[gi]))
    torch.cuda.synchronize()
    assert steps.tolist() == [2.0, 9.0] and [float(s) for s in rsteps] == [2.0, 9.0]
    inside = torch.zeros(4096, dtype=torch.bool)
    for o, n, _ in SEG_LAYOUT:
        inside[o:o + n] = True
    for name, a, r, b in zip(KINDS, arenas, ref, before):
        bad = (a != r).nonzero().flatten().tolist()
        assert not bad, (name, len(bad), bad[:8], a[bad[:4]].tolist(), r[bad[:4]].tolist())
        assert torch.equal(a, r), name                                # bit for bit
        assert torch.equal(a.cpu()[~inside], b.cpu()[~inside]), name  # sentinels untouched
    for name, a, b in zip(KINDS[:3], arenas, before):
        assert not torch.equal(a.cpu()[inside], b.cpu()[inside]), name
    # group 1 has no amsgrad: its part of the max arena is untouched as well
    for o, n, gi in SEG_LAYOUT:
        if gi == 1:
            assert torch.equal(arenas[3][o:o + n], before[3][o:o + n])


def test_segment_kernel_found_inf_changes_nothing():
    table = _seg_table(SEG_LAYOUT)
    arenas, grads = _seg_arenas()
    before = [a.clone() for a in arenas]
    steps = torch.tensor([4.0, 7.0], device=DEV)
    hps = [dict(hp) for hp in SEG_HP]
    _call_segments(arenas, grads[0], table, hps, steps, found_inf=torch.ones(1, device=DEV),
                   grad_scale=torch.full((), 2.0, device=DEV))
    torch.cuda.synchronize()
    for a, b in zip(arenas, before):
        assert torch.equal(a, b)
    assert steps.tolist() == [4.0, 7.0]


# ---- 4 / 5. the optimizer on the model -------------------------------------------------------
def _model(g, seed=5):
    from models.fast_scnn import FastSCNN
    m = FastSCNN(int(g["num_classes"]))
    m.load_state_dict(golden_sd(g))
    m = m.to(DEV).train()
    m._dropout_seed = seed
    return m


def _case_groups(case, names, shapes):
    """-> (groups: [(names, hyperparameters)], frozen names, constructor keywords)"""
    if case == "single":
        return [(names, {})], [], {}
    if case == "amsgrad":
        return [(names, {})], [], {"amsgrad": True}
    if case == "decay_nodecay":  # the standard AdamW grouping: BatchNorm and biases undecayed
        nd = [n for n in names if len(shapes[n]) == 1]
        assert nd and len(nd) < len(names)
        return [([n for n in names if n not in nd], {"weight_decay": 0.05}),
                (nd, {"weight_decay": 0.0, "lr": 2e-3})], [], {}
    if case == "frozen":
        return [(names, {})], [n for n in names if "bottleneck2.1" in n], {}
    if case == "nine_groups":
        return [([n for i, n in enumerate(names) if i % 9 == k],
                 {"lr": 1e-3 * (k + 1), "weight_decay": 0.01 * k, "betas": (0.9 - 0.05 * k, 0.999)})
                for k in range(9)], [], {}
    raise ValueError(case)


@functools.lru_cache(maxsize=None)
def _run_case(case, steps=4):
    """FusedAdamW on FastSCNN(2)'s arena against the two torch twins, fed the same real
    forward_loss gradients.  Returns what the tests assert on, computed once per case."""
    from fast_scnn_pytorch_amd import _lib as lib
    from fast_scnn_pytorch_amd.optim import FusedAdamW
    g = load_golden("train_c2")
    x, t = golden_input(g).to(DEV), golden_target(g).to(DEV)
    m = _model(g)
    prm = dict(m.named_parameters())
    names = list(prm)
    groups, frozen, kw = _case_groups(case, names, {n: p.shape for n, p in prm.items()})
    opt = FusedAdamW([{"params": [prm[n] for n in ns], **hp} for ns, hp in groups], lr=1e-3, **kw)
    for n in frozen:
        prm[n].requires_grad_(False)
    start = {n: p.detach().clone() for n, p in prm.items()}
    idx = {n: i for i, n in enumerate(names)}
    twins = [_twin([start[n] for n in names], [([idx[n] for n in ns], hp) for ns, hp in groups],
                   dt, lr=1e-3, **kw) for dt in (torch.float64, torch.float32)]
    calls = []
    real = lib.call
    counts = []
    lib.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        for it in range(steps):
            opt.zero_grad(set_to_none=True)
            m.forward_loss(x, t).backward()
            grads = [prm[n].grad for n in names]
            opt.param_groups[0]["lr"] = 1e-3 * (1 + it)  # a scheduler: lr changes every step
            del calls[:]
            opt.step()
            counts.append({k: calls.count(k) for k in ("fscnn_adamw_segments", "fscnn_adamw")})
            for ps, topt in twins:
                topt.param_groups[0]["lr"] = 1e-3 * (1 + it)
                _twin_step(ps, topt, grads)
    finally:
        lib.call = real
    torch.cuda.synchronize()
    live = [n for n in names if n not in frozen]
    ours = {"p": torch.cat([prm[n].detach().flatten() for n in names])}
    for k in KINDS[1:]:
        ts = [opt.state[prm[n]][k].flatten() for n in live if k in opt.state[prm[n]]]
        if ts:
            ours[k] = torch.cat(ts)
    res = {"ours": {k: v.cpu() for k, v in ours.items()},
           "twins": [_twin_kinds(ps, topt) for ps, topt in twins], "counts": counts,
           "frozen_ok": all(torch.equal(prm[n].detach(), start[n]) and len(opt.state[prm[n]]) == 0
                            for n in frozen),
           "n_frozen": len(frozen),
           "steps": sorted({float(opt.state[prm[n]]["step"]) for n in live}),
           "state_keys": sorted(opt.state[prm[live[0]]].keys()),
           "moved": not torch.equal(ours["p"].cpu(), torch.cat([start[n].flatten().cpu()
                                                                 for n in names]))}
    return res


CASES = ["single", "decay_nodecay", "frozen", "nine_groups", "amsgrad"]


@pytest.mark.parametrize("case", CASES)
def test_optimizer_on_the_model_matches_torch(case):
    res = _run_case(case)
    assert res["moved"] and res["steps"] == [4.0]
    _check(res["ours"], res["twins"][0], res["twins"][1], "model " + case)
    assert res["frozen_ok"]
    assert (res["n_frozen"] > 0) == (case == "frozen")
    want = ["exp_avg", "exp_avg_sq"] + (["max_exp_avg_sq"] if case == "amsgrad" else []) + ["step"]
    assert res["state_keys"] == sorted(want)


@pytest.mark.parametrize("case", CASES)
def test_steady_state_step_is_one_launch_per_eight_groups(case):
    counts = _run_case(case)["counts"]
    want = 2 if case == "nine_groups" else 1
    for c in counts:  # every step, the plan-building first one included
        assert c == {"fscnn_adamw_segments": want, "fscnn_adamw": 0}, counts


# ---- 6. GradScaler ---------------------------------------------------------------------------
def test_gradscaler_skips_on_overflow_without_reading_back(monkeypatch):
    """train_bdd100k.py:258-266 with FusedAdamW: scaler.scale(loss).backward(); scaler.step(opt);
    scaler.update().  A finite step agrees with torch on the unscaled gradients; an overflowing
    step leaves parameters, state and step bit-unchanged and halves the scale; no step reads a
    device value back (Tensor.item raises while scaler.step runs)."""
    from fast_scnn_pytorch_amd.loss import MixSoftmaxCrossEntropyLoss
    from fast_scnn_pytorch_amd.optim import FusedAdamW
    g = load_golden("train_c19")
    x, t = golden_input(g).to(DEV), golden_target(g).to(DEV)
    crit = MixSoftmaxCrossEntropyLoss(aux=False, ignore_label=-1)
    m = _model(g)
    params = list(m.parameters())
    opt = FusedAdamW(params, lr=1e-3, weight_decay=0.01)
    twins = [_twin(params, [(list(range(len(params))), {})], dt, lr=1e-3, weight_decay=0.01)
             for dt in (torch.float64, torch.float32)]
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 10)

    def backward():
        opt.zero_grad()
        with torch.autocast("cuda"):
            loss = crit(m(x), t)
        scaler.scale(loss).backward()

    def snapshot():
        st = opt.state[params[0]]
        return ([p.detach().clone() for p in params] +
                [opt.state[p][k].clone() for p in params for k in ("exp_avg", "exp_avg_sq")] +
                [st["step"].clone()])

    def no_item(self):
        raise AssertionError("Tensor.item() during scaler.step(optimizer)")

    # two finite steps: the second is steady state and must not read anything back
    for it in range(2):
        backward()
        scale = scaler.get_scale()
        grads = [p.grad.detach() / scale for p in params]  # exact: a power of two
        assert all(torch.isfinite(gr).all() for gr in grads)
        if it == 1:
            with monkeypatch.context() as mp:
                mp.setattr(torch.Tensor, "item", no_item)
                scaler.step(opt)
        else:
            scaler.step(opt)
        scaler.update()
        for ps, topt in twins:
            _twin_step(ps, topt, grads)
    assert scaler.get_scale() == 2.0 ** 10
    ours = {"p": torch.cat([p.detach().flatten() for p in params]),
            "exp_avg": torch.cat([opt.state[p]["exp_avg"].flatten() for p in params]),
            "exp_avg_sq": torch.cat([opt.state[p]["exp_avg_sq"].flatten() for p in params])}
    _check(ours, _twin_kinds(*twins[0]), _twin_kinds(*twins[1]), "gradscaler finite")
    assert float(opt.state[params[0]]["step"]) == 2.0

    # overflow: everything stays, the scale halves
    scaler.update(2.0 ** 40)
    before = snapshot()
    backward()
    assert not all(torch.isfinite(p.grad).all() for p in params)  # the overflow really happened
    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "item", no_item)
        scaler.step(opt)
    scaler.update()
    assert scaler.get_scale() == 2.0 ** 39
    for a, b in zip(before, snapshot()):
        assert torch.equal(a, b)

    # the next finite step moves them again
    scaler.update(2.0 ** 10)
    backward()
    scaler.step(opt)
    scaler.update()
    after = snapshot()
    assert float(after[-1]) == 3.0
    assert all(torch.isfinite(a).all() for a in after)
    assert any(not torch.equal(a, b) for a, b in zip(before[:len(params)], after[:len(params)]))
    assert not torch.equal(before[len(params)], after[len(params)])


def test_step_after_unscale_has_no_grad_scale():
    """scaler.unscale_(opt) before scaler.step(opt) (gradient clipping): GradScaler then hands
    grad_scale = None and the already unscaled gradients are used as they are."""
    from fast_scnn_pytorch_amd.optim import FusedAdamW
    arena = torch.randn(64, device=DEV)
    p = torch.nn.Parameter(arena[:40])
    q = p.detach().clone()
    gr = torch.randn(40, device=DEV)
    opt = FusedAdamW([p], lr=1e-2)
    scaler = torch.amp.GradScaler("cuda", init_scale=8.0)
    assert float(scaler.scale(torch.ones((), device=DEV))) == 8.0  # (initialises the scale)
    p.grad = gr * 8.0
    scaler.unscale_(opt)
    scaler.step(opt)
    scaler.update()
    q = torch.nn.Parameter(q)
    q.grad = gr.clone()
    ref = FusedAdamW([q], lr=1e-2)
    ref.step()
    assert torch.equal(p.detach(), q.detach())
    assert not hasattr(opt, "grad_scale") and not hasattr(opt, "found_inf")


# ---- 7. state interchange with torch.optim.AdamW ---------------------------------------------
SIZES = [40, 1, 2100]  # three tensors of one flat arena at 16-float aligned offsets


def _arena_params(seed=3):
    gen = torch.Generator().manual_seed(seed)
    offs, o = [], 0
    for n in SIZES:
        offs.append(o)
        o += (n + 15) // 16 * 16
    arena = torch.randn(o, generator=gen).to(DEV)
    params = [torch.nn.Parameter(arena[a:a + n]) for a, n in zip(offs, SIZES)]
    grads = [torch.randn(o, generator=gen).to(DEV) for _ in range(4)]
    return params, offs, grads


def _set_grads(params, offs, flat):
    flat = flat.clone()  # a new flat buffer every step, as a backward produces
    for p, a in zip(params, offs):
        p.grad = flat[a:a + p.numel()]


def _gslices(offs, flat):
    return [flat[a:a + n] for a, n in zip(offs, SIZES)]


def _ours_kinds(params, opt):
    out = {"p": torch.cat([p.detach().flatten() for p in params])}
    for k in KINDS[1:]:
        ts = [opt.state[p][k].flatten() for p in params if k in opt.state[p]]
        if ts:
            out[k] = torch.cat(ts)
    return out


HP7 = dict(lr=3e-3, betas=(0.9, 0.99), weight_decay=0.02, amsgrad=True)


@pytest.mark.parametrize("source", ["cpu_steps", "device_steps"])
def test_torch_state_dict_loads_and_training_continues(source):
    from fast_scnn_pytorch_amd.optim import FusedAdamW
    params, offs, grads = _arena_params()
    start = [p.detach().clone() for p in params]
    twins = [_twin(start, [([0, 1, 2], {})], dt, **HP7) for dt in (torch.float64, torch.float32)]
    for flat in grads:
        for ps, topt in twins:
            _twin_step(ps, topt, _gslices(offs, flat))
    # two steps of torch.optim.AdamW ...
    if source == "cpu_steps":   # torch's default: step is a CPU scalar
        tp, topt = _twin(start, [([0, 1, 2], {})], torch.float32, **HP7)
        for flat in grads[:2]:
            _twin_step(tp, topt, _gslices(offs, flat))
    else:                       # fused=True keeps step on the device
        tp = [s.clone().requires_grad_(True) for s in start]
        topt = torch.optim.AdamW(tp, fused=True, **HP7)
        for flat in grads[:2]:
            for p, gs in zip(tp, _gslices(offs, flat)):
                p.grad = gs.clone()
            topt.step()
    sd = topt.state_dict()
    assert sd["state"][0]["step"].is_cuda == (source == "device_steps")
    # ... then two of FusedAdamW from its state
    with torch.no_grad():
        for p, s in zip(params, tp):
            p.copy_(s.detach())
    opt = FusedAdamW(params)
    opt.load_state_dict(sd)
    lib = _lib()
    calls, real = [], lib.call
    lib.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        for flat in grads[2:]:
            _set_grads(params, offs, flat)
            opt.step()
    finally:
        lib.call = real
    assert calls == ["fscnn_adamw_segments"] * 2  # equal loaded steps: the fused path
    _check(_ours_kinds(params, opt), _twin_kinds(*twins[0]), _twin_kinds(*twins[1]),
           "torch -> fused (%s)" % source)
    assert float(opt.state[params[0]]["step"]) == 4.0
    # the state tensors are views of the flat arenas at the parameters' offsets
    base = opt.state[params[0]]["exp_avg"].untyped_storage().data_ptr()
    for p, a in zip(params, offs):
        for k in KINDS[1:]:
            s = opt.state[p][k]
            assert s.untyped_storage().data_ptr() == opt.state[params[0]][k].untyped_storage(
            ).data_ptr() and s.storage_offset() == a - offs[0] and s.shape == p.shape
    assert base % 16 == 0


def test_fused_state_dict_loads_into_torch():
    from fast_scnn_pytorch_amd.optim import FusedAdamW
    params, offs, grads = _arena_params()
    start = [p.detach().clone() for p in params]
    twins = [_twin(start, [([0, 1, 2], {})], dt, **HP7) for dt in (torch.float64, torch.float32)]
    for flat in grads:
        for ps, topt in twins:
            _twin_step(ps, topt, _gslices(offs, flat))
    opt = FusedAdamW(params, **HP7)
    for flat in grads[:2]:
        _set_grads(params, offs, flat)
        opt.step()
    sd = opt.state_dict()
    # exactly torch's keys, state and groups
    tkeys = twins[1][1].state_dict()
    assert set(sd["state"]) == set(tkeys["state"]) == {0, 1, 2}
    for i in range(3):
        assert set(sd["state"][i]) == set(tkeys["state"][i]) == set(KINDS[1:]) | {"step"}
        assert sd["state"][i]["step"].device.type == "cpu" and float(sd["state"][i]["step"]) == 2.0
    assert set(sd["param_groups"][0]) == set(tkeys["param_groups"][0])
    tp, topt = _twin([p.detach() for p in params], [([0, 1, 2], {})], torch.float32)
    topt.load_state_dict(sd)
    assert topt.param_groups[0]["lr"] == HP7["lr"] and topt.param_groups[0]["amsgrad"] is True
    for flat in grads[2:]:
        _twin_step(tp, topt, _gslices(offs, flat))
    assert float(topt.state[tp[0]]["step"]) == 4.0  # each parameter's own step: no sharing
    _check({k: v for k, v in _twin_kinds(tp, topt).items()}, _twin_kinds(*twins[0]),
           _twin_kinds(*twins[1]), "fused -> torch")
    # and back into a fresh FusedAdamW: its own state_dict round-trips
    opt2 = FusedAdamW(params)
    opt2.load_state_dict(sd)
    assert opt2.param_groups[0]["betas"] == HP7["betas"]


def test_unequal_steps_take_the_per_tensor_path_and_match_torch():
    """A loaded state whose parameters have taken different numbers of steps (one was unfrozen
    later): every parameter steps with its own count, as in torch."""
    from fast_scnn_pytorch_amd.optim import FusedAdamW
    params, offs, grads = _arena_params()
    start = [p.detach().clone() for p in params]
    gen = torch.Generator().manual_seed(11)
    st0 = [{"step": s, "exp_avg": torch.randn(n, generator=gen) * 0.1,
            "exp_avg_sq": torch.rand(n, generator=gen) * 0.01} for s, n in zip((2, 5, 2), SIZES)]
    hp = dict(lr=3e-3, weight_decay=0.02)
    twins = [_twin(start, [([0, 1, 2], {})], dt, st0, **hp) for dt in (torch.float64, torch.float32)]
    opt = FusedAdamW(params)
    opt.load_state_dict(twins[1][1].state_dict())
    lib = _lib()
    calls, real = [], lib.call
    lib.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        for flat in grads[:3]:
            _set_grads(params, offs, flat)
            opt.step()
            for ps, topt in twins:
                _twin_step(ps, topt, _gslices(offs, flat))
    finally:
        lib.call = real
    assert calls == ["fscnn_adamw"] * 9
    assert [float(opt.state[p]["step"]) for p in params] == [5.0, 8.0, 5.0]
    _check(_ours_kinds(params, opt), _twin_kinds(*twins[0]), _twin_kinds(*twins[1]),
           "unequal steps")


def test_parameter_unfrozen_later_matches_torch():
    from fast_scnn_pytorch_amd.optim import FusedAdamW
    params, offs, grads = _arena_params()
    start = [p.detach().clone() for p in params]
    twins = [_twin(start, [([0, 1, 2], {})], dt, **HP7) for dt in (torch.float64, torch.float32)]
    opt = FusedAdamW(params, **HP7)
    for it, flat in enumerate(grads):
        _set_grads(params, offs, flat)
        gs = _gslices(offs, flat)
        if it < 2:  # the middle tensor has no gradient for two steps
            params[1].grad = None
            gs[1] = None
        opt.step()
        if it == 1:
            assert len(opt.state[params[1]]) == 0
            assert torch.equal(params[1].detach(), start[1])
        for ps, topt in twins:
            _twin_step(ps, topt, gs)
    assert [float(opt.state[p]["step"]) for p in params] == [4.0, 2.0, 4.0]
    _check(_ours_kinds(params, opt), _twin_kinds(*twins[0]), _twin_kinds(*twins[1]), "unfrozen")


# ---- 8. fallback -----------------------------------------------------------------------------
def test_free_standing_tensors_take_one_launch_each():
    from fast_scnn_pytorch_amd.optim import FusedAdamW
    gen = torch.Generator().manual_seed(21)
    big = torch.randn(1026, generator=gen).to(DEV)
    big0 = float(big[0])
    params = [torch.nn.Parameter(torch.randn(1, generator=gen).to(DEV)),
              torch.nn.Parameter(torch.randn(5, generator=gen).to(DEV)),
              torch.nn.Parameter(big[1:])]  # 4-byte aligned only
    assert params[2].data_ptr() % 16 == 4 and params[2].numel() == 1025
    start = [p.detach().clone() for p in params]
    hp = dict(lr=2e-3, weight_decay=0.03, amsgrad=True)
    twins = [_twin(start, [([0, 1, 2], {})], dt, **hp) for dt in (torch.float64, torch.float32)]
    opt = FusedAdamW(params, **hp)
    lib = _lib()
    calls, real = [], lib.call
    lib.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        for _ in range(3):
            gs = [torch.randn(p.numel(), generator=gen).to(DEV).view_as(p) for p in params]
            for p, g in zip(params, gs):
                p.grad = g
            opt.step()
            for ps, topt in twins:
                _twin_step(ps, topt, gs)
    finally:
        lib.call = real
    assert calls == ["fscnn_adamw"] * 9
    assert [float(opt.state[p]["step"]) for p in params] == [3.0] * 3
    _check(_ours_kinds(params, opt), _twin_kinds(*twins[0]), _twin_kinds(*twins[1]), "fallback")
    assert float(big[0]) == big0  # the element before the view is not part of the span


def test_cpu_parameter_among_gpu_parameters_raises():
    from fast_scnn_pytorch_amd.optim import FusedAdamW
    a = torch.nn.Parameter(torch.zeros(4, device=DEV))
    b = torch.nn.Parameter(torch.zeros(4))
    a.grad, b.grad = torch.ones(4, device=DEV), torch.ones(4)
    opt = FusedAdamW([a, b])
    with pytest.raises(RuntimeError):
        opt.step()
    c = torch.nn.Parameter(torch.zeros(4, device=DEV, dtype=torch.float16))
    c.grad = torch.ones_like(c)
    with pytest.raises(RuntimeError):
        FusedAdamW([c]).step()
