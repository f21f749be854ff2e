"""The depthwise 3x3 tile kernels (csrc/dwconv.hip) on every path they take: the compile-time
channel-chunk instantiations (cbv 4 / 6 / 8), the run-time-cbv kernel every other width falls back
to, interior tiles (no clamps, no edge guards) next to edge, corner and ragged tiles, and maps
smaller than a tile -- through the C ABI, in fp32, bf16 and fp16.

References and bounds are those of tests/test_gpu_train_kernels.py (helpers copied from there):
fp64 conv2d / conv_transpose2d with the absolute-value companion and check_elem for stored
tensors, check_sum for per-channel sums, statistics against the STORED tensor to 1e-5 (mean,
running statistics) and 1e-4 (invstd, scale, shift) of the largest reference value; the weight
gradient to the fp32 accumulation bound (M + 2) 2^-24 sum |dy x| of test_gpu_train_gemm.py.

Geometry per dtype and stride: N = 2 and an output map of 3 full tiles plus one pixel each way
(bf16 stride 1: 25 x 49, fp32 stride 1: 25 x 97), so interior, edge, corner and ragged tiles are
all present and a tile's halo crosses the boundary between the two images; plus the maps 1 x 1,
1 x 37, 3 x 5 and one exactly one tile large.  Channel widths on the first geometry: 16-bit
C in {8, 24, 32, 40, 48, 56, 64, 576}, fp32 C in {4, 12, 16, 20, 24, 28, 32} (cbv 1..8, every
instantiation, the fallback, a multi-chunk grid); the smallest and 64 / 32 on the rest.

test_dw_fast_path_matches_generic: FSCNN_DW_GENERIC=1 forces the bounds-checked kernels; two fresh
child processes (tests/_dw_paths_worker.py), one per setting, write every output, record and slab
of a handful of these cases, and the files must be byte-equal.  fscnn_dw3x3_ct_width reports which
kernels a shape takes, so the test also knows both paths really ran.
"""
import json
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from fast_scnn_pytorch_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTS = [F32, BF16, F16]
U = {F32: 2.0 ** -24, BF16: 2.0 ** -8, F16: 2.0 ** -11}
E24 = 2.0 ** -24
S = _lib.stream_ptr
P = _lib.ptr
M_MAX = 65539   # 2e-6 < 1 / (4 M): the per-channel sum bound resolves one row


# ---- helpers of tests/test_gpu_train_kernels.py ---------------------------------------------------

def dname(dt):
    return str(dt).replace("torch.", "")


def rnd(*shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.rand(*shape, generator=g, dtype=torch.float64) * (hi - lo) + lo


def randn(*shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def q(t, dt):
    """Round to the storage type: the exact operand both sides see."""
    return t.to(dt)


def dev(t):
    return t.contiguous().to(DEV)


def f32(t):
    return t.to(torch.float32)


def d64(t):
    return t.detach().to("cpu").double()


def sync():
    torch.cuda.synchronize()


def report(what, ratio):
    print("%-58s worst err / bound %.3f" % (what, ratio))


def check_elem(what, got, ref, A, dt):
    """An element-wise output stored in T against its fp64 value."""
    got, ref, A = d64(got), d64(ref), d64(A)
    bound = U[dt] * ref.abs() + 1e-6 * A + (2.0 ** -24 if dt == F16 else 0.0)
    err = (got - ref).abs()
    assert bool(torch.isfinite(got).all()), "%s: non-finite output" % what
    ratio = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    report(what, ratio)
    bad = err > bound
    assert not bool(bad.any()), "%s: %d of %d elements out of bound, worst err / bound %.3f" % (
        what, int(bad.sum()), bad.numel(), ratio)


def check_bound(what, got, ref, bound):
    """|got - ref| <= bound element by element."""
    got, ref, bound = d64(got), d64(ref), d64(bound)
    assert bool(torch.isfinite(got).all()), "%s: non-finite output" % what
    r = (got - ref).abs() / bound.clamp_min(1e-300)
    report(what, r.max().item())
    assert not bool((r > 1).any()), "%s: %d of %d elements out of bound, worst %.3f" % (
        what, int((r > 1).sum()), r.numel(), r.max().item())


def check_sum(what, got, ref, a):
    """A per-channel fp32 sum against fp64: 2e-6 a + 1e-6."""
    got, ref, a = d64(got), d64(ref), d64(a)
    bound = 2e-6 * a + 1e-6
    err = (got - ref).abs()
    assert bool(torch.isfinite(got).all()), "%s: non-finite output" % what
    ratio = (err / bound).max().item()
    report(what, ratio)
    assert ratio <= 1.0, "%s: worst err / bound %.3f" % (what, ratio)


def bn_tables(z64, seed, C):
    """mean / invstd of z [M][C] (fp64 -> fp32, as a forward would have stored them) and an affine
    with gammas of both signs; returns fp32 CPU tensors (mean, invstd, scale, shift)."""
    mean = f32(z64.mean(0))
    invstd = f32(1.0 / torch.sqrt(z64.var(0, unbiased=False) + 1e-5))
    gamma = f32(rnd(C, seed=seed, lo=0.5, hi=1.5))
    gamma[1::5] *= -1.0
    beta = f32(rnd(C, seed=seed + 1, lo=-0.5, hi=0.5))
    scale = gamma * invstd
    shift = beta - mean * scale
    return mean, invstd, scale, shift


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _dw_scratch():
    return (torch.zeros(512, dtype=torch.int32, device=DEV),
            torch.zeros(32 * 3 * 1024, dtype=torch.float64, device=DEV))


def nans(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


# ---- the cases --------------------------------------------------------------------------------------

# output tile (rows, cols) of the tile kernels (DwCfg in csrc/dwconv.hip)
TILE = {(4, 1): (8, 32), (4, 2): (4, 16), (2, 1): (8, 16), (2, 2): (8, 8)}
WIDTHS = {4: [4, 12, 16, 20, 24, 28, 32], 2: [8, 24, 32, 40, 48, 56, 64, 576]}


def esize(dt):
    return 4 if dt == F32 else 2


def in_size(o, stride):
    """The (odd, for stride 2) input size whose output size is o."""
    return o if stride == 1 else 2 * o - 1


def cases(dt, stride):
    """(H, W, C) of the input maps: the 3-tiles-plus-one-pixel map at every width, then the
    degenerate maps and the one-tile map at the smallest width and at 64 / 32."""
    th, tw = TILE[(esize(dt), stride)]
    widths = WIDTHS[esize(dt)]
    ends = [widths[0], 32 if dt == F32 else 64]
    out = [(in_size(3 * th + 1, stride), in_size(3 * tw + 1, stride), C) for C in widths]
    for H, W in [(1, 1), (1, 37), (3, 5), (th * stride, tw * stride)]:
        out += [(H, W, C) for C in ends]
    return out


ALL = [(dt, s, H, W, C) for dt in DTS for s in (1, 2) for H, W, C in cases(dt, s)]


def cid(c):
    return "%s-s%d-%dx%d-c%d" % (dname(c[0]), c[1], c[2], c[3], c[4])


N = 2


def osize(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


# ---- the launches (also run by tests/_dw_paths_worker.py) -------------------------------------------

def run_fwd_train(dt, stride, H, W, C, lazy):
    """fscnn_dw3x3_fwd_train -> (inputs, outputs)."""
    code = _lib.dtype_code(dt)
    Ho, Wo = osize(H, W, stride)
    i = dict(x=q(randn(N, H, W, C, seed=61), dt), w=f32(rnd(C, 9, seed=62) * 0.5),
             isc=f32(rnd(C, seed=63, lo=-1.5, hi=1.5)), ish=f32(rnd(C, seed=64, lo=-0.3, hi=1.0)),
             gamma=f32(rnd(C, seed=65, lo=0.5, hi=1.5)), beta=f32(rnd(C, seed=66, lo=-0.5, hi=0.5)),
             rm0=f32(rnd(C, seed=67, lo=-0.5, hi=0.5)), rv0=f32(rnd(C, seed=68, lo=0.5, hi=1.5)))
    i["gamma"][::3] *= -1.0
    xd, wd, iscd, ishd, gd, bd = (dev(i[k]) for k in ("x", "w", "isc", "ish", "gamma", "beta"))
    parts = _lib.load().fscnn_dw3x3_parts(N, H, W, C, stride, code, 0)
    assert parts >= 1
    counters, tsum = _dw_scratch()
    o = dict(part=nans(parts * 3 * C), rm=dev(i["rm0"]), rv=dev(i["rv0"]),
             z=nans(N, Ho, Wo, C, dtype=dt), mean=nans(C), invstd=nans(C), scale=nans(C), shift=nans(C))
    nbt = torch.full((1,), 3, dtype=torch.int64, device=DEV)
    _lib.call("fscnn_dw3x3_fwd_train", P(xd), code, N, H, W, C, stride, P(wd),
              P(iscd) if lazy else None, P(ishd) if lazy else None, P(o["z"]), P(o["part"]),
              P(counters), P(tsum), P(gd), P(bd), P(o["rm"]), P(o["rv"]), P(nbt), _lib.c_float(0.1),
              P(o["mean"]), P(o["invstd"]), P(o["scale"]), P(o["shift"]), None, S())
    sync()
    assert int(counters.abs().sum().item()) == 0, "counters not left zero"
    assert int(nbt.item()) == 4
    return i, o


def run_dgrad_bn(dt, stride, H, W, C, mode):
    """fscnn_dw3x3_dgrad_bn -> (inputs, outputs)."""
    code = _lib.dtype_code(dt)
    Ho, Wo = osize(H, W, stride)
    M = N * H * W
    i = dict(dy=q(rnd(N, Ho, Wo, C, seed=71), dt), w=f32(rnd(C, 9, seed=72) * 0.5),
             zb=q(randn(N, H, W, C, seed=73) * 2 + 0.7, dt))
    i["tabs"] = bn_tables(i["zb"].double().reshape(M, C), 74, C)
    dyd, wd, zd = dev(i["dy"]), dev(i["w"]), dev(i["zb"])
    md, id_, sd, hd = (dev(t) for t in i["tabs"])
    parts = _lib.load().fscnn_dw3x3_parts(N, H, W, C, stride, code, 1)
    assert parts >= 1
    counters, tsum = _dw_scratch()
    o = dict(part=nans(parts * 2 * C), dx=nans(N, H, W, C, dtype=dt), dgamma=nans(C), dbeta=nans(C),
             coef=nans(2 * C))
    _lib.call("fscnn_dw3x3_dgrad_bn", P(dyd), code, N, H, W, C, stride, P(wd), P(o["dx"]), P(zd), P(md),
              P(id_), P(sd) if mode == 2 else None, P(hd) if mode == 2 else None, mode, P(o["part"]),
              P(counters), P(tsum), P(o["dgamma"]), P(o["dbeta"]), P(o["coef"]), None, S())
    sync()
    assert int(counters.abs().sum().item()) == 0, "counters not left zero"
    return i, o


def run_wgrad(dt, stride, H, W, C, lazy):
    """fscnn_dw3x3_wgrad_train over the lazy x, or fscnn_dw3x3_wgrad -> (inputs, outputs)."""
    code = _lib.dtype_code(dt)
    Ho, Wo = osize(H, W, stride)
    i = dict(x=q(randn(N, H, W, C, seed=161) * 2 + 0.7, dt), dy=q(rnd(N, Ho, Wo, C, seed=162), dt),
             xsc=f32(rnd(C, seed=163, lo=-1.5, hi=1.5)), xsh=f32(rnd(C, seed=164, lo=0.2, hi=1.5)))
    xd, dyd, scd, shd = dev(i["x"]), dev(i["dy"]), dev(i["xsc"]), dev(i["xsh"])
    o = dict(slab=nans(_lib.load().fscnn_dw3x3_wgrad_slab_floats(N, H, W, C, stride, code)), dw=nans(C, 9))
    if lazy:
        _lib.call("fscnn_dw3x3_wgrad_train", P(xd), P(dyd), code, N, H, W, C, stride, P(scd), P(shd),
                  P(o["slab"]), P(o["dw"]), S())
    else:
        _lib.call("fscnn_dw3x3_wgrad", P(xd), P(dyd), code, N, H, W, C, stride, P(o["slab"]),
                  P(o["dw"]), S())
    sync()
    return i, o


def run_plain(dt, stride, H, W, C):
    """fscnn_dw3x3_fwd (folded BN + ReLU, no statistics) and fscnn_dw3x3_dgrad -> (inputs, outputs)."""
    code = _lib.dtype_code(dt)
    Ho, Wo = osize(H, W, stride)
    i = dict(x=q(randn(N, H, W, C, seed=81), dt), w=f32(rnd(C, 9, seed=82) * 0.5),
             sc=f32(rnd(C, seed=83, lo=-1.5, hi=1.5)), sh=f32(rnd(C, seed=84, lo=-0.3, hi=1.0)),
             dy=q(rnd(N, Ho, Wo, C, seed=85), dt))
    xd, wd, scd, shd, dyd = (dev(i[k]) for k in ("x", "w", "sc", "sh", "dy"))
    o = dict(y=nans(N, Ho, Wo, C, dtype=dt), dx=nans(N, H, W, C, dtype=dt))
    _lib.call("fscnn_dw3x3_fwd", P(xd), code, N, H, W, C, stride, P(wd), P(scd), P(shd), 1, P(o["y"]), S())
    _lib.call("fscnn_dw3x3_dgrad", P(dyd), code, N, H, W, C, stride, P(wd), P(o["dx"]), S())
    sync()
    return i, o


def lazy_operand(x, sc, sh, dt):
    """relu(fmaf(x, sc, sh)) in fp32, rounded to T (bn_apply's value), as fp64."""
    return (x.double() * sc.double() + sh.double()).to(torch.float32).clamp_min(0.0).to(dt).double()


# ---- the tests --------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ALL, ids=cid)
def test_dw_paths_fwd_train(case):
    """z = conv(x) and conv(relu(BN(x))) applied on load (shift > 0 on most channels: a padded tap
    taken as relu(shift) instead of 0 shows at the border), the statistics of the stored z."""
    dt, stride, H, W, C = case
    for lazy in (1, 0):
        i, o = run_fwd_train(dt, stride, H, W, C, lazy)
        tag = "dw paths fwd_train %s lazy %d" % (cid(case), lazy)
        v = lazy_operand(i["x"], i["isc"], i["ish"], dt) if lazy else i["x"].double()
        w_ = i["w"].double().reshape(C, 1, 3, 3)
        vn = nchw(v)
        ref = F.conv2d(vn, w_, stride=stride, padding=1, groups=C)
        A = F.conv2d(vn.abs(), w_.abs(), stride=stride, padding=1, groups=C)
        check_elem(tag + " z", nchw(o["z"]), ref, A, dt)
        zs = d64(o["z"]).reshape(-1, C)
        Mz = zs.shape[0]
        mu, var = zs.mean(0), zs.var(0, unbiased=False)
        istd = 1.0 / torch.sqrt(var + 1e-5)
        gamma, beta = i["gamma"].double(), i["beta"].double()

        def close(what, got, ref_, tol):
            err = (d64(got) - ref_).abs().max().item()
            lim = tol * (ref_.abs().max().item() + 1e-12)
            report("%s %s" % (tag, what), err / lim)
            assert bool(torch.isfinite(got).all()) and err <= lim, "%s %s" % (tag, what)
        close("mean", o["mean"], mu, 1e-5)
        close("invstd", o["invstd"], istd, 1e-4)
        close("scale", o["scale"], gamma * istd, 1e-4)
        close("shift", o["shift"], beta - mu * gamma * istd, 1e-4)
        close("running_mean", o["rm"], 0.9 * i["rm0"].double() + 0.1 * mu, 1e-5)
        close("running_var", o["rv"], 0.9 * i["rv0"].double() + 0.1 * var * Mz / (Mz - 1), 1e-5)


@pytest.mark.parametrize("case", ALL, ids=cid)
def test_dw_paths_dgrad_bn(case):
    """dx plus the BN-backward sums of the STORED dx, modes 0 and 2 (stride 1: the flipped tile
    kernel; stride 2: the gather kernel)."""
    dt, stride, H, W, C = case
    M = N * H * W
    assert M <= M_MAX
    Ho, Wo = osize(H, W, stride)
    for mode in (0, 2):
        i, o = run_dgrad_bn(dt, stride, H, W, C, mode)
        tag = "dw paths dgrad_bn %s mode %d" % (cid(case), mode)
        w_ = i["w"].double().reshape(C, 1, 3, 3)
        gn = nchw(i["dy"].double())
        op = (H - ((Ho - 1) * stride + 1), W - ((Wo - 1) * stride + 1))
        ref = F.conv_transpose2d(gn, w_, stride=stride, padding=1, output_padding=op, groups=C)
        A = F.conv_transpose2d(gn.abs(), w_.abs(), stride=stride, padding=1, output_padding=op, groups=C)
        assert tuple(ref.shape) == (N, C, H, W)
        check_elem(tag + " dx", nchw(o["dx"]), ref, A, dt)
        mean, invstd, scale, shift = (t.double() for t in i["tabs"])
        zb_ = i["zb"].double().reshape(M, C)
        g = d64(o["dx"]).reshape(M, C)                      # the stored dx is that BN's dy
        if mode == 2:
            g = torch.where(zb_ * scale + shift > 0, g, torch.zeros_like(g))
        xhat = (zb_ - mean) * invstd
        check_sum(tag + " dbeta", o["dbeta"], g.sum(0), g.abs().sum(0))
        check_sum(tag + " dgamma", o["dgamma"], (g * xhat).sum(0), (g * xhat).abs().sum(0))
        torch.testing.assert_close(d64(o["coef"][:C]), d64(o["dbeta"]) / M, rtol=1e-6, atol=0)
        torch.testing.assert_close(d64(o["coef"][C:]), d64(o["dgamma"]) / M, rtol=1e-6, atol=0)


@pytest.mark.parametrize("case", ALL, ids=cid)
def test_dw_paths_wgrad(case):
    """dW[c][kh][kw] = sum dy x, over the lazy x (positive shifts: padding must stay zero, not
    relu(shift)) and over the stored x."""
    dt, stride, H, W, C = case
    Ho, Wo = osize(H, W, stride)
    for lazy in (1, 0):
        i, o = run_wgrad(dt, stride, H, W, C, lazy)
        x = lazy_operand(i["x"], i["xsc"], i["xsh"], dt) if lazy else i["x"].double()
        xu = F.unfold(nchw(x), 3, padding=1, stride=stride).reshape(N, C, 9, Ho * Wo)
        g = nchw(i["dy"].double()).reshape(N, C, 1, Ho * Wo)
        ref = (xu * g).sum((0, 3))
        bound = (N * Ho * Wo + 2) * E24 * (xu * g).abs().sum((0, 3))
        check_bound("dw paths wgrad %s lazy %d dW" % (cid(case), lazy), o["dw"], ref, bound)


@pytest.mark.parametrize("case", ALL, ids=cid)
def test_dw_paths_plain(case):
    """The eval forward (folded BN + ReLU in the epilogue) and the plain dgrad."""
    dt, stride, H, W, C = case
    Ho, Wo = osize(H, W, stride)
    i, o = run_plain(dt, stride, H, W, C)
    tag = "dw paths plain %s" % cid(case)
    w_ = i["w"].double().reshape(C, 1, 3, 3)
    xn = nchw(i["x"].double())
    sc, sh = i["sc"].double().reshape(1, C, 1, 1), i["sh"].double().reshape(1, C, 1, 1)
    ref = (F.conv2d(xn, w_, stride=stride, padding=1, groups=C) * sc + sh).clamp_min(0.0)
    A = F.conv2d(xn.abs(), w_.abs(), stride=stride, padding=1, groups=C) * sc.abs() + sh.abs()
    check_elem(tag + " y", nchw(o["y"]), ref, A, dt)
    gn = nchw(i["dy"].double())
    op = (H - ((Ho - 1) * stride + 1), W - ((Wo - 1) * stride + 1))
    ref = F.conv_transpose2d(gn, w_, stride=stride, padding=1, output_padding=op, groups=C)
    A = F.conv_transpose2d(gn.abs(), w_.abs(), stride=stride, padding=1, output_padding=op, groups=C)
    check_elem(tag + " dx", nchw(o["dx"]), ref, A, dt)


# ---- fast path against the generic kernels ------------------------------------------------------------

def worker_cases():
    """A handful of the cases above: per dtype and stride the 3-tiles-plus-one-pixel map at a
    compile-time width of each kind (cbv 4 or 6, and 8 in a multi-chunk grid) and the 3 x 5 map."""
    out = []
    for dt in DTS:
        for s in (1, 2):
            cs = cases(dt, s)
            H, W = cs[0][0], cs[0][1]
            out += [(dt, s, H, W, C) for C in ([24, 32] if dt == F32 else [32, 48, 576])]
            out.append((dt, s, 3, 5, 32 if dt == F32 else 64))
    return out


def _worker(tmp_path, switch):
    out = str(tmp_path / ("dw_%s.bin" % (switch or "default").replace("=", "_")))
    env = dict(os.environ)
    env.pop("FSCNN_DW_GENERIC", None)
    if switch:
        k, v = switch.split("=")
        env[k] = v
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_dw_paths_worker.py"), out],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    with open(out, "rb") as f:
        return json.loads(r.stdout.strip().splitlines()[-1])["widths"], f.read()


def _first_difference(a, b):
    """The header of the record in which two worker files first differ."""
    n = min(len(a), len(b))
    i = next((k for k in range(n) if a[k] != b[k]), n)
    heads = re.findall(rb"([\w\- .]+ torch\.\w+ \([\d, ]*\))\n", a[:i])
    return heads[-1].decode() if heads else "byte %d" % i


def test_dw_fast_path_matches_generic(tmp_path):
    """Every output, BN record and weight-gradient slab of the compile-time-cbv kernels is
    byte-equal to the run-time-cbv, bounds-checked kernels' (FSCNN_DW_GENERIC=1); the default run
    really took the compile-time kernels and the switch really took them away."""
    wf, fast = _worker(tmp_path, None)
    wg, gen = _worker(tmp_path, "FSCNN_DW_GENERIC=1")
    assert len(wf) == len(worker_cases()) and all(w in (4, 6, 8) for w in wf), wf
    assert {4, 6, 8} <= set(wf)
    assert wg == [0] * len(wf), wg
    assert len(fast) > 1 << 20
    assert fast == gen, "fast and generic paths differ, first in: %s" % _first_difference(fast, gen)
