"""Per-kernel parity of the kernels that only a train step runs, in fp32, bf16 and fp16, through
the C ABI in the executor's form (include/fastscnn.h, "kernels that only a train step runs"):
bn_apply, bn_bwd (reduce / finalize / apply, the paired FFM form), the PPM branch convs and
upsample both ways, dropout, and the train forms of the depthwise conv.

Operands are drawn on the CPU with fixed seeds and rounded to the storage type first, so they are
exact; the reference is fp64 torch on the CPU from the same operands, and from the kernel's own
stored intermediates where the kernel consumes them.  With u_T = 2^-8 (bf16), 2^-11 (fp16),
2^-24 (fp32):

* element-wise outputs stored in T: |err| <= u_T |ref| + 1e-6 A (+ 2^-24 for fp16 subnormals),
  A the sum of the absolute values of the expression's terms (fewer than 16 fp32 roundings each,
  16 x 2^-24 < 1e-6);
* ReLU masks are reproduced exactly: fmaf(z, scale, shift) > 0 has the sign of the fp64
  z*scale + shift (the product of two fp32 values is exact in fp64), y > 0 is read from the
  stored y; no near-tie exclusions;
* per-channel sums: |err| <= 2e-6 a + 1e-6, a the sum of |terms| (the bound of
  test_gpu_literal.py), coef = sum / M to rtol 1e-6; every such case has M <= 65539 so that
  2e-6 < 1 / (4 M): one dropped or doubled row of typical size cannot hide;
* PPM: z to u_T |ref| + 1e-5 max|ref| (16-bit) / 2e-4 max|ref| (fp32); its statistics, formed in
  fp64 by the kernel, to 1e-6 relative (+ 1e-7 max|z| for the mean-like values); the backward's
  dz is reproduced at the kernel's rounding points (fp64 -> fp32 -> T; where the one-step
  fp64 -> T rounding differs, an exact tie, either value is accepted: _ppm_run), dW is held to
  the fp32 accumulation bound (M + 2) 2^-24 sum_m |dz x| and dX to u_T |ref| + 34 x 2^-24
  sum_c |dz w|;
* ppm_up forward: A counts the terms of the fp32 lerp weights too (test_ppm_up_fwd); the
  backward's bound is derived in test_ppm_up_bwd.

Every check prints its worst error / bound ratio.  Measured on the MI355X (worst over all cases):
16-bit element-wise outputs 0.88 .. 0.997 (one storage rounding), fp32 element-wise <= 0.21,
per-channel sums <= 0.06, PPM statistics <= 0.18, PPM dW <= 0.92 and dX <= 0.994, ppm_up
backward <= 0.99 (16-bit) / 0.02 (fp32).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fast_scnn_pytorch_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTS = [F32, BF16, F16]
U = {F32: 2.0 ** -24, BF16: 2.0 ** -8, F16: 2.0 ** -11}
S = _lib.stream_ptr
P = _lib.ptr
M_MAX = 65539   # 2e-6 < 1 / (4 M): the per-channel sum bound resolves one row


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


def round_once(t64, dt):
    """fp64 -> T in one correctly rounded step (round to nearest even)."""
    if dt == F32:
        return t64.to(torch.float32).double()
    if dt == F16:   # numpy converts double -> half directly (torch goes through float)
        return torch.from_numpy(t64.numpy().astype(np.float16).astype(np.float64))
    m, e = torch.frexp(t64)                       # bf16: 8 significant bits (normal range)
    return torch.ldexp(torch.round(m * 256.0), e - 8)


def dev(t):
    return t.contiguous().to(DEV)


def f32(t):
    return t.to(torch.float32)


def d64(t):
    return t.detach().to("cpu").double()


def padded(t2d, ld, fill):
    """[M][C] -> a [M][ld] buffer (ld >= C) whose pad columns hold `fill`, and the device copy."""
    M, C = t2d.shape
    buf = torch.full((M, ld), fill, dtype=t2d.dtype)
    buf[:, :C] = t2d
    return dev(buf)


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
    """|got - ref| <= bound element by element; a failure names the worst element."""
    got, ref, bound = d64(got), d64(ref), d64(bound)
    assert bool(torch.isfinite(got).all()), "%s: non-finite output" % what
    r = (got - ref).abs() / bound.clamp_min(1e-300)
    report(what, r.max().item())
    if bool((r > 1).any()):
        i = int(r.argmax())
        idx = tuple(int(v) for v in np.unravel_index(i, tuple(r.shape)))
        raise AssertionError("%s: %d of %d elements out of bound; worst at %s: got %.9e ref %.9e bound %.3e"
                             % (what, int((r > 1).sum()), r.numel(), idx, got.flatten()[i].item(),
                                ref.flatten()[i].item(), bound.flatten()[i].item()))


def check_sum(what, got, ref, a):
    """A per-channel fp32 sum against fp64: 2e-6 a + 1e-6."""
    got, ref, a = d64(got), d64(ref), d64(a)
    bound = 2e-6 * a + 1e-6
    err = (got - ref).abs()
    assert bool(torch.isfinite(got).all()), "%s: non-finite output" % what
    ratio = (err / bound).max().item()
    report(what, ratio)
    assert ratio <= 1.0, "%s: worst err / bound %.3f" % (what, ratio)


def check_rel(what, got, ref, rtol, atol=0.0):
    got, ref = d64(got), d64(ref)
    bound = rtol * ref.abs() + atol
    err = (got - ref).abs()
    assert bool(torch.isfinite(got).all()), "%s: non-finite output" % what
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    report(what, ratio)
    assert bool((err <= bound).all()), "%s: worst err / bound %.3f" % (what, ratio)


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


# ---- bn_apply ---------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTS, ids=dname)
@pytest.mark.parametrize("M,C", [(37, 32), (1043, 48), (523, 576)])
def test_bn_apply(dt, M, C):
    """y = act(z*scale + shift [+ z2*scale2 + shift2] [+ res]): plain, the FFM's second branch, a
    shortcut, and row strides != C on every operand (pad columns of y stay untouched)."""
    z = q(randn(M, C, seed=1) * 2 + 0.7, dt)
    z2 = q(randn(M, C, seed=2), dt)
    res = q(rnd(M, C, seed=3, lo=-2, hi=2), dt)
    sc, sc2 = f32(rnd(C, seed=4, lo=-1.5, hi=1.5)), f32(rnd(C, seed=5, lo=-1.5, hi=1.5))
    sh, sh2 = f32(rnd(C, seed=6)), f32(rnd(C, seed=7))
    scd, shd, sc2d, sh2d = dev(sc), dev(sh), dev(sc2), dev(sh2)
    z_, z2_, r_ = z.double(), z2.double(), res.double()
    t1 = z_ * sc.double()
    t2 = z2_ * sc2.double()
    for name, use2, user, relu, strided in [("plain", 0, 0, 1, 0), ("no relu", 0, 0, 0, 0),
                                            ("second branch", 1, 0, 1, 0), ("residual", 0, 1, 0, 0),
                                            ("both, strided", 1, 1, 1, 1), ("plain, strided", 0, 0, 1, 1)]:
        ldz, ldz2, ldr, ldy = (C + 8, C + 16, C + 24, C + 32) if strided else (C, C, C, C)
        zd, z2d, rd = padded(z, ldz, 1e4), padded(z2, ldz2, 1e4), padded(res, ldr, 1e4)
        y = torch.full((M, ldy), 7.0, dtype=dt, device=DEV)
        _lib.call("fscnn_bn_apply", M, C, P(zd), ldz, P(scd), P(shd), P(z2d) if use2 else None, ldz2,
                  P(sc2d) if use2 else None, P(sh2d) if use2 else None, P(rd) if user else None, ldr,
                  relu, P(y), ldy, _lib.dtype_code(dt), S())
        sync()
        ref = t1 + sh.double()
        A = t1.abs() + sh.double().abs()
        if use2:
            ref = ref + t2 + sh2.double()
            A = A + t2.abs() + sh2.double().abs()
        if user:
            ref = ref + r_
            A = A + r_.abs()
        if relu:
            ref = ref.clamp_min(0.0)
        check_elem("bn_apply %s (%d, %d) %s" % (dname(dt), M, C, name), y[:, :C], ref, A, dt)
        assert bool((y[:, C:] == 7.0).all()), "bn_apply wrote past C"


# ---- bn_bwd -----------------------------------------------------------------------------------

def _bn_bwd_call(dt, M, C, dyd, lddy, mkd, ldmask, zd, tabs, mode, frozen, pair=None):
    """One fscnn_bn_bwd call with NaN-filled records; returns the outputs and (P, rows)."""
    mean, invstd, scale, shift = tabs
    part = torch.full((2048 * 2 * C * (2 if pair else 1),), float("nan"), device=DEV)
    counters = torch.zeros(512, dtype=torch.int32, device=DEV)
    dz = torch.full((M, C), float("nan"), dtype=dt, device=DEV)
    dgamma, dbeta = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
    coef = torch.full((4 * C,), float("nan"), device=DEV)
    dz2 = dgamma2 = dbeta2 = None
    z2d = m2 = i2 = s2 = None
    if pair:
        z2d, (m2, i2, s2) = pair
        dz2 = torch.full((M, C), float("nan"), dtype=dt, device=DEV)
        dgamma2, dbeta2 = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
    Pn, rpb = _lib.c_int(-1), _lib.c_int(-1)
    _lib.call("fscnn_bn_bwd", M, C, P(dyd), lddy, P(mkd) if mode == 1 else None, ldmask, P(zd),
              P(mean), P(invstd), P(scale), P(shift), mode, frozen, P(z2d), P(m2), P(i2), P(s2),
              P(part), P(counters), P(dz), P(dz2), P(dgamma), P(dbeta), P(dgamma2), P(dbeta2),
              P(coef), _lib.dtype_code(dt), _lib.ctypes.byref(Pn), _lib.ctypes.byref(rpb), S())
    sync()
    assert int(counters.abs().sum().item()) == 0, "arrival counters not left zero"
    # the reduce wrote every record it reported (they were NaN) ...
    recs = part[:Pn.value * 2 * C * (2 if pair else 1)]
    assert Pn.value >= 1 and rpb.value >= 1 and (Pn.value - 1) * rpb.value < M <= Pn.value * rpb.value
    # ... (folded records are rewritten in place, so only finiteness is checked)
    assert bool(torch.isfinite(recs).all()), "an unwritten BN-backward record"
    return dz, dz2, dgamma, dbeta, dgamma2, dbeta2, coef, Pn.value, rpb.value


def _bn_sums(gm, z_, mean, invstd):
    """fp64 reference sums of the masked gradient gm: (xhat, s1, a1, s2, a2)."""
    xhat = (z_ - mean) * invstd
    t = gm * xhat
    return xhat, gm.sum(0), gm.abs().sum(0), t.sum(0), t.abs().sum(0)


def _bn_bwd_check(tag, dt, M, C, gm, sums, scale, frozen, dz, dgamma, dbeta, coef):
    """dbeta / dgamma against the fp64 sums, the coefficients, and dz from the stored
    coefficients."""
    xhat, s1, a1, s2, a2 = sums
    check_sum(tag + " dbeta", dbeta, s1, a1)
    check_sum(tag + " dgamma", dgamma, s2, a2)
    c0, c1 = d64(coef[:C]), d64(coef[C:2 * C])
    if frozen:
        assert bool((c0 == 0).all()) and bool((c1 == 0).all()), tag + ": frozen coefficients not zero"
    else:
        torch.testing.assert_close(c0, d64(dbeta) / M, rtol=1e-6, atol=0)
        torch.testing.assert_close(c1, d64(dgamma) / M, rtol=1e-6, atol=0)
    t = xhat * c1
    ref = scale * (gm - c0 - t)
    A = scale.abs() * (gm.abs() + c0.abs() + t.abs())
    check_elem(tag + " dz", dz, ref, A, dt)


BN_BWD_CASES = [(1, 32, DTS), (37, 32, DTS), (37, 48, DTS),
                (523, 128, [F32]), (1043, 128, [BF16, F16]),     # P > 64: the fold level
                (300, 576, DTS),                                 # partial last channel block
                (11001, 384, DTS)]                               # fp32: the U = 4 apply sweep


@pytest.mark.parametrize("M,C,dt", [(M, C, dt) for M, C, dts in BN_BWD_CASES for dt in dts],
                         ids=lambda v: dname(v) if isinstance(v, torch.dtype) else str(v))
def test_bn_bwd(M, C, dt):
    """reduce -> finalize -> apply in the executor's order: modes 0 (no ReLU), 1 (mask tensor),
    2 (mask recomputed from z); train, frozen statistics (the executor's form: zero coefficients
    passed to the apply) and the apply's own no-coefficient form."""
    assert M <= M_MAX
    z = q(randn(M, C, seed=11) * 2 + 0.7, dt)
    dy = q(rnd(M, C, seed=12), dt)
    z_, g_ = z.double(), dy.double()
    tabs = bn_tables(z_, 13, C)
    mean, invstd, scale, shift = (t.double() for t in tabs)
    pre = z_ * scale + shift                      # sign = that of fmaf(z, scale, shift)
    mk = q(pre.clamp_min(0.0), dt)                # the saved ReLU output (mode 1 reads mk > 0)
    lddy, ldmask = C + 8, C + 16
    dyd, mkd, zd = padded(dy, lddy, 1e4), padded(mk, ldmask, 1e4), dev(z)
    tabs_d = tuple(dev(t) for t in tabs)
    masks = {0: torch.ones(M, C, dtype=torch.bool), 1: mk.double() > 0, 2: pre > 0}
    for mode in (0, 1, 2):
        gm = torch.where(masks[mode], g_, torch.zeros_like(g_))
        sums = _bn_sums(gm, z_, mean, invstd)
        for frozen in (0, 1, 2):
            dz, _, dgamma, dbeta, _, _, coef, Pn, rpb = _bn_bwd_call(
                dt, M, C, dyd, lddy, mkd, ldmask, zd, tabs_d, mode, frozen)
            if M in (523, 1043):
                assert Pn > 64, "expected the fold level (P = %d)" % Pn
            tag = "bn_bwd %s (%d, %d) mode %d frozen %d P %d" % (dname(dt), M, C, mode, frozen, Pn)
            _bn_bwd_check(tag, dt, M, C, gm, sums, scale, frozen, dz, dgamma, dbeta, coef)


@pytest.mark.parametrize("dt", DTS, ids=dname)
@pytest.mark.parametrize("M", [37, 65539])
def test_bn_bwd_pair(dt, M):
    """The FeatureFusionModule's two BNs on one dy and one mask: one reduce, two finishes, one
    apply."""
    C = 128
    assert M <= M_MAX
    z = q(randn(M, C, seed=21) * 2 + 0.7, dt)
    z2 = q(randn(M, C, seed=22) * 0.5 - 1.1, dt)
    dy = q(rnd(M, C, seed=23), dt)
    z_, z2_, g_ = z.double(), z2.double(), dy.double()
    tabs, tabs2 = bn_tables(z_, 24, C), bn_tables(z2_, 26, C)
    m1, i1, s1, b1 = (t.double() for t in tabs)
    m2, i2, s2, b2 = (t.double() for t in tabs2)
    mk = q((z_ * s1 + b1 + z2_ * s2 + b2).clamp_min(0.0), dt)   # f = relu(BN_l + BN_h)
    gm = torch.where(mk.double() > 0, g_, torch.zeros_like(g_))
    lddy, ldmask = C + 8, C + 16
    dyd, mkd = padded(dy, lddy, 1e4), padded(mk, ldmask, 1e4)
    tabs_d = tuple(dev(t) for t in tabs)
    pair = (dev(z2), tuple(dev(t) for t in tabs2[:3]))
    sums1, sums2 = _bn_sums(gm, z_, m1, i1), _bn_sums(gm, z2_, m2, i2)
    for frozen in (0, 1):
        dz, dz2, dgamma, dbeta, dgamma2, dbeta2, coef, Pn, rpb = _bn_bwd_call(
            dt, M, C, dyd, lddy, mkd, ldmask, dev(z), tabs_d, 1, frozen, pair)
        tag = "bn_bwd pair %s M %d frozen %d P %d" % (dname(dt), M, frozen, Pn)
        _bn_bwd_check(tag + " [1]", dt, M, C, gm, sums1, s1, frozen, dz, dgamma, dbeta, coef[:2 * C])
        _bn_bwd_check(tag + " [2]", dt, M, C, gm, sums2, s2, frozen, dz2, dgamma2, dbeta2, coef[2 * C:])
        assert torch.equal(dbeta, dbeta2), "the shared sum of dy_r differs between the two BNs"


# ---- PPM branch convs -------------------------------------------------------------------------

BINS = (1, 4, 9, 36)


def _ppm_inputs(dt, Ms, K, seed):
    R, nb = sum(Ms), len(Ms)
    x = q(rnd(R, K, seed=seed), dt)
    w = q(rnd(nb, 32, K, seed=seed + 1) / K ** 0.5 * 1.7, dt)
    gamma = f32(rnd(nb, 32, seed=seed + 2, lo=0.5, hi=1.5))
    gamma[:, 2::7] *= -1.0
    beta = f32(rnd(nb, 32, seed=seed + 3, lo=-0.5, hi=0.5))
    rm0 = f32(rnd(nb, 32, seed=seed + 4, lo=-0.5, hi=0.5))
    rv0 = f32(rnd(nb, 32, seed=seed + 5, lo=0.5, hi=1.5))
    # gradients of magnitude 64: fp16 training scales its loss (GradScaler) to keep gradients
    # inside the format's normal range, and the pool-1 BN over two values shrinks dz to ~1e-4 |dy|;
    # a dz below 2^-14 is an fp16 subnormal, outside the relative-rounding model of the bounds
    # (measured: the fp16 matrix-core dW of a channel whose dz are all subnormal is off by up to
    # 1.5 x 2^-40 absolute, 16 fp32 ulps of a 5e-7 sum)
    dy = q(rnd(R, 32, seed=seed + 6, lo=-64.0, hi=64.0), dt)
    return x, w, gamma, beta, rm0, rv0, dy


def _ppm_run(dt, Ms, K):
    """Forward then backward through the C ABI; every check of both."""
    nb, R = len(Ms), sum(Ms)
    tagb = "ppm %s M=%s K=%d" % (dname(dt), list(Ms), K)
    x, w, gamma, beta, rm0, rv0, dy = _ppm_inputs(dt, Ms, K, 31)
    Marr = (_lib.c_int * nb)(*Ms)
    ldy, lddy = 48, 40
    xd, wd, gd, bd = dev(x), dev(w), dev(gamma), dev(beta)
    rm, rv = dev(rm0), dev(rv0)
    nbt = torch.full((nb,), 5, dtype=torch.int64, device=DEV)
    z = torch.full((R, 32), float("nan"), dtype=dt, device=DEV)
    y = torch.full((R, ldy), 7.0, dtype=dt, device=DEV)
    mean, invstd, scale, shift = (torch.full((nb, 32), float("nan"), device=DEV) for _ in range(4))
    code = _lib.dtype_code(dt)
    assert _lib.load().fscnn_ppm_branches_ok(max(Ms), K, code) == 1
    _lib.call("fscnn_ppm_branches_fwd", nb, Marr, K, P(xd), P(wd), P(gd), P(bd), P(rm), P(rv), P(nbt),
              _lib.c_float(0.1), P(z), P(y), ldy, P(mean), P(invstd), P(scale), P(shift), code, S())
    dyd = padded(dy, lddy, 1e4)
    dgamma, dbeta = (torch.full((nb, 32), float("nan"), device=DEV) for _ in range(2))
    dw = torch.full((nb, 32, K), float("nan"), device=DEV)
    dx = torch.full((R, K), float("nan"), dtype=dt, device=DEV)
    _lib.call("fscnn_ppm_branches_bwd", nb, Marr, K, P(dyd), lddy, P(y), ldy, P(z), P(mean), P(invstd),
              P(scale), P(gd), P(xd), P(wd), P(dgamma), P(dbeta), P(dw), P(dx), code, S())
    sync()
    assert nbt.tolist() == [6] * nb
    assert bool((y[:, 32:] == 7.0).all()), "ppm forward wrote past 32 channels of y"
    x_, w_, zs, ys = x.double(), w.double(), d64(z), d64(y[:, :32])
    r0 = 0
    for i, Mi in enumerate(Ms):
        tag = "%s branch %d (M %d)" % (tagb, i, Mi)
        rows = slice(r0, r0 + Mi)
        r0 += Mi
        # forward: the conv output
        zr = x_[rows] @ w_[i].t()
        err = (zs[rows] - zr).abs()
        zb = (U[dt] * zr.abs() + 1e-5 * zr.abs().max()) if dt != F32 else (2e-4 * zr.abs().max()).expand_as(zr)
        report(tag + " z", (err / zb).max().item())
        assert bool((err <= zb).all()), tag + " z"
        # statistics, in fp64 from the stored z
        zi = zs[rows]
        zmax = zi.abs().max().item()
        mu = zi.mean(0)
        var = ((zi - mu) ** 2).mean(0)
        istd = 1.0 / torch.sqrt(var + 1e-5)
        sc = gamma[i].double() * istd
        check_rel(tag + " mean", mean[i], mu, 1e-6, 1e-7 * zmax)
        check_rel(tag + " invstd", invstd[i], istd, 1e-6)
        check_rel(tag + " scale", scale[i], sc, 1e-6)
        check_rel(tag + " shift", shift[i], beta[i].double() - mu * sc, 1e-6, 1e-7 * zmax)
        # running_mean = 0.9 rm0 + 0.1 mean in fp32: three roundings, 2^-24 (0.45 + 0.1 max|z| +
        # |ref|) <= 1e-6 |ref| + 1e-7 max|z| for max|z| >= 0.3 (asserted): the mean's bound
        assert zmax >= 0.3
        check_rel(tag + " running_mean", rm[i], 0.9 * rm0[i].double() + 0.1 * mu, 1e-6, 1e-7 * zmax)
        unb = var * Mi / (Mi - 1) if Mi > 1 else var
        check_rel(tag + " running_var", rv[i], 0.9 * rv0[i].double() + 0.1 * unb, 1e-6)
        # y = relu(fmaf(z, scale, shift)) from the stored tables
        sck, shk = d64(scale[i]), d64(shift[i])
        pre = zi * sck + shk
        check_elem(tag + " y", ys[rows], pre.clamp_min(0.0), (zi * sck).abs() + shk.abs(), dt)
        # backward: the kernel's rounding points (fp64 from the stored z, y, dy; dz fp64 -> fp32 -> T)
        gmi = torch.where(ys[rows] > 0, dy[rows].double(), torch.zeros(Mi, 32, dtype=torch.float64))
        xh = (zi - mu) * istd
        s1, s2 = gmi.sum(0), (gmi * xh).sum(0)
        check_sum(tag + " dbeta", dbeta[i], s1, gmi.abs().sum(0))
        check_sum(tag + " dgamma", dgamma[i], s2, (gmi * xh).abs().sum(0))
        dz64 = sc * (gmi - s1 / Mi - xh * (s2 / Mi))
        dz = dz64.to(torch.float32).to(dt).double()
        # The source rounds dz as round_as<T>((float) fp64).  The compiler may merge the two
        # conversions into one correctly rounded fp64 -> T step (the gfx950 fp16 kernels hold no
        # fp64 -> fp32 conversion for dz); the two differ only where the fp32 value is an exact
        # tie of T (about 2^-13 of the elements in fp16: e.g. 1.25927733... -> 1.2597656 through
        # fp32, 1.2587891 directly).  Either is one rounding of the fp64 dz, so where they differ
        # the kernel may hold either and the products' bounds grow by |difference| there.
        tie = (dz - round_once(dz64, dt)).abs()
        print("%s dz: %d of %d elements are ties of the two roundings" % (tag, int((tie > 0).sum()), tie.numel()))
        xi = x_[rows]
        dwr = dz.t() @ xi
        dwb = (Mi + 2) * 2.0 ** -24 * (dz.abs().t() @ xi.abs()) + tie.t() @ xi.abs()
        check_bound(tag + " dW", dw[i], dwr, dwb)
        dxr = dz @ w_[i]
        # (dX is stored in T: + 2^-24 for fp16 subnormals, as for every element-wise output)
        dxb = (U[dt] * dxr.abs() + 34 * 2.0 ** -24 * (dz.abs() @ w_[i].abs()) + tie @ w_[i].abs()
               + (2.0 ** -24 if dt == F16 else 0.0))
        check_bound(tag + " dX", dx[rows], dxr, dxb)


@pytest.mark.parametrize("dt", DTS, ids=dname)
@pytest.mark.parametrize("N", [2, 3, 4, 6, 8, 9, 14])
def test_ppm_branches(dt, N):
    """K = 128, branch rows N x {1, 4, 9, 36}.  N = 2: the pool-1 BN over two values (ill
    conditioned: the fp64 in-kernel BN must still match); 3: odd, rows no multiple of 16; 4 / 6 / 8:
    the 16-bit matrix-core backward with 2 / 3 / 4 workgroups per branch (8: its 288-row limit);
    9 and 14: 16-bit falls back to the FMA backward (14: 504 rows, near the 512 limit)."""
    _ppm_run(dt, tuple(N * b for b in BINS), 128)


@pytest.mark.parametrize("dt", DTS, ids=dname)
def test_ppm_branches_k64(dt):
    """The generic (K != 128) forms the launcher accepts."""
    _ppm_run(dt, tuple(3 * b for b in BINS), 64)


@pytest.mark.parametrize("dt", DTS, ids=dname)
def test_ppm_branches_refuse_batch_15(dt):
    """540 rows: ppm_branches_ok is false and both calls return an error without a launch."""
    Ms = tuple(15 * b for b in BINS)
    code = _lib.dtype_code(dt)
    assert _lib.load().fscnn_ppm_branches_ok(max(Ms), 128, code) == 0
    Marr = (_lib.c_int * 4)(*Ms)
    t = torch.zeros(16, device=DEV)
    with pytest.raises(RuntimeError, match="fscnn_ppm_branches_fwd"):
        _lib.call("fscnn_ppm_branches_fwd", 4, Marr, 128, *([P(t)] * 7), _lib.c_float(0.1), P(t), P(t),
                  32, *([P(t)] * 4), code, S())
    with pytest.raises(RuntimeError, match="fscnn_ppm_branches_bwd"):
        _lib.call("fscnn_ppm_branches_bwd", 4, Marr, 128, P(t), 32, P(t), 32, *([P(t)] * 11), code, S())
    sync()
    assert bool((t == 0).all())


# ---- PPM upsample -----------------------------------------------------------------------------

LEVELS = (1, 2, 3, 6)
BASE = (0, 1, 5, 14)


UP_SHAPES = [(2, 3, 5), (3, 32, 64), (2, 65, 7), (1, 80, 9)]


def _level(feats, lv, N):
    """Level lv of the bin-major feats [50][N][32] as NCHW fp64 [N][32][k][k]."""
    k = LEVELS[lv]
    return feats[BASE[lv]:BASE[lv] + k * k].double().reshape(k, k, N, 32).permute(2, 3, 0, 1).contiguous()


def _axis_terms(k, L):
    """align_corners taps of one axis, output length L from k bins: indices (i0, i1) and the sums
    of the absolute values of the terms each weight is made of.  The kernel (as aten) forms
    pos = scale * o, l1 = pos - i0, l0 = 1 - l1 in fp32: l1 has the terms pos and i0, l0 the terms
    1, pos and i0.  (k == L: the identity, l0 = 1 and l1 = 0 exactly.)"""
    o = torch.arange(L, dtype=torch.float64)
    if k == L:
        i0 = o.long()
        return i0, i0, torch.ones(L, dtype=torch.float64), torch.zeros(L, dtype=torch.float64)
    pos = o * ((k - 1) / (L - 1) if L > 1 else 0.0)
    i0 = pos.floor().long().clamp_max(k - 1)
    i1 = (i0 + 1).clamp_max(k - 1)
    t = pos + i0.double()
    return i0, i1, 1.0 + t, t


@pytest.mark.parametrize("dt", DTS, ids=dname)
@pytest.mark.parametrize("N,H,W", UP_SHAPES)
def test_ppm_up_fwd(dt, N, H, W):
    """The four levels into channels [128, 256) of a 256-wide concat row against F.interpolate
    (bilinear, align_corners=True) in fp64.  A, the sum of the absolute values of the expression's
    terms, counts the terms of the lerp weights too (_axis_terms): a weight is a difference of
    rounded fp32 values as large as k - 1 = 5, so its rounding error is relative to those, not to
    the weight.  (With A = sum |weight x tap| alone the fp32 kernel measured up to 6.6x the bound
    at (2, 65, 7) level 3, where an exact position 1.0 evaluates to 0.99999994 in fp32 and the
    two taps trade places; 16-bit stayed below 0.6.)"""
    ldy, coff = 256, 128
    feats = q(rnd(50, N, 32, seed=41), dt)
    fd = dev(feats)
    y = torch.full((N, H, W, ldy), 7.0, dtype=dt, device=DEV)
    _lib.call("fscnn_ppm_up_fwd", P(fd), _lib.dtype_code(dt), N, H, W, P(y), ldy, coff, S())
    sync()
    assert bool((y[..., :coff] == 7.0).all()), "ppm_up_fwd wrote outside its channel slice"
    for lv, k in enumerate(LEVELS):
        f = _level(feats, lv, N)
        ref = F.interpolate(f, (H, W), mode="bilinear", align_corners=True)
        ih0, ih1, LH0, LH1 = _axis_terms(k, H)
        iw0, iw1, LW0, LW1 = _axis_terms(k, W)
        fa = f.abs()
        A = torch.zeros_like(ref)
        for ih, LHa in ((ih0, LH0), (ih1, LH1)):
            for iw, LWb in ((iw0, LW0), (iw1, LW1)):
                A += fa[:, :, ih][:, :, :, iw] * LHa[:, None] * LWb[None, :]
        sl = slice(coff + 32 * lv, coff + 32 * lv + 32)
        check_elem("ppm_up %s (%d, %d, %d) fwd level %d" % (dname(dt), N, H, W, k),
                   y[..., sl].permute(0, 3, 1, 2), ref, A, dt)


@pytest.mark.parametrize("dt", DTS, ids=dname)
@pytest.mark.parametrize("N,H,W", UP_SHAPES)
def test_ppm_up_bwd(dt, N, H, W):
    """dfeats from the [128, 256) slice of a gradient buffer whose other channels hold non-zero
    values, against the autograd of the same interpolate in fp64.  (2, 65, 7) and (1, 80, 9): the
    second 64-row pass."""
    ldy, coff = 256, 128
    g = q(rnd(N, H, W, ldy, seed=42), dt)       # non-zero everywhere
    gd = dev(g)
    dfe = torch.full((50, N, 32), float("nan"), dtype=dt, device=DEV)
    _lib.call("fscnn_ppm_up_bwd", P(gd), _lib.dtype_code(dt), N, H, W, ldy, coff, P(dfe), S())
    sync()
    for lv, k in enumerate(LEVELS):
        tag = "ppm_up %s (%d, %d, %d) bwd level %d" % (dname(dt), N, H, W, k)
        sl = slice(coff + 32 * lv, coff + 32 * lv + 32)
        gl = g[..., sl].double().permute(0, 3, 1, 2).contiguous()
        f = torch.zeros(N, 32, k, k, dtype=torch.float64, requires_grad=True)
        F.interpolate(f, (H, W), mode="bilinear", align_corners=True).backward(gl)
        fa = torch.zeros(N, 32, k, k, dtype=torch.float64, requires_grad=True)
        F.interpolate(fa, (H, W), mode="bilinear", align_corners=True).backward(gl.abs())
        a = fa.grad                                            # sum |w g|
        G = gl.abs().sum((2, 3), keepdim=True)                 # sum |g| over the map
        # fp32 sums in a fixed order: a thread adds <= ceil(W / 8) products of its row (one fma
        # each), three butterfly adds join the 8 column segments, then H multiply-adds run down the
        # rows: (H + W / 8 + 8) 2^-24 a.  The kernel's lerp weights are fp32 (scale = (k-1)/(L-1),
        # pos = scale * o: two roundings of a value <= k - 1 = 5), so each differs from the fp64
        # weight by <= 10 x 2^-24 per axis: 20 x 2^-24 sum |g|.  Stored in T: u_T |ref| (+ 2^-24
        # for fp16 subnormals).
        bound = (U[dt] * f.grad.abs() + (H + W / 8 + 8) * 2.0 ** -24 * a + 20 * 2.0 ** -24 * G
                 + (2.0 ** -24 if dt == F16 else 0.0))
        got = dfe[BASE[lv]:BASE[lv] + k * k].reshape(k, k, N, 32).permute(2, 3, 0, 1)
        check_bound(tag, got, f.grad, bound)


# ---- dropout ----------------------------------------------------------------------------------

def _oracle_keep(seed, N, H, W, C, p):
    from oracle.fast_scnn_ref import dropout_mask
    return dropout_mask(seed, (N, C, H, W), p).permute(0, 2, 3, 1).reshape(N * H * W, C)


def _dropout(dt, N, H, W, C, x, ldx, p, seed=0, slot=None, add=0, xs=None, xh=None, ldy=None):
    ldy = ldy or C
    y = torch.full((N * H * W, ldy), 7.0, dtype=dt, device=DEV)
    _lib.call("fscnn_dropout", P(x), ldx, _lib.dtype_code(dt), N, H, W, C, seed, P(slot), add,
              _lib.c_float(p), P(xs), P(xh), P(y), ldy, S())
    sync()
    assert bool((y[:, C:] == 7.0).all()), "dropout wrote past C"
    return y[:, :C]


@pytest.mark.parametrize("dt", DTS, ids=dname)
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("N,H,W", [(2, 3, 5), (3, 12, 20), (1, 131, 313)])
def test_dropout(dt, p, N, H, W):
    """(1, 131, 313): 41,003 pixels, 5 (fp32) / 2 (16-bit) pixels per thread, so the 4-pixel sweep
    runs whole and partial batches."""
    C, M, seed = 128, N * H * W, 0x1234567 + N
    v = rnd(M, C, seed=51, lo=0.1, hi=2.0) * torch.where(rnd(M, C, seed=52) < 0, -1.0, 1.0)
    x = q(v, dt)
    ldx = C + 8
    xd = padded(x, ldx, 1e4)
    keep = _oracle_keep(seed, N, H, W, C, p)
    tag = "dropout %s (%d, %d, %d) p %.1f" % (dname(dt), N, H, W, p)
    y = _dropout(dt, N, H, W, C, xd, ldx, p, seed=seed, ldy=C + 16)
    # the keep mask bit for bit (no operand is zero and none underflows)
    assert torch.equal((y != 0).cpu(), keep), tag + ": keep mask differs from the oracle"
    ref = torch.where(keep, x.double() / (1.0 - float(np.float32(p))), torch.zeros(M, C, dtype=torch.float64))
    check_elem(tag, y, ref, ref.abs(), dt)
    # seed_add = 1 is the oracle's seed + 1; the device slot equals the seed by value
    y1 = _dropout(dt, N, H, W, C, xd, ldx, p, seed=seed, add=1)
    assert torch.equal((y1 != 0).cpu(), _oracle_keep(seed + 1, N, H, W, C, p)), tag + ": seed_add"
    slot = torch.tensor([seed], dtype=torch.int64, device=DEV)
    ys = _dropout(dt, N, H, W, C, xd, ldx, p, seed=99, slot=slot, ldy=C + 16)
    assert torch.equal(ys, y), tag + ": the seed by device slot differs from the seed by value"
    # lazy BN+ReLU form == dropout of bn_apply's stored output
    sc, sh = dev(f32(rnd(C, seed=53, lo=-1.5, hi=1.5))), dev(f32(rnd(C, seed=54)))
    a = torch.empty(M, C, dtype=dt, device=DEV)
    _lib.call("fscnn_bn_apply", M, C, P(xd), ldx, P(sc), P(sh), None, 0, None, None, None, 0, 1, P(a), C,
              _lib.dtype_code(dt), S())
    ya = _dropout(dt, N, H, W, C, a, C, p, seed=seed)
    yl = _dropout(dt, N, H, W, C, xd, ldx, p, seed=seed, xs=sc, xh=sh)
    assert torch.equal(ya, yl), tag + ": x_scale form differs from dropout(bn_apply(x))"
    kept = (ya != 0).cpu()
    assert bool((kept <= keep).all()) and bool(kept.any()), tag + ": x_scale form keeps dropped elements"


# ---- depthwise conv, train forms ----------------------------------------------------------------

DW_SHAPES = [(2, 17, 23, 32), (3, 9, 8, 48), (1, 31, 63, 384), (2, 16, 32, 128)]


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _dw_scratch():
    return (torch.zeros(512, dtype=torch.int32, device=DEV),
            torch.zeros(32 * 3 * 1024, dtype=torch.float64, device=DEV))


@pytest.mark.parametrize("dt", DTS, ids=dname)
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("N,H,W,C", DW_SHAPES)
def test_dw3x3_fwd_train(dt, stride, N, H, W, C):
    """z = conv(relu(BN(x))) with the input BN+ReLU applied on load (shift > 0 on most channels:
    a padded tap taken as relu(shift) instead of 0 shows at the border), the BN statistics
    records of the stored z and their finish."""
    code = _lib.dtype_code(dt)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = q(randn(N, H, W, C, seed=61), dt)
    w = f32(rnd(C, 9, seed=62) * 0.5)
    isc = f32(rnd(C, seed=63, lo=-1.5, hi=1.5))
    ish = f32(rnd(C, seed=64, lo=-0.3, hi=1.0))
    gamma = f32(rnd(C, seed=65, lo=0.5, hi=1.5))
    gamma[::3] *= -1.0
    beta = f32(rnd(C, seed=66, lo=-0.5, hi=0.5))
    rm0, rv0 = f32(rnd(C, seed=67, lo=-0.5, hi=0.5)), f32(rnd(C, seed=68, lo=0.5, hi=1.5))
    xd, wd, iscd, ishd, gd, bd = dev(x), dev(w), dev(isc), dev(ish), dev(gamma), dev(beta)
    w_ = w.double().reshape(C, 1, 3, 3)
    for lazy in (1, 0):
        parts = _lib.load().fscnn_dw3x3_parts(N, H, W, C, stride, code, 0)
        assert parts >= 1
        part = torch.full((parts * 3 * C,), float("nan"), device=DEV)
        counters, tsum = _dw_scratch()
        rm, rv = dev(rm0), dev(rv0)
        nbt = torch.full((1,), 3, dtype=torch.int64, device=DEV)
        z = torch.full((N, Ho, Wo, C), float("nan"), dtype=dt, device=DEV)
        mean, invstd, scale, shift = (torch.full((C,), float("nan"), device=DEV) for _ in range(4))
        ink = _lib.c_int(-1)
        _lib.call("fscnn_dw3x3_fwd_train", P(xd), code, N, H, W, C, stride, P(wd),
                  P(iscd) if lazy else None, P(ishd) if lazy else None, P(z), P(part), P(counters),
                  P(tsum), P(gd), P(bd), P(rm), P(rv), P(nbt), _lib.c_float(0.1), P(mean), P(invstd),
                  P(scale), P(shift), _lib.ctypes.byref(ink), S())
        sync()
        tag = "dw fwd_train %s s%d (%d, %d, %d, %d) lazy %d" % (dname(dt), stride, N, H, W, C, lazy)
        assert ink.value == 1, tag + ": these record counts fit the in-kernel finish"
        assert int(counters.abs().sum().item()) == 0, tag + ": counters not left zero"
        assert int(nbt.item()) == 4
        if lazy:   # the staged operand: relu(fmaf(x, sc, sh)) in fp32, rounded to T (bn_apply's value)
            v = (x.double() * isc.double() + ish.double()).to(torch.float32).clamp_min(0.0).to(dt).double()
        else:
            v = x.double()
        vn = nchw(v)
        ref = F.conv2d(vn, w_, stride=stride, padding=1, groups=C)
        A = F.conv2d(vn.abs(), w_.abs(), stride=stride, padding=1, groups=C)
        check_elem(tag + " z", nchw(z), ref, A, dt)
        # statistics of the stored z (tolerances of test_gemm_bn_statistics in fp32: 1e-5 of the
        # largest reference value, 10x for invstd)
        zs = d64(z).reshape(-1, C)
        Mz = zs.shape[0]
        mu, var = zs.mean(0), zs.var(0, unbiased=False)
        istd = 1.0 / torch.sqrt(var + 1e-5)

        def close(what, got, ref_, tol):
            err = (d64(got) - ref_).abs().max().item()
            lim = tol * (ref_.abs().max().item() + 1e-12)
            report("%s %s" % (tag, what), err / lim)
            assert bool(torch.isfinite(got).all()) and err <= lim, "%s %s" % (tag, what)
        close("mean", mean, mu, 1e-5)
        close("invstd", invstd, istd, 1e-4)
        close("scale", scale, gamma.double() * istd, 1e-4)
        close("shift", shift, beta.double() - mu * gamma.double() * istd, 1e-4)
        close("running_mean", rm, 0.9 * rm0.double() + 0.1 * mu, 1e-5)
        close("running_var", rv, 0.9 * rv0.double() + 0.1 * var * Mz / (Mz - 1), 1e-5)


@pytest.mark.parametrize("dt", DTS, ids=dname)
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("N,H,W,C", DW_SHAPES)
def test_dw3x3_dgrad_bn(dt, stride, N, H, W, C):
    """dx of the depthwise conv plus the BN-backward sums of the STORED dx (modes 0 and 2) and
    their finish: in the kernel's last workgroups for stride 1, a launch of its own for stride 2."""
    code = _lib.dtype_code(dt)
    M = N * H * W
    assert M <= M_MAX
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    dy = q(rnd(N, Ho, Wo, C, seed=71), dt)
    w = f32(rnd(C, 9, seed=72) * 0.5)
    zb = q(randn(N, H, W, C, seed=73) * 2 + 0.7, dt)
    zb_ = zb.double().reshape(M, C)
    tabs = bn_tables(zb_, 74, C)
    mean, invstd, scale, shift = (t.double() for t in tabs)
    dyd, wd, zd = dev(dy), dev(w), dev(zb)
    md, id_, sd, hd = (dev(t) for t in tabs)
    w_ = w.double().reshape(C, 1, 3, 3)
    gn = nchw(dy.double())
    op = (H - ((Ho - 1) * stride + 1), W - ((Wo - 1) * stride + 1))
    ref = F.conv_transpose2d(gn, w_, stride=stride, padding=1, output_padding=op, groups=C)
    A = F.conv_transpose2d(gn.abs(), w_.abs(), stride=stride, padding=1, output_padding=op, groups=C)
    assert tuple(ref.shape) == (N, C, H, W)
    for mode in (0, 2):
        parts = _lib.load().fscnn_dw3x3_parts(N, H, W, C, stride, code, 1)
        assert parts >= 1
        part = torch.full((parts * 2 * C,), float("nan"), device=DEV)
        counters, tsum = _dw_scratch()
        dx = torch.full((N, H, W, C), float("nan"), dtype=dt, device=DEV)
        dgamma, dbeta = (torch.full((C,), float("nan"), device=DEV) for _ in range(2))
        coef = torch.full((2 * C,), float("nan"), device=DEV)
        ink = _lib.c_int(-1)
        _lib.call("fscnn_dw3x3_dgrad_bn", P(dyd), code, N, H, W, C, stride, P(wd), P(dx), P(zd), P(md),
                  P(id_), P(sd) if mode == 2 else None, P(hd) if mode == 2 else None, mode, P(part),
                  P(counters), P(tsum), P(dgamma), P(dbeta), P(coef), _lib.ctypes.byref(ink), S())
        sync()
        tag = "dw dgrad_bn %s s%d (%d, %d, %d, %d) mode %d" % (dname(dt), stride, N, H, W, C, mode)
        assert ink.value == (1 if stride == 1 else 0), tag + ": finish path"
        assert int(counters.abs().sum().item()) == 0, tag + ": counters not left zero"
        check_elem(tag + " dx", nchw(dx), ref, A, dt)
        g = d64(dx).reshape(M, C)                      # the stored dx is that BN's dy
        if mode == 2:
            g = torch.where(zb_ * scale + shift > 0, g, torch.zeros_like(g))
        xhat = (zb_ - mean) * invstd
        check_sum(tag + " dbeta", dbeta, g.sum(0), g.abs().sum(0))
        check_sum(tag + " dgamma", dgamma, (g * xhat).sum(0), (g * xhat).abs().sum(0))
        torch.testing.assert_close(d64(coef[:C]), d64(dbeta) / M, rtol=1e-6, atol=0)
        torch.testing.assert_close(d64(coef[C:]), d64(dgamma) / M, rtol=1e-6, atol=0)
