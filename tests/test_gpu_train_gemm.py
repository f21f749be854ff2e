"""Per-kernel parity of the pointwise (1x1) conv's three matrix-core kernels in the forms only a
train step runs, in fp32, bf16 and fp16, through the C ABI in the executor's form
(include/fastscnn.h, fscnn_pw_fwd_train / fscnn_pw_wgrad_train / fscnn_pw_dgrad_train), plus the
aux head's im2col3 / col2im3 and the depthwise weight gradient over a lazy input.

Conventions of test_gpu_train_kernels.py (whose helpers are used): operands drawn on the CPU with
fixed seeds and rounded to the storage type first, reference fp64 torch on the CPU, u_T = 2^-8
(bf16), 2^-11 (fp16), 2^-24 (fp32), every check prints its worst error / bound ratio.  Bounds:

* a GEMM output stored in T: |err| <= u_T |ref| + (K + 2) 2^-24 sum_k |a w| (fp32 accumulation
  over K, the bias and a residual counted among the terms; fp16: + 2^-25, half the spacing of its
  subnormals, which u_T |ref| does not cover below 2^-14);
* the lazy operand relu(fmaf(z, sc[k], sh[k])) rounded to T is taken from fscnn_bn_apply on the
  same z and tables (its stored output is the `a` of the fp64 reference); the plain form run on
  that stored operand must give the lazy form's output within two output bounds (whether the two
  are bit-identical is printed, not required);
* forward statistics, referenced in fp64 from the kernel's own stored z: mean to 1e-6 relative +
  1e-7 max|z|, invstd to 1e-6 relative, scale / shift / running mean / running var (unbiased,
  momentum 0.1) to 1e-6 relative + 1e-7 of the sum of their terms' magnitudes, nbt == 1, records
  past the reported count untouched (NaN-filled);
* backward sums of the stored dX: check_sum's 2e-6 a + 1e-6, coef to rtol 1e-6, M <= M_MAX;
* the BN-backward operand table (common.hpp bwdx_apply): dz = al*mask*dy + gz*z + be evaluated in
  fp64 from the table against scale*(dy_r - c1 - xhat*c2) from the fp64 sums of the stored dX, to
  1e-6 A (A: the magnitudes of every term of either expression) plus the sums' own bound
  propagated, |scale| (d1 + |xhat| d2) with d = (2e-6 a + 1e-6) / M; (sc, sh) is the forward affine
  exactly in mode 2 and (0, 1) in mode 0;
* the dgrad's output dropout: torch.equal to fscnn_dropout of the same call's undropped dX;
* dW (fp32): (M + 2) 2^-24 sum_m |d x|; dbias: check_sum;
* im2col3 bit-exact; col2im3 u_T |ref| + 10 x 2^-24 sum |terms| (+ u_T |ref| when accumulating).

The route each call reports (0 streaming kernel, 1 tiled kernel finishing its BN in its last
workgroups, 2 tiled kernel + finalize launch) is asserted, so a retuned threshold fails here
instead of silently changing what a case covers.  A pointwise conv with N = 384, K = 64 never takes
route 2 (12 column groups fit the in-kernel finish below M = 4096, the streaming kernel takes it
from there): route 2 is pinned at N = 576, K = 96 (a bottleneck expand), M = 300.

Measured on the MI355X (worst err / bound over all cases): GEMM outputs 0.998 (16-bit, one storage
rounding) / 0.38 (fp32); lazy against plain bit-identical in all 51 comparisons; forward mean 0.10,
invstd 0.10, scale 0.12, shift 0.63, running mean 0.62, running var 0.12; backward sums 0.008; table
law 0.005; pointwise dW 0.001, dbias 0.02, depthwise dW 0.02; col2im3 0.996 (16-bit) / 0.20 (fp32).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fast_scnn_pytorch_amd import _lib
from test_gpu_train_kernels import (BF16, DEV, DTS, F16, F32, M_MAX, P, S, U, _dropout, bn_tables,
                                    check_bound, check_rel, check_sum, d64, dev, dname, f32, nchw,
                                    padded, q, randn, report, rnd, sync)

pytestmark = pytest.mark.gpu

byref = _lib.ctypes.byref
E24 = 2.0 ** -24


def vw(dt):
    return 4 if dt == F32 else 8


def rup(n, v):
    return (n + v - 1) // v * v


def scratch():
    """Arrival counters (zeroed; every call must leave them zero) and the fp64 team sums."""
    return (torch.zeros(512, dtype=torch.int32, device=DEV),
            torch.zeros(32 * 3 * 1024, dtype=torch.float64, device=DEV))


def nans(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def ids(v):
    return dname(v) if isinstance(v, torch.dtype) else str(v)


def bn_apply(zd, ldz, M, C, sc, sh, dt):
    """The stored lazy operand: fscnn_bn_apply (tested in test_gpu_train_kernels.py) with ReLU."""
    a = nans(M, C, dtype=dt)
    _lib.call("fscnn_bn_apply", M, C, P(zd), ldz, P(sc), P(sh), None, 0, None, None, None, 0, 1, P(a), C,
              _lib.dtype_code(dt), S())
    sync()
    assert bool(torch.isfinite(a).all()) and bool((a >= 0).all())
    return a


def stored(dt, ref, acc):
    """The bound of a value accumulated in fp32 (error acc) and stored in T: one rounding, u_T |ref|,
    or half the spacing of the fp16 subnormals (2^-25) where that is larger."""
    return U[dt] * ref.abs() + acc + (2.0 ** -25 if dt == F16 else 0.0)


def same(what, a, b):
    print("%-58s bit-identical: %s" % (what, bool(torch.equal(a, b))))


# ---- forward: fscnn_pw_fwd_train ----------------------------------------------------------------

# (M, N, K, ldc, bias, route)
FWD_CASES = [(4133, 48, 32, 48, 1, 0),      # streaming
             (4133, 64, 48, 64, 0, 0),      # streaming; 16-bit: the K tail inside a k-step
             (4133, 128, 128, 128, 0, 0),   # streaming
             (4133, 64, 384, 64, 0, 1),     # below the deep-K threshold: tiled
             (4133, 128, 768, 128, 0, 1),   # tiled; K = G_ATMAX
             (4133, 96, 576, 96, 0, 1),     # tiled
             (300, 96, 576, 96, 1, 1),      # tiled
             (129, 64, 384, 64, 0, 1),      # tiled; one full tile plus one row
             (4133, 19, 128, 24, 1, 1),     # N < 32: the scalar column tail; z's pad columns stay
             (300, 576, 96, 576, 0, 2)]     # 18 column groups > 14: the finalize launch


def _fwd_call(dt, M, N, K, A, lda, a_sc, a_sh, B, ldb, bias, ldc, gamma, beta, rm0, rv0):
    code = _lib.dtype_code(dt)
    rows = (M + 127) // 128 + 2
    part = nans(rows * 3 * N)
    counters, tsum = scratch()
    z = torch.full((M, ldc), 7.0, dtype=dt, device=DEV)
    rm, rv = dev(rm0), dev(rv0)
    nbt = torch.zeros(1, dtype=torch.int64, device=DEV)
    mean, invstd, scale, shift = (nans(N) for _ in range(4))
    route, recs = _lib.c_int(-1), _lib.c_int(-1)
    _lib.call("fscnn_pw_fwd_train", M, N, K, P(A), lda, P(a_sc), P(a_sh), P(B), ldb, P(bias), P(z), ldc,
              P(part), P(counters), P(tsum), P(gamma), P(beta), P(rm), P(rv), P(nbt), _lib.c_float(0.1),
              P(mean), P(invstd), P(scale), P(shift), code, byref(route), byref(recs), S())
    sync()
    host = _lib.c_int(-1)
    assert _lib.load().fscnn_pw_fwd_train_route(M, N, K, lda, ldc, int(a_sc is not None), code,
                                                byref(host)) == route.value
    assert host.value == recs.value
    assert int(counters.abs().sum().item()) == 0, "arrival counters not left zero"
    assert 1 <= recs.value <= (M + 127) // 128
    assert bool(torch.isnan(part[recs.value * 3 * N:]).all()), "a record past the reported count was written"
    assert bool((z[:, N:] == 7.0).all()), "z written past N"
    assert int(nbt.item()) == 1
    return z[:, :N], (mean, invstd, scale, shift, rm, rv), route.value, recs.value


def _fwd_stats(tag, z, out, gamma, beta, rm0, rv0):
    """The finished statistics against fp64 from the kernel's own stored z."""
    mean, invstd, scale, shift, rm, rv = out
    zs = d64(z)
    M = zs.shape[0]
    zmax = zs.abs().max().item()
    mu = zs.mean(0)
    var = ((zs - mu) ** 2).mean(0)
    istd = 1.0 / torch.sqrt(var + 1e-5)
    g_, b_ = gamma.double(), beta.double()
    sc = g_ * istd
    unb = var * M / (M - 1)

    def terms(what, got, ref, t):
        check_bound(tag + " " + what, got, ref, 1e-6 * ref.abs() + 1e-7 * t)
    check_rel(tag + " mean", mean, mu, 1e-6, 1e-7 * zmax)
    check_rel(tag + " invstd", invstd, istd, 1e-6)
    terms("scale", scale, sc, sc.abs())
    terms("shift", shift, b_ - mu * sc, b_.abs() + (mu * sc).abs())
    terms("running_mean", rm, 0.9 * rm0.double() + 0.1 * mu, 0.9 * rm0.double().abs() + 0.1 * mu.abs())
    terms("running_var", rv, 0.9 * rv0.double() + 0.1 * unb, 0.9 * rv0.double().abs() + 0.1 * unb.abs())


@pytest.mark.parametrize("dt", DTS, ids=dname)
@pytest.mark.parametrize("M,N,K,ldc,has_bias,route", FWD_CASES, ids=ids)
def test_pw_fwd_train(dt, M, N, K, ldc, has_bias, route):
    """Exec::pw's train form: z = a . W^T (+ bias) with the batch statistics of the stored z
    finished by the GEMM (all three finishes), a the lazy BN+ReLU of a raw conv output (both
    kernels) and the same operand stored (the plain form)."""
    assert M <= M_MAX
    V = vw(dt)
    lda, ldb = K + V, K + 2 * V
    # the raw producer output and its BN affine: most channels land near +3 (the statistics of z
    # then cancel), every fourth straddles zero so the ReLU clamps about half of it
    zin = q(randn(M, K, seed=101) * 2 + 0.7, dt)
    a_sc = f32(rnd(K, seed=102, lo=-0.5, hi=0.5))
    a_sh = f32(rnd(K, seed=103, lo=2.0, hi=4.0))
    a_sh[::4] = f32(rnd(K, seed=104, lo=-0.5, hi=0.5))[::4]
    w = q(rnd(N, K, seed=105) / np.sqrt(K), dt)
    bias = f32(rnd(N, seed=106, lo=-2.0, hi=2.0)) if has_bias else None
    gamma = f32(rnd(N, seed=107, lo=0.5, hi=1.5))
    gamma[::3] *= -1.0
    beta = f32(rnd(N, seed=108, lo=-0.5, hi=0.5))
    rm0, rv0 = f32(rnd(N, seed=109, lo=-0.5, hi=0.5)), f32(rnd(N, seed=110, lo=0.5, hi=1.5))
    zind, wd = padded(zin, lda, 1e4), padded(w, ldb, 1e4)
    a_scd, a_shd, gd, bd = dev(a_sc), dev(a_sh), dev(gamma), dev(beta)
    biasd = dev(bias) if has_bias else None
    a = bn_apply(zind, lda, M, K, a_scd, a_shd, dt)          # the exact operand, stored
    a_ = d64(a)
    assert 0.05 < float((a_ == 0).double().mean()) < 0.5      # the ReLU clamps some, not most
    w_ = w.double()
    ref = a_ @ w_.t()
    T = a_.abs() @ w_.abs().t()
    if has_bias:
        ref = ref + bias.double()
        T = T + bias.double().abs()
    bound = stored(dt, ref, (K + 2) * E24 * T)
    tag = "pw fwd_train %s (%d, %d, %d)" % (dname(dt), M, N, K)
    zl, outl, rl, nl = _fwd_call(dt, M, N, K, zind, lda, a_scd, a_shd, wd, ldb, biasd, ldc, gd, bd, rm0, rv0)
    zp, outp, rp, np_ = _fwd_call(dt, M, N, K, a, K, None, None, wd, ldb, biasd, ldc, gd, bd, rm0, rv0)
    print("%s: route lazy %d plain %d, records %d / %d" % (tag, rl, rp, nl, np_))
    assert rl == route and rp == route, tag + ": route"
    check_bound(tag + " lazy z", zl, ref, bound)
    check_bound(tag + " plain z", zp, ref, bound)
    check_bound(tag + " lazy z vs plain z", zl, d64(zp), 2 * bound)
    same(tag + " lazy z vs plain z", zl, zp)
    _fwd_stats(tag + " lazy", zl, outl, gamma, beta, rm0, rv0)
    _fwd_stats(tag + " plain", zp, outp, gamma, beta, rm0, rv0)


# ---- weight gradient: fscnn_pw_wgrad_train -------------------------------------------------------

# (M, N, K, ldd or 0)
WGRAD_CASES = [(4100, 64, 64, 0),      # 16 splits of 320 rows: the last three are empty
               (4133, 48, 32, 0),      # both tile tails (N, K < 64)
               (1000, 128, 576, 0),    # 2 x 9 tiles
               (777, 19, 128, 24),     # the classifier conv: D's pad columns carry a sentinel
               (4133, 32, 576, 0)]     # the aux conv over its im2col columns


@pytest.mark.parametrize("dt", DTS, ids=dname)
@pytest.mark.parametrize("M,N,K,ldd", WGRAD_CASES, ids=ids)
def test_pw_wgrad_train(dt, M, N, K, ldd):
    """pw_bwd's weight-gradient half: dW = D^T x over the lazy X (positive shifts: a padded row or
    column left unmasked after the transform contributes relu(shift)) and over the same operand
    stored, and the bias gradient (colsum)."""
    assert M <= M_MAX
    V = vw(dt)
    code = _lib.dtype_code(dt)
    ldd = ldd or rup(N, V) + V
    ldx = K + V
    d = q(rnd(M, N, seed=121), dt)
    xin = q(randn(M, K, seed=122) * 2 + 0.7, dt)
    x_sc = f32(rnd(K, seed=123, lo=-1.5, hi=1.5))
    x_sh = f32(rnd(K, seed=124, lo=0.2, hi=1.5))
    dd, xind = padded(d, ldd, 1e4), padded(xin, ldx, 1e4)
    x_scd, x_shd = dev(x_sc), dev(x_sh)
    x = bn_apply(xind, ldx, M, K, x_scd, x_shd, dt)
    d_, x_ = d.double(), d64(x)
    ref = d_.t() @ x_
    bound = (M + 2) * E24 * (d_.abs().t() @ x_.abs())
    tag = "pw wgrad_train %s (%d, %d, %d)" % (dname(dt), M, N, K)
    slab_floats = _lib.load().fscnn_pw_wgrad_slab_floats(M, N, K)
    out = []
    for lazy in (1, 0):
        slab = nans(slab_floats)
        bias_part = nans((M + 1023) // 1024 * N)
        dW, dbias = nans(N, K), nans(N)
        splits = _lib.c_int(-1)
        _lib.call("fscnn_pw_wgrad_train", M, N, K, P(dd), ldd, P(xind) if lazy else P(x), ldx if lazy else K,
                  P(x_scd) if lazy else None, P(x_shd) if lazy else None, P(slab), P(dW), P(bias_part),
                  P(dbias), code, byref(splits), S())
        sync()
        s = splits.value
        assert s * N * K == slab_floats
        rows = rup((M + s - 1) // s, 64)
        print("%s lazy %d: %d splits of %d rows" % (tag, lazy, s, rows))
        if (M, N, K) == (4100, 64, 64):
            assert rows * (s - 1) >= M, tag + ": expected an empty trailing split"
        check_bound(tag + " lazy %d dW" % lazy, dW, ref, bound)
        check_sum(tag + " lazy %d dbias" % lazy, dbias, d_.sum(0), d_.abs().sum(0))
        out.append(dW)
    check_bound(tag + " lazy dW vs plain dW", out[0], d64(out[1]), 2 * bound)
    same(tag + " lazy dW vs plain dW", out[0], out[1])


# ---- dgrad: fscnn_pw_dgrad_train -----------------------------------------------------------------

def _dgrad_call(dt, M, N, K, Dd, ldd, Bd, ldb, Rd, zd, tabs_d, mode, drop=None):
    """drop: (hw, p, seed, seed_add, slot tensor or None)."""
    code = _lib.dtype_code(dt)
    md, id_, sd, hd = tabs_d
    rows = (M + 127) // 128 + 2
    part = nans(rows * 2 * N)
    counters, tsum = scratch()
    dX = nans(M, N, dtype=dt)
    dgamma, dbeta, coef, tab = nans(N), nans(N), nans(2 * N), nans(N, 8)
    hw, p, seed, add, slot = drop or (0, 0.0, 0, 0, None)
    route, recs = _lib.c_int(-1), _lib.c_int(-1)
    _lib.call("fscnn_pw_dgrad_train", M, N, K, P(Dd), ldd, P(Bd), ldb, P(Rd), N, P(dX), N, P(zd), N,
              P(md), P(id_), P(sd), P(hd), mode, P(part), P(counters), P(tsum), P(dgamma), P(dbeta),
              P(coef), P(tab), hw, _lib.c_float(p), seed, add, P(slot), code, byref(route),
              byref(recs), S())
    sync()
    host = _lib.c_int(-1)
    assert _lib.load().fscnn_pw_dgrad_train_route(M, N, K, ldd, N, int(Rd is not None), hw, code,
                                                  byref(host)) == route.value
    assert host.value == recs.value
    assert int(counters.abs().sum().item()) == 0, "arrival counters not left zero"
    assert 1 <= recs.value <= (M + 127) // 128
    assert bool(torch.isnan(part[recs.value * 2 * N:]).all()), "a record past the reported count was written"
    return dX, dgamma, dbeta, coef, tab, route.value, recs.value


def _dgrad_sums_and_table(tag, M, N, dX, dgamma, dbeta, coef, tab, z_, tabs, mode):
    """dbeta / dgamma / coef from the stored dX (that BN's dy), and the operand table's law."""
    assert M <= M_MAX
    mean, invstd, scale, shift = (t.double() for t in tabs)
    g = d64(dX)
    mask = (z_ * scale + shift > 0) if mode == 2 else torch.ones_like(g, dtype=torch.bool)
    gm = torch.where(mask, g, torch.zeros_like(g))
    xhat = (z_ - mean) * invstd
    s1, a1 = gm.sum(0), gm.abs().sum(0)
    s2, a2 = (gm * xhat).sum(0), (gm * xhat).abs().sum(0)
    check_sum(tag + " dbeta", dbeta, s1, a1)
    check_sum(tag + " dgamma", dgamma, s2, a2)
    torch.testing.assert_close(d64(coef[:N]), d64(dbeta) / M, rtol=1e-6, atol=0)
    torch.testing.assert_close(d64(coef[N:]), d64(dgamma) / M, rtol=1e-6, atol=0)
    t = tab.cpu()
    assert bool(torch.isfinite(t[:, :5]).all()), tag + ": table not written"
    if mode == 2:
        assert torch.equal(t[:, 3], tabs[2]) and torch.equal(t[:, 4], tabs[3]), tag + ": (sc, sh) != forward affine"
    else:
        assert bool((t[:, 3] == 0).all()) and bool((t[:, 4] == 1).all()), tag + ": (sc, sh) != (0, 1)"
    al, be, gz, sc, sh = (t[:, i].double() for i in range(5))
    rows = torch.cat([torch.arange(0, 96), torch.arange(97, M - 96, 61), torch.arange(M - 96, M)])
    zr, gr, xr = z_[rows], g[rows], xhat[rows]
    tmask = zr * sc + sh > 0                                  # the table's own mask
    got = al * torch.where(tmask, gr, torch.zeros_like(gr)) + gz * zr + be
    c1, c2 = s1 / M, s2 / M
    gmr = gm[rows]
    ref = scale * (gmr - c1 - xr * c2)
    A = ((al * gr).abs() + (gz * zr).abs() + be.abs() + (scale * c1).abs() + (gz * mean).abs()
         + (scale * gmr).abs() + (scale * xr * c2).abs())
    d1, d2 = (2e-6 * a1 + 1e-6) / M, (2e-6 * a2 + 1e-6) / M
    check_bound(tag + " table law", got, ref, 1e-6 * A + scale.abs() * (d1 + xr.abs() * d2))


@pytest.mark.parametrize("dt", DTS, ids=dname)
@pytest.mark.parametrize("mode", [0, 2])
def test_pw_dgrad_train_sums_and_table(dt, mode):
    """pw_dgrad_args + set_btarget at (4133, 64, 128): dX, the BN-backward sums of the stored dX
    and the operand table, without and with a residual; the streaming kernel in 16-bit, the tiled
    kernel with its in-kernel finish in fp32."""
    M, N, K = 4133, 64, 128
    D = q(rnd(M, K, seed=131), dt)
    Bt = q(rnd(N, K, seed=132) / np.sqrt(K), dt)
    R = q(rnd(M, N, seed=133), dt)
    z = q(randn(M, N, seed=134) * 2 + 0.7, dt)
    z_ = z.double()
    tabs = bn_tables(z_, 135, N)
    V = vw(dt)
    ldd, ldb = K + V, K + 2 * V
    Dd, Bd, Rd, zd = padded(D, ldd, 1e4), padded(Bt, ldb, 1e4), dev(R), dev(z)
    tabs_d = tuple(dev(t) for t in tabs)
    D_, B_ = D.double(), Bt.double()
    base, T = D_ @ B_.t(), D_.abs() @ B_.abs().t()
    for res in (0, 1):
        ref = base + R.double() if res else base
        Tr = T + R.double().abs() if res else T
        dX, dgamma, dbeta, coef, tab, route, recs = _dgrad_call(
            dt, M, N, K, Dd, ldd, Bd, ldb, Rd if res else None, zd, tabs_d, mode)
        tag = "pw dgrad_train %s (%d, %d, %d) mode %d res %d" % (dname(dt), M, N, K, mode, res)
        print("%s: route %d, records %d" % (tag, route, recs))
        assert route == (1 if dt == F32 else 0), tag + ": route"
        check_bound(tag + " dX", dX, ref, stored(dt, ref, (K + 2) * E24 * Tr))
        _dgrad_sums_and_table(tag, M, N, dX, dgamma, dbeta, coef, tab, z_, tabs, mode)


# (n, h, w, K, lda, residual, p, seed_add, dtypes): M = n h w >= 4096, N = 128
DROP_CASES = [(2, 37, 61, 19, 24, 0, 0.1, 0, [BF16, F16]),
              (3, 37, 37, 2, 8, 0, 0.5, 1, DTS),     # (K <= 16: the fp32 kernel takes it too)
              (2, 37, 61, 19, 24, 1, 0.1, 1, [BF16, F16])]


@pytest.mark.parametrize("n,h,w,K,lda,res,p,add,dt",
                         [c[:8] + (dt,) for c in DROP_CASES for dt in c[8]], ids=ids)
def test_pw_dgrad_train_dropout(n, h, w, K, lda, res, p, add, dt):
    """The classifier conv's dgrad with the Dropout mask applied in its epilogue (streaming kernel,
    one k-step): the stored dX is fscnn_dropout of the same call's undropped dX bit for bit, the BN
    sums and the table are those of the dropped dX, and the device seed slot equals the seed by
    value."""
    M, N, hw = n * h * w, 128, h * w
    assert 4096 <= M <= M_MAX
    seed = 0x5eed1234 + K
    D = q(rnd(M, K, seed=141), dt)
    Bt = q(rnd(N, K, seed=142), dt)
    R = q(rnd(M, N, seed=143), dt)
    z = q(randn(M, N, seed=144) * 2 + 0.7, dt)
    z_ = z.double()
    tabs = bn_tables(z_, 145, N)
    Dd, Bd, zd = padded(D, lda, 1e4), padded(Bt, lda, 1e4), dev(z)
    Rd = dev(R) if res else None
    tabs_d = tuple(dev(t) for t in tabs)
    tag = "pw dgrad_train dropout %s (%d x %d x %d, %d, %d) res %d p %.1f" % (dname(dt), n, h, w, N, K, res, p)
    ref = D.double() @ Bt.double().t()
    T = D.double().abs() @ Bt.double().abs().t()
    if res:
        ref, T = ref + R.double(), T + R.double().abs()
    dX0, _, _, _, _, r0, _ = _dgrad_call(dt, M, N, K, Dd, lda, Bd, lda, Rd, zd, tabs_d, 2)
    check_bound(tag + " undropped dX", dX0, ref, stored(dt, ref, (K + 2) * E24 * T))
    dX, dgamma, dbeta, coef, tab, r1, recs = _dgrad_call(dt, M, N, K, Dd, lda, Bd, lda, Rd, zd, tabs_d, 2,
                                                         drop=(hw, p, seed, add, None))
    print("%s: route %d / %d, records %d" % (tag, r0, r1, recs))
    assert r0 == 0 and r1 == 0, tag + ": streaming kernel expected"
    want = _dropout(dt, n, h, w, N, dX0, N, p, seed=seed, add=add)
    assert torch.equal(dX, want), tag + ": fused dX != dropout(undropped dX): %d of %d elements differ" % (
        int((dX != want).sum()), dX.numel())
    dropped = float((dX == 0).double().mean())
    assert abs(dropped - p) < 0.01, tag + ": dropped fraction %.4f" % dropped
    _dgrad_sums_and_table(tag, M, N, dX, dgamma, dbeta, coef, tab, z_, tabs, 2)
    slot = torch.tensor([seed], dtype=torch.int64, device=DEV)
    dXs, dgs, dbs, _, tabs_s, _, _ = _dgrad_call(dt, M, N, K, Dd, lda, Bd, lda, Rd, zd, tabs_d, 2,
                                                 drop=(hw, p, 99, add, slot))
    assert torch.equal(dXs, dX), tag + ": the seed by device slot differs from the seed by value"
    assert torch.equal(dgs, dgamma) and torch.equal(dbs, dbeta) and torch.equal(tabs_s[:, :5], tab[:, :5])


# ---- the aux head's column kernels -----------------------------------------------------------------

@pytest.mark.parametrize("dt", DTS, ids=dname)
@pytest.mark.parametrize("H,W", [(5, 7), (1, 3)])
def test_im2col3_col2im3(dt, H, W):
    N, C = 2, 64
    M = N * H * W
    code = _lib.dtype_code(dt)
    ldx, ldcol = C + 8, 9 * C + 8
    x = q(randn(N, H, W, C, seed=151), dt)
    xd = padded(x.reshape(M, C), ldx, 1e4)
    col = torch.full((M, ldcol), 7.0, dtype=dt, device=DEV)
    _lib.call("fscnn_im2col3", P(xd), ldx, code, N, H, W, C, P(col), ldcol, S())
    sync()
    tag = "%s (%d, %d, %d, %d)" % (dname(dt), N, H, W, C)
    # unfold's row order is c*9 + kh*3 + kw, im2col3's column order
    want = F.unfold(nchw(x.double()), 3, padding=1).permute(0, 2, 1).reshape(M, 9 * C)
    assert torch.equal(d64(col[:, :9 * C]), want), "im2col3 " + tag
    assert bool((col[:, 9 * C:] == 7.0).all()), "im2col3 wrote past 9 C"
    print("im2col3 %s: bit-exact" % tag)
    dcol = q(rnd(M, 9 * C, seed=152), dt)
    dcold = padded(dcol, ldcol, 1e4)
    cols = dcol.double().reshape(N, H * W, 9 * C).permute(0, 2, 1)
    s = F.fold(cols, (H, W), 3, padding=1).permute(0, 2, 3, 1).reshape(M, C)
    a = F.fold(cols.abs(), (H, W), 3, padding=1).permute(0, 2, 3, 1).reshape(M, C)
    dx0 = q(rnd(M, C, seed=153, lo=-3, hi=3), dt)
    for acc in (0, 1):
        dx = torch.full((M, ldx), 7.0, dtype=dt, device=DEV)
        dx[:, :C] = dev(dx0)
        _lib.call("fscnn_col2im3", P(dcold), ldcol, code, N, H, W, C, P(dx), ldx, acc, S())
        sync()
        ref = s + dx0.double() if acc else s
        T = a + dx0.double().abs() if acc else a
        check_bound("col2im3 %s accumulate %d" % (tag, acc), dx[:, :C], ref,
                    stored(dt, ref, 10 * E24 * T) + acc * U[dt] * ref.abs())
        assert bool((dx[:, C:] == 7.0).all()), "col2im3 wrote past C"


# ---- depthwise weight gradient over a lazy input ---------------------------------------------------

@pytest.mark.parametrize("dt", DTS, ids=dname)
@pytest.mark.parametrize("N,H,W,C,stride", [(2, 17, 23, 48, 2), (1, 9, 8, 128, 1)])
def test_dw3x3_wgrad_train(dt, N, H, W, C, stride):
    """dW[c][kh][kw] = sum dy x over the lazy x (positive shifts: padding must stay zero, not
    relu(shift)), against the stored operand; the plain form on that operand agrees."""
    code = _lib.dtype_code(dt)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    M = N * H * W
    xin = q(randn(N, H, W, C, seed=161) * 2 + 0.7, dt)
    dy = q(rnd(N, Ho, Wo, C, seed=162), dt)
    x_sc = f32(rnd(C, seed=163, lo=-1.5, hi=1.5))
    x_sh = f32(rnd(C, seed=164, lo=0.2, hi=1.5))
    xind, dyd, x_scd, x_shd = dev(xin), dev(dy), dev(x_sc), dev(x_sh)
    x = bn_apply(xind, C, M, C, x_scd, x_shd, dt)
    xu = F.unfold(nchw(d64(x).reshape(N, H, W, C)), 3, padding=1, stride=stride).reshape(N, C, 9, Ho * Wo)
    g = nchw(dy.double()).reshape(N, C, 1, Ho * Wo)
    ref = (xu * g).sum((0, 3))
    bound = (N * Ho * Wo + 2) * E24 * (xu * g).abs().sum((0, 3))
    slab_floats = _lib.load().fscnn_dw3x3_wgrad_slab_floats(N, H, W, C, stride, code)
    tag = "dw wgrad_train %s s%d (%d, %d, %d, %d)" % (dname(dt), stride, N, H, W, C)
    out = []
    for lazy in (1, 0):
        slab, dw = nans(slab_floats), nans(C, 9)
        _lib.call("fscnn_dw3x3_wgrad_train", P(xind) if lazy else P(x), P(dyd), code, N, H, W, C, stride,
                  P(x_scd) if lazy else None, P(x_shd) if lazy else None, P(slab), P(dw), S())
        sync()
        check_bound(tag + " lazy %d dW" % lazy, dw, ref, bound)
        out.append(dw)
    check_bound(tag + " lazy dW vs plain dW", out[0], d64(out[1]), 2 * bound)
    same(tag + " lazy dW vs plain dW", out[0], out[1])
