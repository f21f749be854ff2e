"""The per-kernel entry points of the train-only kernels (include/fastscnn.h, "kernels that only
a train step runs") on a machine without a GPU: every one resolves, and each refuses a null or
inconsistent call with a non-zero code and a message that names it.  A refusal comes before any
HIP call, so the (never dereferenced) pointers below are arbitrary non-null addresses."""
import pytest

from fast_scnn_pytorch_amd import _lib

F32, BF16, F16 = _lib.DT_F32, _lib.DT_BF16, _lib.DT_F16
X = _lib.c_vp(0x1000)   # a non-null pointer no refused call may touch
NUL = None

NEW = ["fscnn_bn_apply", "fscnn_bn_bwd", "fscnn_ppm_branches_ok", "fscnn_ppm_branches_fwd",
       "fscnn_ppm_branches_bwd", "fscnn_ppm_up_fwd", "fscnn_ppm_up_bwd", "fscnn_dropout",
       "fscnn_dw3x3_parts", "fscnn_dw3x3_fwd_train", "fscnn_dw3x3_dgrad_bn",
       "fscnn_dw3x3_wgrad_train", "fscnn_pw_fwd_train_route", "fscnn_pw_fwd_train",
       "fscnn_pw_wgrad_train", "fscnn_pw_dgrad_train_route", "fscnn_pw_dgrad_train",
       "fscnn_im2col3", "fscnn_col2im3"]


def test_new_entry_points_resolve():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None


def _ints(*v):
    return (_lib.c_int * len(v))(*v)


def bn_apply(M=37, C=32, z=X, ldz=32, scale=X, shift=X, z2=NUL, ldz2=0, scale2=NUL, shift2=NUL,
             res=NUL, ldres=0, y=X, ldy=32, dt=BF16):
    return ("fscnn_bn_apply", (M, C, z, ldz, scale, shift, z2, ldz2, scale2, shift2, res, ldres, 1,
                               y, ldy, dt, NUL))


def bn_bwd(M=37, C=128, dy=X, lddy=128, mask=NUL, ldmask=0, shift=X, mode=0, frozen=0, z2=NUL,
           second=NUL, part=X, dz=X, dt=BF16):
    return ("fscnn_bn_bwd", (M, C, dy, lddy, mask, ldmask, X, X, X, X, shift, mode, frozen, z2,
                             second, second, second, part, X, dz, second, X, X, second, second, X,
                             dt, None, None, NUL))


def ppm_fwd(M=(2, 8, 18, 72), K=128, x=X, ldy=32, dt=BF16):
    return ("fscnn_ppm_branches_fwd", (len(M), _ints(*M), K, x, X, X, X, X, X, X, 0.1, X, X, ldy,
                                       X, X, X, X, dt, NUL))


def ppm_bwd(M=(2, 8, 18, 72), K=128, dx=X, lddy=32, dt=BF16):
    return ("fscnn_ppm_branches_bwd", (len(M), _ints(*M), K, X, lddy, X, 32, X, X, X, X, X, X, X,
                                       X, X, X, dx, dt, NUL))


def up_fwd(H=32, ldy=256, coff=128, y=X, dt=BF16):
    return ("fscnn_ppm_up_fwd", (X, dt, 2, H, 64, y, ldy, coff, NUL))


def up_bwd(H=32, ldy=256, coff=128, dfeats=X, dt=BF16):
    return ("fscnn_ppm_up_bwd", (X, dt, 2, H, 64, ldy, coff, dfeats, NUL))


def dropout(C=128, ldx=128, ldy=128, p=0.1, xs=NUL, xh=NUL, y=X, dt=BF16):
    return ("fscnn_dropout", (X, ldx, dt, 2, 3, 5, C, 7, NUL, 0, p, xs, xh, y, ldy, NUL))


def dw_fwd(C=32, stride=1, in_scale=NUL, in_shift=NUL, tsum=X, dt=BF16):
    return ("fscnn_dw3x3_fwd_train", (X, dt, 2, 17, 23, C, stride, X, in_scale, in_shift, X, X, X,
                                      tsum, X, X, X, X, NUL, 0.1, X, X, X, X, None, NUL))


def dw_dgrad(C=32, stride=1, mode=0, shift=X, z=X, dt=BF16):
    return ("fscnn_dw3x3_dgrad_bn", (X, dt, 2, 17, 23, C, stride, X, X, z, X, X, X, shift, mode,
                                     X, X, X, X, X, X, None, NUL))


def dw_wgrad(C=32, stride=1, xs=NUL, xh=NUL, dw=X, dt=BF16):
    return ("fscnn_dw3x3_wgrad_train", (X, X, dt, 2, 17, 23, C, stride, xs, xh, X, dw, NUL))


def pw_fwd(M=300, N=96, K=576, A=X, lda=576, a_sc=NUL, a_sh=NUL, ldb=576, ldc=96, tsum=X, mean=X,
           dt=BF16):
    return ("fscnn_pw_fwd_train", (M, N, K, A, lda, a_sc, a_sh, X, ldb, NUL, X, ldc, X, X, tsum, X, X,
                                   X, X, NUL, 0.1, mean, X, X, X, dt, None, None, NUL))


def pw_wgrad(M=777, N=19, K=128, D=X, ldd=24, ldx=128, xs=NUL, xh=NUL, bias_part=NUL, dbias=NUL,
             dt=BF16):
    return ("fscnn_pw_wgrad_train", (M, N, K, D, ldd, X, ldx, xs, xh, X, X, bias_part, dbias, dt,
                                     None, NUL))


def pw_dgrad(M=4514, N=128, K=19, ldd=24, ldb=24, R=NUL, ldr=0, lddx=128, ldz=128, mode=2, tab=X,
             coef=X, hw=0, p=0.1, dt=BF16):
    return ("fscnn_pw_dgrad_train", (M, N, K, X, ldd, X, ldb, R, ldr, X, lddx, X, ldz, X, X, X, X, mode,
                                     X, X, X, X, X, coef, tab, hw, p, 7, 0, NUL, dt, None, None, NUL))


def im2col(x=X, ldx=64, ldcol=576, C=64, dt=BF16):
    return ("fscnn_im2col3", (x, ldx, dt, 2, 5, 7, C, X, ldcol, NUL))


def col2im(dx=X, lddx=64, ldcol=576, H=5, dt=BF16):
    return ("fscnn_col2im3", (X, ldcol, dt, 2, H, 7, 64, dx, lddx, 1, NUL))


REFUSED = {
    "bn_apply null z": bn_apply(z=NUL),
    "bn_apply C % V (bf16: 8)": bn_apply(C=36, ldz=40, ldy=40),
    "bn_apply C % V (fp32: 4)": bn_apply(C=34, ldz=36, ldy=36, dt=F32),
    "bn_apply ldz < C": bn_apply(ldz=24),
    "bn_apply ldy % V": bn_apply(ldy=36),
    "bn_apply second branch without its scale": bn_apply(z2=X, ldz2=32),
    "bn_apply residual stride": bn_apply(res=X, ldres=20),
    "bn_apply dtype": bn_apply(dt=5),
    "bn_apply M = 0": bn_apply(M=0),
    "bn_bwd null dy": bn_bwd(dy=NUL),
    "bn_bwd paired BN without a mask": bn_bwd(z2=X, second=X),
    "bn_bwd paired BN, recomputed mask": bn_bwd(z2=X, second=X, mode=2),
    "bn_bwd paired BN without its statistics": bn_bwd(z2=X, mask=X, ldmask=128, mode=1),
    "bn_bwd paired BN too wide": bn_bwd(C=576, lddy=576, z2=X, second=X, mask=X, ldmask=576,
                                        mode=1),
    "bn_bwd mask mode without a mask": bn_bwd(mode=1),
    "bn_bwd mask given, mode 0": bn_bwd(mask=X, ldmask=128),
    "bn_bwd relu_z without shift": bn_bwd(mode=2, shift=NUL),
    "bn_bwd C % V": bn_bwd(C=36, lddy=40),
    "bn_bwd lddy < C": bn_bwd(lddy=64),
    "bn_bwd relu_mode 3": bn_bwd(mode=3),
    "bn_bwd frozen 3": bn_bwd(frozen=3),
    "bn_bwd no scratch": bn_bwd(part=NUL),
    "ppm_fwd M > 512": ppm_fwd(M=(15, 60, 135, 540)),
    "ppm_fwd null x": ppm_fwd(x=NUL),
    "ppm_fwd K % 8": ppm_fwd(K=100),
    "ppm_fwd empty branch": ppm_fwd(M=(2, 0)),
    "ppm_fwd five branches": ppm_fwd(M=(2, 2, 2, 2, 2)),
    "ppm_fwd ldy < 32": ppm_fwd(ldy=16),
    "ppm_fwd dtype": ppm_fwd(dt=-1),
    "ppm_bwd M > 512": ppm_bwd(M=(15, 60, 135, 540)),
    "ppm_bwd M > 512 (fp32)": ppm_bwd(M=(513,), dt=F32),
    "ppm_bwd null dx": ppm_bwd(dx=NUL),
    "ppm_bwd lddy < 32": ppm_bwd(lddy=8),
    "ppm_up_fwd null y": up_fwd(y=NUL),
    "ppm_up_fwd slice past the row": up_fwd(ldy=128, coff=64),
    "ppm_up_fwd coff % V": up_fwd(coff=4, ldy=256),
    "ppm_up_bwd H > 80": up_bwd(H=81),
    "ppm_up_bwd H > 80 (fp32)": up_bwd(H=96, dt=F32),
    "ppm_up_bwd null dfeats": up_bwd(dfeats=NUL),
    "ppm_up_bwd ldy % V": up_bwd(ldy=260),
    "dropout ldx % V": dropout(ldx=132),
    "dropout ldx % V (fp32)": dropout(ldx=130, dt=F32),
    "dropout ldy < C": dropout(ldy=64),
    "dropout C % V": dropout(C=36, ldx=40, ldy=40),
    "dropout p = 1": dropout(p=1.0),
    "dropout x_scale without x_shift": dropout(xs=X),
    "dropout null y": dropout(y=NUL),
    "dw_fwd_train in_scale without in_shift": dw_fwd(in_scale=X),
    "dw_fwd_train C % V": dw_fwd(C=36),
    "dw_fwd_train stride 3": dw_fwd(stride=3),
    "dw_fwd_train no team sums": dw_fwd(tsum=NUL),
    "dw_fwd_train dtype": dw_fwd(dt=3),
    "dw_dgrad_bn relu_mode 1": dw_dgrad(mode=1),
    "dw_dgrad_bn relu_z without shift": dw_dgrad(mode=2, shift=NUL),
    "dw_dgrad_bn C % V (fp32)": dw_dgrad(C=30, dt=F32),
    "dw_dgrad_bn null z": dw_dgrad(z=NUL),
    "dw_dgrad_bn stride 0": dw_dgrad(stride=0),
    "dw_wgrad_train x_scale without x_shift": dw_wgrad(xs=X),
    "dw_wgrad_train x_shift without x_scale": dw_wgrad(xh=X),
    "dw_wgrad_train null dw": dw_wgrad(dw=NUL),
    "dw_wgrad_train C % V": dw_wgrad(C=36),
    "dw_wgrad_train stride 3": dw_wgrad(stride=3),
    "dw_wgrad_train dtype": dw_wgrad(dt=3),
    "pw_fwd_train null A": pw_fwd(A=NUL),
    "pw_fwd_train null mean": pw_fwd(mean=NUL),
    "pw_fwd_train no team sums": pw_fwd(tsum=NUL),
    "pw_fwd_train a_scale without a_shift": pw_fwd(a_sc=X),
    "pw_fwd_train a_shift without a_scale": pw_fwd(a_sh=X),
    "pw_fwd_train lda < K": pw_fwd(lda=568),
    "pw_fwd_train lda % V": pw_fwd(lda=580),
    "pw_fwd_train ldb % V (fp32: 4)": pw_fwd(ldb=578, dt=F32),
    "pw_fwd_train ldc < N": pw_fwd(ldc=64),
    "pw_fwd_train lazy K % V": pw_fwd(K=572, a_sc=X, a_sh=X, dt=BF16),
    "pw_fwd_train lazy K > 768": pw_fwd(K=776, lda=776, ldb=776, a_sc=X, a_sh=X),
    "pw_fwd_train N > 1024": pw_fwd(N=1032, ldc=1032),
    "pw_fwd_train M = 0": pw_fwd(M=0),
    "pw_fwd_train dtype": pw_fwd(dt=3),
    "pw_wgrad_train null D": pw_wgrad(D=NUL),
    "pw_wgrad_train x_scale without x_shift": pw_wgrad(xs=X),
    "pw_wgrad_train dbias without its scratch": pw_wgrad(dbias=X),
    "pw_wgrad_train scratch without dbias": pw_wgrad(bias_part=X),
    "pw_wgrad_train ldd < N": pw_wgrad(ldd=16),
    "pw_wgrad_train ldd % V": pw_wgrad(ldd=20),
    "pw_wgrad_train ldx < K": pw_wgrad(ldx=120),
    "pw_wgrad_train lazy K % V": pw_wgrad(K=124, xs=X, xh=X),
    "pw_wgrad_train dtype": pw_wgrad(dt=-1),
    "pw_dgrad_train null tab": pw_dgrad(tab=NUL),
    "pw_dgrad_train null coef": pw_dgrad(coef=NUL),
    "pw_dgrad_train tab alignment": pw_dgrad(tab=_lib.c_vp(0x1004)),
    "pw_dgrad_train relu_mode 1": pw_dgrad(mode=1),
    "pw_dgrad_train ldd < K": pw_dgrad(ldd=16),
    "pw_dgrad_train ldb % V": pw_dgrad(ldb=28),
    "pw_dgrad_train lddx < N": pw_dgrad(lddx=64),
    "pw_dgrad_train ldz % V": pw_dgrad(ldz=132),
    "pw_dgrad_train residual stride": pw_dgrad(R=X, ldr=64),
    "pw_dgrad_train dropout p = 1": pw_dgrad(hw=2257, p=1.0),
    "pw_dgrad_train dropout M % hw": pw_dgrad(hw=2000),
    "pw_dgrad_train dropout hw < 0": pw_dgrad(hw=-1),
    "pw_dgrad_train dropout below the streaming kernel's M": pw_dgrad(M=300, hw=100),
    "pw_dgrad_train dropout, two k-steps": pw_dgrad(K=48, ldd=48, ldb=48, hw=2257),
    "pw_dgrad_train dropout, fp32 K = 19": pw_dgrad(hw=2257, dt=F32),
    "pw_dgrad_train dtype": pw_dgrad(dt=3),
    "im2col3 null x": im2col(x=NUL),
    "im2col3 ldx < C": im2col(ldx=32),
    "im2col3 ldcol < 9 C": im2col(ldcol=512),
    "im2col3 C = 0": im2col(C=0, ldx=0, ldcol=0),
    "im2col3 dtype": im2col(dt=3),
    "col2im3 null dx": col2im(dx=NUL),
    "col2im3 lddx < C": col2im(lddx=32),
    "col2im3 ldcol < 9 C": col2im(ldcol=575),
    "col2im3 H = 0": col2im(H=0),
    "col2im3 dtype": col2im(dt=-1),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refused_before_any_launch(case):
    name, args = REFUSED[case]
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    assert rc != 0, "%s was accepted" % case
    msg = lib.fscnn_last_error().decode()
    assert name in msg, "%s: the message does not name the entry point: %r" % (case, msg)


def test_ppm_branches_ok_limits():
    lib = _lib.load()
    for dt in (F32, BF16, F16):
        assert lib.fscnn_ppm_branches_ok(36 * 14, 128, dt) == 1    # batch 14: 504 rows
        assert lib.fscnn_ppm_branches_ok(512, 128, dt) == 1
        assert lib.fscnn_ppm_branches_ok(36 * 15, 128, dt) == 0    # batch 15: 540 rows
        assert lib.fscnn_ppm_branches_ok(108, 64, dt) == 1
        assert lib.fscnn_ppm_branches_ok(108, 100, dt) == 0        # K % 8
    assert lib.fscnn_ppm_branches_ok(108, 128, 3) == 0             # not a storage type


def test_dw3x3_parts_counts_and_refusal():
    lib = _lib.load()
    # fp32 stride 1: 8 x 32 output tiles; 16-bit: 8 x 16; stride 2 forward: 4 x 16 / 8 x 8
    assert lib.fscnn_dw3x3_parts(2, 17, 23, 32, 1, F32, 0) == 2 * 3 * 1
    assert lib.fscnn_dw3x3_parts(2, 17, 23, 32, 1, BF16, 0) == 2 * 3 * 2
    assert lib.fscnn_dw3x3_parts(2, 17, 23, 32, 2, F32, 0) == 2 * 3 * 1
    assert lib.fscnn_dw3x3_parts(2, 17, 23, 32, 2, F16, 0) == 2 * 2 * 2
    assert lib.fscnn_dw3x3_parts(2, 17, 23, 32, 1, BF16, 1) == 2 * 3 * 2
    assert lib.fscnn_dw3x3_parts(2, 17, 23, 32, 2, BF16, 1) > 0
    assert lib.fscnn_dw3x3_parts(2, 17, 23, 36, 1, BF16, 0) == -1
    assert lib.fscnn_dw3x3_parts(2, 17, 23, 32, 3, BF16, 0) == -1
    assert b"fscnn_dw3x3_parts" in lib.fscnn_last_error()


# (M, N, K, ldc) -> route of fscnn_pw_fwd_train: 0 streaming kernel, 1 tiled kernel finishing its
# BN itself, 2 tiled kernel + finalize launch (the shapes of tests/test_gpu_train_gemm.py)
FWD_ROUTES = [((4133, 48, 32, 48), 0), ((4133, 64, 48, 64), 0), ((4133, 128, 128, 128), 0),
              ((4133, 64, 384, 64), 1), ((4133, 128, 768, 128), 1), ((4133, 96, 576, 96), 1),
              ((300, 96, 576, 96), 1), ((129, 64, 384, 64), 1), ((4133, 19, 128, 24), 1),
              ((300, 576, 96, 576), 2),
              # N = 384, K = 64 never takes route 2: 12 column groups fit the in-kernel finish
              # below M = 4096, the streaming kernel takes it from there
              ((300, 384, 64, 384), 1), ((4095, 384, 64, 384), 1), ((4096, 384, 64, 384), 0),
              ((65539, 384, 64, 384), 0)]


def test_pw_fwd_train_routes():
    lib = _lib.load()
    for (M, N, K, ldc), route in FWD_ROUTES:
        for dt in (F32, BF16, F16):
            for lazy in (0, 1):
                recs = _lib.c_int(-1)
                got = lib.fscnn_pw_fwd_train_route(M, N, K, K + 8, ldc, lazy, dt, _lib.ctypes.byref(recs))
                assert got == route, (M, N, K, dt, lazy, got)
                assert 1 <= recs.value <= (M + 127) // 128
                if route:
                    assert recs.value == (M + 127) // 128   # the tiled kernel: one record per tile
    assert lib.fscnn_pw_fwd_train_route(300, 96, 572, 576, 96, 1, BF16, None) == -1
    assert b"fscnn_pw_fwd_train" in lib.fscnn_last_error()


def test_pw_dgrad_train_routes():
    lib = _lib.load()
    recs = _lib.c_int(-1)
    r = _lib.ctypes.byref(recs)
    # the classifier dgrad with its dropout: one k-step, streaming, 16-bit (fp32: K <= 16 only)
    for dt in (BF16, F16):
        assert lib.fscnn_pw_dgrad_train_route(2 * 37 * 61, 128, 19, 24, 128, 0, 37 * 61, dt, r) == 0
        assert lib.fscnn_pw_dgrad_train_route(2 * 37 * 61, 128, 19, 24, 128, 1, 37 * 61, dt, r) == 0
        assert lib.fscnn_pw_dgrad_train_route(4133, 64, 128, 136, 64, 0, 0, dt, r) == 0
    assert lib.fscnn_pw_dgrad_train_route(2 * 37 * 61, 128, 19, 24, 128, 0, 37 * 61, F32, r) == -1
    assert b"fscnn_pw_dgrad_train" in lib.fscnn_last_error()
    for dt in (F32, BF16, F16):
        assert lib.fscnn_pw_dgrad_train_route(3 * 37 * 37, 128, 2, 8, 128, 0, 37 * 37, dt, r) == 0
    assert lib.fscnn_pw_dgrad_train_route(4133, 64, 128, 132, 64, 0, 0, F32, r) == 1
    assert recs.value == 33
