"""Every executor switch left in the library (`env_on` / `env_int`, the only `getenv` in
fast-scnn-pytorch_amd/csrc) keeps its non-default path parity-green.  The switches are read once per process, so each case runs in a
fresh child process:

* ``FSCNN_SIDE_STREAM=0`` — every weight gradient on the caller's stream (one stream);
* ``FSCNN_F32_SPLIT=0``   — exact fp32 MFMA in the eval pointwise GEMM launches instead of the
  three-way bf16 split of each fp32 operand (the fused stem and DSConv always split);
* ``FSCNN_GRAPHS=1``      — whole forward / backward-stage calls captured into hipGraphs and
  replayed (the dropout seed then travels through a device slot the forward writes);
* ``FSCNN_LTD_FUSED=0``   — (16-bit train plans) LTD.dsconv1.dw's input gradient stored and
  conv0's weight gradient its own launch, instead of the fused ltd_c0_bwd pass;
* ``FSCNN_SIDE_PRIO=0``   — the weight-gradient side stream as a plain stream instead of one at
  the device's lowest priority;
* ``FSCNN_SIDE_FENCE=1``  — the side stream's fork / join events with the default system-scope
  fence (the default drops it: both ends are kernels of the device); train steps bit-identical;
* ``FSCNN_DROP_FUSED=0``  — the classifier's Dropout backward and dsconv2 pw's BN-backward reduce
  as their own passes instead of in the classifier conv's dgrad epilogue (the fused form runs only
  at M >= 4096 low-res pixels in 16-bit plans: test_drop_fused_matches_separate_passes).
* ``FSCNN_STEM_FUSED=0``  — (inference) conv0, LTD.dsconv1.dw and .pw as three launches instead of
  the fused stem (csrc/stem.hip): bit-identical outputs (test_stem_fused_bit_identical).
* ``FSCNN_DSCONV_FUSED=0`` — (inference) each classifier DSConv as its depthwise and pointwise
  launches instead of one fused launch (csrc/dsconv.hip): bit-identical outputs
  (test_dsconv_fused_bit_identical).
* ``FSCNN_IR_S2=0``       — (inference) the stride-2 bottlenecks (1.0, 2.0) as their three unfused
  launches instead of the fused stride-2 block (csrc/ir.hip).
* ``FSCNN_FFM_HI=0``      — (inference) the FFM's high-res branch (conv_higher_res + BN) as its own
  GEMM, added as a stored residual by the fused launch, instead of a second GEMM inside it
  (test_ffm_hi_fused_bit_identical).
* ``FSCNN_LTD2_FUSED=0``  — (inference) LearningToDownsample.dsconv2 as its depthwise and pointwise
  launches instead of one (csrc/dsconv.hip ds2_fwd): bit-identical outputs
  (test_ltd2_fused_bit_identical).
* ``FSCNN_PPM_FUSED=0``   — (inference) the four PPM branch convs as four pointwise launches instead
  of one launch of 16-row matrix-core tiles (csrc/ppm.hip): bit-identical outputs
  (test_ppm_fused_bit_identical).

(Round 5 removed the measured-slower variants and their switches: FSCNN_DW_LOOP, FSCNN_GEMM_PF,
FSCNN_CE_HEAD, FSCNN_CE_PACK, FSCNN_GEMM_MINT; round 6's clean-up removed the training recompute
of the bottleneck's expanded tensor and its switch, measured +0.21 ms per step.)

Each child re-runs the oracle / golden parity tests that cover the path (fp32 train golden +
bf16 emulated budget; eval goldens for the fp32 GEMM switch).  The graph switch also replays
train steps with Dropout active and changing seeds; the losses, gradients and running statistics
must be bit-identical to direct launches (tests/_switch_worker.py).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = ["tests/test_gpu_model.py::test_train_fp32_vs_oracle_and_golden",
         "tests/test_gpu_model.py::test_fused_loss_head_vs_oracle",
         "tests/test_gpu_model.py::test_train_aux_vs_oracle_and_golden",
         "tests/test_gpu_fullsize.py::test_bf16_train_step_within_emulated_bf16_budget"]
EVAL = ["tests/test_gpu_model.py::test_eval_fp32_vs_golden",
        "tests/test_gpu_model.py::test_eval_fp32_literal_configs",
        "tests/test_gpu_model.py::test_eval_odd_sizes_vs_oracle",
        "tests/test_gpu_fullsize.py::test_eval_goldens_argmax_bit_exact"]
HEAD16 = ["tests/test_gpu_literal.py::test_fused_ce_head_16bit_vs_fp64"]
BF16 = ["tests/test_gpu_model.py::test_bf16_forward_within_bf16_budget"]
# (FSCNN_GRAPHS=1 + HEAD16: the int8 target pack forked to the side stream and joined before the
# head, inside a captured forward)
CASES = {"FSCNN_SIDE_STREAM=0": TRAIN, "FSCNN_F32_SPLIT=0": EVAL,
         "FSCNN_GRAPHS=1": TRAIN + EVAL + HEAD16 + ["tests/test_gpu_autograd.py"],
         "FSCNN_LTD_FUSED=0": TRAIN[-1:] + BF16, "FSCNN_SIDE_PRIO=0": TRAIN[:1],
         "FSCNN_SIDE_FENCE=1": TRAIN[:1],
         "FSCNN_DROP_FUSED=0": TRAIN[:1] + HEAD16, "FSCNN_STEM_FUSED=0": EVAL,
         "FSCNN_DSCONV_FUSED=0": EVAL, "FSCNN_IR_S2=0": EVAL, "FSCNN_FFM_HI=0": EVAL,
         "FSCNN_PPM_FUSED=0": EVAL, "FSCNN_LTD2_FUSED=0": EVAL}


def _env(switch):
    env = dict(os.environ)
    if switch:
        k, v = switch.split("=")
        env[k] = v
    return env


@pytest.mark.parametrize("switch", sorted(CASES))
def test_switch_keeps_oracle_parity(switch):
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider",
           "--timeout", "200", "--timeout-method", "thread"] + CASES[switch]
    r = subprocess.run(cmd, cwd=ROOT, env=_env(switch), capture_output=True, text=True,
                       timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    print(switch, tail[-400:])
    assert r.returncode == 0, "%s: parity tests failed\n%s" % (switch, tail)


def _worker(tmp_path, switch, half=None):
    out = str(tmp_path / ("%s%s.npz" % ((switch or "default").replace("=", "_"), half or "")))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_switch_worker.py"), out] +
                       ([half] if half else []),
                       cwd=ROOT, env=_env(switch), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return dict(np.load(out))


def _stem_worker(tmp_path, switch, dsconv=False, ppm=False):
    out = str(tmp_path / ("stem_%s%s.npz" % ((switch or "default").replace("=", "_"),
                                               "_ds" if dsconv else ("_ppm" if ppm else ""))))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_stem_worker.py"), out] +
                       (["--dsconv"] if dsconv else []) + (["--ppm"] if ppm else []),
                       cwd=ROOT, env=_env(switch), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return dict(np.load(out))


def _assert_outputs_bit_identical(ref, got):
    """Every output of the two _stem_worker runs (all keys but the launch counter): finite and
    bit-identical."""
    for k in ref:
        if k == "stem_launches":
            continue
        assert np.isfinite(got[k]).all(), k
        assert np.array_equal(ref[k], got[k]), "%s: max |diff| %g" % (
            k, float(np.abs(ref[k].astype(np.float64) - got[k]).max()))


def test_stem_fused_bit_identical(tmp_path):
    """The fused inference stem (conv0 + LTD.dsconv1 dw + pw in one launch, csrc/stem.hip) gives
    bit-identical outputs to the three unfused launches: fp32 / bf16 / fp16 images, autocast fp16
    over an fp32 image, partial edge tiles (tests/_stem_worker.py).  The default run really took
    the fused launch; the unaligned-width case falls back to the unfused launches."""
    ref = _stem_worker(tmp_path, "FSCNN_STEM_FUSED=0")
    got = _stem_worker(tmp_path, None)
    assert int(ref["stem_launches"]) == 0 and int(got["stem_launches"]) == 1
    _assert_outputs_bit_identical(ref, got)


def test_dsconv_fused_bit_identical(tmp_path):
    """The fused inference DSConv (depthwise + BN + ReLU and pointwise + BN (+ residual) + ReLU in
    one launch, csrc/dsconv.hip: the classifier's dsconv1 / dsconv2 and the FFM's upsample +
    dwconv + conv_lower_res + conv_higher_res) gives bit-identical outputs to the unfused launches: fp32 / bf16 / fp16
    images, autocast fp16, partial strips and row segments (tests/_stem_worker.py --dsconv).  The
    default run really took the three fused launches."""
    ref = _stem_worker(tmp_path, "FSCNN_DSCONV_FUSED=0", dsconv=True)
    got = _stem_worker(tmp_path, None, dsconv=True)
    # (+1 in both: LearningToDownsample.dsconv2's fused launch, FSCNN_LTD2_FUSED)
    assert int(ref["stem_launches"]) == 1 and int(got["stem_launches"]) == 4
    _assert_outputs_bit_identical(ref, got)


def test_ffm_hi_fused_bit_identical(tmp_path):
    """The FFM's high-res branch computed inside the fused launch (a second GEMM on the strip)
    gives bit-identical outputs to its own GEMM launch + the stored residual (FSCNN_FFM_HI=0)."""
    ref = _stem_worker(tmp_path, "FSCNN_FFM_HI=0", dsconv=True)
    got = _stem_worker(tmp_path, None, dsconv=True)
    assert int(ref["stem_launches"]) == 4 and int(got["stem_launches"]) == 4
    _assert_outputs_bit_identical(ref, got)


def test_ltd2_fused_bit_identical(tmp_path):
    """LearningToDownsample.dsconv2 in one launch (depthwise 3x3 s2 + BN + ReLU, pointwise
    48 -> 64 + BN + ReLU; csrc/dsconv.hip ds2_fwd) gives bit-identical outputs to its depthwise
    and pointwise launches: fp32 / bf16 / fp16 images, autocast fp16, partial 4 x 16 tiles
    (tests/_stem_worker.py --dsconv: the maps give >= 4096 dsconv2 pixels, where the unfused
    pointwise takes the streaming GEMM whose MFMA order the fused launch reproduces).  The
    default run really took the fused launch (4 DSConv launches against 3)."""
    ref = _stem_worker(tmp_path, "FSCNN_LTD2_FUSED=0", dsconv=True)
    got = _stem_worker(tmp_path, None, dsconv=True)
    assert int(ref["stem_launches"]) == 3 and int(got["stem_launches"]) == 4
    _assert_outputs_bit_identical(ref, got)


def test_ppm_fused_bit_identical(tmp_path):
    """The inference PPM branch convs (conv1..conv4 + folded BN + ReLU) as one launch of 16-row
    matrix-core tiles give bit-identical outputs to the four pointwise GEMM launches: fp32 (the
    three-term split) / bf16 / fp16 / autocast fp16, bins of 1..288 rows with partial tiles
    (tests/_stem_worker.py --ppm).  The default run really took the one launch."""
    ref = _stem_worker(tmp_path, "FSCNN_PPM_FUSED=0", ppm=True)
    got = _stem_worker(tmp_path, None, ppm=True)
    assert int(ref["stem_launches"]) == 0 and int(got["stem_launches"]) == 1
    _assert_outputs_bit_identical(ref, got)


@pytest.mark.parametrize("switch", ["FSCNN_GRAPHS=1", "FSCNN_SIDE_STREAM=0", "FSCNN_SIDE_FENCE=1"])
def test_switch_train_steps_bit_identical_with_dropout(tmp_path, switch):
    ref = _worker(tmp_path, None)
    got = _worker(tmp_path, switch)
    assert sorted(ref) == sorted(got)
    # the seeds differ between steps 0/1 (and repeat at 2/3): the dropout mask really changes
    assert not np.array_equal(ref["grad0"], ref["grad1"])
    # and the same seed gives the same step (train-mode BN does not read the running statistics)
    assert np.array_equal(ref["grad0"], ref["grad2"])
    for k in ref:
        assert np.array_equal(ref[k], got[k]), "%s: %s differs" % (switch, k)


def test_ltd_fused_backward_matches_two_pass(tmp_path):
    """The fused LTD.dsconv1.dw-dgrad + conv0-wgrad pass (conv0.hip ltd_c0_bwd) against the
    two-launch form it replaces, bf16 train plan, 4 steps: every gradient other than conv0's
    weight and its BN's gamma / beta is bit-identical (the fused pass changes no other value); those
    three differ only by summation order and by dz no longer being rounded to bf16 before the
    product (dW = al*A + gz*Zx + be*B in fp32): within 1e-2 of the tensor's max |value|."""
    ref = _worker(tmp_path, "FSCNN_LTD_FUSED=0", "bf16")
    got = _worker(tmp_path, None, "bf16")
    names = [str(n) for n in ref["names"]]
    off = np.concatenate([[0], np.cumsum(ref["sizes"])])
    loose = {"learning_to_downsample.conv.conv.0.weight", "learning_to_downsample.conv.conv.1.weight",
             "learning_to_downsample.conv.conv.1.bias"}
    assert loose <= set(names)
    for i in range(4):
        assert ref["loss%d" % i] == got["loss%d" % i]
        a, b = ref["grad%d" % i], got["grad%d" % i]
        for j, n in enumerate(names):
            x, y = a[off[j]:off[j + 1]], b[off[j]:off[j + 1]]
            if n in loose:
                scale = float(np.abs(x).max())
                assert scale > 0 and float(np.abs(x - y).max()) <= 1e-2 * scale, (i, n)
            else:
                assert np.array_equal(x, y), (i, n)


def test_ltd_fused_backward_with_shifted_bn_mean(tmp_path):
    """conv0's weight gradient with its BN mean far from 0 (image + 4.0, 2 x 3 x 512 x 1024),
    against fp64 from the step's stored tensors (g, z, BN statistics, image; the two-launch run
    keeps g): the fused pass accumulates sum x (z - mean) (conv0.hip ltd_c0_bwd), so
    dW = al*A + gz*Zc + (be + gz*mean)*B has no cancellation of terms growing with |mean| / std.
    Everything upstream of conv0's weight gradient is bit-identical in both runs (previous test),
    so both are measured against the same exact value: the fused one must be within 1e-3 of the
    tensor's scale, and no worse than the two-launch path (which rounds dz to bf16 before its
    sum over ~500 K pixels of x ~ 4: that rounding no longer cancels)."""
    ref = _worker(tmp_path, "FSCNN_LTD_FUSED=0", "bf16shift")
    got = _worker(tmp_path, None, "bf16shift")
    names = [str(n) for n in ref["names"]]
    off = np.concatenate([[0], np.cumsum(ref["sizes"])])
    j = names.index("learning_to_downsample.conv.conv.0.weight")
    exact = ref["c0exact0"].astype(np.float64)
    two = ref["grad0"][off[j]:off[j + 1]].astype(np.float64)
    fused = got["grad0"][off[j]:off[j + 1]].astype(np.float64)
    scale = float(np.abs(exact).max())
    e_two, e_fused = float(np.abs(two - exact).max()), float(np.abs(fused - exact).max())
    print("conv0 dW (shifted mean) vs fp64: fused %.3e, two-launch %.3e, scale %.3e"
          % (e_fused, e_two, scale))
    assert scale > 0 and e_fused <= 1e-3 * scale
    assert e_fused <= e_two


def test_drop_fused_matches_separate_passes(tmp_path):
    """The classifier's Dropout backward and dsconv2 pw's BN-backward reduce fused into the
    classifier conv's dgrad epilogue (net.cpp backward_head; the streaming kernel's form, 16-bit
    plans at M >= 4096 low-res pixels: 2 x 3 x 256 x 512 bf16, Dropout active) against the
    separate dropout and reduce passes (FSCNN_DROP_FUSED=0), 4 steps: the losses and the classifier
    conv's own gradients are bit-identical (same inputs); the BN whose backward sums the epilogue
    forms (classifier.dsconv2 pw) within 1e-3 of its scale (summation order only); every other
    tensor within 1e-1 of its scale and the whole gradient at cosine >= 0.999 (a last-bit change
    of a BN-backward coefficient moves bf16 roundings downstream, and 20 train-mode BatchNorms
    amplify them on the way to conv0: measured worst 7.0e-2, LTD conv0's BN weight, r05)."""
    ref = _worker(tmp_path, "FSCNN_DROP_FUSED=0", "bf16drop")
    got = _worker(tmp_path, None, "bf16drop")
    names = [str(n) for n in ref["names"]]
    off = np.concatenate([[0], np.cumsum(ref["sizes"])])
    exact = {"classifier.conv.1.weight", "classifier.conv.1.bias"}
    near = {"classifier.dsconv2.conv.4.weight", "classifier.dsconv2.conv.4.bias"}
    assert exact <= set(names) and near <= set(names)
    worst = (0.0, None)
    for i in range(4):
        assert ref["loss%d" % i] == got["loss%d" % i]
        a, b = ref["grad%d" % i], got["grad%d" % i]
        assert not np.array_equal(a, ref["grad%d" % ((i + 1) % 4)])  # the seed matters
        cos = float(a.astype(np.float64) @ b / (np.linalg.norm(a) * np.linalg.norm(b)))
        assert cos >= 0.999, (i, cos)
        for j, n in enumerate(names):
            x, y = a[off[j]:off[j + 1]], b[off[j]:off[j + 1]]
            if n in exact:
                assert np.array_equal(x, y), (i, n)
                continue
            scale = float(np.abs(x).max())
            err = float(np.abs(x - y).max())
            worst = max(worst, (err / max(scale, 1e-30), n))
            # (floor: 1e-3 of the whole gradient's largest element -- the project BNs' biases
            # feed a train-mode BN's input gradient, whose per-channel sum vanishes identically,
            # so theirs are rounding noise, ~1e-5 of the weights')
            floor = 1e-3 * float(np.abs(a).max())
            assert err <= (1e-3 if n in near else 1e-1) * scale + floor, (i, n, err, scale)
    print("drop fused vs separate: worst relative %.2e (%s)" % worst)
