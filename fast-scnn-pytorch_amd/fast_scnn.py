"""Fast-SCNN with the reference interface, executed by the gfx950 HIP library.

Drop-in for ``models/fast_scnn.py`` of Shinokawa/Fast-SCNN-pytorch:

* ``__all__ = ['FastSCNN', 'get_fast_scnn']`` (reference :13);
* ``FastSCNN(num_classes, aux=False, **kwargs)`` (:16-17) with the same submodule tree, so
  ``state_dict()`` keys / shapes (Appendix A of SURVEY.md) and attribute paths such as
  ``model.classifier.conv[1].out_channels`` or ``ppm.conv1.conv[0]`` are unchanged;
* ``forward(x)`` returns a ``tuple`` of NCHW logits at the input resolution (:33-46);
* ``get_fast_scnn(dataset, pretrained, root, map_cpu, **kwargs)`` (:240-256) with a static
  NUM_CLASS table instead of importing the data loaders (no torchvision dependency).

The parameters are re-homed into one flat fp32 arena (64-B aligned tensors, layout owned by the
C++ executor), running statistics into a second arena; ``.grad`` tensors returned by backward
are views of one flat gradient arena, so the fused SGD and the RCCL all-reduce each touch a
single buffer.  The submodules are parameter containers only: the whole network runs as one
native forward and one staged native backward.  CPU tensors raise — there is no fallback.
"""
import collections
import os
import threading

import torch
import torch.nn as nn

from . import _lib
from .arch import NUM_CLASS

__all__ = ["FastSCNN", "get_fast_scnn"]


# ---------------------------------------------------------------------------------------------
# parameter containers (attribute schema of models/fast_scnn.py:49-237)
# ---------------------------------------------------------------------------------------------
class _Container(nn.Module):
    def forward(self, *args, **kwargs):  # pragma: no cover - guard
        raise RuntimeError("%s is a parameter container; call the FastSCNN module"
                           % type(self).__name__)


def _seq_conv_bn_relu(cin, cout, k, stride, padding, groups=1):
    return nn.Sequential(nn.Conv2d(cin, cout, k, stride, padding, groups=groups, bias=False),
                         nn.BatchNorm2d(cout), nn.ReLU(True))


class _ConvBNReLU(_Container):
    """models/fast_scnn.py:49-61 (padding defaults to 0)."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=0, **kwargs):
        super().__init__()
        self.conv = _seq_conv_bn_relu(in_channels, out_channels, kernel_size, stride, padding)


class _DSConv(_Container):
    """models/fast_scnn.py:64-79: dw3x3 → BN → ReLU → pw → BN → ReLU."""

    def __init__(self, dw_channels, out_channels, stride=1, **kwargs):
        super().__init__()
        dw = _seq_conv_bn_relu(dw_channels, dw_channels, 3, stride, 1, groups=dw_channels)
        pw = _seq_conv_bn_relu(dw_channels, out_channels, 1, 1, 0)
        self.conv = nn.Sequential(*dw, *pw)


class _DWConv(_Container):
    """models/fast_scnn.py:82-92."""

    def __init__(self, dw_channels, out_channels, stride=1, **kwargs):
        super().__init__()
        self.conv = _seq_conv_bn_relu(dw_channels, out_channels, 3, stride, 1, groups=dw_channels)


class LinearBottleneck(_Container):
    """models/fast_scnn.py:95-115 (t = 6, shortcut iff stride 1 and Cin == Cout)."""

    def __init__(self, in_channels, out_channels, t=6, stride=2, **kwargs):
        super().__init__()
        self.use_shortcut = stride == 1 and in_channels == out_channels
        e = in_channels * t
        self.block = nn.Sequential(_ConvBNReLU(in_channels, e, 1), _DWConv(e, e, stride),
                                   nn.Conv2d(e, out_channels, 1, bias=False),
                                   nn.BatchNorm2d(out_channels))


class PyramidPooling(_Container):
    """models/fast_scnn.py:118-145."""

    def __init__(self, in_channels, out_channels, **kwargs):
        super().__init__()
        inter = int(in_channels / 4)
        for i in range(1, 5):
            setattr(self, "conv%d" % i, _ConvBNReLU(in_channels, inter, 1))
        self.out = _ConvBNReLU(in_channels * 2, out_channels, 1)


class LearningToDownsample(_Container):
    """models/fast_scnn.py:148-161."""

    def __init__(self, dw_channels1=32, dw_channels2=48, out_channels=64, **kwargs):
        super().__init__()
        self.conv = _ConvBNReLU(3, dw_channels1, 3, 2)
        self.dsconv1 = _DSConv(dw_channels1, dw_channels2, 2)
        self.dsconv2 = _DSConv(dw_channels2, out_channels, 2)


class GlobalFeatureExtractor(_Container):
    """models/fast_scnn.py:164-187."""

    def __init__(self, in_channels=64, block_channels=(64, 96, 128), out_channels=128, t=6,
                 num_blocks=(3, 3, 3), **kwargs):
        super().__init__()
        strides = (2, 2, 1)
        cin = in_channels
        for i, (cout, n, s) in enumerate(zip(block_channels, num_blocks, strides)):
            blocks = [LinearBottleneck(cin if j == 0 else cout, cout, t, s if j == 0 else 1)
                      for j in range(n)]
            setattr(self, "bottleneck%d" % (i + 1), nn.Sequential(*blocks))
            cin = cout
        self.ppm = PyramidPooling(block_channels[2], out_channels)


class FeatureFusionModule(_Container):
    """models/fast_scnn.py:190-218."""

    def __init__(self, highter_in_channels, lower_in_channels, out_channels, scale_factor=4,
                 **kwargs):
        super().__init__()
        self.scale_factor = scale_factor
        self.dwconv = _DWConv(lower_in_channels, out_channels, 1)
        self.conv_lower_res = nn.Sequential(nn.Conv2d(out_channels, out_channels, 1),
                                            nn.BatchNorm2d(out_channels))
        self.conv_higher_res = nn.Sequential(nn.Conv2d(highter_in_channels, out_channels, 1),
                                             nn.BatchNorm2d(out_channels))
        self.relu = nn.ReLU(True)


class Classifer(_Container):
    """models/fast_scnn.py:221-237 (reference spelling kept)."""

    def __init__(self, dw_channels, num_classes, stride=1, **kwargs):
        super().__init__()
        self.dsconv1 = _DSConv(dw_channels, dw_channels, stride)
        self.dsconv2 = _DSConv(dw_channels, dw_channels, stride)
        self.conv = nn.Sequential(nn.Dropout(0.1), nn.Conv2d(dw_channels, num_classes, 1))


# ---------------------------------------------------------------------------------------------
# native network handle + plans
# ---------------------------------------------------------------------------------------------
class _Native:
    """Owns the C++ fscnn_net and a cache of fscnn_plan handles."""

    def __init__(self, num_classes, aux):
        lib = _lib.load()
        h = _lib.c_vp()
        _lib.check(lib.fscnn_net_create(num_classes, int(aux), _lib.ctypes.byref(h)),
                   "fscnn_net_create")
        self.h = h
        self.lib = lib
        n, tot = _lib.c_int(), _lib.c_ll()
        _lib.check(lib.fscnn_net_param_count(h, _lib.ctypes.byref(n), _lib.ctypes.byref(tot)))
        self.p_total = tot.value
        self.params = [self._info("fscnn_net_param_info", i) for i in range(n.value)]
        nb, rtot, nbn = _lib.c_int(), _lib.c_ll(), _lib.c_int()
        _lib.check(lib.fscnn_net_buffer_count(h, _lib.ctypes.byref(nb), _lib.ctypes.byref(rtot),
                                              _lib.ctypes.byref(nbn)))
        self.r_total, self.n_bn = rtot.value, nbn.value
        self.buffers = [self._info("fscnn_net_buffer_info", i) for i in range(nb.value)]
        self.stage_ranges = []
        for s in range(4):
            b, e = _lib.c_ll(), _lib.c_ll()
            _lib.check(lib.fscnn_net_stage_range(h, s, _lib.ctypes.byref(b), _lib.ctypes.byref(e)))
            self.stage_ranges.append((b.value, e.value))
        self.plans = {}
        self._lock = threading.Lock()

    def _info(self, fn, i):
        name, off, numel = _lib.c_char_p(), _lib.c_ll(), _lib.c_ll()
        _lib.check(getattr(self.lib, fn)(self.h, i, _lib.ctypes.byref(name), _lib.ctypes.byref(off),
                                         _lib.ctypes.byref(numel)), fn)
        return name.value.decode(), off.value, numel.value

    def plan(self, N, H, W, dtype_code, train, device=None):
        """Plan of one (N, H, W, dtype, mode) on one device.  Plans are per device (each owns its
        side stream and graph cache) and created under a lock: DataParallel's worker threads
        (train.py:170-171 -> parallel_apply) reach here concurrently."""
        key = (None if device is None else device.index, N, H, W, dtype_code, int(train))
        p = self.plans.get(key)
        if p is not None:
            return p
        with self._lock:
            p = self.plans.get(key)
            if p is not None:
                return p
            h = _lib.c_vp()
            _lib.check(self.lib.fscnn_plan_create(self.h, N, H, W, dtype_code, int(train),
                                                  _lib.ctypes.byref(h)), "fscnn_plan_create")
            fw, bw = _lib.c_ll(), _lib.c_ll()
            _lib.check(self.lib.fscnn_plan_workspace(h, _lib.ctypes.byref(fw),
                                                     _lib.ctypes.byref(bw)))
            p = (h, fw.value, bw.value)
            self.plans[key] = p
        return p

    def __del__(self):
        try:
            for h, _, _ in self.plans.values():
                self.lib.fscnn_plan_destroy(h)
            self.lib.fscnn_net_destroy(self.h)
        except Exception:
            pass


class _Shared:
    """State a FastSCNN shares with its DataParallel replicas: ``replicate()``
    (torch/nn/parallel/replicate.py, driven by train.py:170-171) shallow-copies the module's
    ``__dict__``, so every replica sees this same object — one native net handle and one plan
    cache for the whole wrapper.  A deep copy / pickle of the model starts a fresh one."""

    def __init__(self):
        self.native = None
        self.lock = threading.Lock()

    def __deepcopy__(self, memo):
        return _Shared()

    def __getstate__(self):
        return {}

    def __setstate__(self, state):
        self.__init__()


MODE_EVAL, MODE_TRAIN, MODE_EVAL_GRAD = 0, 1, 2  # plan modes (include/fastscnn.h fscnn_plan_create)
E_UNSUPPORTED = -2  # the library's "this kernel does not take the geometry" status


class _FastSCNNFunction(torch.autograd.Function):
    """Whole-network forward / staged backward; grads are views of one flat arena.

    train mode: the training forward keeps its workspace (every pre-BN tensor) for the backward.
    eval mode (the reference module stays differentiable: models/fast_scnn.py:33-46 has no
    no_grad, and eval.py:43 calls it with grad enabled): the forward is the fused inference path
    (same speed and memory as under no_grad), and the backward first recomputes the forward as a
    differentiable-inference plan (mode 2: every BatchNorm normalised by its running statistics,
    Dropout off) and then runs the staged backward of that plan.  The parameters are saved for
    the backward, so autograd refuses one that changed in place in between, as it would for the
    reference's convolution weights."""

    @staticmethod
    def forward(ctx, x, model, ar, *params):
        ctx.model, ctx.ar = model, ar
        if model.training:
            outs, ws, seed, dt, xc = model._run_forward(x, MODE_TRAIN, ar=ar)
            ctx.mode, ctx.ws, ctx.seed, ctx.dt = MODE_TRAIN, ws, seed, dt
        else:
            outs, _, _, dt, xc = model._run_forward(x, MODE_EVAL, ar=ar)
            ctx.mode, ctx.ws, ctx.seed, ctx.dt = MODE_EVAL_GRAD, None, 0, dt
            # the backward recomputes this forward from the running statistics: remember their
            # version (a train-mode forward or a load_state_dict in between bumps it)
            ctx.r_version = ar["R"]._version
        ctx.x_dtype = x.dtype
        # the converted dense NCHW fp32/bf16 copy the forward read, not the caller's tensor: the
        # conv0 weight gradient re-reads it as dense NCHW (channels_last / fp16 / expanded inputs)
        ctx.save_for_backward(xc, *params)
        return outs if len(outs) > 1 else outs[0]

    @staticmethod
    def backward(ctx, *gouts):
        x = ctx.saved_tensors[0]  # (autograd checks the saved parameters' versions here)
        gaux = gouts[1] if len(gouts) > 1 else None
        model, ws = ctx.model, ctx.ws
        if ctx.mode == MODE_EVAL_GRAD:
            if ctx.ar["R"]._version != ctx.r_version:
                raise RuntimeError(
                    "one of the variables needed for gradient computation has been modified by an "
                    "inplace operation: the BatchNorm running statistics changed (a train-mode "
                    "forward or a state_dict load) between this eval-mode forward and its backward")
            # (in the forward's arithmetic: autocast is not active where autograd runs backward)
            _, ws, _, _, _ = model._run_forward(x, MODE_EVAL_GRAD, ar=ctx.ar, dt=ctx.dt)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        grads = model._run_backward(gouts[0], x, ws, ctx.seed, ctx.dt, ctx.ar, gaux=gaux,
                                    mode=ctx.mode, dx=dx)
        ctx.ws = ctx.ar = None
        if dx is not None and dx.dtype != ctx.x_dtype:
            dx = dx.to(ctx.x_dtype)
        return (dx, None, None) + tuple(grads)


def _head_spec(criterion, ignore_index=-1):
    """The fused loss head a criterion object maps to, as a tuple:

    ``("ce", ignore_index)`` or ``("dice", smooth, dice_weight, focal_weight, alpha, gamma)``.

    Duck-typed on the class name and the attributes of utils/loss.py, so this package's criteria
    (``loss.py``) and the reference's own ``utils.loss`` objects (what train.py:183-191 builds)
    resolve alike; ``None`` is the CE head with the given ``ignore_index``.  Criteria without a
    fused head (the OHEM criterion, anything unknown) raise ``RuntimeError``."""
    if criterion is None:
        return ("ce", int(ignore_index))
    names = [c.__name__ for c in type(criterion).__mro__]
    if "SoftmaxCrossEntropyOHEMLoss" in names or "MixSoftmaxCrossEntropyOHEMLoss" in names:
        raise RuntimeError("forward_loss: the OHEM criterion has no fused loss head here; use "
                           "forward_loss_ohem(x, target, criterion), or the unfused path, "
                           "criterion(model(x), target)")
    if "FocalDiceLoss" in names:
        inner = getattr(criterion, "dice_loss", None)  # the reference keeps smooth there
        smooth = inner.smooth if inner is not None else criterion.smooth
        dw = float(criterion.dice_weight)
        return ("dice", float(smooth), dw, 1.0 - dw, float(criterion.alpha),
                float(criterion.gamma))
    if "MixDiceLoss" in names:
        return ("dice", float(criterion.dice_loss.smooth), 1.0, 0.0, 0.5, 2.0)
    if "DiceLoss" in names:
        return ("dice", float(criterion.smooth), 1.0, 0.0, 0.5, 2.0)
    if "MixSoftmaxCrossEntropyLoss" in names:
        return ("ce", int(criterion.ignore_index))
    raise RuntimeError("forward_loss: no fused loss head for %s; use the unfused path, "
                       "criterion(model(x), target)" % type(criterion).__name__)


def _ohem_spec(criterion):
    """The fused OHEM head's arguments of a criterion object, as the tuple
    ``("ohem", ignore_label, thresh, min_kept, weight_or_None)``.

    Duck-typed like ``_head_spec``: ``SoftmaxCrossEntropyOHEMLoss`` /
    ``MixSoftmaxCrossEntropyOHEMLoss`` of this package (class weights in ``.weight``) or of
    utils/loss.py:127-206 (class weights in ``.criterion.weight``, the inner
    ``nn.CrossEntropyLoss``).  Anything else raises ``RuntimeError``."""
    names = [c.__name__ for c in type(criterion).__mro__]
    if "SoftmaxCrossEntropyOHEMLoss" not in names and "MixSoftmaxCrossEntropyOHEMLoss" not in names:
        raise RuntimeError("forward_loss_ohem: %s is not the OHEM criterion "
                           "(SoftmaxCrossEntropyOHEMLoss / MixSoftmaxCrossEntropyOHEMLoss); use "
                           "forward_loss, or the unfused path, criterion(model(x), target)"
                           % type(criterion).__name__)
    try:
        inner = getattr(criterion, "criterion", None)  # the reference keeps the weights there
        weight = inner.weight if inner is not None else criterion.weight
        return ("ohem", int(criterion.ignore_label), float(criterion.thresh),
                int(criterion.min_kept), weight)
    except AttributeError as e:
        raise RuntimeError("forward_loss_ohem: %s lacks the OHEM criterion's attributes (%s); "
                           "use the unfused path, criterion(model(x), target)"
                           % (type(criterion).__name__, e))


def _aux_head_spec(criterion):
    """The fused aux loss heads (``forward_loss_aux``) a two-output criterion maps to, as a tuple
    whose second entry is ``aux_weight``:

    ``("ce", aux_weight, ignore_index)``, ``("dice", aux_weight, smooth)`` or
    ``("ohem", aux_weight, ignore_label, thresh, min_kept, weight_or_None)``.

    Duck-typed like ``_head_spec`` / ``_ohem_spec``: ``MixSoftmaxCrossEntropyLoss``,
    ``MixDiceLoss`` and ``MixSoftmaxCrossEntropyOHEMLoss`` of this package or of utils/loss.py
    (what train.py:183-191 builds with ``--aux``).  A criterion with ``aux`` false, the
    single-output criteria (``DiceLoss``, ``FocalDiceLoss``, ``SoftmaxCrossEntropyOHEMLoss``) and
    anything unknown raise ``RuntimeError``."""
    names = [c.__name__ for c in type(criterion).__mro__]
    unfused = "use the unfused path, criterion(model(x), target)"
    try:
        if "MixSoftmaxCrossEntropyOHEMLoss" in names:
            spec = ("ohem", float(criterion.aux_weight)) + _ohem_spec(criterion)[1:]
        elif "MixDiceLoss" in names:
            spec = ("dice", float(criterion.aux_weight), float(criterion.dice_loss.smooth))
        elif "MixSoftmaxCrossEntropyLoss" in names:
            spec = ("ce", float(criterion.aux_weight), int(criterion.ignore_index))
        else:
            raise RuntimeError("forward_loss_aux: no fused aux loss heads for %s (they take "
                               "MixSoftmaxCrossEntropyLoss, MixDiceLoss and "
                               "MixSoftmaxCrossEntropyOHEMLoss); %s"
                               % (type(criterion).__name__, unfused))
        aux = bool(criterion.aux)
    except AttributeError as e:
        raise RuntimeError("forward_loss_aux: %s lacks the criterion's attributes (%s); %s"
                           % (type(criterion).__name__, e, unfused))
    if not aux:
        raise RuntimeError("forward_loss_aux: the criterion has aux=False (it would drop the aux "
                           "output); build it with aux=True, or %s" % unfused)
    return spec


# what a native forward's prologue hands its entry (FastSCNN._prologue): the plan, the buffers and
# converted tensors, and the C call's common arguments -- src = (plan, x, x_dtype) leads, mem =
# (P, R, NBT, ws) and end = ([seed, p, momentum,] stream) close it
_Call = collections.namedtuple("_Call", "plan fw ws dt x target N H W dev p seed ar src mem end")
# what the backward needs of a fused loss head: its C backward entry, the entry's arguments
# between grad_loss and x, the head's own workspace or None, and what those point to (kept alive)
_Head = collections.namedtuple("_Head", "entry lead head_ws keep")
_ONE_SAMPLE = ("Expected more than 1 value per channel when training, got input size "
               "torch.Size([1, 32, 1, 1])")


class _FastSCNNLossFunction(torch.autograd.Function):
    """Fused train step heads: loss = criterion(upsample(logits_lowres), target) at low
    resolution, for an aux model L(out) + aux_weight * L(aux_out).  ``entry`` names the model's
    method; ``spec`` is its criterion tuple (``_head_spec``, ``_ohem_spec`` or ``_aux_head_spec``;
    OHEM weights on the device), whose first item picks the forward.  The forward's ``_Head``
    travels to the backward.  The returned loss shares the storage of the head's loss tensor."""

    @staticmethod
    def forward(ctx, x, target, entry, spec, model, ar, *params):
        if spec[0] == "dice" and ctx.needs_input_grad[0]:
            raise RuntimeError("%s: the fused Dice head does not form the input image's "
                               "gradient; use criterion(model(x), target)" % entry)
        aux = entry == "forward_loss_aux"
        run = model._run_forward_loss_aux if aux else {
            "ce": model._run_forward_loss, "dice": model._run_forward_loss_dice,
            "ohem": model._run_forward_loss_ohem}[spec[0]]
        loss, c, ctx.head = run(x, target, spec, ar)
        ctx.model, ctx.ar = model, ar
        ctx.ws, ctx.seed, ctx.dt = c.ws, c.seed, c.dt
        ctx.x_dtype = x.dtype
        ctx.save_for_backward(c.x, *params)
        if aux:
            model._last_loss_terms = loss[1:]
        # the first element of what the head wrote (CE / OHEM: the (mean, count) pair), as a
        # tensor sharing its storage but not an autograd view (a view created here would refuse
        # the in-place ops the reference's loss tensor allows: loss /= accum_steps); the backward
        # never reads it
        out = torch.empty((), dtype=loss.dtype, device=loss.device)
        return out.set_(loss.untyped_storage(), loss.storage_offset(), (), ())

    @staticmethod
    def backward(ctx, gloss):
        x = ctx.saved_tensors[0]
        g = gloss.to(torch.float32).reshape(1).contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        grads = ctx.model._run_backward(None, x, ctx.ws, ctx.seed, ctx.dt, ctx.ar, gloss=g,
                                        dx=dx, head=ctx.head)
        ctx.ws = ctx.ar = ctx.head = None
        if dx is not None and dx.dtype != ctx.x_dtype:
            dx = dx.to(ctx.x_dtype)
        return (dx, None, None, None, None, None) + tuple(grads)


class FastSCNN(nn.Module):
    """Fast-SCNN (models/fast_scnn.py:16-46) on the MI355X HIP path."""

    def __init__(self, num_classes, aux=False, **kwargs):
        super().__init__()
        self.aux = aux
        self.learning_to_downsample = LearningToDownsample(32, 48, 64)
        self.global_feature_extractor = GlobalFeatureExtractor(64, [64, 96, 128], 128, 6, [3, 3, 3])
        self.feature_fusion = FeatureFusionModule(64, 128, 128)
        self.classifier = Classifer(128, num_classes)
        if self.aux:
            self.auxlayer = nn.Sequential(nn.Conv2d(64, 32, 3, padding=1, bias=False),
                                          nn.BatchNorm2d(32), nn.ReLU(True), nn.Dropout(0.1),
                                          nn.Conv2d(32, num_classes, 1))
        self.num_classes = num_classes
        object.__setattr__(self, "_shared", _Shared())
        object.__setattr__(self, "_arena", None)
        object.__setattr__(self, "grad_stage_hook", None)
        object.__setattr__(self, "_last_validate_fused", None)  # route of the last validate()

    # ---- arenas ----------------------------------------------------------------------------
    def native(self):
        sh = self._shared
        if sh.native is None:
            with sh.lock:
                if sh.native is None:
                    nat = _Native(self.num_classes, self.aux)
                    names = [n for n, _ in self._named_params()]
                    if names != [p[0] for p in nat.params]:
                        raise RuntimeError("FastSCNN: parameter table mismatch with the native "
                                           "executor")
                    sh.native = nat
        return sh.native

    def _is_dp_replica(self):
        return bool(getattr(self, "_is_replica", False))

    def _named_params(self):
        """named_parameters() of the module, or of a DataParallel replica: ``replicate()`` keeps
        a replica's (non-leaf, broadcast) parameter tensors as plain attributes and lists them in
        each submodule's ``_former_parameters`` in ``_parameters`` order."""
        if not self._is_dp_replica():
            return list(self.named_parameters())
        out = []
        for mname, m in self.named_modules():
            for k, t in getattr(m, "_former_parameters", {}).items():
                if t is not None:
                    out.append((mname + "." + k if mname else k, t))
        return out

    def _apply(self, fn, recurse=True):
        r = super()._apply(fn, recurse)
        object.__setattr__(self, "_arena", None)
        return r

    def _pack_arena(self):
        """Re-home params / buffers into the executor's flat arenas on their current device."""
        nat = self.native()
        params = list(self.parameters())
        dev = params[0].device
        P = torch.zeros(nat.p_total, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, (_, off, numel) in zip(params, nat.params):
                if p.numel() != numel or p.dtype != torch.float32:
                    raise RuntimeError("FastSCNN: parameter %s has unexpected shape/dtype" % (_,))
                P[off:off + numel].copy_(p.detach().reshape(-1))
                p.data = P[off:off + numel].view(p.shape)
            R = torch.zeros(nat.r_total, dtype=torch.float32, device=dev)
            NBT = torch.zeros(nat.n_bn, dtype=torch.int64, device=dev)
            mods = dict(self.named_modules())
            for name, off, numel in nat.buffers:
                mname, bname = name.rsplit(".", 1)
                m = mods[mname]
                cur = m._buffers[bname]
                if bname == "num_batches_tracked":
                    NBT[off].copy_(cur.reshape(()))
                    m._buffers[bname] = NBT[off]
                else:
                    R[off:off + numel].copy_(cur.reshape(-1))
                    m._buffers[bname] = R[off:off + numel]
        arena = {"P": P, "R": R, "NBT": NBT, "params": params,
                 "ptrs": (params[0].data_ptr(), params[-1].data_ptr())}
        object.__setattr__(self, "_arena", arena)
        return arena

    def arena(self):
        a = self._arena
        params = None
        if a is not None:
            params = a["params"]
            if (params[0].data_ptr(), params[-1].data_ptr()) != a["ptrs"] or \
                    params[0].data_ptr() != a["P"].data_ptr():
                a = None
        if a is None:
            a = self._pack_arena()
        return a

    def _replica_arena(self, dev):
        """Arenas of a DataParallel replica (train.py:170-171) on ``dev``.

        Replica 0 aliases the module's own tensors (``comm.broadcast_coalesced`` returns the
        source device's inputs), so its parameters and buffers already are views of the packed
        arenas.  Any other replica holds broadcast copies: they are packed into fresh arenas on
        its device for this call (one multi-tensor copy each), and the running statistics the
        train forward updates are written back into the replica's own buffers, as aten's
        batch_norm would have updated them.  ``params`` are always the replica's tensors, so the
        autograd Function's gradients flow back through ``Broadcast`` (reduce-add to cuda:0)."""
        nat = self.native()
        params = [t for _, t in self._named_params()]
        if len(params) != len(nat.params):
            raise RuntimeError("FastSCNN replica: %d parameters, executor expects %d"
                               % (len(params), len(nat.params)))
        mods = dict(self.named_modules())
        bufs = []
        for name, off, numel in nat.buffers:
            mname, bname = name.rsplit(".", 1)
            bufs.append((mods[mname]._buffers[bname], off, numel, bname == "num_batches_tracked"))
        m = self._arena  # the module's arenas, as they were when replicate() copied __dict__
        if m is not None and m["P"].device == dev:
            P, R, NBT = m["P"], m["R"], m["NBT"]
            pb, rb, nb = P.data_ptr(), R.data_ptr(), NBT.data_ptr()
            alias = all(t.data_ptr() == pb + 4 * off
                        for t, (_, off, _n) in zip((params[0], params[-1]),
                                                   (nat.params[0], nat.params[-1])))
            alias = alias and all(t.data_ptr() == (nb + 8 * off if isn else rb + 4 * off)
                                  for t, off, _n, isn in (bufs[0], bufs[-1], bufs[1]))
            if alias:
                return {"P": P, "R": R, "NBT": NBT, "params": params, "writeback": None}
        with torch.no_grad():
            P = torch.zeros(nat.p_total, dtype=torch.float32, device=dev)
            R = torch.zeros(nat.r_total, dtype=torch.float32, device=dev)
            NBT = torch.zeros(nat.n_bn, dtype=torch.int64, device=dev)
            pv = [P[off:off + numel] for _, off, numel in nat.params]
            torch._foreach_copy_(pv, [p.detach().reshape(-1) for p in params])
            rv = [NBT[off] if isn else R[off:off + numel] for _, off, numel, isn in bufs]
            bt = [b if isn else b.reshape(-1) for b, _o, _n, isn in bufs]
            torch._foreach_copy_(rv, bt)
        return {"P": P, "R": R, "NBT": NBT, "params": params, "writeback": (bt, rv)}

    def _exec_arena(self, dev):
        return self._replica_arena(dev) if self._is_dp_replica() else self.arena()

    @staticmethod
    def _writeback(ar):
        """Running statistics of a replica's packed copy -> the replica's own buffers."""
        wb = ar.get("writeback")
        if wb is not None:
            with torch.no_grad():
                torch._foreach_copy_(wb[0], wb[1])

    def load_state_dict(self, state_dict, strict=True, assign=False):
        r = super().load_state_dict(state_dict, strict=strict, assign=assign)
        if assign:
            object.__setattr__(self, "_arena", None)
        return r

    # ---- execution ----------------------------------------------------------------------------
    def _compute_dtype(self, x, train):
        """Arithmetic of the call, as the reference's convolutions would run it.

        * Under ``torch.autocast("cuda")`` (train.py:269's ``torch.cuda.amp.autocast()``, fp16 by
          default; test_specific_images.py:121's inference): autocast's dtype — fp16 unless the
          caller asked for bf16.  16-bit activations and logits, fp32 master weights, BN
          statistics, accumulation and weight gradients.
        * Otherwise the input's dtype: fp32 (cfg1 / cfg2), bf16 (cfg3's arithmetic), fp16
          (cfg5's fp16 images).
        ``train`` does not change the choice: every dtype has forward and backward kernels."""
        if torch.is_autocast_enabled("cuda"):
            dt = torch.get_autocast_dtype("cuda")
            if dt in (torch.float16, torch.bfloat16):
                return dt
            raise RuntimeError("FastSCNN: unsupported autocast dtype %s" % (dt,))
        if x.dtype in (torch.float32, torch.bfloat16, torch.float16):
            return x.dtype
        raise RuntimeError("FastSCNN: unsupported input dtype %s" % (x.dtype,))

    @staticmethod
    def _input(x):
        """Dense NCHW copy of the input in a dtype conv0 reads (fp32 / bf16 / fp16)."""
        if x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            x = x.float()
        return x.contiguous()

    def _momentum(self):
        m = self.learning_to_downsample.conv.conv[1].momentum
        if m is None:
            raise RuntimeError("FastSCNN: BatchNorm momentum=None (cumulative) is not supported")
        return float(m)

    def _dropout_p(self):
        return float(self.classifier.conv[0].p)

    def _prologue(self, who, x, mode, ar=None, target=None, check=None, dt=None, refuse=None,
                  checks="", scalars=True):
        """What every native forward does before its C call, as a ``_Call`` record.

        ``who``: the entry's name (messages); ``mode``: the plan mode; ``ar``: the arenas
        (default: ``_exec_arena``); ``target``: the label map of the entries that take one, cast
        to dense int64; ``check``: its ``loss.CHECK_TARGETS`` law, ``("ce", ignore_index)`` or
        ``("dice",)``; ``dt``: the arithmetic (default: ``_compute_dtype``); ``scalars``: whether
        the C entry takes seed, dropout p and BN momentum.  ``checks`` names the refusals of the
        entry, which come in this order: ``dim`` and ``cuda`` (the image), ``tensors`` (image and
        target on the device), ``refuse`` (a head's own refusal, a message or None), ``arena``,
        ``shape`` (of the target) and ``size``.  A train-mode batch of one raises ``ValueError``
        like the reference's PPM BatchNorm (SURVEY §0 trap 5).  The dropout seed is one draw
        from the global CPU generator per train-mode forward with p > 0 (``_dropout_seed``
        pins it: oracle parity in the tests)."""
        checks, train = checks.split(), mode == MODE_TRAIN
        if "dim" in checks and (x.dim() != 4 or x.shape[1] != 3):
            raise RuntimeError("FastSCNN: expected input [N, 3, H, W], got %s" % (tuple(x.shape),))
        if "cuda" in checks and not x.is_cuda:
            if who == "forward":
                raise RuntimeError("FastSCNN: the HIP path needs a ROCm device tensor (got %s); "
                                   "move the model and input to 'cuda'" % (x.device,))
            raise RuntimeError("FastSCNN.%s: the HIP path needs a ROCm device tensor" % who)
        if "tensors" in checks and not (x.is_cuda and target.is_cuda):
            raise RuntimeError("FastSCNN.%s: the HIP path needs ROCm device tensors" % who)
        if refuse is not None:
            raise RuntimeError(refuse)
        nat = self.native()
        if ar is None:
            ar = self._exec_arena(x.device)
        if "arena" in checks and ar["P"].device != x.device:
            raise RuntimeError("FastSCNN: input on %s but parameters on %s"
                               % (x.device, ar["P"].device))
        N, _, H, W = x.shape
        if "shape" in checks and tuple(target.shape) != (N, H, W):
            raise RuntimeError("%s: target %s does not match input %s"
                               % (who, tuple(target.shape), tuple(x.shape)))
        if "size" in checks and (H < 32 or W < 32):
            raise RuntimeError("FastSCNN: input %dx%d too small (needs >= 32x32)" % (H, W))
        one = train and N < 2
        if one and target is not None:  # (the loss entries refuse before they look at the dtype)
            raise ValueError(_ONE_SAMPLE)
        if dt is None:
            dt = self._compute_dtype(x, train)
        x = self._input(x)
        if one:
            raise ValueError(_ONE_SAMPLE)
        if target is not None:
            target = target.to(torch.int64).contiguous()
            from . import loss as _loss
            if _loss.CHECK_TARGETS and check[0] == "dice":  # no ignore_index in Dice
                bad = (target < 0) | (target >= self.num_classes)
                if bool(bad.any()):
                    raise IndexError("Target %d is out of bounds." % int(target[bad].flatten()[0]))
            elif _loss.CHECK_TARGETS:
                _loss.check_targets(target, self.num_classes, check[1])
        dev = x.device
        plan, fw, _ = nat.plan(N, H, W, _lib.dtype_code(dt), mode, dev)
        ws = torch.empty(max(fw, 1), dtype=torch.uint8, device=dev)
        p = self._dropout_p() if train else 0.0
        seed = 0
        if train and p > 0:
            fixed = getattr(self, "_dropout_seed", None)
            seed = int(fixed) if fixed is not None else int(torch.randint(0, 2 ** 62, (1,)).item())
        end = (_lib.stream_ptr(dev),)
        if scalars:
            end = (_lib.c_ull(seed), _lib.c_float(p), _lib.c_float(self._momentum())) + end
        return _Call(plan, fw, ws, dt, x, target, N, H, W, dev, p, seed, ar,
                     (plan, _lib.ptr(x), _lib.dtype_code(x.dtype)),
                     (_lib.ptr(ar["P"]), _lib.ptr(ar["R"]), _lib.ptr(ar["NBT"]), _lib.ptr(ws)), end)

    def _epilogue(self, c, train=True, **debug):
        """After the C call of a forward whose prologue gave ``c``; ``debug``: the entry's extra
        ``_debug`` keys."""
        if train:
            self._writeback(c.ar)
            # the running statistics changed: an eval-mode graph recorded before this forward
            # must not backpropagate through them (_FastSCNNFunction.backward checks)
            torch.autograd.graph.increment_version(c.ar["R"])
        if getattr(self, "_keep_ws", False):
            self._debug = dict(plan=c.plan, ws=c.ws, dt=c.dt, **debug)

    def _run_forward(self, x, mode, ar=None, dt=None):
        """One native forward; mode: MODE_EVAL (0), MODE_TRAIN (1), MODE_EVAL_GRAD (2); dt: the
        arithmetic (default: _compute_dtype)."""
        c = self._prologue("forward", x, mode, ar, dt=dt, checks="dim cuda arena size")
        # (autocast: the reference's final F.interpolate returns fp16 logits)
        out = torch.empty((c.N, self.num_classes, c.H, c.W), dtype=c.dt, device=c.dev)
        outs = (out, torch.empty_like(out)) if self.aux else (out,)  # models/fast_scnn.py:42-45
        with torch.cuda.device(c.dev):
            _lib.call("fscnn_forward_aux" if self.aux else "fscnn_forward", *c.src,
                      *[_lib.ptr(o) for o in outs], _lib.dtype_code(c.dt), *c.mem, *c.end)
        self._epilogue(c, train=mode == MODE_TRAIN)
        return outs, c.ws, c.seed, c.dt, c.x

    def predict(self, x, dtype=torch.int64):
        """``torch.argmax(self(x)[0], 1)`` of an eval-mode model (eval.py:43-45, demo.py:43-48)
        without the upsampled logits: the final bilinear upsample and the argmax over classes run
        as one kernel that writes only the labels (int64 like torch.argmax, or uint8)."""
        if self.training:
            raise RuntimeError("predict is the inference path; call model.eval() first")
        if dtype not in (torch.int64, torch.uint8):
            raise RuntimeError("predict: labels are int64 or uint8, not %s" % (dtype,))
        c = self._prologue("predict", x, MODE_EVAL, checks="dim cuda size", scalars=False)
        labels = torch.empty((c.N, c.H, c.W), dtype=dtype, device=c.dev)
        with torch.cuda.device(c.dev):
            _lib.call("fscnn_predict", *c.src, _lib.ptr(labels), 1 if dtype == torch.uint8 else 0,
                      *c.mem, *c.end)
        self._epilogue(c, train=False)
        return labels

    def validate(self, x, target, criterion=None, metric=None, ignore_index=-1):
        """One batch of ``Trainer.validation`` (train.py:370-439): the loss ``criterion`` gives on
        ``self(x)`` as a 0-dim fp32 device tensor, and ``metric.update(argmax(self(x)[0], 1),
        target)`` added into ``metric`` (this package's ``SegmentationMetric``, or None for the
        loss alone).  Requires ``model.eval()``; runs under ``no_grad``, touches no parameter or
        running statistic and reads nothing back to the host.

        Where the criterion has a fused head (``_head_spec``: None = cross entropy with
        ``ignore_index``, the CE and Dice / Focal+Dice criteria of this package or the reference)
        the forward ends in one kernel over the low-resolution logits that forms every upsampled
        logit exactly as ``forward`` stores it and keeps only the loss sums and the counters: no
        full-resolution logits, no labels.  A criterion with ``aux=True`` on an aux model adds
        ``aux_weight`` times the aux output's loss (a second, loss-only pass).  A CE batch without
        a valid pixel gives NaN, like the mean over no element.

        Everything else -- the OHEM criterion, unknown criteria, geometries the head does not
        take, ``FSCNN_VAL_FUSED=0`` -- computes the same two results by the unfused route,
        ``criterion(self(x), target)`` (``self(x)[0]`` for the criteria that take a tensor) and
        ``metric.update``.  ``_last_validate_fused`` records which route ran."""
        if self.training:
            raise RuntimeError("validate is the evaluation step; call model.eval() first")
        if x.dim() != 4 or x.shape[1] != 3:
            raise RuntimeError("FastSCNN: expected input [N, 3, H, W], got %s" % (tuple(x.shape),))
        if not x.is_cuda or not target.is_cuda:
            raise RuntimeError("FastSCNN.validate: the HIP path needs ROCm device tensors")
        N, _, H, W = x.shape
        if tuple(target.shape) != (N, H, W):
            raise RuntimeError("validate: target %s does not match input %s"
                               % (tuple(target.shape), tuple(x.shape)))
        if metric is not None and metric.nclass != self.num_classes:
            raise RuntimeError("validate: metric counts %d classes, the model has %d"
                               % (metric.nclass, self.num_classes))
        with torch.no_grad():
            loss = None
            if os.environ.get("FSCNN_VAL_FUSED", "1") != "0":
                try:
                    spec = _head_spec(criterion, ignore_index)
                except RuntimeError:  # no fused head for this criterion
                    spec = None
                if spec is not None:
                    loss = self._validate_fused(x, target, criterion, spec, metric)
            fused = loss is not None
            if not fused:
                loss = self._validate_unfused(x, target, criterion, metric, ignore_index)
        self._last_validate_fused = fused
        return loss

    def _validate_fused(self, x, target, criterion, spec, metric):
        """The fused route of ``validate``; None when the library does not take the geometry."""
        dice = spec[0] == "dice"
        c = self._prologue("validate", x, MODE_EVAL, None, target, checks="size", check=spec,
                           scalars=False)
        ignore = 0 if dice else spec[1]
        coef = spec[1:] if dice else (1e-6, 1.0, 0.0, 0.5, 2.0)  # smooth, dice_weight, ...
        aux_w = 0.0
        if self.aux and criterion is not None and getattr(criterion, "aux", False):
            aux_w = float(criterion.aux_weight)
        lib = _lib.load()
        hb = int(lib.fscnn_validate_ws_bytes(c.plan))
        if hb < 0:
            _lib.check(hb, "fscnn_validate_ws_bytes")
        head_ws = torch.empty(max(hb, 1), dtype=torch.uint8, device=c.dev)
        loss = torch.empty(1, dtype=torch.float32, device=c.dev)
        counts = metric.device_counts(c.dev) if metric is not None else None
        with torch.cuda.device(c.dev):
            rc = lib.fscnn_validate(*c.src, _lib.ptr(c.target), 1 if dice else 0, int(ignore),
                                    *[_lib.c_float(v) for v in coef], _lib.c_float(aux_w),
                                    _lib.ptr(loss), _lib.ptr(counts), *c.mem, _lib.ptr(head_ws),
                                    *c.end)
        if rc == E_UNSUPPORTED:  # nothing was launched: the geometry check comes first
            return None
        _lib.check(rc, "fscnn_validate")
        self._epilogue(c, train=False)
        return loss.reshape(())

    def _validate_unfused(self, x, target, criterion, metric, ignore_index):
        """The same two results from full-resolution logits (criteria without a fused head)."""
        outs = self._run_forward(x, MODE_EVAL)[0]
        if criterion is None:
            from . import loss as _loss
            loss = _loss.cross_entropy(outs[0], target, ignore_index)
        else:
            names = [c.__name__ for c in type(criterion).__mro__]
            takes_tensor = "FocalDiceLoss" in names or (
                "DiceLoss" in names and "MixDiceLoss" not in names)
            loss = criterion(outs[0] if takes_tensor else outs, target)
        if metric is not None:
            metric.update(torch.argmax(outs[0], 1), target)
        return loss.to(torch.float32).reshape(())

    def debug_buffer(self, name):
        """Tensor view of a named plan buffer of the last forward/backward (set ``_keep_ws``).

        Debug / stage-level parity helper: returns [rows, cols] in the compute dtype."""
        d = self._debug
        off, rows, cols, ld, inb = (_lib.c_ll(), _lib.c_ll(), _lib.c_int(), _lib.c_int(),
                                    _lib.c_int())
        _lib.check(_lib.load().fscnn_plan_buffer(d["plan"], name.encode(), _lib.ctypes.byref(off),
                                                 _lib.ctypes.byref(rows), _lib.ctypes.byref(cols),
                                                 _lib.ctypes.byref(ld), _lib.ctypes.byref(inb)),
                   "fscnn_plan_buffer")
        base = d["bws"] if inb.value else d["ws"]
        dt = d["dt"] if not name.endswith((".scale", ".shift", ".mean", ".invstd")) else torch.float32
        esz = torch.tensor([], dtype=dt).element_size()
        n = (rows.value - 1) * ld.value + cols.value
        flat = base[off.value:off.value + n * esz].view(dt)
        return flat.as_strided((rows.value, cols.value), (ld.value, 1))

    def _main_output_only(self, who, criterion):
        if self.aux:
            raise RuntimeError("%s: the fused loss head covers the main output only; with "
                               "aux=True use forward_loss_aux(x, target, criterion), or "
                               "%s(aux=True)(model(x), target)" % (who, criterion))

    def _run_forward_loss(self, x, target, spec, ar):
        """The forward of the fused CE head (``spec``: ``("ce", ignore_index)``).  The head writes
        ``loss2`` = (mean, count); the backward reads only the count."""
        self._main_output_only("forward_loss", "MixSoftmaxCrossEntropyLoss")
        c = self._prologue("forward_loss", x, MODE_TRAIN, ar, target, checks="tensors shape",
                           check=spec)
        loss2 = torch.empty(2, dtype=torch.float32, device=c.dev)
        with torch.cuda.device(c.dev):
            _lib.call("fscnn_forward_loss", *c.src, _lib.ptr(c.target), int(spec[1]),
                      _lib.ptr(loss2), *c.mem, *c.end)
        self._epilogue(c)
        return loss2, c, _Head("fscnn_backward_loss", (_lib.ptr(loss2),), None, (loss2,))

    def _run_forward_loss_dice(self, x, target, spec, ar):
        """The forward of the fused Dice / Focal+Dice head (``spec``: a Dice ``_head_spec``); its
        coefficient planes (``head_ws``) and sums (``stats``) travel to the backward."""
        self._main_output_only("forward_loss", "MixDiceLoss")
        refuse = None
        if not 2 <= self.num_classes <= 32:
            refuse = ("forward_loss: the fused Dice head takes 2 .. 32 classes; use "
                      "criterion(model(x), target)")
        c = self._prologue("forward_loss", x, MODE_TRAIN, ar, target, refuse=refuse,
                           checks="tensors shape", check=("dice",))
        hb = int(_lib.load().fscnn_dice_head_ws_bytes(c.plan))
        if hb < 0:
            _lib.check(hb, "fscnn_dice_head_ws_bytes")
        head_ws = torch.empty(max(hb, 1), dtype=torch.uint8, device=c.dev)
        stats = torch.empty(4, dtype=torch.float64, device=c.dev)
        loss1 = torch.empty(1, dtype=torch.float32, device=c.dev)
        coef = tuple(_lib.c_float(v) for v in spec[1:])  # smooth, dice_weight, focal_weight, ...
        with torch.cuda.device(c.dev):
            _lib.call("fscnn_forward_loss_dice", *c.src, _lib.ptr(c.target), *coef,
                      _lib.ptr(loss1), _lib.ptr(stats), *c.mem, _lib.ptr(head_ws), *c.end)
        self._epilogue(c)
        return loss1, c, _Head("fscnn_backward_loss_dice", (_lib.ptr(stats),) + coef[:3], head_ws,
                               (stats,))

    def forward_loss(self, x, target, ignore_index=-1, criterion=None):
        """Fused train-step head: ``criterion(self(x)[0], target)`` of train.py:270-271, computed
        at the low-res logit resolution without materialising full-resolution logits.  Same loss
        and gradients as the unfused path (tests/test_gpu_model.py, tests/test_gpu_dice_head.py);
        requires train mode.

        ``criterion=None``: ``nn.CrossEntropyLoss(ignore_index)`` (utils/loss.py:103-124).
        Otherwise the criterion object the training script built, this package's or the
        reference's own (``_head_spec``): ``DiceLoss``, ``MixDiceLoss`` and ``FocalDiceLoss``
        (utils/loss.py:12-100) take the fused Dice head, ``MixSoftmaxCrossEntropyLoss`` the CE
        head with the criterion's ``ignore_index``; the OHEM criterion (its fused head is
        ``forward_loss_ohem``) and anything else raise ``RuntimeError`` (use
        ``criterion(model(x), target)``).

        Dice targets outside ``[0, num_classes)`` are a caller error, as in the reference (its
        focal term raises): with ``loss.CHECK_TARGETS`` they raise ``IndexError``, otherwise they
        count as ``t = 0``.  The Dice head does not form the input image's gradient."""
        if not self.training:
            raise RuntimeError("forward_loss is the training step; call model.train() first")
        if not x.is_cuda:
            raise RuntimeError("FastSCNN.forward_loss: the HIP path needs ROCm device tensors")
        spec = _head_spec(criterion, ignore_index)
        ar = self._exec_arena(x.device)
        return _FastSCNNLossFunction.apply(x, target, "forward_loss", spec, self, ar,
                                           *ar["params"])

    def _ohem_weight(self, weight, device):
        """The criterion's class weights as a device fp32 vector, moved once per (tensor,
        version, device) and kept on the model: later steps do no H2D copy."""
        if weight is None:
            return None
        if weight.numel() != self.num_classes:
            raise RuntimeError("weight tensor should be defined either for all %d classes or no "
                               "classes but got weight tensor of shape: [%d]"
                               % (self.num_classes, weight.numel()))
        if weight.device == device and weight.dtype == torch.float32 and weight.is_contiguous():
            return weight.detach()
        cache = self.__dict__.setdefault("_ohem_wcache", {})
        key = (id(weight), weight._version, str(device))
        hit = cache.get(key)
        if hit is None or hit[0] is not weight:
            cache.clear()
            hit = cache[key] = (weight, weight.detach().to(device=device, dtype=torch.float32)
                                .contiguous())
        return hit[1]

    def _run_forward_loss_ohem(self, x, target, spec, ar):
        """The forward of the fused OHEM head (``spec``: an ``_ohem_spec`` tuple whose weights
        are on the device).  It leaves ``loss2`` and the low-res gradient planes in the CE head's
        format: same backward."""
        _, ignore_index, thresh, min_kept, weight = spec
        c = self._prologue("forward_loss_ohem", x, MODE_TRAIN, ar, target,
                           checks="tensors shape", check=("ce", ignore_index))
        loss2 = torch.empty(2, dtype=torch.float32, device=c.dev)
        prob = torch.empty(c.N * c.H * c.W, dtype=torch.float32, device=c.dev)
        thr = torch.empty(1, dtype=torch.float32, device=c.dev)
        counts = torch.empty(2, dtype=torch.int64, device=c.dev)  # zeroed inside the native run
        work = torch.empty(2056, dtype=torch.int32, device=c.dev)
        lib = _lib.load()
        with torch.cuda.device(c.dev):
            rc = lib.fscnn_forward_loss_ohem(
                *c.src, _lib.ptr(c.target), int(ignore_index), _lib.c_float(thresh),
                int(min_kept), _lib.ptr(weight), _lib.ptr(loss2), _lib.ptr(prob), _lib.ptr(thr),
                _lib.ptr(counts), _lib.ptr(work), *c.mem, *c.end)
        if rc == E_UNSUPPORTED:  # nothing was launched
            raise RuntimeError("forward_loss_ohem: no fused OHEM head for this model (%s); use "
                               "the unfused path, criterion(model(x), target)"
                               % lib.fscnn_last_error().decode(errors="replace"))
        _lib.check(rc, "fscnn_forward_loss_ohem")
        self._epilogue(c, ohem={"prob": prob.view(c.N, c.H, c.W), "thr": thr, "counts": counts})
        return loss2, c, _Head("fscnn_backward_loss", (_lib.ptr(loss2),), None, (loss2,))

    def forward_loss_ohem(self, x, target, criterion):
        """Fused train-step head for the OHEM criterion: ``criterion(self(x), target)`` of
        train.py:189-191 / 270-271 with ``SoftmaxCrossEntropyOHEMLoss`` /
        ``MixSoftmaxCrossEntropyOHEMLoss`` (this package's or the reference's own object,
        ``_ohem_spec``), computed from the low-res logits without materialising full-resolution
        logits or their gradient.  Returns the scalar loss; requires train mode.

        The label probabilities, the threshold rule (``thresh``, ``min_kept``) and the class
        weights all stay on the device: no host synchronisation in forward or backward.  The
        loss covers the main output only (``aux=True`` models raise); targets outside
        ``[0, num_classes)`` count as ignored (``loss.CHECK_TARGETS`` raises instead).
        ``forward_loss(criterion=<OHEM>)`` and ``validate`` keep refusing the criterion: this
        method is the head's one entry."""
        spec = _ohem_spec(criterion)
        if not self.training:
            raise RuntimeError("forward_loss_ohem is the training step; call model.train() first")
        if not x.is_cuda:
            raise RuntimeError("FastSCNN.forward_loss_ohem: the HIP path needs ROCm device tensors")
        self._main_output_only("forward_loss_ohem", "MixSoftmaxCrossEntropyOHEMLoss")
        spec = spec[:4] + (self._ohem_weight(spec[4], x.device),)
        ar = self._exec_arena(x.device)
        return _FastSCNNLossFunction.apply(x, target, "forward_loss_ohem", spec, self, ar,
                                           *ar["params"])

    def _run_forward_loss_aux(self, x, target, spec, ar):
        """The forward of the fused aux loss heads (``spec``: an ``_aux_head_spec`` tuple whose
        OHEM weights are on the device).  Its loss is the device ``loss3`` = (total, main, aux);
        the backward takes the ``fscnn_aux_head`` struct and the ``head_ws`` buffer again."""
        kind, aux_weight = spec[0], spec[1]
        head = _lib.AuxHead()
        head.aux_weight = aux_weight
        head.ignore_index = -1
        if kind == "ce":
            head.head, head.ignore_index = 0, spec[2]
        elif kind == "dice":  # MixDiceLoss: plain Dice on each output
            head.head, head.smooth, head.dice_weight, head.focal_weight = 1, spec[2], 1.0, 0.0
            head.alpha, head.gamma = 0.5, 2.0
        else:
            _, _, ign, thresh, min_kept, weight = spec
            head.head, head.ignore_index, head.thresh, head.min_kept = 2, ign, thresh, min_kept
            head.class_weight = weight.data_ptr() if weight is not None else None
        refuse = None
        if not (2 if kind == "dice" else 1) <= self.num_classes <= 32:
            refuse = ("forward_loss_aux: the fused heads take 1 .. 32 classes (Dice: 2 .. 32); "
                      "use the unfused path, criterion(model(x), target)")
        c = self._prologue("forward_loss_aux", x, MODE_TRAIN, ar, target, refuse=refuse,
                           checks="tensors shape",
                           check=("dice",) if kind == "dice" else ("ce", int(head.ignore_index)))
        lib = _lib.load()
        hb = int(lib.fscnn_aux_head_ws_bytes(c.plan, head.head))
        if hb < 0:
            _lib.check(hb, "fscnn_aux_head_ws_bytes")
        head_ws = torch.empty(hb, dtype=torch.uint8, device=c.dev)
        loss3 = torch.empty(3, dtype=torch.float32, device=c.dev)
        with torch.cuda.device(c.dev):
            rc = lib.fscnn_forward_loss_aux(*c.src, _lib.ptr(c.target), _lib.ctypes.byref(head),
                                            _lib.ptr(loss3), *c.mem, _lib.ptr(head_ws), *c.end)
        if rc == E_UNSUPPORTED:  # nothing was launched
            raise RuntimeError("forward_loss_aux: no fused aux loss heads for this model (%s); "
                               "use the unfused path, criterion(model(x), target)"
                               % lib.fscnn_last_error().decode(errors="replace"))
        _lib.check(rc, "fscnn_forward_loss_aux")
        debug = {"head_ws": head_ws}
        if kind == "ohem" and getattr(self, "_keep_ws", False):
            # each head's plane, threshold and counters, as views of head_ws
            def view(field, which, n, tdt):
                off = int(lib.fscnn_aux_head_ws_offset(c.plan, 2, field, which))
                if off < 0:
                    _lib.check(off, "fscnn_aux_head_ws_offset")
                nb = n * torch.tensor([], dtype=tdt).element_size()
                return head_ws[off:off + nb].view(tdt)
            debug["ohem"] = [{"prob": view(b"prob", i, c.N * c.H * c.W, torch.float32)
                              .view(c.N, c.H, c.W),
                              "thr": view(b"thr", i, 1, torch.float32),
                              "counts": view(b"counts", i, 2, torch.int64),
                              # (weighted mean, sum of the kept pixels' weights)
                              "pair": view(b"pair", i, 2, torch.float32)}
                             for i in range(2)]
        self._epilogue(c, **debug)
        # (spec: the OHEM class weights the struct points to stay alive until the backward)
        return loss3, c, _Head("fscnn_backward_loss_aux", (_lib.ctypes.byref(head),), head_ws,
                               (head, spec))

    def forward_loss_aux(self, x, target, criterion):
        """Fused train-step heads of an ``aux=True`` model: ``criterion(self(x), target)`` =
        ``L(out) + aux_weight * L(aux_out)`` of train.py:270-271 run with ``--aux``, both terms
        computed from the low-res logits: no full-resolution logits or gradient of either output
        is written and nothing is read back by the host.  Returns the scalar loss; requires train
        mode, an aux model and a criterion built with ``aux=True``.

        ``criterion`` (this package's or the reference's own object, ``_aux_head_spec``):
        ``MixSoftmaxCrossEntropyLoss`` (CE head, the criterion's ``ignore_index``),
        ``MixDiceLoss`` (Dice head; it does not form the input image's gradient) or
        ``MixSoftmaxCrossEntropyOHEMLoss`` (OHEM head: each output has its own probability plane,
        threshold and kept set, as utils/loss.py:191-198 calls the single-output law once per
        prediction).  Anything else raises ``RuntimeError``: use ``criterion(model(x), target)``.

        ``self._last_loss_terms`` is then the device fp32 tensor ``[L(out), L(aux_out)]``, the
        unweighted terms (logging)."""
        spec = _aux_head_spec(criterion)
        if not self.training:
            raise RuntimeError("forward_loss_aux is the training step; call model.train() first")
        if not self.aux:
            raise RuntimeError("forward_loss_aux: this model has no aux head (aux=False); use "
                               "forward_loss / forward_loss_ohem, or the unfused path, "
                               "criterion(model(x), target)")
        if not x.is_cuda:
            raise RuntimeError("FastSCNN.forward_loss_aux: the HIP path needs ROCm device tensors")
        if spec[0] == "ohem":
            spec = spec[:5] + (self._ohem_weight(spec[5], x.device),)
        ar = self._exec_arena(x.device)
        return _FastSCNNLossFunction.apply(x, target, "forward_loss_aux", spec, self, ar,
                                           *ar["params"])

    def _run_backward(self, gout, x, ws, seed, dt, ar, gloss=None, gaux=None, mode=MODE_TRAIN,
                      dx=None, head=None):
        """The staged native backward of a MODE_TRAIN / MODE_EVAL_GRAD forward whose workspace
        is ``ws``; parameter gradients are views of one flat arena G, and ``dx`` (dense NCHW,
        the dtype of ``x``) receives the input gradient when given.  ``head``: the ``_Head`` of a
        fused loss forward (then ``gloss`` is d(loss)), or None for the gradients of the logits."""
        nat = self.native()
        N, _, H, W = x.shape
        plan, _, bw = nat.plan(N, H, W, _lib.dtype_code(dt), mode, x.device)
        if gout is not None:
            gout = gout.to(dt).contiguous()
        if self.aux and head is None:
            gaux = torch.zeros_like(gout) if gaux is None else gaux.to(dt).contiguous()
        # every element of every parameter's gradient is written by the backward (a reduction,
        # a BN finish or the PPM kernel; tests/test_gpu_model.py fills G with NaN to check), so
        # the arena is not zeroed; only the 64-B alignment gaps between tensors are left as is
        G = torch.empty(nat.p_total, dtype=torch.float32, device=x.device)
        if getattr(self, "_debug_fill_grads", None) is not None:
            G.fill_(self._debug_fill_grads)
        bws = torch.empty(max(bw, 1), dtype=torch.uint8, device=x.device)
        p = self._dropout_p() if mode == MODE_TRAIN else 0.0
        if getattr(self, "_keep_ws", False):
            self._debug["bws"] = bws
        hook = self.grad_stage_hook
        # without a hook, one native call for the four stages: their weight-gradient reductions
        # run once at its end, so the main stream does not wait for the side stream between stages
        for s0, s1 in [(0, 3)] if hook is None else [(s, s) for s in range(4)]:
            with torch.cuda.device(x.device):
                self._backward_stage(plan, (s0, s1), gout, gaux, gloss, head, x, ar, G, ws, bws,
                                     seed, p, dx)
            if hook is not None:
                b, e = nat.stage_ranges[s0]
                hook(s0, G, b, e)
        return [G[off:off + numel].view(prm.shape)
                for prm, (_, off, numel) in zip(ar["params"], nat.params)]

    def _backward_stage(self, plan, stages, gout, gaux, gloss, head, x, ar, G, ws, bws, seed, p,
                        dx=None):
        """Backward stages s0 .. s1 (0: head ... 3: LearningToDownsample) by the C entry the
        forward's head names; every entry ends in the same arguments."""
        xa = (_lib.ptr(x), _lib.dtype_code(x.dtype))
        dxa = (_lib.ptr(dx), _lib.dtype_code(dx.dtype if dx is not None else x.dtype))
        mem = (_lib.ptr(ar["P"]), _lib.ptr(G), _lib.ptr(ws), _lib.ptr(bws))
        end = (_lib.c_ull(seed), _lib.c_float(p)) + tuple(stages) + (_lib.stream_ptr(x.device),)
        if head is None:  # from the gradients of the logits
            if dx is not None:  # the general entry point: also writes the input gradient (stage 3)
                _lib.call("fscnn_backward_dx", plan, _lib.ptr(gout), _lib.ptr(gaux), None, None,
                          *xa, *dxa, *mem, *end)
            elif self.aux:
                _lib.call("fscnn_backward_aux", plan, _lib.ptr(gout), _lib.ptr(gaux), *xa, *mem,
                          *end)
            else:
                _lib.call("fscnn_backward", plan, _lib.ptr(gout), *xa, *mem, *end)
        elif head.entry == "fscnn_backward_loss" and dx is not None:  # (the general entry again)
            _lib.call("fscnn_backward_dx", plan, None, None, _lib.ptr(gloss), *head.lead, *xa,
                      *dxa, *mem, *end)
        else:
            takes_dx = head.entry == "fscnn_backward_loss_aux"
            hws = () if head.head_ws is None else (_lib.ptr(head.head_ws),)
            _lib.call(head.entry, plan, _lib.ptr(gloss), *head.lead, *xa,
                      *(dxa if takes_dx else ()), *mem, *hws, *end)

    def _needs_graph(self, x):
        """Whether this call is differentiable, as the reference's would be: train mode with
        grad enabled (the training step), or any mode when autograd would record the call (an
        input or a parameter requires grad).  eval() under torch.no_grad() is the inference path."""
        if not torch.is_grad_enabled():
            return False
        if self.training or x.requires_grad:
            return True
        return any(p.requires_grad for p in self.parameters())

    def forward(self, x):
        mode = MODE_TRAIN if self.training else MODE_EVAL
        if self._needs_graph(x):
            if not x.is_cuda:
                self._run_forward(x, mode)  # raises the device error
            ar = self._exec_arena(x.device)
            out = _FastSCNNFunction.apply(x, self, ar, *ar["params"])
            return tuple(out) if self.aux else (out,)
        return self._run_forward(x, mode)[0]


def get_fast_scnn(dataset="citys", pretrained=False, root="./weights", map_cpu=False, **kwargs):
    """models/fast_scnn.py:240-256 without the torchvision-importing data_loader lookup."""
    acronyms = {"pascal_voc": "voc", "pascal_aug": "voc", "ade20k": "ade", "coco": "coco",
                "citys": "citys", "tusimple": "tusimple"}
    if dataset not in NUM_CLASS:
        raise KeyError(dataset)
    model = FastSCNN(NUM_CLASS[dataset], **kwargs)
    if pretrained:
        path = os.path.join(root, "fast_scnn_%s.pth" % acronyms[dataset])
        sd = torch.load(path, map_location="cpu" if map_cpu else None, weights_only=True)
        model.load_state_dict(strip_module_prefix(sd))
    return model


def strip_module_prefix(state_dict):
    """Checkpoints saved from the DataParallel / DistributedFastSCNN wrapper (train.py:449 saves
    ``model.state_dict()`` with a ``module.`` prefix) load into a bare FastSCNN (SURVEY §8(f) row
    4); other keys are left as they are."""
    if all(k.startswith("module.") for k in state_dict):
        return type(state_dict)((k[len("module."):], v) for k, v in state_dict.items())
    return state_dict
