"""Fused multi-tensor optimizers on the HIP path: FusedSGD (torch.optim.SGD semantics,
train.py:195-198) and FusedAdamW (torch.optim.AdamW under GradScaler,
train_bdd100k.py:183-188, 258-266).

FusedSGD:

When every parameter of a group is a view of one flat arena and every ``.grad`` a view of one
flat gradient buffer at the same offsets (what ``FastSCNN`` produces), the whole step is ONE
kernel over the arena (one per contiguous run when frozen parameters or another group's tensors
sit inside the group's span: those are never touched).  Otherwise it falls back to one launch
per tensor (still the HIP kernel).
State keeps torch's ``momentum_buffer`` key so ``state_dict()`` interoperates.

FusedAdamW:

Same fast-path condition, but one launch (``fscnn_adamw_segments``) covers every run of up to
eight parameter groups: a device-resident segment table names each run's range and group, and
the groups' hyperparameters travel by value in the kernel arguments, so a changing ``lr`` costs
nothing.  The step count lives on the device and ``GradScaler``'s ``grad_scale`` / ``found_inf``
tensors are read there: a skipped step changes nothing and no step reads anything back to the
host.  State keeps torch's keys (``step``, ``exp_avg``, ``exp_avg_sq``, ``max_exp_avg_sq``).
"""
import ctypes

import torch

from . import _lib


def _flat_base(tensors):
    """(base tensor storage pointer, [offsets]) if all tensors are contiguous views of one
    storage, else None."""
    st = tensors[0].untyped_storage().data_ptr()
    offs = []
    for t in tensors:
        if not t.is_contiguous() or t.untyped_storage().data_ptr() != st:
            return None
        offs.append(t.storage_offset())
    return st, offs


def _runs(offs, numels, align=16):
    """Split tensors (sorted by offset) into maximal runs that tile a flat span with nothing but
    alignment padding between neighbours: [(lo, hi)] in elements.  A parameter of another group,
    or one without a gradient (frozen), that lies between two tensors breaks the run, so the
    fused launch never touches it (torch.optim.SGD skips grad-None parameters)."""
    order = sorted(range(len(offs)), key=lambda i: offs[i])
    runs = []
    lo = hi = None
    for i in order:
        o, n = offs[i], numels[i]
        if lo is not None and o == (hi + align - 1) // align * align:
            hi = o + n
            continue
        if lo is not None:
            runs.append((lo, hi))
        lo, hi = o, o + n
    if lo is not None:
        runs.append((lo, hi))
    return runs


class FusedSGD(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-2, momentum=0.0, dampening=0.0, weight_decay=0.0,
                 nesterov=False, grad_scale=1.0):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening,
                        weight_decay=weight_decay, nesterov=nesterov, grad_scale=grad_scale)
        super().__init__(params, defaults)
        self._aux = {}  # group index -> {"flat": momentum arena, "plan": cached fused plan}

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._aux = {}  # momentum buffers were replaced: rebuild the flat view on the next step

    def _launch(self, p, g, buf, n, group, first):
        _lib.call("fscnn_sgd", _lib.c_vp(p), _lib.c_vp(g), _lib.c_vp(buf), n,
                  _lib.c_float(group["lr"]), _lib.c_float(group["momentum"]),
                  _lib.c_float(group["dampening"]), _lib.c_float(group["weight_decay"]),
                  int(group["nesterov"]), int(first), _lib.c_float(group["grad_scale"]),
                  _lib.stream_ptr())

    def _launch_runs(self, pbase, gbase, flat, lo, runs, group, first):
        for a, b in runs:
            self._launch(pbase + a * 4, gbase + a * 4, flat.data_ptr() + (a - lo) * 4, b - a,
                         group, first)

    def _fast_step(self, gi, group):
        """Steady-state path: same parameter views as the cached fused plan and every grad a
        view of one base at the parameters' offsets (what FastSCNN's backward returns) -> one
        launch per contiguous run without re-deriving the plan.  False when it does not apply."""
        aux = self._aux.get(gi)
        plan = aux.get("plan") if aux else None
        params = group["params"]
        if plan is None or len(params) != plan["n"]:
            return False
        if params[0].data_ptr() != plan["p0"] or params[-1].data_ptr() != plan["p1"]:
            return False
        g0 = params[0].grad
        if g0 is None or g0.dtype != torch.float32:
            return False
        base = g0._base
        if base is None:
            return False
        offs = plan["offs"]
        for p, o in zip(params, offs):
            g = p.grad
            if g is None or g._base is not base or g.storage_offset() != o:
                return False
        gptr = base.untyped_storage().data_ptr()
        self._launch_runs(plan["pbase"], gptr, aux["flat"], plan["lo"], plan["runs"], group,
                          False)
        return True

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            if self._fast_step(gi, group):
                continue
            aux = self._aux.setdefault(gi, {})
            params = [p for p in group["params"] if p.grad is not None]
            if not params:
                continue
            for p in params:
                if not p.is_cuda or p.dtype != torch.float32:
                    raise RuntimeError("FusedSGD needs fp32 ROCm parameters")
            grads = [p.grad for p in params]
            first = any("momentum_buffer" not in self.state[p] for p in params)
            pb, gb = _flat_base([p.data for p in params]), _flat_base(grads)
            fused = (pb is not None and gb is not None and pb[1] == gb[1] and
                     all(p.grad.dtype == torch.float32 for p in params) and
                     not any(("momentum_buffer" in self.state[p]) != (not first) for p in params))
            if fused:
                runs = _runs(pb[1], [p.numel() for p in params])
                lo, hi = runs[0][0], runs[-1][1]
                flat = aux.get("flat")
                if flat is None or flat.numel() != hi - lo or first:
                    flat = torch.zeros(hi - lo, dtype=torch.float32, device=params[0].device)
                    aux["flat"] = flat
                    for o, p in zip(pb[1], params):
                        view = flat[o - lo:o - lo + p.numel()].view_as(p)
                        old = self.state[p].get("momentum_buffer")
                        if old is not None and not first:  # e.g. after load_state_dict
                            view.copy_(old)
                        self.state[p]["momentum_buffer"] = view
                # pointer base of element 0 of the storage: offsets are in elements
                self._launch_runs(pb[0], gb[0], flat, lo, runs, group, first)
                if len(params) == len(group["params"]):
                    aux["plan"] = {"n": len(params), "p0": params[0].data_ptr(),
                                   "p1": params[-1].data_ptr(), "offs": list(gb[1]),
                                   "pbase": pb[0], "lo": lo, "runs": runs}
                else:
                    aux.pop("plan", None)
            else:
                for p in params:
                    st = self.state[p]
                    f = "momentum_buffer" not in st
                    if f:
                        st["momentum_buffer"] = torch.zeros_like(p)
                    g = p.grad.float().contiguous()
                    self._launch(p.data_ptr(), g.data_ptr(), st["momentum_buffer"].data_ptr(),
                                 p.numel(), group, f)
        return loss


ADAMW_CHUNK = 2048      # FSCNN_ADAMW_CHUNK: elements per workgroup of fscnn_adamw_segments
ADAMW_MAX_GROUPS = 8    # FSCNN_ADAMW_MAX_GROUPS: groups per launch


class _AdamwSeg(ctypes.Structure):  # fscnn_adamw_seg
    _fields_ = [("begin", ctypes.c_longlong), ("end", ctypes.c_longlong),
                ("group", ctypes.c_int), ("chunk0", ctypes.c_int)]


class _AdamwGroup(ctypes.Structure):  # fscnn_adamw_group
    _fields_ = [("lr", ctypes.c_double), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double),
                ("eps", ctypes.c_double), ("weight_decay", ctypes.c_double),
                ("amsgrad", ctypes.c_int), ("maximize", ctypes.c_int),
                ("step_slot", ctypes.c_int)]


def _segments(offs, numels, groups, align=16, chunk=ADAMW_CHUNK):
    """The segment table of one fscnn_adamw_segments launch, from the tensors' element offsets,
    sizes and group indices (in any order): ([(begin, end, group, chunk0)], [segment of each
    chunk]).  Neighbours of one group with nothing but alignment padding between them merge into
    one segment (as in ``_runs``); a tensor of another group, or one that is not listed (frozen),
    ends it.  chunk0 is the segment's first ``chunk``-element chunk, one workgroup each."""
    order = sorted(range(len(offs)), key=lambda i: offs[i])
    spans = []
    for i in order:
        o, n, g = offs[i], numels[i], groups[i]
        if spans and spans[-1][2] == g and o == (spans[-1][1] + align - 1) // align * align:
            spans[-1][1] = o + n
        else:
            spans.append([o, o + n, g])
    segs, chunk_seg = [], []
    for s, (lo, hi, g) in enumerate(spans):
        segs.append((lo, hi, g, len(chunk_seg)))
        chunk_seg += [s] * ((hi - lo + chunk - 1) // chunk)
    return segs, chunk_seg


class FusedAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW (train_bdd100k.py:183-188) on the HIP kernels; drop-in under
    ``torch.amp.GradScaler`` (``scaler.step(opt)``, train_bdd100k.py:258-266)."""

    _step_supports_amp_scaling = True  # GradScaler hands over grad_scale / found_inf tensors

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 amsgrad=False, *, maximize=False):
        if isinstance(lr, torch.Tensor):
            raise ValueError("FusedAdamW does not take a tensor lr")
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
        # the last five are torch.optim.AdamW's own group keys, fixed at what this class does, so
        # that a state_dict() moves between the two classes in both directions
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad,
                        maximize=maximize, foreach=None, capturable=False, differentiable=False,
                        fused=None, decoupled_weight_decay=True)
        super().__init__(params, defaults)
        self._plan = None

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._plan = None  # state tensors were replaced: rebuild the arenas on the next step

    def state_dict(self):
        """torch's layout: ``step`` is a CPU fp32 scalar per parameter, as torch.optim.AdamW
        keeps it (here the parameters of a group share one device scalar)."""
        sd = super().state_dict()
        host = {}
        state = {}
        for k, st in sd["state"].items():
            st = dict(st)
            step = st.get("step")
            if torch.is_tensor(step):
                if id(step) not in host:
                    host[id(step)] = step.detach().to("cpu", torch.float32).reshape(())
                st["step"] = host[id(step)].clone()
            state[k] = st
        sd["state"] = state
        return sd

    # ---- plan: which parameters go through the segment launch, which one by one -------------
    def _build(self):
        groups = self.param_groups
        plan = {"n": [len(g["params"]) for g in groups],
                "ams": [bool(g["amsgrad"]) for g in groups],
                "absent": [p for g in groups for p in g["params"] if p.grad is None],
                "fused": None, "slow": []}
        active = [[p for p in g["params"] if p.grad is not None] for g in groups]
        for ps in active:
            for p in ps:
                if not p.is_cuda or p.dtype != torch.float32:
                    raise RuntimeError("FusedAdamW needs fp32 ROCm parameters")
                if p.grad.is_sparse or not p.is_contiguous():
                    raise RuntimeError("FusedAdamW needs dense contiguous parameters")
        # a group whose parameters have all taken the same number of steps can share one step
        start = {}  # group index -> the common step (float, or the shared device scalar)
        own = {}    # parameter -> its own step (float), for the groups that cannot
        for gi, ps in enumerate(active):
            steps = [self.state[p].get("step") for p in ps]
            if not ps:
                continue
            if all(s is None for s in steps):
                start[gi] = 0.0
            elif torch.is_tensor(steps[0]) and steps[0].is_cuda and all(s is steps[0]
                                                                        for s in steps):
                start[gi] = steps[0]
            else:  # after load_state_dict, or a parameter that joined later: read them once
                vals = [0.0 if s is None else float(s) for s in steps]
                if all(v == vals[0] for v in vals):
                    start[gi] = vals[0]
                else:
                    own.update(zip(ps, vals))
        cand = [(gi, p) for gi, ps in enumerate(active) if gi in start for p in ps]
        pb = gb = None
        if cand and all(p.grad.dtype == torch.float32 for _, p in cand):
            pb = _flat_base([p.data for _, p in cand])
            gb = _flat_base([p.grad for _, p in cand])
        fusable = (pb is not None and gb is not None and pb[1] == gb[1] and pb[0] % 16 == 0 and
                   all(o % 16 == 0 for o in pb[1]))
        for gi, ps in enumerate(active):
            if fusable and gi in start:
                continue
            for p in ps:  # one launch per tensor, each with its own step
                s = own[p] if p in own else start[gi]
                dev = p.device
                st = self.state[p]
                st["step"] = (s.clone() if torch.is_tensor(s) else
                              torch.full((), s, dtype=torch.float32, device=dev))
                keys = ["exp_avg", "exp_avg_sq"] + (["max_exp_avg_sq"] if groups[gi]["amsgrad"]
                                                    else [])
                for k in keys:
                    old = st.get(k)
                    if old is None:
                        st[k] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    elif not old.is_contiguous():
                        st[k] = old.contiguous()
                plan["slow"].append((gi, p))
        if not fusable:
            return plan
        dev = cand[0][1].device
        offs = pb[1]
        lo = min(offs)
        hi = max(o + p.numel() for o, (_, p) in zip(offs, cand))
        keys = ["exp_avg", "exp_avg_sq"] + (["max_exp_avg_sq"] if any(
            groups[gi]["amsgrad"] for gi in start) else [])
        flat = {k: torch.zeros(hi - lo, dtype=torch.float32, device=dev) for k in keys}
        steps = torch.zeros(len(groups), dtype=torch.float32, device=dev)
        slot = {}
        for gi, s in start.items():
            if torch.is_tensor(s):
                steps[gi].copy_(s)
            else:
                steps[gi].fill_(s)
            slot[gi] = steps[gi]
        for o, (gi, p) in zip(offs, cand):
            st = self.state[p]
            for k in keys:
                if k == "max_exp_avg_sq" and not groups[gi]["amsgrad"]:
                    continue
                view = flat[k][o - lo:o - lo + p.numel()].view_as(p)
                old = st.get(k)
                if old is not None:  # after load_state_dict, or a layout change
                    view.copy_(old)
                st[k] = view
            st["step"] = slot[gi]
        launches = []
        gis = sorted(start)
        for k in range(0, len(gis), ADAMW_MAX_GROUPS):
            batch = gis[k:k + ADAMW_MAX_GROUPS]
            local = {gi: j for j, gi in enumerate(batch)}
            sel = [(o, p.numel(), local[gi]) for o, (gi, p) in zip(offs, cand) if gi in local]
            segs, chunk_seg = _segments([s[0] for s in sel], [s[1] for s in sel],
                                        [s[2] for s in sel])
            hsegs = (_AdamwSeg * len(segs))(*segs)
            launches.append({
                "groups": batch, "cgroups": (_AdamwGroup * len(batch))(),
                "hsegs": hsegs, "nseg": len(segs), "nchunks": len(chunk_seg),
                "dsegs": torch.frombuffer(bytearray(hsegs), dtype=torch.uint8).to(dev),
                "dchunk": torch.tensor(chunk_seg, dtype=torch.int32, device=dev)})
        plan["fused"] = {
            "params": [p for _, p in cand], "offs": list(offs),
            "p0": cand[0][1].data_ptr(), "p1": cand[-1][1].data_ptr(), "pbase": pb[0],
            # arena pointers of storage element 0, so that one offset serves p, g and the state
            "state": [flat[k].data_ptr() - lo * 4 for k in ("exp_avg", "exp_avg_sq")] +
                     [flat["max_exp_avg_sq"].data_ptr() - lo * 4
                      if "max_exp_avg_sq" in flat else None],
            "flat": flat, "steps": steps, "launches": launches}
        return plan

    def _grad_base(self, plan):
        """Pointer of element 0 of the gradients' storage if the cached plan still describes the
        parameters and gradients (what FastSCNN's backward returns every step: views of one new
        flat buffer at the parameters' offsets); None: rebuild.  0 when nothing is fused."""
        groups = self.param_groups
        if len(groups) != len(plan["n"]):
            return None
        for g, n, ams in zip(groups, plan["n"], plan["ams"]):
            if len(g["params"]) != n or bool(g["amsgrad"]) != ams:
                return None
        for p in plan["absent"]:
            if p.grad is not None:
                return None
        for _, p in plan["slow"]:
            if p.grad is None:
                return None
        f = plan["fused"]
        if f is None:
            return 0
        ps = f["params"]
        if ps[0].data_ptr() != f["p0"] or ps[-1].data_ptr() != f["p1"]:
            return None
        g0 = ps[0].grad
        if g0 is None:
            return None
        # every gradient at its parameter's offset of a storage that starts at one address: one
        # storage (a view's _base is not a stable object to compare, addresses are)
        gptr = g0.data_ptr() - 4 * f["offs"][0]
        f32 = torch.float32
        for p, o in zip(ps, f["offs"]):
            g = p.grad
            if (g is None or g.dtype is not f32 or g.storage_offset() != o or
                    g.data_ptr() != gptr + 4 * o or not g.is_contiguous()):
                return None
        return gptr if gptr % 16 == 0 else None

    def _run(self, plan, gptr):
        if plan["fused"] is None and not plan["slow"]:
            return  # no parameter has a gradient
        groups = self.param_groups
        scale = _lib.ptr(getattr(self, "grad_scale", None))
        inf = _lib.ptr(getattr(self, "found_inf", None))
        stream = _lib.stream_ptr()
        f = plan["fused"]
        if f is not None:
            m, v, vmax = f["state"]
            steps = f["steps"]
            for L in f["launches"]:
                for c, gi in zip(L["cgroups"], L["groups"]):
                    g = groups[gi]
                    c.lr, (c.beta1, c.beta2) = float(g["lr"]), g["betas"]  # lr: any scalar type
                    c.eps, c.weight_decay = g["eps"], g["weight_decay"]
                    c.amsgrad, c.maximize, c.step_slot = g["amsgrad"], g["maximize"], gi
                _lib.call("fscnn_adamw_segments", f["pbase"], gptr, m, v, vmax,
                          _lib.ptr(L["dsegs"]), L["hsegs"], L["nseg"], _lib.ptr(L["dchunk"]),
                          L["nchunks"], L["cgroups"], len(L["groups"]), _lib.ptr(steps),
                          steps.numel(), int(L is f["launches"][-1]), scale, inf, stream)
        for gi, p in plan["slow"]:
            g = groups[gi]
            st = self.state[p]
            grad = p.grad
            if grad.dtype != torch.float32 or not grad.is_contiguous():
                grad = grad.float().contiguous()
            _lib.call("fscnn_adamw", _lib.ptr(p), _lib.ptr(grad), _lib.ptr(st["exp_avg"]),
                      _lib.ptr(st["exp_avg_sq"]),
                      _lib.ptr(st["max_exp_avg_sq"] if g["amsgrad"] else None), p.numel(),
                      float(g["lr"]), g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"],
                      int(g["amsgrad"]), int(g["maximize"]), _lib.ptr(st["step"]), 1, scale, inf,
                      stream)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for name in ("grad_scale", "found_inf"):
            t = getattr(self, name, None)
            if t is not None and (not t.is_cuda or t.dtype != torch.float32 or t.numel() != 1):
                raise RuntimeError("FusedAdamW: %s must be one fp32 element on the GPU" % name)
        plan = self._plan
        gptr = None if plan is None else self._grad_base(plan)
        if gptr is None:
            plan = self._plan = self._build()
            gptr = self._grad_base(plan)
            if gptr is None:
                raise RuntimeError("FusedAdamW: the parameter layout changed during step()")
        self._run(plan, gptr)
        return loss
