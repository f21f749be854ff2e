"""CPU-side checks of FusedAdamW: the two C-ABI entry points are declared, exported and bound with
one ctypes argument per declared parameter; the segment-table builder on hand-written layouts;
the constructor's validation and the GradScaler protocol attributes.  No kernel runs here."""
import inspect
import os
import re
import subprocess

import pytest
import torch

from fast_scnn_pytorch_amd import _lib
from fast_scnn_pytorch_amd.optim import ADAMW_CHUNK, FusedAdamW, _segments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fscnn_adamw", "fscnn_adamw_segments"]


def _declared_params(name):
    src = open(os.path.join(ROOT, "include", "fastscnn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, "%s is not declared in include/fastscnn.h" % name
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", NAMES)
def test_entry_point_is_declared_exported_and_bound(name):
    params = _declared_params(name)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    assert re.search(r"\bT %s$" % name, out, flags=re.M), name
    res, args = _lib.SIGNATURES[name]
    assert res is _lib.c_int
    assert len(args) == len(params), (len(args), params)
    for a, decl in zip(args, params):
        if "*" in decl:
            assert a is _lib.c_vp, decl
        elif decl.startswith("double"):
            assert a is _lib.c_double, decl
        elif decl.startswith("long long"):
            assert a is _lib.c_ll, decl
        else:
            assert decl.startswith("int") and a is _lib.c_int, decl
    assert hasattr(_lib.load(), name)


def test_header_index_names_both_entry_points():
    head = open(os.path.join(ROOT, "include", "fastscnn.h")).read().split("#ifndef FASTSCNN_H")[0]
    assert "fscnn_adamw / fscnn_adamw_segments" in head


def test_header_constants_match_the_python_side():
    from fast_scnn_pytorch_amd import optim
    src = open(os.path.join(ROOT, "include", "fastscnn.h")).read()
    assert int(re.search(r"#define FSCNN_ADAMW_CHUNK (\d+)", src).group(1)) == optim.ADAMW_CHUNK
    assert (int(re.search(r"#define FSCNN_ADAMW_MAX_GROUPS (\d+)", src).group(1)) ==
            optim.ADAMW_MAX_GROUPS)
    import ctypes
    assert ctypes.sizeof(optim._AdamwSeg) == 24 and ctypes.sizeof(optim._AdamwGroup) == 56


def _span_args(**kw):
    """fscnn_adamw arguments that pass every host check (the pointers are never dereferenced on
    the host; each test below breaks one so that the call returns before any launch)."""
    a = dict(p=0x1000, g=0x2000, m=0x3000, v=0x4000, vmax=0x5000, n=8, amsgrad=1, step=0x6000)
    a.update(kw)
    return (a["p"], a["g"], a["m"], a["v"], a["vmax"], a["n"], 1e-3, 0.9, 0.999, 1e-8, 1e-2,
            a["amsgrad"], 0, a["step"], 1, None, None, None)


@pytest.mark.parametrize("kw", [{"n": -1}, {"m": None}, {"v": None}, {"step": None},
                                {"vmax": None}, {"p": None}, {"g": None}])
def test_span_entry_point_rejects_bad_arguments(kw):
    lib = _lib.load()
    assert lib.fscnn_adamw(*_span_args(**kw)) == -1
    assert b"adamw" in lib.fscnn_last_error()
    with pytest.raises(RuntimeError):
        _lib.call("fscnn_adamw", *_span_args(**kw))


def _segment_args(segs=((0, 16, 0, 0), (16, 5000, 1, 1)), nchunks=4, ngroups=2, slots=(0, 1),
                  nslots=2, amsgrad=0, **kw):
    from fast_scnn_pytorch_amd.optim import _AdamwGroup, _AdamwSeg
    hsegs = (_AdamwSeg * len(segs))(*segs)
    groups = (_AdamwGroup * max(ngroups, 1))()
    for c, s in zip(groups, slots):
        c.lr, c.beta1, c.beta2, c.eps, c.weight_decay = 1e-3, 0.9, 0.999, 1e-8, 1e-2
        c.amsgrad, c.step_slot = amsgrad, s
    a = dict(p=0x1000, g=0x2000, m=0x3000, v=0x4000, vmax=None, segs=0x5000, chunk=0x6000,
             steps=0x7000)
    a.update(kw)
    return (a["p"], a["g"], a["m"], a["v"], a["vmax"], a["segs"], hsegs, len(segs), a["chunk"],
            nchunks, groups, ngroups, a["steps"], nslots, 1, None, None, None)


@pytest.mark.parametrize("kw", [
    {"ngroups": 9, "slots": tuple(range(9)), "nslots": 9},  # more groups than one launch takes
    {"ngroups": 0},
    {"segs": ((0, 16, 0, 0), (16, 5000, 2, 1))},            # group index outside the groups
    {"segs": ((0, 16, 0, 0), (16, 5000, -1, 1))},
    {"segs": ((0, 16, 0, 0), (24, 5000, 1, 1))},            # begin not 16-float aligned
    {"segs": ((0, 16, 0, 0), (16, 5000, 1, 2))},            # chunk0 out of step
    {"nchunks": 3}, {"nchunks": 5},                         # chunk count and lengths disagree
    {"slots": (0, 2)},                                      # step slot outside steps
    {"m": None}, {"v": None}, {"steps": None}, {"p": None}, {"g": None},
    {"amsgrad": 1},                                         # amsgrad without max_exp_avg_sq
    {"p": 0x1004},                                          # arena not 16-byte aligned
])
def test_segment_entry_point_rejects_bad_arguments(kw):
    lib = _lib.load()
    assert lib.fscnn_adamw_segments(*_segment_args(**kw)) == -1
    assert b"adamw_segments" in lib.fscnn_last_error()


def test_segments_contiguous_tensors_are_one_segment():
    # 16-float aligned neighbours [0,10) [16,40) [48,64) of one group
    segs, chunks = _segments([0, 16, 48], [10, 24, 16], [0, 0, 0])
    assert segs == [(0, 64, 0, 0)]
    assert chunks == [0]


def test_segments_split_around_a_foreign_tensor():
    # [16, 40) belongs to nobody (frozen, or not handed to the optimizer)
    segs, chunks = _segments([0, 48], [10, 16], [0, 0])
    assert segs == [(0, 10, 0, 0), (48, 64, 0, 1)]
    assert chunks == [0, 1]


def test_segments_interleaved_groups_alternate():
    offs = [0, 16, 32, 48, 64]
    segs, chunks = _segments(offs, [16] * 5, [0, 1, 0, 1, 0])
    assert [s[2] for s in segs] == [0, 1, 0, 1, 0]
    assert [(s[0], s[1]) for s in segs] == [(o, o + 16) for o in offs]
    assert chunks == [0, 1, 2, 3, 4]
    # neighbours of one group merge, the other group's tensor still splits
    segs, _ = _segments(offs, [16] * 5, [0, 0, 1, 0, 0])
    assert segs == [(0, 32, 0, 0), (32, 48, 1, 1), (48, 80, 0, 2)]


def test_segments_are_order_independent():
    a = _segments([0, 16, 48, 4096], [10, 24, 16, 5000], [0, 0, 1, 0])
    b = _segments([4096, 48, 0, 16], [5000, 16, 10, 24], [0, 1, 0, 0])
    assert a == b


def test_segments_chunk_counts_follow_the_lengths():
    lens = [1, ADAMW_CHUNK - 1, ADAMW_CHUNK, ADAMW_CHUNK + 1, 3 * ADAMW_CHUNK + 5]
    offs, o = [], 0
    for n in lens:
        offs.append(o)
        o += (n + 15) // 16 * 16 + 16  # a 16-float hole after each: nothing merges
    segs, chunks = _segments(offs, lens, [0] * len(lens))
    assert len(segs) == len(lens)
    want = [1, 1, 1, 2, 4]
    c0 = 0
    for s, (seg, n, w) in enumerate(zip(segs, lens, want)):
        assert seg == (offs[s], offs[s] + n, 0, c0)
        assert chunks[c0:c0 + w] == [s] * w
        c0 += w
    assert len(chunks) == c0
    assert _segments([], [], []) == ([], [])


@pytest.mark.parametrize("kw", [{"lr": -1e-3}, {"eps": -1e-8}, {"weight_decay": -0.1},
                                {"betas": (1.0, 0.999)}, {"betas": (0.9, 1.0)},
                                {"betas": (-0.1, 0.999)}, {"betas": (0.9, -0.5)}])
def test_constructor_validation(kw):
    p = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(ValueError):
        FusedAdamW([p], **kw)
    with pytest.raises(ValueError):
        torch.optim.AdamW([p], **kw)  # the same arguments torch refuses


def test_constructor_defaults_and_amp_protocol():
    p = torch.nn.Parameter(torch.zeros(4))
    opt = FusedAdamW([p])
    g = opt.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"], g["amsgrad"], g["maximize"]) == \
        (1e-3, (0.9, 0.999), 1e-8, 1e-2, False, False)
    assert opt._step_supports_amp_scaling is True
    assert "grad_scaler" not in inspect.signature(opt.step).parameters
    assert "grad_scaler" not in inspect.signature(FusedAdamW.step).parameters
    with pytest.raises(TypeError):
        FusedAdamW([p], 1e-3, (0.9, 0.999), 1e-8, 1e-2, False, True)  # maximize is keyword-only
    FusedAdamW([p], betas=(0.0, 0.0), lr=0.0, eps=0.0, weight_decay=0.0)  # the closed ends


def test_step_on_cpu_parameters_raises():
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    opt = FusedAdamW([p])
    with pytest.raises(RuntimeError):
        opt.step()
    assert torch.equal(p.detach(), torch.zeros(4)) and len(opt.state[p]) == 0


def test_parameters_without_gradients_get_no_state():
    p = torch.nn.Parameter(torch.zeros(4))
    opt = FusedAdamW([p])
    opt.step()  # nothing to do: no gradient anywhere, no kernel, no state
    assert len(opt.state) == 0
    assert opt.state_dict()["state"] == {}
