"""The plan layout is pinned byte for byte: every workspace total and every named buffer's
(offset, rows, cols, ld, in_bws) of 135 plans must equal the recorded fixture
tests/golden/plan_layout.npz.  No GPU is needed: plans are host-side tables.

The two workspace totals pin the arenas that carry no name (weight-gradient slabs, dz, bnpart,
team sums, split planes): any change to their sizing moves the totals.

    python tests/test_plan_layout_cpu.py --record      # rewrite the fixture from the built library
"""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "plan_layout.npz")

NETS = [(19, 0), (2, 0), (19, 1)]
SHAPES = [(1, 33, 47), (3, 64, 96), (2, 128, 256), (1, 768, 768), (8, 1024, 2048)]
DTYPES = [0, 1, 2]   # f32, bf16, f16
TRAIN = [0, 1, 2]

UNITS = (["c0", "l1dw", "l1pw", "l2dw", "l2pw"]
         + ["lb%s%d" % (k, i) for i in range(9) for k in "edp"]
         + ["ppk%d" % i for i in range(4)]
         + ["po", "fdw", "flow", "fhigh", "c1dw", "c1pw", "c2dw", "c2pw", "aux0"])
FIELDS = [".a", ".z", ".scale", ".shift", ".mean", ".invstd", ".ga"]
NAMES = ([u + f for u in UNITS for f in FIELDS]
         + ["concat", "up_low", "f", "drop", "logits", "g_logits", "g_f", "g_up", "g_concat", "dz"])
ABSENT = -1  # all five fields of a name the plan does not have
ROW = 2 + 5 * len(NAMES)


def configs(net=None):
    return [(nc, aux, N, H, W, dt, tr) for nc, aux in NETS if net in (None, (nc, aux))
            for N, H, W in SHAPES for dt in DTYPES for tr in TRAIN]


def plan_row(lib, net, N, H, W, dt, tr):
    """[fwd_bytes, bwd_bytes] + (offset, rows, cols, ld, in_bws) of every probed name."""
    from fast_scnn_pytorch_amd import _lib
    plan = _lib.c_vp()
    _lib.check(lib.fscnn_plan_create(net, N, H, W, dt, tr, ctypes.byref(plan)), "fscnn_plan_create")
    try:
        fw, bw = _lib.c_ll(), _lib.c_ll()
        _lib.check(lib.fscnn_plan_workspace(plan, ctypes.byref(fw), ctypes.byref(bw)))
        row = [fw.value, bw.value]
        off, rows = _lib.c_ll(), _lib.c_ll()
        cols, ld, bws = _lib.c_int(), _lib.c_int(), _lib.c_int()
        for name in NAMES:
            rc = lib.fscnn_plan_buffer(plan, name.encode(), ctypes.byref(off), ctypes.byref(rows),
                                       ctypes.byref(cols), ctypes.byref(ld), ctypes.byref(bws))
            row += [ABSENT] * 5 if rc else [off.value, rows.value, cols.value, ld.value, bws.value]
        return row
    finally:
        lib.fscnn_plan_destroy(plan)


def record(net=None):
    """int64 [plans][ROW], plans in configs(net) order."""
    from fast_scnn_pytorch_amd import _lib
    lib = _lib.load()
    out, handles = [], {}
    try:
        for nc, aux, N, H, W, dt, tr in configs(net):
            if (nc, aux) not in handles:
                h = _lib.c_vp()
                _lib.check(lib.fscnn_net_create(nc, aux, ctypes.byref(h)), "fscnn_net_create")
                handles[(nc, aux)] = h
            out.append(plan_row(lib, handles[(nc, aux)], N, H, W, dt, tr))
    finally:
        for h in handles.values():
            lib.fscnn_net_destroy(h)
    return np.asarray(out, dtype=np.int64)


@pytest.fixture(scope="module")
def golden():
    g = np.load(FIXTURE)["layout"]
    assert g.dtype == np.int64 and g.shape == (len(configs()), ROW)
    return g


@pytest.mark.parametrize("net", NETS, ids=["c19", "c2", "c19aux"])
def test_plan_layout_matches_fixture(net, golden):
    want = golden[[i for i, c in enumerate(configs()) if c[:2] == net]]
    got = record(net)
    assert got.shape == want.shape
    for cfg, g, w in zip(configs(net), got, want):
        bad = np.nonzero(g != w)[0]
        if bad.size:
            j = int(bad[0])
            what = ("fwd_bytes", "bwd_bytes")[j] if j < 2 else \
                "%s[%s]" % (NAMES[(j - 2) // 5], ("offset", "rows", "cols", "ld", "in_bws")[(j - 2) % 5])
            pytest.fail("plan (classes, aux, N, H, W, dtype, train) = %r: %s is %d, recorded %d "
                        "(%d fields differ)" % (cfg, what, g[j], w[j], bad.size))


def test_fixture_spot_values(golden):
    """Figures of one plan, written down when the fixture was first recorded: they guard the
    recorder itself (a recorder that stored the wrong thing would still agree with itself)."""
    row = golden[configs().index((19, 0, 3, 64, 96, 1, 1))]
    assert (row[0], row[1]) == (10552064, 10252544)
    absent = [n for k, n in enumerate(NAMES) if row[2 + 5 * k] == ABSENT]
    assert len(absent) == 13
    # no gradient buffer of its own: PPM branches, FFM 1x1 branches; no aux head in this net
    assert absent == ["ppk%d.ga" % i for i in range(4)] + ["flow.ga", "fhigh.ga"] + \
        ["aux0" + f for f in FIELDS]
    # an inference plan has no backward workspace and no gradient names
    row = golden[configs().index((19, 0, 1, 768, 768, 0, 0))]
    assert row[1] == 0 and row[2 + 5 * NAMES.index("c0.ga")] == ABSENT


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    sys.path.insert(0, ROOT)
    import _fscnn_boot
    _fscnn_boot.load()
    layout = record()
    np.savez_compressed(FIXTURE, layout=layout)
    print("recorded %s: %d plans x %d fields, %d bytes" % (FIXTURE, layout.shape[0], layout.shape[1],
                                                           os.path.getsize(FIXTURE)))
