"""CPU-side checks of the overlay tail: the numpy restatement of the law (tests/overlay_ref.py)
against a literal per-pixel loop of the reference's ``create_visualization`` and at the law's edge
cases, and the boundary of the feature -- the three C-ABI functions are declared, exported and
bound, and ``overlay`` / ``overlay_mask`` refuse CPU tensors and bad arguments.  No compute call
is made (there is no GPU here)."""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import overlay_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fscnn_overlay_mask", "fscnn_e2e_overlay", "fscnn_forward_e2e_overlay")


def create_visualization_by_pixel(img, mask, alpha):
    """kuruma/core/preprocessing.py:85-104 one pixel at a time, in exact rational arithmetic: green
    where mask > 0, then saturate_cast<uchar>(img * 1.0 + green * alpha + 0), half to even.
    ``img`` is ``[h, w, 3]``, ``mask`` ``[h, w]``."""
    h, w, _ = img.shape
    out = np.zeros_like(img)
    al = Fraction(alpha)
    for y in range(h):
        for x in range(w):
            green = (0, 255, 0) if mask[y, x] > 0 else (0, 0, 0)
            for k in range(3):
                t = Fraction(int(img[y, x, k])) + green[k] * al
                out[y, x, k] = min(max(round(t), 0), 255)  # round(): half to even
    return out


@pytest.mark.parametrize("alpha", [0.5, 0.25, 1.0])
def test_restatement_matches_create_visualization(alpha):
    """Dyadic weights: every fp32 operation of the law is exact, so the restatement must equal the
    rational-arithmetic loop on every pixel."""
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (9, 13, 3), dtype=np.uint8)
    img[0, :4] = [[0, 0, 0], [0, 1, 0], [255, 255, 255], [3, 2, 1]]  # ties at alpha 0.5, saturation
    mask = (rng.random((9, 13)) < 0.5).astype(np.uint8) * 255
    mask[0, :4] = 255
    want = create_visualization_by_pixel(img, mask, alpha)
    got, resized = overlay_ref.overlay(img[None], mask[None], alpha=alpha, channels_last=True)
    assert np.array_equal(got[0], want)
    assert np.array_equal(resized[0], mask)
    planes, _ = overlay_ref.overlay(img.transpose(2, 0, 1)[None], mask[None], alpha=alpha)
    assert np.array_equal(planes[0].transpose(1, 2, 0), want)


def test_half_to_even():
    """a + 127.5: a = 0 and a = 1 both give 128."""
    got = overlay_ref.blend(np.array([0, 1, 2, 3]), np.full(4, 255), 1.0, 0.5, 0.0)
    assert got.tolist() == [128, 128, 130, 130]


def test_saturation_and_nan():
    assert overlay_ref.blend([200, 255], [255, 255], 1.0, 1.0, 0.0).tolist() == [255, 255]
    assert overlay_ref.blend([0, 10, 100], [0, 0, 255], 1.0, 0.5, -50.0).tolist() == [0, 0, 178]
    assert overlay_ref.blend([7], [9], float("nan"), 0.5, 0.0).tolist() == [0]
    assert overlay_ref.blend([7], [9], 1.0, 0.5, float("inf")).tolist() == [255]


def test_weights_select_frame_or_colour():
    rng = np.random.default_rng(6)
    frames = rng.integers(0, 256, (2, 3, 5, 7), dtype=np.uint8)
    mask = rng.integers(0, 2, (2, 5, 7), dtype=np.uint8) * 255
    same, _ = overlay_ref.overlay(frames, mask, alpha=0.0, frame_weight=1.0)
    assert np.array_equal(same, frames)
    only, _ = overlay_ref.overlay(frames, mask, alpha=1.0, frame_weight=0.0, color=(9, 8, 7))
    want = np.where(mask[:, None] != 0, np.array([9, 8, 7], dtype=np.uint8).reshape(1, 3, 1, 1), 0)
    assert np.array_equal(only, want)


@pytest.mark.parametrize("size,src", [(7, 7), (50, 37), (37, 50), (1920, 640), (3, 16384),
                                      (16384, 3), (2, 1)])
def test_nearest_map(size, src):
    """floor(x * src / size) as a rational: starts at 0, never leaves the mask, is monotone, and
    is the identity at equal sizes."""
    idx = overlay_ref.nearest_index(size, src)
    assert idx[0] == 0 and 0 <= idx.min() and idx.max() <= src - 1
    assert idx[-1] == ((size - 1) * src) // size
    assert (np.diff(idx) >= 0).all()
    assert [int(v) for v in idx[:5]] == [int(Fraction(x * src, size).__floor__())
                                          for x in range(min(size, 5))]
    if size == src:
        assert np.array_equal(idx, np.arange(size))
    if size < src:   # down-scaling skips source pixels, up-scaling repeats them
        assert len(set(idx.tolist())) == size
    else:
        assert set(idx.tolist()) == set(range(src))


def test_palette_ids_past_the_palette_get_no_colour():
    pal = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], dtype=np.uint8)
    ids = np.array([[[0, 1, 2, 3, 255]]], dtype=np.uint8)
    c = overlay_ref.colors(ids, palette=pal)
    assert c[0, 0].tolist() == [[1, 2, 3], [4, 5, 6], [7, 8, 9], [0, 0, 0], [0, 0, 0]]
    frames = np.full((1, 1, 5, 3), 10, dtype=np.uint8)
    got, _ = overlay_ref.overlay(frames, ids, alpha=1.0, frame_weight=1.0, palette=pal,
                                 channels_last=True)
    assert got[0, 0].tolist() == [[11, 12, 13], [14, 15, 16], [17, 18, 19], [10, 10, 10],
                                  [10, 10, 10]]


# ---- the boundary (these fail without the feature) ----------------------------------------------------
def test_symbols_declared_exported_bound():
    from fast_scnn_pytorch_amd import _lib
    src = open(os.path.join(ROOT, "include", "fastscnn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (fscnn_\w+)", out))
    for s in NEW:
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % s, src)
        assert m, "%s is not declared in include/fastscnn.h" % s
        assert s in exported, s
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s)
        assert len(_lib.SIGNATURES[s][1]) == len(m.group(1).split(",")), s


def test_class_table_is_one_form_for_both_modes():
    from fast_scnn_pytorch_amd import vis
    table, bits = vis.class_table(2, 255, (0, 255, 0), None)
    assert list(table[:6]) == [0, 255, 0, 0, 255, 0] and not any(table[6:]) and bits == 0b10
    assert vis.class_table(19, 1, (1, 2, 3), None)[1] == (1 << 19) - 2
    assert vis.class_table(3, 128, (1, 2, 3), None)[1] == 0b010  # 2 * 128 wraps to 0
    assert vis.class_table(40, 1, (1, 2, 3), None)[1] == (1 << 32) - 2
    pal = [[9, 9, 9], [1, 2, 3]]
    table, bits = vis.class_table(19, 255, (0, 255, 0), pal)
    assert list(table[:9]) == [9, 9, 9, 1, 2, 3, 0, 0, 0] and bits == 0b11
    table, bits = vis.class_table(2, 255, None, torch.arange(15, dtype=torch.uint8).view(5, 3))
    assert list(table[:9]) == [0, 1, 2, 3, 4, 5, 0, 0, 0] and bits == 0b11


def test_overlay_refuses_cpu_tensors_and_bad_arguments():
    from fast_scnn_pytorch_amd.deploy import EndToEndFastSCNN
    from fast_scnn_pytorch_amd.vis import overlay_mask
    from models.fast_scnn import FastSCNN
    frames = torch.zeros((1, 3, 8, 8), dtype=torch.uint8)
    mask = torch.zeros((1, 8, 8), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="device"):
        overlay_mask(frames, mask)
    with pytest.raises(RuntimeError, match="4-d"):
        overlay_mask(frames[0], mask)
    e2e =EndToEndFastSCNN(FastSCNN(2), input_size=(8, 8), base_size=32).eval()
    with pytest.raises(RuntimeError, match="device"):
        e2e.overlay(frames)
    with pytest.raises(RuntimeError, match="4-d"):
        e2e.overlay(frames[0])
    e2e.train()
    with pytest.raises(RuntimeError, match="eval"):
        e2e.overlay(frames)
    # colour arguments are checked on the host by the helper both entry points share
    from fast_scnn_pytorch_amd import vis
    for bad in (np.zeros((0, 3), dtype=np.uint8), np.zeros((257, 3), dtype=np.uint8),
                np.zeros((4, 4), dtype=np.uint8), [[0, 0, 256]],
                torch.zeros((4, 3), dtype=torch.float32)):
        with pytest.raises(RuntimeError, match="palette"):
            vis.class_table(19, 255, (0, 255, 0), bad)
    for bad in ((0, 255), (0, 256, 0), (-1, 0, 0), 7):
        with pytest.raises(RuntimeError, match="color"):
            vis.class_table(19, 255, bad, None)
