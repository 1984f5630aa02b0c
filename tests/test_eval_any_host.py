"""Host side of the ragged MS-SSIM (rgbac.metrics.any_size): the per-image level geometry, the
descriptor table and the input errors that are raised before the GPU is touched.  No GPU."""
import ctypes
import struct

import pytest
import torch
import torch.nn.functional as F

from rgbac.metrics import any_size as ma
from rgbac.metrics import masked_ms_ssim_any, ms_ssim_any

HW = [(161, 177), (177, 161), (200, 250), (250, 200), (192, 256), (176, 250), (161, 161),
      (163, 165), (255, 257), (375, 500), (500, 375), (321, 199), (1000, 161)]


@pytest.mark.parametrize("h,w", HW)
def test_level_sizes_are_avg_pool2d_shapes(h, w):
    x = torch.zeros((1, 1, h, w))
    want = [(h, w)]
    for _ in range(4):
        x = F.avg_pool2d(x, kernel_size=2, padding=(x.shape[2] % 2, x.shape[3] % 2))
        want.append((x.shape[2], x.shape[3]))
    assert ma.level_sizes(h, w, 5) == want


def test_level_sizes_of_the_smallest_side():
    assert [h for h, _ in ma.level_sizes(161, 250, 5)] == [161, 81, 41, 21, 11]
    assert [w for _, w in ma.level_sizes(161, 250, 5)] == [250, 125, 63, 32, 16]


def _restated_table(sizes, levels, ws, canvas):
    """Plain Python: per level and image (h, w, tiles per row, tiles), the planes, the largest
    tile count."""
    cur = list(sizes)
    rows, planes, mt = [], [], []
    for l in range(levels):
        row = []
        for h, w in cur:
            ty, tx = (h - ws + 1 + 15) // 16, (w - ws + 1 + 15) // 16
            row.append((h, w, tx, tx * ty))
        rows.append(row)
        planes.append(canvas if l == 0 else (max(h for h, _ in cur), max(w for _, w in cur)))
        mt.append(max(r[3] for r in row))
        cur = [((h + 2 * (h % 2) - 2) // 2 + 1, (w + 2 * (w % 2) - 2) // 2 + 1) for h, w in cur]
    return rows, planes, mt


@pytest.mark.parametrize("ws", [7, 11])
def test_descriptor_table(ws):
    sizes = [(161, 177), (192, 256), (176, 250)]
    t = ma.level_table(sizes, 5, ws, canvas=(192, 256))
    rows, planes, mt = _restated_table(sizes, 5, ws, (192, 256))
    assert t["rows"] == rows and t["planes"] == planes and t["max_tiles"] == mt
    if ws == 11:
        assert t["rows"][4][0] == (11, 12, 1, 1)            # a 1 x 2 valid map: one tile
        assert planes == [(192, 256), (96, 128), (48, 64), (24, 32), (12, 16)]
    raw = ma.pack_table(t)
    from rgbac import _lib
    assert ctypes.sizeof(_lib.SsimAnyDesc) == 16 and len(raw) == 16 * 5 * 3
    flat = [r for level in rows for r in level]
    assert [struct.unpack_from("<4i", raw, 16 * k) for k in range(15)] == flat


def test_table_without_canvas_uses_the_largest_image():
    t = ma.level_table([(161, 300), (200, 170)], 5, 11)
    assert t["planes"][0] == (200, 300) and t["planes"][1] == (100, 150)


def _xy(B=2, hp=192, wp=256):
    return torch.zeros((B, 3, hp, wp)), torch.zeros((B, 3, hp, wp))


def test_errors_before_the_gpu():
    X, Y = _xy()
    ok = [(161, 177), (192, 256)]
    with pytest.raises(ValueError, match="image 1 .*160x200.* level 4"):
        ms_ssim_any(X, Y, [(161, 177), (160, 200)])
    with pytest.raises(ValueError, match="image 0 .*161x160"):
        masked_ms_ssim_any(X, Y, torch.ones((2, 1, 192, 256)), [(161, 160), (192, 256)])
    with pytest.raises(ValueError, match="odd"):
        ms_ssim_any(X, Y, ok, win_size=10)
    with pytest.raises(ValueError, match="at most 15"):
        ms_ssim_any(X, Y, ok, win_size=17)
    with pytest.raises(ValueError, match="image 1 .*exceeds the 192x256 canvas"):
        ms_ssim_any(X, Y, [(161, 177), (193, 256)])
    with pytest.raises(ValueError, match="image 0 .*exceeds"):
        ms_ssim_any(X, Y, [(161, 257), (192, 256)])
    with pytest.raises(ValueError, match="1 sizes for a batch of 2"):
        ms_ssim_any(X, Y, ok[:1])
    with pytest.raises(ValueError, match="mask must be"):
        masked_ms_ssim_any(X, Y, torch.ones((2, 3, 192, 256)), ok)
    with pytest.raises(ValueError, match="requires grad"):
        ms_ssim_any(X, Y.clone().requires_grad_(True), ok)
    # a smaller window admits a smaller image: 7 taps, five levels -> sides above 96
    assert ma.level_table([(97, 97)], 5, 7)["rows"][4][0][:2] == (7, 7)
    with pytest.raises(ValueError, match="level 4"):
        ma.level_table([(96, 97)], 5, 7)


def test_valid_cpu_inputs_are_refused_as_cpu():
    X, Y = _xy()
    with pytest.raises(RuntimeError, match="GPU"):
        ms_ssim_any(X, Y, [(161, 177), (192, 256)])
