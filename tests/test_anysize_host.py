"""CPU: the any-size geometry layer (rgbac/anysize.py, csrc/anysize.hip) without a GPU: the
canvas rule, the C entry points' argument checks (no launch), the descriptor's ctypes layout
against the C header, and the Python entry points' input validation."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rgbac.h")


def test_padded_size_and_canvas():
    from rgbac import anysize as az
    assert az.padded_size(1, 1) == (64, 64)
    assert az.padded_size(64, 64) == (64, 64)
    assert az.padded_size(65, 64) == (128, 64)
    assert az.padded_size(64, 129) == (64, 192)
    assert az.canvas([(1, 1)]) == (64, 64)
    assert az.canvas([(64, 64), (65, 64)]) == (128, 64)
    assert az.canvas([(1, 1), (5, 7), (64, 64), (63, 65), (70, 130)]) == (128, 192)
    assert az.canvas([(500, 375)] * 8) == (512, 384)
    for bad in [(0, 5), (5, 0), (-1, 64)]:
        with pytest.raises(ValueError):
            az.padded_size(*bad)
        with pytest.raises(ValueError):
            az.canvas([(64, 64), bad])
    with pytest.raises(ValueError):
        az.canvas([])


def _good(name):
    """A valid argument list of each entry point (pointers are never dereferenced: every case
    below breaks one argument, and the checks run before any launch)."""
    p = 4096                                                  # non-null, aligned
    return {
        "rgbac_rgba_pack": [2, p, 64, 128, 0, p, p, p, None],
        "rgbac_pad_nchw": [2, 3, 50, 100, 64, 128, 0, p, p + (1 << 30), None],
        "rgbac_rgba_unpack": [2, p, 64, 128, p, p, 1, None],
        "rgbac_region_error": [2, 3, p, 64, 128, p, p, p, p, p, p, p, p, None],
    }[name]


# (entry point, index of the argument to break, bad value, message)
_BAD = [
    ("rgbac_rgba_pack", 0, 0, "batch"),
    ("rgbac_rgba_pack", 1, None, "null descriptor"),
    ("rgbac_rgba_pack", 2, 65, "multiples of 64"),
    ("rgbac_rgba_pack", 3, 100, "multiples of 64"),
    ("rgbac_rgba_pack", 4, 2, "pad mode"),
    ("rgbac_rgba_pack", 4, -1, "pad mode"),
    ("rgbac_pad_nchw", 0, 0, "batch"),
    ("rgbac_pad_nchw", 4, 50, "multiples of 64"),
    ("rgbac_pad_nchw", 5, 100, "multiples of 64"),
    ("rgbac_pad_nchw", 6, 2, "pad mode"),
    ("rgbac_pad_nchw", 2, 65, "shape"),                      # h > hp
    ("rgbac_pad_nchw", 7, None, "null pointer"),
    ("rgbac_pad_nchw", 8, 4096, "alias"),
    ("rgbac_rgba_unpack", 0, 0, "batch"),
    ("rgbac_rgba_unpack", 1, None, "null descriptor"),
    ("rgbac_rgba_unpack", 2, 32, "multiples of 64"),
    ("rgbac_rgba_unpack", 4, None, "null pointer"),
    ("rgbac_region_error", 0, 0, "batch"),
    ("rgbac_region_error", 1, 0, "channels"),
    ("rgbac_region_error", 2, None, "null descriptor"),
    ("rgbac_region_error", 3, 63, "multiples of 64"),
    ("rgbac_region_error", 8, None, "null pointer"),         # scratch
]


@pytest.mark.parametrize("name,idx,value,msg", _BAD)
def test_argument_errors_are_reported_without_launching(name, idx, value, msg):
    from rgbac import _lib
    args = _good(name)
    args[idx] = value
    with pytest.raises(RuntimeError, match=f"{name} failed.*{msg}"):
        _lib.call(name, *args)


def test_rgba_pack_needs_an_output():
    from rgbac import _lib
    args = _good("rgbac_rgba_pack")
    args[5] = args[6] = args[7] = None
    with pytest.raises(RuntimeError, match="no output"):
        _lib.call("rgbac_rgba_pack", *args)


def test_region_error_blocks_query():
    from rgbac import _lib
    lib = _lib.load()
    assert lib.rgbac_region_error_blocks(0, 64) == 0
    small, big = lib.rgbac_region_error_blocks(64, 64), lib.rgbac_region_error_blocks(4096, 4096)
    assert 1 <= small <= big
    assert lib.rgbac_region_error_blocks(1 << 14, 1 << 14) == big      # capped


def test_image_desc_layout_matches_c(tmp_path):
    """Compile a probe against include/rgbac.h with gcc and compare offsets with ctypes."""
    from rgbac import _lib
    cls = _lib.ImageDesc
    fields = [f for f, _ in cls._fields_]
    src = tmp_path / "probe.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"',
             'int main(void){', 'printf("%zu\\n", sizeof(rgbac_image_desc));']
    lines += [f'printf("%zu\\n", offsetof(rgbac_image_desc, {f}));' for f in fields]
    lines += ['printf("%d %d\\n", (int)RGBAC_PAD_TRANSPARENT, (int)RGBAC_PAD_REPLICATE);',
              'return 0;}']
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-O0", str(src), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True,
                                           text=True).stdout.split()]
    assert vals[0] == ctypes.sizeof(cls) == 24
    for f, off in zip(fields, vals[1:-2]):
        assert getattr(cls, f).offset == off, f
    assert vals[-2:] == [_lib.PAD_MODES["transparent"], _lib.PAD_MODES["replicate"]]


def test_pack_rgba_rejects_bad_input():
    from rgbac import anysize as az
    ok = np.zeros((5, 7, 4), dtype=np.uint8)
    with pytest.raises(ValueError, match="empty batch"):
        az.pack_rgba([])
    for bad in [np.zeros((5, 7, 4), dtype=np.float32),        # dtype
                np.zeros((5, 7, 3), dtype=np.uint8),          # RGB, not RGBA
                np.zeros((5, 7), dtype=np.uint8),             # rank
                np.zeros((1, 5, 7, 4), dtype=np.uint8),       # rank
                np.zeros((0, 7, 4), dtype=np.uint8),          # empty
                torch.zeros((5, 7, 4), dtype=torch.int32)]:
        with pytest.raises(ValueError, match="uint8 RGBA"):
            az.pack_rgba([ok, bad])
    with pytest.raises(ValueError, match="pad must be"):
        az.pack_rgba([ok], pad="reflect")
    with pytest.raises(RuntimeError, match="GPU"):            # no CPU path
        az.pack_rgba([ok], device="cpu")


class _NoModel:
    """compress / decompress must not be reached by any rejected call."""

    def compress(self, *a, **k):
        raise AssertionError("model.compress reached")

    def decompress(self, *a, **k):
        raise AssertionError("model.decompress reached")


def test_compress_any_rejects_bad_input():
    from rgbac import anysize as az
    m = _NoModel()
    x, a = torch.zeros((2, 3, 50, 100)), torch.ones((2, 1, 50, 100))
    for bx, ba in [(x[0], a),                                  # rank
                   (torch.zeros((2, 4, 50, 100)), a),         # channels
                   (x, torch.ones((2, 3, 50, 100))),          # mask channels
                   (x, torch.ones((2, 1, 50, 99))),           # mask size
                   (x, torch.ones((1, 1, 50, 100))),          # mask batch
                   (x.to(torch.uint8), a),                     # dtype
                   (torch.zeros((2, 3, 0, 100)), torch.ones((2, 1, 0, 100)))]:
        with pytest.raises(ValueError):
            az.compress_any(m, bx, ba)
    with pytest.raises(ValueError, match="pad must be"):
        az.compress_any(m, x, a, pad="zeros")
    with pytest.raises(RuntimeError, match="GPU"):            # CPU tensors: the existing check
        az.compress_any(m, x, a)


def test_decompress_any_rejects_bad_input():
    from rgbac import anysize as az
    m = _NoModel()
    a = torch.ones((2, 1, 50, 100))
    strings = [[b""], [b"", b""]]
    with pytest.raises(ValueError, match="size says"):        # mask is not `size`
        az.decompress_any(m, strings, (1, 2), a, (50, 99))
    with pytest.raises(ValueError, match="does not belong"):  # shape of another canvas
        az.decompress_any(m, strings, (1, 1), a, (50, 100))
    with pytest.raises(ValueError, match="does not belong"):
        az.decompress_any(m, strings, torch.Size((2, 2)), a, (50, 100))
    with pytest.raises(ValueError):
        az.decompress_any(m, strings, (1, 2), a[:, 0], (50, 100))      # rank
    with pytest.raises(ValueError):
        az.decompress_any(m, strings, (1, 2), torch.ones((2, 3, 50, 100)), (50, 100))
    with pytest.raises(ValueError, match="pad must be"):
        az.decompress_any(m, strings, (1, 2), a, (50, 100), pad="edge")
    with pytest.raises(RuntimeError, match="GPU"):
        az.decompress_any(m, strings, (1, 2), a, (50, 100))


def test_tensor_entry_points_reject_bad_input():
    from rgbac import anysize as az
    x = torch.zeros((2, 3, 64, 128))
    with pytest.raises(ValueError):
        az.unpack_rgba(x, None, [(50, 100)])                  # one size for two images
    with pytest.raises(ValueError):
        az.unpack_rgba(x, None, [(50, 100), (65, 90)])        # larger than the canvas
    with pytest.raises(ValueError):
        az.unpack_rgba(x[..., :100], None, [(50, 100), (64, 90)])      # canvas not 64-aligned
    with pytest.raises(ValueError):
        az.region_error(x, x[:, :2], [(50, 100), (64, 90)])   # channel mismatch
    with pytest.raises(ValueError):
        az.region_error(x, x, [(50, 100), (64, 90)], mask=x)  # mask channels
    with pytest.raises(RuntimeError, match="GPU"):
        az.region_error(x, x, [(50, 100), (64, 90)])
    with pytest.raises(RuntimeError, match="GPU"):
        az.unpack_rgba(x, None, [(50, 100), (64, 90)])
    with pytest.raises(RuntimeError, match="GPU"):
        az.pad_planes(x[..., :50, :100])
