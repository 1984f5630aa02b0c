"""MS-SSIM and masked MS-SSIM for a batch of images of different sizes on one canvas
(csrc/msssim_any.hip) -- the evaluation metric of trainRGB.py:308-312 without falling back to
batch 1.

``X, Y (B, C, hp, wp)`` are canvas tensors as `rgbac.anysize` makes them: image b is the
top-left ``h_b x w_b`` of its planes, ``sizes = [(h_b, w_b), ...]``.  Every image is scored as
``ms_ssim`` scores its crop alone: nothing outside its rectangle enters its value, whatever the
canvas holds there (replicated rows, zeros, a taller neighbour's coarser levels).  The canvas is
read in place; there are no crop copies.

Per image the scale pyramid is its own: level 0 ``(h_b, w_b)``, level l+1
``((h + 2(h%2) - 2)//2 + 1, (w + 2(w%2) - 2)//2 + 1)`` (the reference's ``F.avg_pool2d(kernel 2,
padding (h%2, w%2))``, ms_ssim_torch.py:183-185).  The host computes every image's size and
tile grid at every level and uploads them once as one descriptor table (levels x B).  Launches
for L levels: L tile launches (one per scale for the whole batch), L - 1 pooling launches (all
planes of X and Y -- and the mask -- at once), one reduce, one combine: 2L + 1 = 11 for the
default five, against 19 per image (and the crop copies) for a loop of ``ms_ssim`` over crops.

Evaluation only: there is no backward, and an input that requires grad raises.
"""
import ctypes

import torch

from .. import _lib
from .. import runtime as rt
from .ms_ssim_torch import _TILE, _WEIGHTS, _consts, _device_const, _win_1d

MAX_WIN = 15            # the LDS patch of the tile kernels (csrc/msssim.hip SS_MAXWS)
MAX_LEVELS = 8


def next_level(h, w):
    """(h, w) of one image -> its size after F.avg_pool2d(kernel 2, padding (h%2, w%2))."""
    return (h + 2 * (h % 2) - 2) // 2 + 1, (w + 2 * (w % 2) - 2) // 2 + 1


def level_sizes(h, w, levels):
    """[(h_0, w_0), ..., (h_{levels-1}, w_{levels-1})] of one image."""
    out = [(int(h), int(w))]
    for _ in range(levels - 1):
        out.append(next_level(*out[-1]))
    return out


def _tiles(h, w, ws):
    """(tiles per row, tiles) of the 16 x 16 tile grid over the (h-ws+1) x (w-ws+1) valid map."""
    tx, ty = -(-(w - ws + 1) // _TILE), -(-(h - ws + 1) // _TILE)
    return tx, tx * ty


def level_table(sizes, levels, win_size, canvas=None):
    """The host geometry of one ragged call.  sizes: [(h_b, w_b)]; canvas: (hp, wp) of level 0
    (default: the largest image).  Returns {"rows": rows[l][b] = (h, w, tiles_x, ntiles),
    "planes": [(Hc_l, Wc_l)], "max_tiles": [the largest image's tile count per level], "levels",
    "win_size"}.  Raises
    ValueError, naming the image, for a bad window, a size outside the canvas, or an image that
    is smaller than the window at some level."""
    ws = int(win_size)
    if ws < 1 or ws % 2 != 1:
        raise ValueError(f"ms_ssim_any: the window size must be odd, got {ws}")
    if ws > MAX_WIN:
        raise ValueError(f"ms_ssim_any: the window size must be at most {MAX_WIN}, got {ws}")
    levels = int(levels)
    if not 1 <= levels <= MAX_LEVELS:
        raise ValueError(f"ms_ssim_any: 1 to {MAX_LEVELS} levels (weights), got {levels}")
    sizes = [(int(h), int(w)) for h, w in sizes]
    if not sizes:
        raise ValueError("ms_ssim_any: empty batch")
    per_image = []
    for b, (h, w) in enumerate(sizes):
        if h < 1 or w < 1:
            raise ValueError(f"ms_ssim_any: image {b} has size {h}x{w}")
        if canvas is not None and (h > canvas[0] or w > canvas[1]):
            raise ValueError(f"ms_ssim_any: image {b} ({h}x{w}) exceeds the "
                             f"{canvas[0]}x{canvas[1]} canvas")
        lv = level_sizes(h, w, levels)
        for l, (hl, wl) in enumerate(lv):
            if hl < ws or wl < ws:
                raise ValueError(
                    f"ms_ssim_any: image {b} ({h}x{w}) is {hl}x{wl} at level {l}, smaller than "
                    f"the {ws}-tap window; with {levels} levels each side must exceed "
                    f"{(ws - 1) * 2 ** (levels - 1)}")
        per_image.append(lv)
    rows, planes, max_tiles = [], [], []
    for l in range(levels):
        row = [(hl, wl) + _tiles(hl, wl, ws) for hl, wl in (lv[l] for lv in per_image)]
        rows.append(row)
        planes.append((max(r[0] for r in row), max(r[1] for r in row)))
        max_tiles.append(max(r[3] for r in row))
    if canvas is not None:
        planes[0] = (int(canvas[0]), int(canvas[1]))
    return {"rows": rows, "planes": planes, "max_tiles": max_tiles, "levels": levels,
            "win_size": ws}


def pack_table(table):
    """The table's rows as the bytes of rgbac_ssim_any_desc[levels][B] (one upload)."""
    rows = [r for level in table["rows"] for r in level]
    arr = (_lib.SsimAnyDesc * len(rows))()
    for k, r in enumerate(rows):
        arr[k] = _lib.SsimAnyDesc(*r)
    return bytes(arr)


def _check_inputs(X, Y, mask, sizes, who):
    for name, t in (("X", X), ("Y", Y), ("mask", mask)):
        if t is None:
            continue
        if not torch.is_tensor(t) or t.dim() != 4 or not t.is_floating_point():
            raise ValueError(f"{who}: {name} must be a 4-d floating-point tensor")
        if t.requires_grad:
            raise ValueError(f"{who}: {name} requires grad; this metric is evaluation only and "
                             "has no backward (use rgbac.metrics.ms_ssim_torch for a loss)")
    if X.shape != Y.shape:
        raise ValueError(f"{who}: X {tuple(X.shape)} and Y {tuple(Y.shape)} differ")
    B, C, hp, wp = X.shape
    if mask is not None and tuple(mask.shape) != (B, 1, hp, wp):
        raise ValueError(f"{who}: the mask must be ({B}, 1, {hp}, {wp}), got {tuple(mask.shape)}")
    sizes = [(int(h), int(w)) for h, w in sizes]
    if len(sizes) != B:
        raise ValueError(f"{who}: {len(sizes)} sizes for a batch of {B}")
    return sizes


def _run(X, Y, mask, sizes, win_size, win_sigma, data_range, weights, who):
    sizes = _check_inputs(X, Y, mask, sizes, who)
    B, C, hp, wp = X.shape
    wts_host = _WEIGHTS if weights is None else weights
    levels = int(torch.as_tensor(wts_host).numel())
    table = level_table(sizes, levels, win_size, canvas=(hp, wp))     # ValueErrors: no launch yet
    rt.check_gpu(X, Y, mask)
    dev = X.device
    masked = mask is not None
    with torch.no_grad():
        wts = _device_const(wts_host, dev)
        w1d = _win_1d(None, table["win_size"], win_sigma, dev)
        ws = table["win_size"]
        x, y = X.contiguous().float(), Y.contiguous().float()
        m = mask.contiguous().float() if masked else None
        lib = _lib.load()
        descs = torch.frombuffer(bytearray(pack_table(table)), dtype=torch.uint8).to(dev)
        dsize = ctypes.sizeof(_lib.SsimAnyDesc)
        offsets, total = [], 0
        for mt in table["max_tiles"]:
            offsets.append(total)
            total += int(lib.rgbac_ssim_any_partial_floats(B, C, mt, 1 if masked else 0))
        part = torch.empty((total,), dtype=torch.float32, device=dev)
        units = B * C if masked else B
        ssim_t = torch.empty((levels, units), dtype=torch.float32, device=dev)
        cs_t = torch.empty((levels, units), dtype=torch.float32, device=dev)
        c1, c2 = _consts(data_range)
        st = _lib.stream_ptr(dev)
        for l in range(levels):
            hc, wc = table["planes"][l]
            dl = descs.data_ptr() + l * B * dsize
            _lib.call("rgbac_ssim_any_level", B, C, hc, wc, ws, dl, table["max_tiles"][l],
                      x.data_ptr(), y.data_ptr(), _lib.ptr(m), w1d.data_ptr(), c1, c2,
                      part.data_ptr() + 4 * offsets[l], st)
            if l + 1 < levels:     # the reference's last pool feeds nothing
                ho, wo = table["planes"][l + 1]
                xo = torch.empty((B, C, ho, wo), dtype=torch.float32, device=dev)
                yo = torch.empty((B, C, ho, wo), dtype=torch.float32, device=dev)
                mo = torch.empty((B, 1, ho, wo), dtype=torch.float32, device=dev) if masked else None
                _lib.call("rgbac_avgpool2_any", B, C, hc, wc, ho, wo, dl, x.data_ptr(),
                          y.data_ptr(), _lib.ptr(m), xo.data_ptr(), yo.data_ptr(), _lib.ptr(mo), st)
                x, y, m = xo, yo, mo
        ph = (ctypes.c_int32 * levels)(*[p[0] for p in table["planes"]])
        pw = (ctypes.c_int32 * levels)(*[p[1] for p in table["planes"]])
        mt = (ctypes.c_int32 * levels)(*table["max_tiles"])
        off = (ctypes.c_int64 * levels)(*offsets)
        _lib.call("rgbac_ssim_any_reduce", levels, B, C, ws, 1 if masked else 0, descs.data_ptr(),
                  ctypes.addressof(ph), ctypes.addressof(pw), ctypes.addressof(mt),
                  ctypes.addressof(off), total, part.data_ptr(), ssim_t.data_ptr(),
                  cs_t.data_ptr(), st)
        out = torch.empty((B,), dtype=torch.float32, device=dev)
        if masked:
            _lib.call("rgbac_masked_msssim_combine", levels, B, C, cs_t.data_ptr(),
                      ssim_t[levels - 1].data_ptr(), wts.data_ptr(), out.data_ptr(), None, st)
        else:
            _lib.call("rgbac_msssim_combine", levels, B, cs_t.data_ptr(),
                      ssim_t[levels - 1].data_ptr(), wts.data_ptr(), out.data_ptr(), None, st)
    return out


def ms_ssim_any(X, Y, sizes, win_size=11, win_sigma=1.5, data_range=1.0, weights=None):
    """MS-SSIM (ms_ssim_torch.py:135-194) of every image of a ragged batch -> (B,) fp32 on the
    device; value b is ``ms_ssim(X[b:b+1, :, :h_b, :w_b], Y[...], size_average=False)``.
    Raises ValueError before any launch when an image is smaller than the window at some level
    (defaults: a side of 160 or less), the window is even or above 15, or a size exceeds the
    canvas."""
    return _run(X, Y, None, sizes, win_size, win_sigma, data_range, weights, "ms_ssim_any")


def masked_ms_ssim_any(X, Y, mask, sizes, win_size=11, win_sigma=1.5, data_range=1.0,
                       weights=None):
    """Masked MS-SSIM (masked_ms_ssim_torch.py:181-265) of every image of a ragged batch ->
    (B,) fp32 on the device; ``mask`` is (B, 1, hp, wp), e.g. the true alpha canvas.  Value b is
    the uniform ``ms_ssim(X_crop, Y_crop, mask_crop, size_average=False)``; an image whose mask
    keeps nothing gives 0.  The same ValueErrors as ms_ssim_any."""
    if mask is None:
        raise ValueError("masked_ms_ssim_any: a mask is required")
    return _run(X, Y, mask, sizes, win_size, win_sigma, data_range, weights, "masked_ms_ssim_any")
