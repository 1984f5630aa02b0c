"""RGBA images of any size: device-side pad, crop and region-restricted error.

The codecs only take heights and widths that are positive multiples of 64 (`check_geometry`,
reference models/AutoEncoderRGB_Journal.py:242); that stays so.  This module is the geometry
layer around them (csrc/anysize.hip):

* a batch of images (h_b, w_b) shares one canvas hp x wp = round_up(max h_b, 64) x
  round_up(max w_b, 64), each image at the top-left;
* ``pad="transparent"`` fills the rest with zeros -- alpha 0 there, so the masked window
  attention drops those windows (`remove_zero_windows`) and the masked distortion
  (`reconstruct_error`, :36-64) never counts them: right for images that have transparency;
* ``pad="replicate"`` repeats each image's edge pixel, alpha included: an opaque image keeps
  `torch.all(mask == 1.0)` true, so no alpha-codec bits are charged (trainRGB.py:299-302);
* the crop back to uint8 RGBA quantises as torchvision's save_image does after the reference's
  clamp (trainRGB.py:290,295-297), and `region_error` is `reconstruct_error` restricted to each
  image's real rectangle.

GPU only, like the rest of the package: CPU tensors and a missing library raise.
"""
import torch

from . import _lib
from . import runtime as rt
from .rgba import _chain, rgba_forward

TILE = 64


def padded_size(h, w):
    """(h, w) -> (hp, wp): each rounded up to a multiple of 64."""
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f"anysize: image size must be at least 1x1, got {h}x{w}")
    return rt.round_up(h, TILE), rt.round_up(w, TILE)


def canvas(sizes):
    """[(h_b, w_b), ...] -> the (hp, wp) canvas the whole batch shares."""
    sizes = [(int(h), int(w)) for h, w in sizes]
    if not sizes:
        raise ValueError("anysize: empty batch")
    for h, w in sizes:
        padded_size(h, w)
    return padded_size(max(h for h, _ in sizes), max(w for _, w in sizes))


def _mode(pad):
    if pad not in _lib.PAD_MODES:
        raise ValueError(f"pad must be 'transparent' or 'replicate', got {pad!r}")
    return _lib.PAD_MODES[pad]


def _gpu_device(device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("rgbac: this module runs on the GPU (HIP) only; there is no CPU "
                           f"fallback in the product path (device={device!r}).")
    return dev


def _upload_descs(entries, dev):
    """[(ptr, h, w, row_stride_bytes), ...] -> device array of rgbac_image_desc (one copy)."""
    arr = (_lib.ImageDesc * len(entries))()
    for k, e in enumerate(entries):
        arr[k] = _lib.ImageDesc(*e)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)


def _check_sizes(sizes, B, hp, wp, who):
    sizes = [(int(h), int(w)) for h, w in sizes]
    if len(sizes) != B:
        raise ValueError(f"{who}: {len(sizes)} sizes for a batch of {B}")
    if hp % TILE or wp % TILE:
        raise ValueError(f"{who}: the canvas {hp}x{wp} is not a multiple of {TILE}")
    for h, w in sizes:
        if not (1 <= h <= hp and 1 <= w <= wp):
            raise ValueError(f"{who}: image size {h}x{w} does not fit the {hp}x{wp} canvas")
    return sizes


def _canvas_tensor(t, channels, who, like=None):
    if t.dim() != 4 or (channels is not None and t.shape[1] != channels):
        raise ValueError(f"{who}: expected (B, {channels or 'C'}, H, W), got {tuple(t.shape)}")
    if not t.is_floating_point():
        raise ValueError(f"{who}: expected a floating-point tensor, got {t.dtype}")
    if like is not None and (t.shape[0] != like.shape[0] or t.shape[2:] != like.shape[2:]):
        raise ValueError(f"{who}: shape {tuple(t.shape)} does not match {tuple(like.shape)}")


def _sources(images, device, who):
    """images -> (device, sizes, descriptor entries, the device tensors behind them)."""
    images = list(images)
    if not images:
        raise ValueError(f"{who}: empty batch")
    ts = []
    for im in images:
        t = torch.as_tensor(im)
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 4 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"{who}: expected (H, W, 4) uint8 RGBA, got {tuple(t.shape)} {t.dtype}")
        ts.append(t)
    dev = _gpu_device(device)
    sizes = [(int(t.shape[0]), int(t.shape[1])) for t in ts]
    entries, keep = [], []
    for t, (h, w) in zip(ts, sizes):
        t = t.to(dev, non_blocking=True)
        # rows of a view into a larger buffer are read in place; anything else is made dense
        if not (t.stride(2) == 1 and t.stride(1) == 4 and t.stride(0) % 4 == 0 and t.stride(0) >= 4 * w):
            t = t.contiguous()
        if t.data_ptr() % 4:
            t = t.clone(memory_format=torch.contiguous_format)
        keep.append(t)
        entries.append((t.data_ptr(), h, w, t.stride(0)))
    return dev, sizes, entries, keep


def _pack(dev, sizes, entries, mode, modes):
    """One pack launch onto the canvas of ``sizes``: ``mode`` for the batch, or a device int32
    tensor ``modes`` with one pad mode per image."""
    hp, wp = canvas(sizes)
    B = len(sizes)
    descs = _upload_descs(entries, dev)
    masked = torch.empty((B, 3, hp, wp), device=dev)
    alpha = torch.empty((B, 1, hp, wp), device=dev)
    rgb = torch.empty((B, 3, hp, wp), device=dev)
    if modes is None:
        _lib.call("rgbac_rgba_pack", B, descs.data_ptr(), hp, wp, mode, alpha.data_ptr(),
                  rgb.data_ptr(), masked.data_ptr(), _lib.stream_ptr(dev))
    else:
        _lib.call("rgbac_rgba_pack_modes", B, descs.data_ptr(), hp, wp, modes.data_ptr(),
                  alpha.data_ptr(), rgb.data_ptr(), masked.data_ptr(), _lib.stream_ptr(dev))
    return {"masked": masked, "alpha": alpha, "rgb": rgb, "sizes": sizes}


def pack_rgba(images, pad="transparent", device="cuda"):
    """images: list of (h, w, 4) uint8 arrays / tensors (decoded RGBA, CPU or GPU, any sizes).
    Returns {"masked": (B,3,hp,wp), "alpha": (B,1,hp,wp), "rgb": (B,3,hp,wp), "sizes", "pad"}:
    fp32 GPU planes on the batch's canvas, masked = where(alpha > 0, rgb, alpha).  One descriptor
    upload and one launch for the batch."""
    mode = _mode(pad)
    dev, sizes, entries, keep = _sources(images, device, "pack_rgba")
    out = _pack(dev, sizes, entries, mode, None)
    # the sources (``keep``) and descriptors may be freed now: the caching allocator orders
    # their reuse after this launch on the same stream
    out["pad"] = pad
    return out


def opaque_flags(images, device="cuda"):
    """-> device int32 (B,): 1 where every alpha byte of the image is 255 (one launch for the
    ragged batch, rgbac_rgba_opaque).  Nothing is read back here."""
    dev, sizes, entries, keep = _sources(images, device, "opaque_flags")
    return _opaque(dev, entries)


def _opaque(dev, entries):
    B = len(entries)
    descs = _upload_descs(entries, dev)
    scratch = torch.empty(B * _lib.OPAQUE_BLOCKS, dtype=torch.int32, device=dev)
    flags = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.call("rgbac_rgba_opaque", B, descs.data_ptr(), scratch.data_ptr(), flags.data_ptr(),
              _lib.stream_ptr(dev))
    return flags


def alpha_class(images, device="cuda"):
    """-> device int32 (B,): 1 where every alpha byte of the image is 255 (exactly where
    opaque_flags says 1), 2 where every one is 0, else 0 (rgbac_rgba_alpha_class).  Nothing is
    read back here."""
    dev, sizes, entries, keep = _sources(images, device, "alpha_class")
    return _alpha_class(dev, entries)


_MAX_RECTS = 65535            # rectangles per launch (the grid's y dimension)


def _alpha_class(dev, entries):
    parts = []
    for lo in range(0, len(entries), _MAX_RECTS):
        part = entries[lo:lo + _MAX_RECTS]
        B = len(part)
        descs = _upload_descs(part, dev)
        scratch = torch.empty(B * _lib.OPAQUE_BLOCKS * 2, dtype=torch.int32, device=dev)
        cls = torch.empty(B, dtype=torch.int32, device=dev)
        _lib.call("rgbac_rgba_alpha_class", B, descs.data_ptr(), scratch.data_ptr(),
                  cls.data_ptr(), _lib.stream_ptr(dev))
        parts.append(cls)
    return parts[0] if len(parts) == 1 else torch.cat(parts)


def pack_rgba_modes(images, modes, device="cuda"):
    """pack_rgba with one pad mode per image: ``modes`` a device int32 (B,) tensor of
    rgbac_pad_mode values (1 replicates, anything else pads transparent, so opaque_flags'
    result can be passed as it is) or a list of "transparent" / "replicate".  Bit-identical,
    image by image, to pack_rgba with that image's mode."""
    dev, sizes, entries, keep = _sources(images, device, "pack_rgba_modes")
    if not isinstance(modes, torch.Tensor):
        modes = torch.tensor([_mode(m) for m in modes], dtype=torch.int32).to(dev)
    rt.check_gpu(modes)
    if modes.dtype != torch.int32 or modes.numel() != len(sizes):
        raise ValueError(f"pack_rgba_modes: need {len(sizes)} int32 pad modes")
    return _pack(dev, sizes, entries, None, modes.contiguous())


def pad_planes(t, pad="transparent"):
    """(B, C, h, w) float tensor -> (B, C, hp, wp) fp32, padded at the bottom / right.  A tensor
    whose size is already a multiple of 64 is returned as it is."""
    mode = _mode(pad)
    _canvas_tensor(t, None, "pad_planes")
    B, C, h, w = t.shape
    hp, wp = padded_size(h, w)
    rt.check_gpu(t)
    if (hp, wp) == (h, w):
        return t
    src = t.contiguous().float()
    out = torch.empty((B, C, hp, wp), device=t.device)
    _lib.call("rgbac_pad_nchw", B, C, h, w, hp, wp, mode, src.data_ptr(), out.data_ptr(),
              _lib.stream_ptr(t.device))
    return out


def unpack_rgba(x_hat, alpha, sizes, zero_transparent=True):
    """Canvas x_hat (B,3,hp,wp) and alpha (B,1,hp,wp; None = opaque) -> list of (h_b, w_b, 4)
    uint8 GPU tensors: u8 = clamp(x*255 + 0.5, 0, 255) truncated, as torchvision's save_image.
    zero_transparent writes RGB = 0 where the alpha byte is 0."""
    _canvas_tensor(x_hat, 3, "unpack_rgba")
    if alpha is not None:
        _canvas_tensor(alpha, 1, "unpack_rgba", like=x_hat)
    B, _, hp, wp = x_hat.shape
    sizes = _check_sizes(sizes, B, hp, wp, "unpack_rgba")
    rt.check_gpu(x_hat, alpha)
    dev = x_hat.device
    xs = x_hat.contiguous().float()
    al = None if alpha is None else alpha.contiguous().float()
    flat = torch.empty(sum(h * w * 4 for h, w in sizes), dtype=torch.uint8, device=dev)
    outs, entries, off = [], [], 0
    for h, w in sizes:
        outs.append(flat[off:off + h * w * 4].view(h, w, 4))
        entries.append((flat.data_ptr() + off, h, w, 4 * w))
        off += h * w * 4
    descs = _upload_descs(entries, dev)
    _lib.call("rgbac_rgba_unpack", B, descs.data_ptr(), hp, wp, xs.data_ptr(), _lib.ptr(al),
              1 if zero_transparent else 0, _lib.stream_ptr(dev))
    return outs


def region_error(x, y, sizes, mask=None):
    """reconstruct_error restricted to each image's real rectangle: x, y (B,C,hp,wp) canvas
    tensors, mask (B,1,hp,wp) or None.  Returns (mse (B,) fp32, psnr (B,) fp32, sse (B,) fp64,
    n (B,) int64): squared error in fp64 over mask > 0 inside (h_b, w_b), n the term count,
    mse = sse / max(n, 1), psnr = 10 log10(1 / mse), 100 when sse == 0.  Bit-reproducible."""
    _canvas_tensor(x, None, "region_error")
    _canvas_tensor(y, x.shape[1], "region_error", like=x)
    if mask is not None:
        _canvas_tensor(mask, 1, "region_error", like=x)
    B, C, hp, wp = x.shape
    sizes = _check_sizes(sizes, B, hp, wp, "region_error")
    rt.check_gpu(x, y, mask)
    dev = x.device
    xs, ys = x.contiguous().float(), y.contiguous().float()
    ms = None if mask is None else mask.contiguous().float()
    descs = _upload_descs([(None, h, w, 0) for h, w in sizes], dev)
    nblk = _lib.load().rgbac_region_error_blocks(hp, wp)
    scratch = torch.empty((B * nblk * 2,), dtype=torch.float64, device=dev)
    sse = torch.empty((B,), dtype=torch.float64, device=dev)
    n = torch.empty((B,), dtype=torch.int64, device=dev)
    mse = torch.empty((B,), dtype=torch.float32, device=dev)
    psnr = torch.empty((B,), dtype=torch.float32, device=dev)
    _lib.call("rgbac_region_error", B, C, descs.data_ptr(), hp, wp, xs.data_ptr(), ys.data_ptr(),
              _lib.ptr(ms), scratch.data_ptr(), sse.data_ptr(), n.data_ptr(), mse.data_ptr(),
              psnr.data_ptr(), _lib.stream_ptr(dev))
    return mse, psnr, sse, n


def _check_pair(input, mask, who):
    if input is not None:
        _canvas_tensor(input, 3, who)
    _canvas_tensor(mask, 1, who, like=input)
    if mask.shape[2] < 1 or mask.shape[3] < 1:
        raise ValueError(f"{who}: empty image {tuple(mask.shape)}")


def compress_any(model, input, mask, pad="transparent", **kw):
    """`model.compress` for an input (B,3,H,W) / mask (B,1,H,W) of any H, W >= 1: both are padded
    to the 64-aligned canvas on the device, then coded.  Returns compress's dict plus
    "size": (H, W) and "pad"; ``**kw`` (coder=, chunk=) goes to compress."""
    _mode(pad)
    _check_pair(input, mask, "compress_any")
    rt.check_gpu(input, mask)
    H, W = int(input.shape[2]), int(input.shape[3])
    out = model.compress(pad_planes(input, pad), pad_planes(mask, pad), **kw)
    out["size"] = (H, W)
    out["pad"] = pad
    return out


def decompress_any(model, strings, shape, mask, size, pad="transparent", **kw):
    """`model.decompress` for a real-size mask (B,1,H,W), size = (H, W) as compress_any returned
    it: the mask is padded the same way, the reconstruction cropped back.  Returns
    {"x_hat": (B,3,H,W)}; ``**kw`` (coder=) goes to decompress."""
    _mode(pad)
    _check_pair(None, mask, "decompress_any")
    H, W = (int(v) for v in size)
    if (int(mask.shape[2]), int(mask.shape[3])) != (H, W):
        raise ValueError(f"decompress_any: the mask is {tuple(mask.shape[2:])}, size says {(H, W)}")
    hp, wp = padded_size(H, W)
    if tuple(int(v) for v in shape) != (hp // TILE, wp // TILE):
        raise ValueError(f"decompress_any: shape {tuple(shape)} does not belong to a {H}x{W} "
                         f"image (canvas {hp}x{wp}: {(hp // TILE, wp // TILE)})")
    rt.check_gpu(mask)
    x_hat = model.decompress(strings, shape, pad_planes(mask, pad), **kw)["x_hat"]
    return {"x_hat": x_hat[..., :H, :W].contiguous()}


@torch.no_grad()
def rgba_forward_any(masknet, net, images, pad="transparent"):
    """One evaluation pass (rgbac.rgba.rgba_forward, trainRGB.py:282-306) for a list of decoded
    RGBA images of any sizes.  Returns {"rgba": list of (h_b, w_b, 4) uint8 reconstructions,
    "mse" / "psnr" / "sse" / "n": per image over its real rectangle and true alpha > 0,
    "bpp": the forward's total rescaled from the canvas to the real pixels, "sizes", "pad",
    "canvas": the canvas tensors behind them}."""
    dev = next(net.parameters()).device
    p = pack_rgba(images, pad, device=dev)
    sizes = p["sizes"]
    img, recon_alpha, mse_c, bpp_c, _, out_mask = rgba_forward(masknet, net, p["masked"], p["alpha"])
    rgba = unpack_rgba(img, recon_alpha, sizes)
    mse, psnr, sse, n = region_error(p["masked"], img, sizes, mask=p["alpha"])
    B, _, hp, wp = img.shape
    # the forward divides the bits by B*hp*wp (:292-293): rescale to the pixels that exist
    scale = (B * hp * wp) / sum(h * w for h, w in sizes)
    bpp = (bpp_c.double() * scale).float()
    return {"rgba": rgba, "mse": mse, "psnr": psnr, "sse": sse, "n": n, "bpp": bpp,
            "sizes": sizes, "pad": pad,
            "canvas": {"masked": p["masked"], "alpha": p["alpha"], "x_hat": img,
                       "recon_alpha": recon_alpha, "mse": mse_c, "bpp_total": bpp_c,
                       "bpp_mask": out_mask[2]}}



@torch.no_grad()
def rgba_eval_any(masknet, net, images, msssim=True, masked_msssim=False):
    """The reference's test loop (trainRGB.py:282-317) for a list of decoded RGBA images of any
    sizes in ONE batched pass: every image gets the three figures the loop prints for it -- its
    own rate, PSNR and MS-SSIM -- as (B,) device tensors.

    Padding is decided per image on the device (rgbac_rgba_opaque; the flags are not read back):
    an opaque image is replicated, so its alpha stays all ones; the others are padded
    transparent.  The chain is rgba_forward's (masknet -> recon_alpha -> RGB net -> clamp) with
    both nets' per-image bits (``per_image=``).  Returns
      "bpp_rgb" = (y_bits + z_bits) / (h_b w_b) of the RGB net, "bpp_alpha" the same of masknet,
      "bpp" = bpp_rgb + (opaque_b ? 0 : bpp_alpha)   (:299-302, decided per image),
      "y_bits" / "z_bits" / "y_bits_alpha" / "z_bits_alpha": (B,) fp64,
      "mse" / "psnr" / "sse" / "n": region_error over the real rectangle and true alpha > 0,
      "ms_ssim" = ms_ssim_any(masked, x_hat, sizes, data_range=1) (:311), "ms_ssim_db" =
      -10 log10(1 - ms_ssim) (:312)   [msssim=True],
      "masked_ms_ssim": masked_ms_ssim_any with the true alpha as the mask [masked_msssim=True],
      "rgba": the uint8 reconstructions, "sizes", "opaque": device int32 (B,), "canvas" (as
      rgba_forward_any's; its bpp_total stays rgba_forward's batch-wide figure).
    An image's bits are all the bits of its canvas latents (what a coder spends), divided by its
    real pixel count.  With the MS-SSIM figures on, every side must exceed 160 (ValueError)."""
    dev = next(net.parameters()).device
    dev, sizes, entries, keep = _sources(images, dev, "rgba_eval_any")
    if msssim or masked_msssim:
        from .metrics.any_size import level_table, masked_ms_ssim_any, ms_ssim_any
        level_table(sizes, 5, 11)                    # too small an image: raise before any launch
    opaque = _opaque(dev, entries)
    p = _pack(dev, sizes, entries, None, opaque)
    bm, br = {}, {}
    img, recon_alpha, mse_c, bpp_c, _, out_mask = _chain(masknet, net, p["masked"], p["alpha"],
                                                        bits_mask=bm, bits_rgb=br)
    rgba = unpack_rgba(img, recon_alpha, sizes)
    mse, psnr, sse, n = region_error(p["masked"], img, sizes, mask=p["alpha"])
    npix = torch.tensor([h * w for h, w in sizes], dtype=torch.float64).to(dev)
    bpp_rgb = (br["y_bits"] + br["z_bits"]) / npix
    bpp_alpha = (bm["y_bits"] + bm["z_bits"]) / npix
    bpp = bpp_rgb + torch.where(opaque == 1, torch.zeros_like(bpp_alpha), bpp_alpha)
    out = {"rgba": rgba, "mse": mse, "psnr": psnr, "sse": sse, "n": n,
           "bpp": bpp.float(), "bpp_rgb": bpp_rgb.float(), "bpp_alpha": bpp_alpha.float(),
           "y_bits": br["y_bits"], "z_bits": br["z_bits"],
           "y_bits_alpha": bm["y_bits"], "z_bits_alpha": bm["z_bits"],
           "sizes": sizes, "opaque": opaque,
           "canvas": {"masked": p["masked"], "alpha": p["alpha"], "x_hat": img,
                      "recon_alpha": recon_alpha, "mse": mse_c, "bpp_total": bpp_c,
                      "bpp_mask": out_mask[2]}}
    if msssim:
        out["ms_ssim"] = ms_ssim_any(p["masked"], img, sizes, data_range=1.0)
        out["ms_ssim_db"] = -10.0 * torch.log10(1.0 - out["ms_ssim"])
    if masked_msssim:
        out["masked_ms_ssim"] = masked_ms_ssim_any(p["masked"], img, p["alpha"], sizes,
                                                   data_range=1.0)
    return out
