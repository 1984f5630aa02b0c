"""RGB codec (reference: models/AutoEncoderRGB_Journal.py), MI355X hot path.

``AutoEncoder().forward(input, mask, reconmask, me1, me2, me3, me4)`` returns
``(x_hat, mse_loss, total_bpp, y_bpp, z_bpp)`` like the reference (:203-296).
Same submodule names / parameter shapes, so reference checkpoints load with
``load_state_dict`` (compressai CDF buffers are resized like compressai does).

Compute dtype: ``model.compute_dtype`` = torch.float32 (parity mode, fp32
MFMA) by default; torch.bfloat16 selects the throughput mode (bf16 storage
and MFMA inputs, fp32 accumulation/epilogues).  With grad enabled (training),
forward builds an autograd graph whose backward is HIP (rgbac/train_forward.py);
under torch.no_grad() it runs the fused, grouped inference path.
"""
import ctypes
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from .. import runtime as rt
from ..entropy import EntropyBottleneck, GaussianConditional
from ..layers.SupplyMask import SupplyMaskToTransform, mask_pyramid
from ..layers.TransformRGB import Analysis_transform, Synthesis_transform
from ..layers._blocks import conv, conv3x3, deconv, subpel_conv3x3  # noqa: F401
from ._latent import latent_path

SCALES_MIN = 0.11
SCALES_MAX = 256
SCALES_LEVELS = 64


def ste_round(x):
    """:31-32"""
    return torch.round(x) - x.detach() + x


def get_scale_table(min=SCALES_MIN, max=SCALES_MAX, levels=SCALES_LEVELS):
    return torch.exp(torch.linspace(math.log(min), math.log(max), levels))


def reconstruct_error(input, output, input_mask, output_mask=None):
    """:36-64 (host-side helper kept for API parity; the forward computes it in
    rgbac_finalize)."""
    m = (input_mask.expand(-1, 3, -1, -1) > 0.0).float()
    se = F.mse_loss(input * m, output * m, reduction="none").sum(dim=(1, 2, 3))
    cnt = torch.clamp(m.sum(dim=(1, 2, 3)), min=1)
    return torch.mean(se / cnt)


# RGBAC_FUSED_PROLOGUE=0: the separate pyramid / NHWC / zero-fill launches (A/B and the
# bit-identity test)
FUSED_PROLOGUE = os.environ.get("RGBAC_FUSED_PROLOGUE", "1") != "0"


class GeometryError(RuntimeError, ValueError):
    """Input size the reference's forward cannot process either (RuntimeError like the
    reference's own failure, ValueError for callers of round 1's API)."""


def check_geometry(H, W):
    """The whole-model forward needs H, W multiples of 64, exactly like the reference: the
    hyper-synthesis output is 8*ceil(H/64) x 8*ceil(W/64) and the slice loop concatenates it
    with the H/8 x W/8 latent slices (AutoEncoderRGB_Journal.py:242,248;
    AutoEncoderMask_Journal.py:271,276), which raises in torch.cat unless H/8, W/8 are
    multiples of 8 -- the mu/scale crop (:245,:251) never makes e.g. 96x96 work.  The L3
    layers (Analysis/Synthesis_transform, window attention) accept multiples of 32."""
    if H % 64 or W % 64 or H <= 0 or W <= 0:
        raise GeometryError(
            f"H and W must be positive multiples of 64 (got {H}x{W}): the reference's slice loop "
            f"concatenates the {8 * -(-H // 64)}x{8 * -(-W // 64)} hyper-synthesis output with "
            f"the {H // 8}x{W // 8} latent (AutoEncoderRGB_Journal.py:242)")


class _CompressionModelMixin:
    """The parts of compressai.models.CompressionModel the reference relies on."""

    def aux_loss(self):
        return sum(m.loss() for m in self.modules() if isinstance(m, EntropyBottleneck))

    def update(self, scale_table=None, force=False):
        """:306-311: GaussianConditional scale table + CDFs, then (CompressionModel.update)
        every EntropyBottleneck's CDFs."""
        if scale_table is None:
            scale_table = get_scale_table()
        updated = self.gaussian_conditional.update_scale_table(scale_table, force=force)
        for m in self.modules():
            if isinstance(m, EntropyBottleneck):
                updated |= m.update(force=force)
        return updated

    def load_state_dict(self, state_dict, strict=True):
        # compressai resizes the (initially empty) CDF buffers before loading
        for name, buf in self.named_buffers():
            base = name.rsplit(".", 1)[-1]
            if base in ("_offset", "_quantized_cdf", "_cdf_length", "scale_table") \
                    and name in state_dict and state_dict[name].shape != buf.shape:
                mod = self.get_submodule(name.rsplit(".", 1)[0])
                setattr(mod, base, torch.empty_like(state_dict[name], device=buf.device))
        return nn.Module.load_state_dict(self, state_dict, strict=strict)


def _stack3(cin, cout=8):
    return nn.Sequential(conv(cin, 224, stride=1, kernel_size=3), nn.GELU(),
                         conv(224, 128, stride=1, kernel_size=3), nn.GELU(),
                         conv(128, cout, stride=1, kernel_size=3))


def _hyper_synthesis(M):
    return nn.Sequential(subpel_conv3x3(192, 192, 2), nn.GELU(), conv3x3(192, 224), nn.GELU(),
                         subpel_conv3x3(224, 256, 2), nn.GELU(), conv3x3(256, 288), nn.GELU(),
                         subpel_conv3x3(288, M, 2))


def _hyper_analysis(M):
    return nn.Sequential(conv3x3(M, 320, stride=2), nn.GELU(), conv3x3(320, 288), nn.GELU(),
                         conv3x3(288, 256, stride=2), nn.GELU(), conv3x3(256, 224), nn.GELU(),
                         conv3x3(224, 192, stride=2))


def finalize(mode, x, x_hat, mask, ypart, zpart, x_hat_nchw=None):
    """rgbac_finalize_ex -> fp32 [mse, bpp, y_bpp, z_bpp] on device; with ``x_hat_nchw`` (fp32
    [B, cx, H, W]) the same pass also writes x_hat's NCHW copy.  (A one-launch form through a
    last-arriving-block ticket measured slower, 20.5 vs 16.4 us: DESIGN 15e.)"""
    B, cx, H, W = x.shape
    dev = x.device
    scratch = torch.empty(_lib.finalize_scratch_doubles(B, H, W), dtype=torch.float64,
                          device=dev)
    out = torch.empty(4, dtype=torch.float32, device=dev)
    _lib.call("rgbac_finalize_ex", _lib.dtype_code(x_hat.t.dtype), mode, B, cx, H, W,
              x.data_ptr(), x_hat.ptr(), x_hat.ldc, _lib.ptr(mask), ypart.data_ptr(),
              ypart.numel(), zpart.data_ptr(), zpart.numel(), scratch.data_ptr(),
              out.data_ptr(), _lib.ptr(x_hat_nchw), _lib.stream_ptr(dev))
    return out


def forward_prologue(model, x, dt, reconmask, levels=4):
    """The forward's head in ONE launch (rgbac_forward_prologue, :209-217): the decoder mask
    pyramid of round(reconmask * 255) / 255, x's NHWC copy, and the zero fill of the slice
    loop's bits partials.  -> (xf, md, ypart)."""
    B, C, H, W = x.shape
    dev = x.device
    a = reconmask.contiguous().float()
    assert a.shape == (B, 1, H, W), "reconmask must be (B, 1, H, W) like the input"
    xf = rt.Feat(torch.empty((B, H, W, rt.round_up(C, 8)), dtype=dt, device=dev), C)
    md, h, w = [], H, W
    for _ in range(levels):
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        md.append(torch.empty((B, 1, h, w), dtype=torch.float32, device=dev))
    rounded = torch.empty_like(a)
    from ._latent import ypart_slots
    ns, nslot = ypart_slots(model, B, H // 8, W // 8)        # x1..x3: three stride-2 convs
    zero = torch.empty((ns, nslot), dtype=torch.float64, device=dev)
    ptrs = (ctypes.c_void_p * levels)(*[o.data_ptr() for o in md])
    _lib.call("rgbac_forward_prologue", _lib.dtype_code(dt), B, C, H, W, x.data_ptr(),
              xf.t.data_ptr(), xf.ldc, a.data_ptr(), 1, rounded.data_ptr(), levels, ptrs,
              zero.data_ptr(), zero.numel(), _lib.stream_ptr(dev))
    return xf, md, zero


class AutoEncoder(_CompressionModelMixin, nn.Module):
    def __init__(self):
        super().__init__()
        self.N = 192
        self.M = 80
        self.Encoder = Analysis_transform(self.N, self.M)
        self.Decoder = Synthesis_transform(self.N, self.M)
        self.EncMakeMask = SupplyMaskToTransform()
        self.DecMakeMask = SupplyMaskToTransform()
        self.num_slices = 10
        self.max_support_slices = 5
        self.h_a = _hyper_analysis(self.M)
        self.h_mean_s = _hyper_synthesis(self.M)
        self.h_scale_s = _hyper_synthesis(self.M)
        ns = self.num_slices
        cs = self.M // ns
        self.cc_mean_transforms = nn.ModuleList(
            _stack3(self.M + cs * min(i, 5), cs) for i in range(ns))
        self.cc_scale_transforms = nn.ModuleList(
            _stack3(self.M + cs * min(i, 5), cs) for i in range(ns))
        self.lrp_transforms = nn.ModuleList(
            _stack3(self.M + cs * min(i + 1, 6), cs) for i in range(ns))
        self.entropy_bottleneck = EntropyBottleneck(192)
        self.gaussian_conditional = GaussianConditional(None)
        self.compute_dtype = torch.float32

    def compress(self, input, mask, *, coder="host", chunk=256):
        """:312-371 on the HIP path (rgbac/models/_codec.py) + the host rANS coder.
        coder="device" writes the chunked stream format instead and codes it on the GPU
        (chunks of ``chunk`` symbols; rgbac/ans.py); the result then holds "coder": "device".
        ``chunk`` trades rate for speed: every chunk costs up to 12 bytes over the single stream
        and is one GPU lane.  256 was the fastest of 256 / 1024 / 4096 at both measured
        configurations at ~0.4 bit per latent symbol; a larger chunk cuts
        that cost in proportion and is slower."""
        from ._codec import compress
        return compress(self, input, mask, coder=coder, chunk=chunk)

    def decompress(self, strings, shape, mask, *, coder="host"):
        """:373-416; decodes the batch of len(strings[1]) images (the reference: 1).  Pass the
        coder compress was called with."""
        from ._codec import decompress
        return decompress(self, strings, shape, mask, coder=coder)

    def set_compute_dtype(self, dtype):
        assert dtype in (torch.float32, torch.bfloat16)
        self.compute_dtype = dtype
        return self

    def forward(self, input, mask, reconmask, me1, me2, me3, me4, *, noise_z=None,
                noise_y=None, debug=None, per_image=None):
        """``per_image``: a dict; the evaluation forward fills it with "y_bits" and "z_bits",
        (B,) fp64 -- every image's own share of the bits behind the returned bpp (latent_path).
        Absent, the forward launches exactly what it launches without this argument."""
        rt.check_gpu(input, mask, reconmask, me2, me3)
        B, _, H, W = input.shape
        check_geometry(H, W)
        if debug is None and torch.is_grad_enabled() and \
                any(p.requires_grad for p in self.parameters()):
            if per_image is not None:
                raise ValueError("per_image= is an evaluation option: call the model under "
                                 "torch.no_grad()")
            # training step (trainRGB.py:178-198): autograd graph over the HIP kernels
            from ..train_forward import rgb_forward_train
            return rgb_forward_train(self, input, mask, reconmask, me2, me3, noise_z, noise_y)
        dt = self.compute_dtype
        with torch.no_grad():
            x = input.contiguous().float()
            # reconmask = round(reconmask*255)/255 ; md1..md4 = DecMakeMask(reconmask)  (:212-215):
            # only the decoder reads md, so the pyramid may run on a side stream beside the
            # encoder (rt.side_streams; off by default: the fork / join measured slower)
            main, side = rt.side_streams(x.device)
            ypart = None
            if side is main and FUSED_PROLOGUE:
                # pyramid + NHWC copy + bits-partial zero fill: one launch
                xf, md, ypart = forward_prologue(self, x, dt, reconmask)
            else:
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    _, md = mask_pyramid(reconmask, 4, round255=True)
                for t in md:
                    t.record_stream(main)
                xf = rt.to_nhwc(x, dt)
            y = self.Encoder.nhwc(xf, me2, me3)                                  # :217
            yh, ypart, zpart = latent_path(self, y, self.training, noise_z, noise_y, debug,
                                           ypart=ypart, per_image=per_image)
            main.wait_stream(side)
            xh = self.Decoder.nhwc(yh, md[1], md[2])                              # :273
            # x_hat's NCHW copy written by the loss pass itself (one read of x_hat)
            x_hat = torch.empty((B, xh.C, H, W), dtype=torch.float32, device=x.device)
            out = finalize(0, x, xh, mask.contiguous().float(), ypart, zpart,     # :280-295
                           x_hat_nchw=x_hat)
        if debug is not None:
            debug.update(y=y)
        return x_hat, out[0], out[1], out[2], out[3]
