"""SSIM / MS-SSIM (reference: metrics/ms_ssim_torch.py:5-259) on the HIP path.

Same functions and arguments as the reference: ``ssim(X, Y, win_size=11, win_sigma=1.5,
win=None, data_range=255, size_average=True, full=False)``, ``ms_ssim(..., weights=None)`` and
the ``SSIM`` / ``MS_SSIM`` modules.  Per scale one tile launch computes the valid ssim/cs maps
and their per-image means (csrc/msssim.hip); the 2x2 average pool and the final weighted
product are kernels too, so the metric never leaves the GPU (trainRGB.py:308-311 evaluates it
on the CPU).  Inputs must be CUDA tensors; they are computed in fp32.

The functions are differentiable with respect to X and Y, so ``1 - ms_ssim(x, x_hat,
data_range=1.0)`` is a training distortion (trainRGB.py:183).  With grad mode off, or when
neither input requires grad, the launches are the ones above and nothing is kept.  Otherwise
the same launches run inside a ``torch.autograd.Function`` that keeps the per-level planes and
the per-level cs / ssim values; its backward is csrc/msssim_bwd.hip: one combine-backward
launch, then one tile launch per level, coarse to fine, with the average pool's adjoint fused
in.  No atomics, fixed summation order: the gradient is bit-reproducible.  The window and the
weights live on the device in a per-(device, values) cache, so a warmed-up call makes no
host-to-device copy and the loss and its backward can be captured in a HIP graph.
"""
import torch

from .. import _lib
from .. import runtime as rt

_TILE = 16
_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)      # :163-164


def _fspecial_gauss_1d(size, sigma):
    """:5-18 (host constant, built exactly as the reference builds it)."""
    coords = torch.arange(size).to(dtype=torch.float)
    coords -= size // 2
    g = torch.exp(-(coords ** 2) / (2 * sigma ** 2))
    g /= g.sum()
    return g.unsqueeze(0).unsqueeze(0)


def _check(X, Y, win_size):
    if len(X.shape) != 4:
        raise ValueError('Input images must 4-d tensor.')
    if not X.type() == Y.type():
        raise ValueError('Input images must have the same dtype.')
    if not X.shape == Y.shape:
        raise ValueError('Input images must have the same dimensions.')
    if not (win_size % 2 == 1):
        raise ValueError('Window size must be odd.')
    rt.check_gpu(X, Y)


_CONSTS = {}


def _cached(make, key, device):
    """fp32 1-D device copy of a small host constant, made once per (device, key): a pageable
    host-to-device copy per call cannot be captured in a graph."""
    k = (device, key)
    if k not in _CONSTS:
        _CONSTS[k] = make().reshape(-1).to(device=device, dtype=torch.float32).contiguous()
    return _CONSTS[k]


def _device_const(t, device):
    """A given window / weight vector (tensor or sequence) as an fp32 1-D device tensor: cached
    by its values when it lives on the host, used as it is when already on a GPU."""
    if torch.is_tensor(t) and t.is_cuda:
        return t.detach().reshape(-1).to(device=device, dtype=torch.float32).contiguous()
    t = torch.as_tensor(t).detach().to(torch.float32).reshape(-1)
    return _cached(lambda: t, ("values",) + tuple(t.tolist()), device)


def _win_1d(win, win_size, win_sigma, device):
    if win is None:
        return _cached(lambda: _fspecial_gauss_1d(win_size, win_sigma),
                       ("gauss", int(win_size), float(win_sigma)), device)
    return _device_const(win[0] if win.dim() == 4 else win, device)


def _needs_grad(*ts):
    return torch.is_grad_enabled() and any(t.requires_grad for t in ts)


def _ssim_level(X, Y, w1d, data_range, K=(0.01, 0.03)):
    """One scale of _ssim (:36-83) with size_average=False -> (ssim[B], cs[B])."""
    B, C, H, W = X.shape
    ws = w1d.numel()
    nt = (-(-(H - ws + 1) // _TILE)) * (-(-(W - ws + 1) // _TILE))
    part = torch.empty((B * C * nt * 2,), dtype=torch.float32, device=X.device)
    s = torch.empty((B,), dtype=torch.float32, device=X.device)
    cs = torch.empty((B,), dtype=torch.float32, device=X.device)
    c1 = (K[0] * data_range) ** 2
    c2 = (K[1] * data_range) ** 2
    _lib.call("rgbac_ssim_level", B, C, H, W, ws, X.data_ptr(), Y.data_ptr(), w1d.data_ptr(),
              c1, c2, part.data_ptr(), s.data_ptr(), cs.data_ptr(), _lib.stream_ptr(X.device))
    return s, cs


def _pool(X):
    B, C, H, W = X.shape
    ph, pw = H % 2, W % 2
    out = torch.empty((B, C, (H + 2 * ph - 2) // 2 + 1, (W + 2 * pw - 2) // 2 + 1),
                      dtype=torch.float32, device=X.device)
    _lib.call("rgbac_avgpool2", B * C, H, W, X.data_ptr(), out.data_ptr(),
              _lib.stream_ptr(X.device))
    return out


def ssim(X, Y, win_size=11, win_sigma=1.5, win=None, data_range=255, size_average=True,
         full=False):
    """:86-132"""
    if win is not None:
        win_size = win.shape[-1]
    _check(X, Y, win_size)
    w1d = _win_1d(win, win_size, win_sigma, X.device)
    X, Y = X.contiguous().float(), Y.contiguous().float()
    if _needs_grad(X, Y):
        ssim_val, cs = _SSIMLevelFn.apply(X, Y, w1d, data_range)
    else:
        ssim_val, cs = _ssim_level(X, Y, w1d, data_range)
    if size_average:
        ssim_val = ssim_val.mean()
        cs = cs.mean()
    if full:
        return ssim_val, cs
    return ssim_val


def ms_ssim(X, Y, win_size=11, win_sigma=1.5, win=None, data_range=255, size_average=True,
            full=False, weights=None):
    """:135-194 (including the broadcast of ssim_val ** w[-1] into every level's factor)."""
    if win is not None:
        win_size = win.shape[-1]
    _check(X, Y, win_size)
    wts = _device_const(_WEIGHTS if weights is None else weights, X.device)
    w1d = _win_1d(win, win_size, win_sigma, X.device)
    X, Y = X.contiguous().float(), Y.contiguous().float()
    if _needs_grad(X, Y):
        return _MSSSIMFn.apply(X, Y, w1d, wts, data_range, size_average)
    mean, per_image, _ = _ms_ssim_forward(X, Y, w1d, wts, data_range)
    return mean if size_average else per_image


def _ms_ssim_forward(X, Y, w1d, wts, data_range, keep=False):
    """The launches of ms_ssim -> (mean, per_image, saved); saved (keep=True) holds what the
    backward reads: the (X, Y) planes of every level, mcs and the last level's ssim."""
    levels = wts.shape[0]
    B = X.shape[0]
    mcs = torch.empty((levels, B), dtype=torch.float32, device=X.device)
    ssim_val = None
    planes = []
    for i in range(levels):
        ssim_val, cs = _ssim_level(X, Y, w1d, data_range)
        mcs[i].copy_(cs)
        if keep:
            planes += [X, Y]
        if i + 1 < levels:     # the reference's last pool feeds nothing
            X, Y = _pool(X), _pool(Y)
    per_image = torch.empty((B,), dtype=torch.float32, device=X.device)
    mean = torch.empty((), dtype=torch.float32, device=X.device)
    _lib.call("rgbac_msssim_combine", levels, B, mcs.data_ptr(), ssim_val.data_ptr(),
              wts.data_ptr(), per_image.data_ptr(), mean.data_ptr(), _lib.stream_ptr(X.device))
    return mean, per_image, (planes + [mcs, ssim_val] if keep else None)


def _consts(data_range, K=(0.01, 0.03)):
    return (K[0] * data_range) ** 2, (K[1] * data_range) ** 2


def _level_bwd(X, Y, w1d, c1, c2, u_cs, u_ssim, gcx, gcy, want_dx, want_dy=True):
    """rgbac_ssim_level_bwd of one level -> (dX or None, dY or None)."""
    B, C, H, W = X.shape
    dX = torch.empty_like(X) if want_dx else None
    dY = torch.empty_like(Y) if want_dy else None
    _lib.call("rgbac_ssim_level_bwd", B, C, H, W, w1d.numel(), X.data_ptr(), Y.data_ptr(),
              w1d.data_ptr(), c1, c2, _lib.ptr(u_cs), _lib.ptr(u_ssim), _lib.ptr(gcx),
              _lib.ptr(gcy), _lib.ptr(dX), _lib.ptr(dY), _lib.stream_ptr(X.device))
    return dX, dY


def _f32c(g):
    return None if g is None else g.contiguous().float()


class _SSIMLevelFn(torch.autograd.Function):
    """(ssim[B], cs[B]) of one scale, differentiable in X and Y (rgbac_ssim_level_bwd)."""

    @staticmethod
    def forward(ctx, X, Y, w1d, data_range):
        ctx.set_materialize_grads(False)
        ctx.data_range = data_range
        ctx.save_for_backward(X, Y, w1d)
        return _ssim_level(X, Y, w1d, data_range)

    @staticmethod
    def backward(ctx, g_ssim, g_cs):
        X, Y, w1d = ctx.saved_tensors
        if g_ssim is None and g_cs is None:
            return None, None, None, None
        dX, dY = _level_bwd(X, Y, w1d, *_consts(ctx.data_range), _f32c(g_cs), _f32c(g_ssim),
                            None, None, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return dX, dY, None, None


class _MSSSIMFn(torch.autograd.Function):
    """ms_ssim, differentiable in X and Y: the forward is _ms_ssim_forward (the no-grad path's
    launches, so the same bits); the backward is rgbac_msssim_combine_bwd, then one
    rgbac_ssim_level_bwd per level from the coarsest up, each taking the coarser level's
    gradient through the fused average-pool adjoint."""

    @staticmethod
    def forward(ctx, X, Y, w1d, wts, data_range, size_average):
        mean, per_image, saved = _ms_ssim_forward(X, Y, w1d, wts, data_range, keep=True)
        ctx.meta = (data_range, size_average)
        ctx.save_for_backward(w1d, wts, *saved)
        return mean if size_average else per_image

    @staticmethod
    def backward(ctx, g):
        data_range, size_average = ctx.meta
        w1d, wts, *planes, mcs, ssim_last = ctx.saved_tensors
        levels, B = mcs.shape
        g = _f32c(g)
        u = torch.empty((levels, B), dtype=torch.float32, device=g.device)
        _lib.call("rgbac_msssim_combine_bwd", levels, B, mcs.data_ptr(), ssim_last.data_ptr(),
                  wts.data_ptr(), g.data_ptr(), 1 if size_average else 0, u.data_ptr(),
                  _lib.stream_ptr(g.device))
        c1, c2 = _consts(data_range)
        want_dx, want_dy = ctx.needs_input_grad[:2]
        dX = dY = None
        for i in reversed(range(levels)):
            last = i == levels - 1
            dX, dY = _level_bwd(planes[2 * i], planes[2 * i + 1], w1d, c1, c2,
                                None if last else u[i], u[i] if last else None, dX, dY,
                                want_dx, want_dy)
        return dX, dY, None, None, None, None


class SSIM(torch.nn.Module):
    """:197-217"""

    def __init__(self, win_size=11, win_sigma=1.5, data_range=None, size_average=True,
                 channel=3):
        super().__init__()
        self.win = _fspecial_gauss_1d(win_size, win_sigma).repeat(channel, 1, 1, 1)
        self.size_average = size_average
        self.data_range = data_range

    def forward(self, X, Y):
        return ssim(X, Y, win=self.win, data_range=self.data_range,
                    size_average=self.size_average)


class MS_SSIM(torch.nn.Module):
    """:219-259"""

    def __init__(self, win_size=11, win_sigma=1.5, data_range=None, size_average=True,
                 channel=3, weights=None):
        super().__init__()
        self.win = _fspecial_gauss_1d(win_size, win_sigma).repeat(channel, 1, 1, 1)
        self.size_average = size_average
        self.data_range = data_range
        self.weights = weights

    def forward(self, X, Y):
        return ms_ssim(X, Y, win=self.win, size_average=self.size_average,
                       data_range=self.data_range, weights=self.weights)
