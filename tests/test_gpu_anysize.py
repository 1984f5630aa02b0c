"""GPU: images of any size (rgbac/anysize.py, csrc/anysize.hip).

Kernel level, against a few lines of torch / numpy on the CPU:
* rgbac_rgba_pack / rgbac_pad_nchw / rgbac_rgba_unpack are bit-exact (torch.equal);
* rgbac_region_error: n exact, sse within 2 (N + 3) 2^-53 relative of numpy's fp64 sum (N terms,
  all non-negative, so the bound holds for any summation order on either side), mse / psnr
  within one fp32 ulp of the fp64 value cast to fp32, bit-reproducible, padding never read into
  a result.
The model-level tests (compress_any / decompress_any / rgba_forward_any) are in
tests/test_gpu_models_anysize.py.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 7), (64, 64), (63, 65), (70, 130)]      # canvas 128 x 192; w % 4 = 1,3,0,1,2
HP, WP = 128, 192
MODES = ["transparent", "replicate"]
TORCH_MODE = {"transparent": "constant", "replicate": "replicate"}


def _pad_to(t, hp, wp, pad):
    """(..., h, w) CPU tensor -> (..., hp, wp): the torch composition the kernels replace."""
    h, w = t.shape[-2:]
    lead = t.shape[:-2]
    t4 = t.reshape(1, -1, h, w)
    out = F.pad(t4, (0, wp - w, 0, hp - h), mode=TORCH_MODE[pad])
    return out.reshape(*lead, hp, wp)


@pytest.fixture(scope="module")
def ragged_u8():
    """Random RGBA bytes for SIZES (alpha holds 0, 1 and 255), CPU (h, w, 4) uint8 tensors."""
    g = torch.Generator().manual_seed(11)
    imgs = []
    for h, w in SIZES:
        im = torch.randint(0, 256, (h, w, 4), generator=g, dtype=torch.uint8)
        u = torch.rand((h, w), generator=g)
        a = im[..., 3]
        a[u < 0.3] = 0
        a[(u >= 0.3) & (u < 0.4)] = 1
        a[(u >= 0.4) & (u < 0.6)] = 255
        imgs.append(im)
    assert {0, 1, 255} <= set(imgs[-1][..., 3].unique().tolist())
    return imgs


@pytest.fixture(scope="module")
def packed_ref(ragged_u8):
    """{pad: (alpha, rgb, masked)} on the canvas, composed image by image with torch on the CPU."""
    out = {}
    for pad in MODES:
        al, rgb, msk = [], [], []
        for im in ragged_u8:
            f = im.permute(2, 0, 1).float().div(255)
            fp = _pad_to(f, HP, WP, pad)
            a, c = fp[3:4], fp[:3]
            al.append(a)
            rgb.append(c)
            msk.append(torch.where(a > 0, c, a))
        out[pad] = (torch.stack(al), torch.stack(rgb), torch.stack(msk))
    return out


def _subviews(imgs, device, fill=0):
    """The images as views into ONE byte buffer: starts at 4, 8 or 12 bytes past a 16-byte
    boundary, at least 4 spare bytes between neighbours.  Returns (buffer, views, byte offsets)."""
    offs, off = [], 0
    for k, im in enumerate(imgs):
        off = (off + 4 + 15) // 16 * 16 + 4 * (k % 3 + 1)
        offs.append(off)
        off += im.numel()
    off += 4
    buf = torch.full((off,), fill, dtype=torch.uint8, device=device)
    views = []
    for im, o in zip(imgs, offs):
        v = buf[o:o + im.numel()].view(im.shape)
        if fill == 0:
            v.copy_(im)
        views.append(v)
    assert all(v.data_ptr() % 4 == 0 for v in views)
    assert all(v.data_ptr() % 16 != 0 for v in views)
    return buf, views, offs


def _descs(views, device):
    from rgbac import anysize as az
    return az._upload_descs([(v.data_ptr(), v.shape[0], v.shape[1], 4 * v.shape[1]) for v in views],
                            device)


@pytest.mark.parametrize("pad", MODES)
def test_rgba_pack_kernel_exact(device, ragged_u8, packed_ref, pad):
    from rgbac import _lib
    from rgbac import anysize as az
    buf, views, _ = _subviews(ragged_u8, device)
    descs = _descs(views, device)
    B = len(SIZES)
    want = packed_ref[pad]
    shapes = [(B, 1, HP, WP), (B, 3, HP, WP), (B, 3, HP, WP)]
    # all three outputs, then each output pointer null in turn
    for skip in (None, 0, 1, 2):
        outs = [None if k == skip else torch.full(s, float("nan"), device=device)
                for k, s in enumerate(shapes)]
        _lib.call("rgbac_rgba_pack", B, descs.data_ptr(), HP, WP, _lib.PAD_MODES[pad],
                  *[_lib.ptr(o) for o in outs], _lib.stream_ptr(device))
        for k, o in enumerate(outs):
            if o is not None:
                assert torch.equal(o.cpu(), want[k]), (pad, skip, k)
    # the Python entry point reads the same views in place (and CPU arrays after one upload)
    for src in (views, [im.numpy() for im in ragged_u8]):
        p = az.pack_rgba(src, pad=pad, device=device)
        assert p["sizes"] == SIZES and p["pad"] == pad
        assert torch.equal(p["alpha"].cpu(), want[0])
        assert torch.equal(p["rgb"].cpu(), want[1])
        assert torch.equal(p["masked"].cpu(), want[2])


@pytest.mark.parametrize("pad", MODES)
def test_pad_nchw_kernel_exact(device, pad):
    from rgbac import _lib
    from rgbac import anysize as az
    g = torch.Generator().manual_seed(3)
    for shape, (hp, wp) in [((2, 3, 50, 100), (64, 128)), ((1, 1, 64, 64), (64, 64))]:
        x = torch.randn(shape, generator=g)
        xd = x.to(device)
        out = torch.full(shape[:2] + (hp, wp), float("nan"), device=device)
        _lib.call("rgbac_pad_nchw", *shape, hp, wp, _lib.PAD_MODES[pad], xd.data_ptr(),
                  out.data_ptr(), _lib.stream_ptr(device))
        want = _pad_to(x, hp, wp, pad)
        assert torch.equal(out.cpu(), want), (pad, shape)
        assert torch.equal(az.pad_planes(xd, pad).cpu(), want)


def _unpack_values():
    """A ramp over [-0.5, 1.5], every tie (k + 0.5) / 255 and both fp32 neighbours of each."""
    t = torch.arange(255, dtype=torch.float32).add(0.5).div(255)
    inf = torch.tensor(float("inf"))
    return torch.cat([t, torch.nextafter(t, inf), torch.nextafter(t, -inf),
                      torch.linspace(-0.5, 1.5, 4096)])


@pytest.fixture(scope="module")
def unpack_case():
    """Canvas x_hat (B,3,HP,WP) / alpha (B,1,HP,WP) with the test values inside each rectangle
    and NaN outside it, and the expected bytes per image, (h, w, 4) with the alpha byte last."""
    pool = _unpack_values()
    x = torch.full((len(SIZES), 3, HP, WP), float("nan"))
    a = torch.full((len(SIZES), 1, HP, WP), float("nan"))
    want = []
    for b, (h, w) in enumerate(SIZES):
        n = 4 * h * w
        v = pool.roll(-97 * b).repeat(-(-n // pool.numel()))[:n].view(4, h, w)
        if b >= 2:
            assert n >= pool.numel()                            # every tie is in the rectangle
        x[b, :, :h, :w] = v[:3]
        a[b, :, :h, :w] = v[3:]
        want.append(v.mul(255).add(0.5).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous())
    return x, a, want


@pytest.mark.parametrize("with_alpha", [True, False])
@pytest.mark.parametrize("zero_transparent", [True, False])
def test_rgba_unpack_kernel_exact(device, unpack_case, with_alpha, zero_transparent):
    from rgbac import _lib
    from rgbac import anysize as az
    x, a, want = unpack_case
    exp = []
    for wv in want:
        e = wv.clone()
        if not with_alpha:
            e[..., 3] = 255
        elif zero_transparent:
            e[..., :3][e[..., 3] == 0] = 0
        exp.append(e)
    if with_alpha:
        assert any((e[..., 3] == 0).any() for e in exp)
    xd, ad = x.to(device), (a.to(device) if with_alpha else None)
    guard = 0xA5
    buf, views, offs = _subviews(want, device, fill=guard)
    descs = _descs(views, device)
    _lib.call("rgbac_rgba_unpack", len(SIZES), descs.data_ptr(), HP, WP, xd.data_ptr(),
              _lib.ptr(ad), int(zero_transparent), _lib.stream_ptr(device))
    for v, e in zip(views, exp):
        assert torch.equal(v.cpu(), e), tuple(e.shape)
    # bytes outside each image's h*w*4 stay untouched
    inside = torch.zeros(buf.numel(), dtype=torch.bool)
    for o, e in zip(offs, exp):
        inside[o:o + e.numel()] = True
    assert bool((buf.cpu()[~inside] == guard).all()) and int((~inside).sum()) >= 4 * (len(SIZES) + 1)
    outs = az.unpack_rgba(xd, ad, SIZES, zero_transparent=zero_transparent)
    for o, e in zip(outs, exp):
        assert o.dtype == torch.uint8 and o.is_cuda and torch.equal(o.cpu(), e)


def _region_ref(x, y, sizes, mask=None):
    """numpy fp64 reference of region_error on CPU canvas tensors."""
    sse, n, mse, psnr = [], [], [], []
    C = x.shape[1]
    for b, (h, w) in enumerate(sizes):
        d = x[b, :, :h, :w].double().numpy() - y[b, :, :h, :w].double().numpy()
        sel = np.ones((h, w), dtype=bool) if mask is None else (mask[b, 0, :h, :w].numpy() > 0)
        s = float(np.sum((d * d)[:, sel]))
        k = C * int(sel.sum())
        m = s / max(k, 1)
        sse.append(s)
        n.append(k)
        mse.append(np.float32(m))
        psnr.append(np.float32(10.0 * np.log10(1.0 / m)) if s > 0 else np.float32(100.0))
    return sse, n, mse, psnr


def _check_region(got, ref):
    mse, psnr, sse, n = (t.cpu().numpy() for t in got)
    r_sse, r_n, r_mse, r_psnr = ref
    assert mse.dtype == np.float32 and psnr.dtype == np.float32
    assert sse.dtype == np.float64 and n.dtype == np.int64
    for b in range(len(r_n)):
        assert int(n[b]) == r_n[b], b
        assert abs(sse[b] - r_sse[b]) <= 2 * (r_n[b] + 3) * 2.0 ** -53 * r_sse[b], (b, sse[b], r_sse[b])
        assert abs(float(mse[b]) - float(r_mse[b])) <= float(np.spacing(r_mse[b])), (b, mse[b], r_mse[b])
        assert abs(float(psnr[b]) - float(r_psnr[b])) <= float(np.spacing(r_psnr[b])), (b, psnr[b])


@pytest.mark.parametrize("masked", [False, True])
def test_region_error_kernel(device, masked):
    from rgbac import anysize as az
    g = torch.Generator().manual_seed(5)
    B, C = len(SIZES), 3
    nan = float("nan")
    x, y = torch.full((B, C, HP, WP), nan), torch.full((B, C, HP, WP), nan)
    m = torch.full((B, 1, HP, WP), nan) if masked else None
    for b, (h, w) in enumerate(SIZES):
        x[b, :, :h, :w] = torch.rand((C, h, w), generator=g)
        y[b, :, :h, :w] = torch.rand((C, h, w), generator=g)
        if masked:
            mb = torch.rand((1, h, w), generator=g)
            mb[mb < 0.35] = 0
            m[b, :, :h, :w] = 0 if b == 1 else mb            # image 1: fully masked out
    ref = _region_ref(x, y, SIZES, m)
    if masked:
        assert ref[1][1] == 0 and ref[2][1] == 0 and ref[3][1] == 100
    xd, yd = x.to(device), y.to(device)
    md = m.to(device) if masked else None
    got = az.region_error(xd, yd, SIZES, mask=md)
    _check_region(got, ref)
    assert not any(bool(torch.isnan(t.double()).any()) for t in got)       # the poisoned padding
    again = az.region_error(xd, yd, SIZES, mask=md)
    assert all(torch.equal(p, q) for p, q in zip(got, again))
