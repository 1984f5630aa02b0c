"""GPU, model level: images of any size through the codecs (rgbac/anysize.py).

compress_any / decompress_any equal the codec run on torch-padded tensors bit for bit (compress
and decompress run under rt.fixed_tiles()), and rgba_forward_any's per-image figures equal
region_error recomputed on the CPU from the canvas tensors of the forward, to the tolerances of
tests/test_gpu_anysize.py (the kernel-level tests, whose helpers are used here).

These tests build two models; they live in a file of their own that sorts behind
tests/test_gpu_data.py, whose loader-throughput test reads lower the more model-level GPU work
the process has done before it (DESIGN.md sections 19 and 20).
"""
import numpy as np
import pytest
import torch

from test_gpu_anysize import MODES, _check_region, _pad_to, _region_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codec_net():
    from rgbac.models.AutoEncoderRGB_Journal import AutoEncoder
    torch.manual_seed(234)
    net = AutoEncoder().eval()
    net.update()
    return net


def _planes(B, H, W, seed):
    """masked RGB (B,3,H,W) and alpha (B,1,H,W): alpha > 0 except a corner block per image."""
    g = torch.Generator().manual_seed(seed)
    x = torch.round(torch.rand((B, 3, H, W), generator=g) * 255) / 255
    a = torch.round(torch.rand((B, 1, H, W), generator=g) * 254 + 1) / 255
    for b in range(B):
        a[b, :, : H // 4, : W // (4 + b)] = 0
    return torch.where(a > 0, x, a), a


def test_any_is_identity_on_aligned_sizes(device, codec_net):
    from rgbac import anysize as az
    net = codec_net.to(device).set_compute_dtype(torch.float32)
    x, a = (t.to(device) for t in _planes(2, 64, 128, seed=2))
    want = net.compress(x, a)
    got = az.compress_any(net, x, a)
    assert got["strings"] == want["strings"] and got["shape"] == want["shape"]
    assert got["size"] == (64, 128) and got["pad"] == "transparent"
    rec = az.decompress_any(net, got["strings"], got["shape"], a, got["size"])["x_hat"]
    assert torch.equal(rec, net.decompress(want["strings"], want["shape"], a)["x_hat"])


@pytest.mark.parametrize("pad,coder", [("transparent", "host"), ("replicate", "host"),
                                       ("transparent", "device")])
def test_any_padding_is_what_it_says(device, codec_net, pad, coder):
    from rgbac import anysize as az
    net = codec_net.to(device).set_compute_dtype(torch.float32)
    H, W = 50, 100
    x, a = _planes(2, H, W, seed=7)
    xp, ap = _pad_to(x, 64, 128, pad).to(device), _pad_to(a, 64, 128, pad).to(device)
    x, a = x.to(device), a.to(device)
    want = net.compress(xp, ap, coder=coder)
    got = az.compress_any(net, x, a, pad=pad, coder=coder)
    assert got["strings"] == want["strings"] and got["shape"] == want["shape"] == torch.Size((1, 2))
    assert got["size"] == (H, W) and got["pad"] == pad
    rec = az.decompress_any(net, got["strings"], got["shape"], a, got["size"], pad=pad,
                            coder=coder)["x_hat"]
    full = net.decompress(want["strings"], want["shape"], ap, coder=coder)["x_hat"]
    assert rec.shape == (2, 3, H, W) and rec.is_contiguous()
    assert torch.equal(rec, full[..., :H, :W])


def test_any_round_trip(device, codec_net):
    from rgbac import anysize as az
    net = codec_net.to(device).set_compute_dtype(torch.float32)
    x, a = (t.to(device) for t in _planes(1, 50, 100, seed=8))
    out = az.compress_any(net, x, a, pad="replicate")
    rec = az.decompress_any(net, out["strings"], out["shape"], a, out["size"], pad=out["pad"])["x_hat"]
    assert rec.shape == (1, 3, 50, 100)
    assert float(rec.min()) >= 0.0 and float(rec.max()) <= 1.0
    with pytest.raises(ValueError):                             # a shape of another canvas
        az.decompress_any(net, out["strings"], (2, 2), a, out["size"])
    with pytest.raises(ValueError):                             # a mask that is not `size`
        az.decompress_any(net, out["strings"], out["shape"], a[..., :49, :], out["size"])


@pytest.fixture(scope="module")
def rgba_nets(codec_net):
    """(RGB codec, alpha codec): the RGB codec is the one the bitstream tests above use."""
    from rgbac.models.AutoEncoderMask_Journal import AutoEncoder as MaskNet
    torch.manual_seed(235)
    return codec_net, MaskNet().eval()


RAGGED = [(50, 100), (64, 90)]                                  # canvas 64 x 128


def _rgba_images(opaque, seed=21):
    """uint8 (h, w, 4): random RGB; alpha an ellipse over most of the image (255 inside with a
    soft rim, 0 outside), or 255 everywhere."""
    g = torch.Generator().manual_seed(seed)
    imgs = []
    for h, w in RAGGED:
        im = torch.randint(0, 256, (h, w, 4), generator=g, dtype=torch.uint8)
        if opaque:
            im[..., 3] = 255
        else:
            yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
            r = (((yy - h / 2) / (0.48 * h)) ** 2 + ((xx - w / 2) / (0.48 * w)) ** 2).sqrt()
            im[..., 3] = torch.clamp((1 - r) * 12, 0, 1).mul(255).round().to(torch.uint8)
            assert float((im[..., 3] > 0).float().mean()) > 0.6
        imgs.append(im)
    return imgs


def _ulp32(v):
    return float(np.spacing(np.float32(v)))


def test_rgba_forward_any(device, rgba_nets):
    from rgbac import anysize as az
    rgb, msk = (n.to(device) for n in rgba_nets)
    imgs = _rgba_images(opaque=False)
    out = az.rgba_forward_any(msk, rgb, imgs)
    assert out["sizes"] == RAGGED and out["pad"] == "transparent"
    cv = {k: v.cpu() for k, v in out["canvas"].items()}
    assert cv["x_hat"].shape == (2, 3, 64, 128)
    # the canvas is the packed batch: zeros outside each rectangle
    for b, (h, w) in enumerate(RAGGED):
        assert out["rgba"][b].shape == (h, w, 4) and out["rgba"][b].dtype == torch.uint8
        assert float(cv["alpha"][b, :, h:, :].abs().sum()) == 0 and float(cv["alpha"][b, :, :, w:].abs().sum()) == 0
        want_a = imgs[b][..., 3].float().div(255)
        assert torch.equal(cv["alpha"][b, 0, :h, :w], want_a)
        # the bytes are the crop of the clipped reconstruction and the reconstructed alpha
        q = torch.cat([cv["x_hat"][b], cv["recon_alpha"][b]])[:, :h, :w]
        q = q.mul(255).add(0.5).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()
        q[..., :3][q[..., 3] == 0] = 0
        assert torch.equal(out["rgba"][b].cpu(), q)
    ref = _region_ref(cv["masked"], cv["x_hat"], RAGGED, cv["alpha"])
    _check_region((out["mse"], out["psnr"], out["sse"], out["n"]), ref)
    assert all(k > 0 for k in ref[1])
    scale = 2 * 64 * 128 / sum(h * w for h, w in RAGGED)
    want_bpp = np.float32(float(cv["bpp_total"].double()) * scale)
    assert abs(float(out["bpp"]) - float(want_bpp)) <= _ulp32(want_bpp)
    assert out["bpp"].dtype == torch.float32 and out["bpp"].dim() == 0


@pytest.mark.parametrize("pad", MODES)
def test_rgba_forward_any_opaque_alpha_bits(device, rgba_nets, pad):
    """Opaque images: replicate padding keeps the canvas alpha all ones, so the total holds no
    alpha-codec bits; transparent padding breaks `all(mask == 1)` and the total holds them."""
    from rgbac import anysize as az
    from rgbac import runtime as rt
    from rgbac.layers.SupplyMask import mask_pyramid
    rgb, msk = (n.to(device) for n in rgba_nets)
    # the RGB codec's own bpp on the same canvas tensors; fixed tiles, so that both runs of the
    # codec sum in the same order
    with torch.no_grad(), rt.fixed_tiles():
        out = az.rgba_forward_any(msk, rgb, _rgba_images(opaque=True), pad=pad)
        cv = out["canvas"]
        levels = mask_pyramid(cv["alpha"], 6)[1]
        bpp_rgb = float(rgb(cv["masked"], cv["alpha"], cv["recon_alpha"], *levels[:4])[2])
    assert bool((cv["alpha"] == 1).all()) == (pad == "replicate")
    bpp_mask = float(cv["bpp_mask"])
    assert bpp_mask > 1e-3 * bpp_rgb                            # the two cases are told apart
    total = bpp_rgb if pad == "replicate" else float(np.float32(bpp_rgb) + np.float32(bpp_mask))
    assert abs(float(cv["bpp_total"]) - total) <= 1e-6 * total
    scale = 2 * 64 * 128 / sum(h * w for h, w in RAGGED)
    want_bpp = np.float32(float(cv["bpp_total"].double()) * scale)
    assert abs(float(out["bpp"]) - float(want_bpp)) <= _ulp32(want_bpp)
    assert abs(float(out["bpp"]) - total * scale) <= 2e-6 * total * scale
