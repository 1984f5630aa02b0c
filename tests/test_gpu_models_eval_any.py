"""GPU, model level: per-image bits of both codecs (``per_image=``) and the batched evaluation
entry point rgbac.anysize.rgba_eval_any, in fp32 on the bench's nets (latent gain: non-zero
symbols).

Three RGBA images share the 192 x 256 canvas, and each alone maps to the same canvas; the second
is fully opaque, the other two have soft-edged alpha.  Sorts behind tests/test_gpu_data.py
(DESIGN.md section 20).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [(161, 200), (192, 256), (176, 250)]
HP, WP = 192, 256


@pytest.fixture(scope="module")
def nets(device):
    """(RGB codec, alpha codec) of the benchmark, fp32."""
    from bench import mask_net, rgb_net
    return rgb_net().to(device), mask_net().to(device)


@pytest.fixture(scope="module")
def images():
    """uint8 (h, w, 4): smooth random RGB; alpha a soft-edged ellipse, or 255 for the second."""
    g = torch.Generator().manual_seed(31)
    out = []
    for k, (h, w) in enumerate(SIZES):
        rgb = torch.rand((1, 3, h // 4 + 2, w // 4 + 2), generator=g)
        rgb = torch.nn.functional.interpolate(rgb, size=(h, w), mode="bilinear")[0]
        rgb = (rgb + 0.04 * torch.randn((3, h, w), generator=g)).clamp(0, 1)
        im = torch.empty((h, w, 4), dtype=torch.uint8)
        im[..., :3] = rgb.permute(1, 2, 0).mul(255).round().to(torch.uint8)
        if k == 1:
            im[..., 3] = 255
        else:
            yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
            r = (((yy - h / 2) / (0.48 * h)) ** 2 + ((xx - w / 2) / (0.48 * w)) ** 2).sqrt()
            im[..., 3] = torch.clamp((1 - r) * 12, 0, 1).mul(255).round().to(torch.uint8)
            assert 0.5 < float((im[..., 3] > 0).float().mean()) < 1.0
        out.append(im)
    return out


@pytest.fixture(scope="module")
def batch_eval(nets, images):
    """rgba_eval_any of the three images under the per-image tile rule, made once."""
    from rgbac import anysize as az
    from rgbac import runtime as rt
    rgb, msk = nets
    with rt.fixed_tiles(per_image=True):
        out = az.rgba_eval_any(msk, rgb, images, msssim=True, masked_msssim=True)
    torch.cuda.synchronize()
    return out


def test_bits_sum_to_the_forwards_bpp(nets, batch_eval):
    """Sum over images of the per-image bits = the forward's own bpp * B * hp * wp: both sum the
    same fp32 terms in fp64, the forward's scalar is fp32."""
    from rgbac import runtime as rt
    from rgbac.layers.SupplyMask import mask_pyramid
    rgb, msk = nets
    cv = batch_eval["canvas"]
    assert cv["x_hat"].shape == (3, 3, HP, WP)
    with torch.no_grad(), rt.fixed_tiles(per_image=True):
        pr, pm = {}, {}
        levels = mask_pyramid(cv["alpha"], 6)[1]
        o_rgb = rgb(cv["masked"], cv["alpha"], cv["recon_alpha"], *levels[:4], per_image=pr)
        o_msk = msk(cv["alpha"], per_image=pm)
    for name, o, d in (("rgb", o_rgb, pr), ("mask", o_msk, pm)):
        assert d["y_bits"].shape == (3,) and d["y_bits"].dtype == torch.float64
        assert d["z_bits"].shape == (3,) and d["z_bits"].dtype == torch.float64
        n = 3 * HP * WP
        for part, bpp in (("y", o[3]), ("z", o[4]), ("total", o[2])):
            got = float((d["y_bits"].sum() if part != "z" else 0.0) +
                        (d["z_bits"].sum() if part != "y" else 0.0))
            want = float(bpp.double()) * n
            print(f"{name} {part}: per-image bits sum {got:.6f}, forward bpp * pixels {want:.6f}, "
                  f"rel {abs(got - want) / want:.2e}")
            assert want > 0 and abs(got - want) <= 1e-6 * want
        assert bool((d["y_bits"] > 0).all()) and bool((d["z_bits"] > 0).all())
    # the entry point's own bits are those of the same forwards
    assert torch.equal(batch_eval["y_bits"], pr["y_bits"])
    assert torch.equal(batch_eval["z_bits"], pr["z_bits"])
    assert torch.equal(batch_eval["y_bits_alpha"], pm["y_bits"])
    assert torch.equal(batch_eval["z_bits_alpha"], pm["z_bits"])


def test_each_image_alone_gives_the_same_figures(nets, images, batch_eval):
    """Under rt.fixed_tiles(per_image=True) an image's bits, mse and MS-SSIM do not depend on
    what else is in the batch."""
    from rgbac import anysize as az
    from rgbac import runtime as rt
    rgb, msk = nets
    for b, im in enumerate(images):
        with rt.fixed_tiles(per_image=True):
            one = az.rgba_eval_any(msk, rgb, [im], msssim=True, masked_msssim=True)
        assert one["canvas"]["x_hat"].shape == (1, 3, HP, WP)
        for key in ("y_bits", "z_bits", "y_bits_alpha", "z_bits_alpha", "mse", "ms_ssim",
                    "masked_ms_ssim", "bpp", "psnr"):
            got, alone = batch_eval[key][b:b + 1], one[key]
            print(f"image {b} {key}: batch {got.tolist()} alone {alone.tolist()}")
            assert torch.isfinite(alone).all(), key
            assert torch.equal(got, alone), (b, key)
        assert torch.equal(batch_eval["rgba"][b], one["rgba"][0])


def test_alpha_bits_are_charged_per_image(batch_eval, images):
    out = batch_eval
    assert out["opaque"].tolist() == [0, 1, 0] and out["sizes"] == SIZES
    bpp, rgb, alpha = (out[k].cpu().numpy() for k in ("bpp", "bpp_rgb", "bpp_alpha"))
    assert all(out[k].shape == (3,) and out[k].dtype == torch.float32
               for k in ("bpp", "bpp_rgb", "bpp_alpha", "ms_ssim", "ms_ssim_db", "mse", "psnr"))
    assert (alpha > 0).all() and (rgb > 0).all()
    assert bpp[1] == rgb[1]                                  # the photograph pays no alpha bits
    for b in (0, 2):
        want = np.float64(rgb[b]) + np.float64(alpha[b])
        assert abs(float(bpp[b]) - want) <= 2 * float(np.spacing(np.float32(want)))
    # bpp = bits / the image's real pixels
    for b, (h, w) in enumerate(SIZES):
        want = float(out["y_bits"][b] + out["z_bits"][b]) / (h * w)
        assert abs(float(rgb[b]) - want) <= float(np.spacing(np.float32(want)))
    ms = out["ms_ssim"].double()
    assert torch.isfinite(ms).all()
    assert torch.allclose(out["ms_ssim_db"].double(), -10 * torch.log10(1 - ms), rtol=1e-5, atol=1e-6)
    for b, (h, w) in enumerate(SIZES):
        assert out["rgba"][b].shape == (h, w, 4) and out["rgba"][b].dtype == torch.uint8


def test_metrics_of_the_entry_point_are_the_crops(batch_eval):
    """ms_ssim / masked_ms_ssim of the batch = the uniform HIP metrics on each image's crop."""
    from rgbac.metrics import masked_ms_ssim_torch as mm
    from rgbac.metrics.ms_ssim_torch import ms_ssim
    cv = batch_eval["canvas"]
    for b, (h, w) in enumerate(SIZES):
        x = cv["masked"][b:b + 1, :, :h, :w].contiguous()
        y = cv["x_hat"][b:b + 1, :, :h, :w].contiguous()
        a = cv["alpha"][b:b + 1, :, :h, :w].contiguous()
        want = ms_ssim(x, y, data_range=1.0, size_average=False)
        wantm = mm.ms_ssim(x, y, a, data_range=1.0, size_average=False)
        assert abs(float(batch_eval["ms_ssim"][b]) - float(want)) < 1e-5
        assert abs(float(batch_eval["masked_ms_ssim"][b]) - float(wantm)) < 1e-5


def test_rgba_forward_any_is_unchanged(nets, images):
    """rgba_forward_any returns the same before and after the new entry point ran."""
    from rgbac import anysize as az
    from rgbac import runtime as rt
    rgb, msk = nets
    with rt.fixed_tiles(per_image=True):
        before = az.rgba_forward_any(msk, rgb, images)
        az.rgba_eval_any(msk, rgb, images, msssim=False)
        after = az.rgba_forward_any(msk, rgb, images)
    assert set(before) == {"rgba", "mse", "psnr", "sse", "n", "bpp", "sizes", "pad", "canvas"}
    assert before["bpp"].dim() == 0 and before["pad"] == "transparent"
    for key in ("mse", "psnr", "sse", "n", "bpp"):
        assert torch.equal(before[key], after[key]), key
    for a, b in zip(before["rgba"], after["rgba"]):
        assert torch.equal(a, b)
    for key in ("x_hat", "recon_alpha", "bpp_total", "bpp_mask"):
        assert torch.equal(before["canvas"][key], after["canvas"][key]), key


def test_small_image_is_refused_before_any_launch(nets):
    from rgbac import anysize as az
    rgb, msk = nets
    small = torch.zeros((160, 200, 4), dtype=torch.uint8)
    with pytest.raises(ValueError, match="image 0"):
        az.rgba_eval_any(msk, rgb, [small])


def test_per_image_needs_no_grad(nets, batch_eval):
    rgb, msk = nets
    cv = batch_eval["canvas"]
    assert torch.is_grad_enabled()
    with pytest.raises(ValueError, match="per_image"):
        msk(cv["alpha"], per_image={})


def test_bf16(nets, images, batch_eval):
    """bf16 runs, gives finite figures, and its bpp is within the project's 5 % bf16 bar."""
    from rgbac import anysize as az
    from rgbac import runtime as rt
    rgb, msk = nets
    try:
        rgb.set_compute_dtype(torch.bfloat16)
        msk.set_compute_dtype(torch.bfloat16)
        with rt.fixed_tiles(per_image=True):
            out = az.rgba_eval_any(msk, rgb, images)
        torch.cuda.synchronize()
    finally:
        rgb.set_compute_dtype(torch.float32)
        msk.set_compute_dtype(torch.float32)
    for key in ("bpp", "bpp_rgb", "bpp_alpha", "mse", "psnr", "ms_ssim"):
        assert torch.isfinite(out[key]).all(), key
    rel = ((out["bpp"] - batch_eval["bpp"]).abs() / batch_eval["bpp"]).tolist()
    print(f"bf16 bpp {out['bpp'].tolist()} fp32 {batch_eval['bpp'].tolist()} rel {rel}")
    assert max(rel) < 0.05
