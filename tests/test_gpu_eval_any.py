"""GPU, kernel level: the ragged MS-SSIM / masked MS-SSIM (rgbac.metrics.any_size,
csrc/msssim_any.hip) and the per-image bits (rgbac_image_bits, csrc/bits_any.hip).

Every image of a ragged batch must score what the CPU oracle (oracle.ref_metrics) gives for its
crop alone, to the 1e-5 bar tests/test_gpu_metrics.py holds the uniform metric to -- whatever the
canvas holds outside the image's rectangle: replicated pixels, or the constant 1e3, which any
read of padding by a kept output or by the pool would carry far above the tolerance.

Sorts behind tests/test_gpu_data.py (its loader-throughput test reads
lower the more GPU work the process did before it).
"""
import numpy as np
import pytest
import torch

from oracle import ref_metrics as rm

pytestmark = pytest.mark.gpu

# 161: the smallest side the default window allows, odd at every scale (161, 81, 41, 21, 11) and
# a 1-pixel-high valid map at the last; 192 x 256: even throughout; 250: odd at levels 1, 2
SIZES = [(161, 177), (192, 256), (176, 250)]
HP, WP = 192, 256
FILLS = ("replicate", "const")
TOL = 1e-5


def _pair(C, H, W, seed, noise=0.05):
    g = torch.Generator().manual_seed(seed)
    X = torch.round(torch.rand((1, C, H, W), generator=g) * 255) / 255
    X = torch.nn.functional.avg_pool2d(X, 3, 1, 1)          # some spatial structure
    Y = torch.clamp(X + noise * torch.randn((1, C, H, W), generator=g), 0, 1)
    return X, Y


def _ellipse(h, w):
    """(1, 1, h, w) soft-edged ellipse, with an all-zero band across it."""
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32),
                            torch.arange(w, dtype=torch.float32), indexing="ij")
    r = (((yy - 0.45 * h) / (0.47 * h)) ** 2 + ((xx - 0.55 * w) / (0.44 * w)) ** 2).sqrt()
    m = torch.clamp((1 - r) * 10, 0, 1)
    m[h // 3: h // 3 + 9, :] = 0
    return m.reshape(1, 1, h, w)


def _on_canvas(t, hp, wp, fill):
    """(1, C, h, w) -> (1, C, hp, wp): the image top-left, the rest replicated or 1e3."""
    h, w = t.shape[2:]
    if fill == "replicate":
        return torch.nn.functional.pad(t, (0, wp - w, 0, hp - h), mode="replicate")
    out = torch.full((1, t.shape[1], hp, wp), 1e3)
    out[..., :h, :w] = t
    return out


@pytest.fixture(scope="module")
def crops():
    """Per image of batch A: (X, Y, mask) crops in [0, 1], made once and never changed."""
    out = []
    for k, (h, w) in enumerate(SIZES):
        X, Y = _pair(3, h, w, seed=100 + k)
        out.append((X, Y, _ellipse(h, w)))
    return out


@pytest.fixture(scope="module")
def oracle(crops):
    """(win_size, data_range) -> ([ms_ssim per image], [masked ms_ssim per image]) on the CPU."""
    memo = {}

    def get(ws, dr):
        if (ws, dr) not in memo:
            plain = [float(rm.ms_ssim(X * dr, Y * dr, win_size=ws, data_range=dr,
                                      size_average=False)[0]) for X, Y, _ in crops]
            msk = [float(rm.masked_ms_ssim(X * dr, Y * dr, M, data_range=dr, size_average=False,
                                           win_size=ws)[0]) for X, Y, M in crops]
            memo[(ws, dr)] = (plain, msk)
        return memo[(ws, dr)]
    return get


def _batch(crops, order, hp, wp, fill, dr, device):
    X = torch.cat([_on_canvas(crops[k][0] * dr, hp, wp, fill) for k in order]).to(device)
    Y = torch.cat([_on_canvas(crops[k][1] * dr, hp, wp, fill) for k in order]).to(device)
    M = torch.cat([_on_canvas(crops[k][2], hp, wp, fill) for k in order]).to(device)
    return X, Y, M, [SIZES[k] for k in order]


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("ws,dr", [(11, 1.0), (7, 1.0), (11, 255.0), (7, 255.0)])
def test_ms_ssim_any_is_the_crop_alone(device, crops, oracle, fill, ws, dr):
    from rgbac.metrics import ms_ssim_any
    X, Y, _, sizes = _batch(crops, (0, 1, 2), HP, WP, fill, dr, device)
    got = ms_ssim_any(X, Y, sizes, win_size=ws, data_range=dr)
    assert got.shape == (3,) and got.dtype == torch.float32 and got.is_cuda
    want = oracle(ws, dr)[0]
    for b in range(3):
        d = abs(float(got[b]) - want[b])
        print(f"ms_ssim_any fill={fill} ws={ws} range={dr} image {b}: {float(got[b]):.7f} "
              f"oracle {want[b]:.7f} diff {d:.2e}")
    assert all(abs(float(got[b]) - want[b]) < TOL for b in range(3))
    assert all(0.0 < w < 1.0 for w in want)


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("ws,dr", [(11, 1.0), (7, 1.0), (11, 255.0), (7, 255.0)])
def test_masked_ms_ssim_any_is_the_crop_alone(device, crops, oracle, fill, ws, dr):
    from rgbac.metrics import masked_ms_ssim_any
    X, Y, M, sizes = _batch(crops, (0, 1, 2), HP, WP, fill, dr, device)
    got = masked_ms_ssim_any(X, Y, M, sizes, win_size=ws, data_range=dr)
    assert got.shape == (3,) and got.dtype == torch.float32 and got.is_cuda
    want = oracle(ws, dr)[1]
    for b in range(3):
        d = abs(float(got[b]) - want[b])
        print(f"masked_ms_ssim_any fill={fill} ws={ws} range={dr} image {b}: "
              f"{float(got[b]):.7f} oracle {want[b]:.7f} diff {d:.2e}")
    assert all(abs(float(got[b]) - want[b]) < TOL for b in range(3))
    assert all(0.0 < w < 1.0 for w in want)


@pytest.mark.parametrize("fill", FILLS)
def test_batch_invariance(device, crops, fill):
    """Image 0's value in batch A, alone on a 192 x 192 canvas, and in the reversed batch: the
    same bits, for both metrics."""
    from rgbac.metrics import masked_ms_ssim_any, ms_ssim_any
    X, Y, M, sizes = _batch(crops, (0, 1, 2), HP, WP, fill, 1.0, device)
    a = ms_ssim_any(X, Y, sizes)
    am = masked_ms_ssim_any(X, Y, M, sizes)
    X1, Y1, M1, s1 = _batch(crops, (0,), 192, 192, fill, 1.0, device)
    Xr, Yr, Mr, sr = _batch(crops, (2, 1, 0), HP, WP, fill, 1.0, device)
    r = ms_ssim_any(Xr, Yr, sr)
    rmk = masked_ms_ssim_any(Xr, Yr, Mr, sr)
    assert torch.equal(a[0:1], ms_ssim_any(X1, Y1, s1))
    assert torch.equal(am[0:1], masked_ms_ssim_any(X1, Y1, M1, s1))
    assert torch.equal(a, r.flip(0)) and torch.equal(am, rmk.flip(0))


def test_image_that_is_its_own_canvas(device):
    """B = 2 uniform 256 x 256: the ragged form against the existing uniform metrics."""
    from rgbac.metrics import masked_ms_ssim_any, ms_ssim_any
    from rgbac.metrics import masked_ms_ssim_torch as mm
    from rgbac.metrics.ms_ssim_torch import ms_ssim
    pairs = [_pair(3, 256, 256, seed=7 + k) for k in range(2)]
    X = torch.cat([p[0] for p in pairs]).to(device)
    Y = torch.cat([p[1] for p in pairs]).to(device)
    M = torch.cat([_ellipse(256, 256)] * 2).to(device)
    sizes = [(256, 256)] * 2
    got, want = ms_ssim_any(X, Y, sizes), ms_ssim(X, Y, data_range=1.0, size_average=False)
    gm = masked_ms_ssim_any(X, Y, M, sizes)
    wm = mm.ms_ssim(X, Y, M, data_range=1.0, size_average=False)
    print(f"own canvas: ragged {got.tolist()} uniform {want.tolist()} bit-identical "
          f"{torch.equal(got, want)}; masked ragged {gm.tolist()} uniform {wm.tolist()} "
          f"bit-identical {torch.equal(gm, wm)}")
    assert (got - want).abs().max().item() < TOL
    assert (gm - wm).abs().max().item() < TOL


def test_empty_mask_gives_zero(device, crops):
    from rgbac.metrics import masked_ms_ssim_any
    X, Y, M, sizes = _batch(crops, (0, 1, 2), HP, WP, "const", 1.0, device)
    M[0, :, :SIZES[0][0], :SIZES[0][1]] = 0           # image 0 keeps nothing; its padding stays 1e3
    got = masked_ms_ssim_any(X, Y, M, sizes)
    assert float(got[0]) == 0.0
    assert float(got[1]) > 0.0 and float(got[2]) > 0.0


def test_gpu_side_errors(device, crops):
    from rgbac.metrics import ms_ssim_any
    X, Y, _, sizes = _batch(crops, (0, 1, 2), HP, WP, "replicate", 1.0, device)
    with pytest.raises(ValueError, match="image 2 .*exceeds"):
        ms_ssim_any(X, Y, [(161, 177), (192, 256), (176, 260)])
    with pytest.raises(ValueError, match="requires grad"):
        ms_ssim_any(X.clone().requires_grad_(True), Y, sizes)


# ---- per-image bits

def _bits_ref(lik):
    """numpy: the same expression in float32, summed in float64 -> (B,)."""
    l32 = lik.astype(np.float32)
    t = (np.float32(-1.0) * np.log(l32 + np.float32(1e-10))) / np.float32(0.69314718055994530942)
    t = np.minimum(np.maximum(t, np.float32(0.0)), np.float32(50.0)).astype(np.float32)
    return t.astype(np.float64).sum(axis=-1)


def _lik(seed=5):
    g = torch.Generator().manual_seed(seed)
    lik = torch.rand((3, 640), generator=g)
    lik[0, 0], lik[0, 1], lik[1, 7], lik[2, 639] = 0.0, 1e-9, 1.0, 1e-40       # 1e-40: denormal
    assert 0 < float(lik[2, 639]) < 1.1754944e-38
    return lik


def test_image_bits(device):
    from rgbac.models._latent import image_bits
    lik = _lik()
    want = _bits_ref(lik.numpy())
    got = image_bits(lik.to(device), 3)
    assert got.shape == (3,) and got.dtype == torch.float64
    rel = np.abs(got.cpu().numpy() - want) / want
    print(f"image_bits: {got.tolist()} numpy {want.tolist()} rel {rel.tolist()}")
    assert (rel < 1e-6).all()
    # one image's row changed changes that image's sum only
    lik2 = lik.clone()
    lik2[1] = torch.rand(640, generator=torch.Generator().manual_seed(6))
    got2 = image_bits(lik2.to(device), 3)
    assert torch.equal(got2[0], got[0]) and torch.equal(got2[2], got[2])
    assert not torch.equal(got2[1], got[1])


def test_image_bits_segments(device):
    """[segments][B][n], the forward's slice layout: segment sums add up, and more than one
    block per image (n above the block size) still matches numpy."""
    from rgbac.models._latent import image_bits
    g = torch.Generator().manual_seed(8)
    lik = torch.rand((4, 3, 1000), generator=g)
    want = sum(_bits_ref(lik[s].numpy()) for s in range(4))
    got = image_bits(lik.to(device), 3, segments=4).cpu().numpy()
    assert (np.abs(got - want) / want < 1e-6).all()
    with pytest.raises(ValueError):
        image_bits(lik.to(device)[..., :999], 3, segments=4)        # not contiguous
