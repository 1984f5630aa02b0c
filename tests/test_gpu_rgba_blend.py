"""GPU: composite-bounded near-lossless RGBA files (csrc/color_blend.hip, rgbac/rgbanear.py with
bound="composite").  The byte-level reference is the numpy twin, the guarantee is checked against
the input: for the cross of sizes, contents and delta the device files equal the twin's, alone,
batched and in reversed order; the decoder and return_recon give the twin's reconstruction; alpha
is exact and a |C^ - C| <= 255 delta on every pixel.  One decode call over files of both versions
holds the flat-table path of the new decoder to csrc/color_near.hip's results."""
import numpy as np
import pytest
import torch

from test_rgba_near_host import KINDS, image

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 7), (16, 16), (17, 33), (17, 1030)]       # the last crosses a group boundary
CASES = [(s, k) for s in SIZES for k in KINDS] + [((16, 16), "every_alpha")]
DELTAS = [1, 3, 16]


def case_image(i):
    (h, w), kind = CASES[i]
    if kind != "every_alpha":
        return image(h, w, kind, i)
    # the smallest input that reads every table entry, alpha 0 and the e = 255 entries included
    im = np.random.default_rng(i).integers(0, 256, (h, w, 4)).astype(np.uint8)
    im[..., 3] = np.arange(256).reshape(h, w)
    return im


@pytest.fixture(scope="module", params=DELTAS)
def coded(request, device):
    """Every case of one delta: the twin once; all images in one ragged call, and again in
    reversed order; all files decoded in one call."""
    from rgbac import decode_rgba_near, encode_rgba_near, encode_rgba_near_host
    delta = request.param
    host = [case_image(i) for i in range(len(CASES))]
    ims = [torch.from_numpy(im).to(device) for im in host]
    blobs, recon = encode_rgba_near(ims, delta, return_recon=True, bound="composite")
    return {"delta": delta, "images": ims, "blobs": blobs, "recon": recon,
            "twin": [encode_rgba_near_host(im, delta, bound="composite") for im in host],
            "rev": encode_rgba_near(ims[::-1], delta, bound="composite")[::-1],
            "outs": decode_rgba_near(blobs)}


@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{h}x{w}-{k}" for (h, w), k in CASES])
def test_files_and_reconstruction(coded, i):
    from rgbac import encode_rgba_near
    delta, x = coded["delta"], coded["images"][i]
    blob, rec = coded["twin"][i]
    rec = torch.from_numpy(rec).to(x.device)
    alone = encode_rgba_near([x], delta, bound="composite")[0]
    assert alone == coded["blobs"][i] == coded["rev"][i]
    assert alone == blob
    assert torch.equal(coded["outs"][i], rec) and torch.equal(coded["recon"][i], rec)
    out = coded["outs"][i]
    vis = x[..., 3] != 0
    assert torch.equal(out[..., 3], x[..., 3])
    seen = x[..., 3:].int() * (out[..., :3].int() - x[..., :3].int()).abs()
    print(f"delta {delta} {CASES[i]}: {len(alone)} bytes, max a |dC| {int(seen.max())}")
    assert int(seen.max()) <= 255 * delta
    assert not out[..., :3][~vis].any()


def test_mixed_versions_in_one_decode(device):
    from rgbac import decode_rgba_near, encode_rgba_near, encode_rgba_near_host
    im = image(17, 33, "soft", 7)
    x = torch.from_numpy(im).to(device)
    jobs = [(d, keep, bound) for d in DELTAS
            for keep, bound in ((False, "pixel"), (True, "pixel"), (False, "composite"))]
    blobs = [encode_rgba_near([x], d, keep_hidden=keep, bound=bound)[0] for d, keep, bound in jobs]
    outs = decode_rgba_near(blobs[::-1])[::-1]
    for (d, keep, bound), out in zip(jobs, outs):
        assert torch.equal(out.cpu(), torch.from_numpy(encode_rgba_near_host(im, d, keep, bound)[1]))
