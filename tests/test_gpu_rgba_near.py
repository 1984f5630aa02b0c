"""GPU: near-lossless RGBA files (csrc/color_near.hip, rgbac/rgbanear.py).  The byte-level
reference is the numpy twin (encode_rgba_near_host), the guarantee is checked against the input:
for the cross of sizes, contents and delta the device files equal the twin's, alone, batched and
in reversed order; the decoder and return_recon give the twin's reconstruction; alpha is exact
and every visible colour byte within delta."""
import pytest
import torch

from test_rgba_near_host import KINDS, image

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 7), (16, 16), (17, 33), (17, 1030)]       # the last crosses a group boundary
CASES = [(s, k, False) for s in SIZES for k in KINDS] + [(s, "soft", True) for s in SIZES]
DELTAS = [1, 3, 16]


@pytest.fixture(scope="module", params=DELTAS)
def coded(request, device):
    """Every case of one delta: the twin once; the images of one keep_hidden in one ragged call,
    and again in reversed order; all files decoded in one call."""
    from rgbac import decode_rgba_near, encode_rgba_near, encode_rgba_near_host
    delta = request.param
    host = [image(h, w, k, i) for i, ((h, w), k, _) in enumerate(CASES)]
    out = {"delta": delta, "host": host, "images": [torch.from_numpy(im).to(device) for im in host],
           "twin": [encode_rgba_near_host(im, delta, c[2]) for im, c in zip(host, CASES)],
           "blobs": [None] * len(CASES), "rev": [None] * len(CASES), "recon": [None] * len(CASES)}
    for keep in (False, True):
        ks = [i for i, c in enumerate(CASES) if c[2] == keep]
        ims = [out["images"][i] for i in ks]
        blobs, recon = encode_rgba_near(ims, delta, keep_hidden=keep, return_recon=True)
        rev = encode_rgba_near(ims[::-1], delta, keep_hidden=keep)[::-1]
        for j, i in enumerate(ks):
            out["blobs"][i], out["rev"][i], out["recon"][i] = blobs[j], rev[j], recon[j]
    out["outs"] = decode_rgba_near(out["blobs"])
    return out


@pytest.mark.parametrize("i", range(len(CASES)),
                         ids=[f"{h}x{w}-{k}{'-keep' if keep else ''}" for (h, w), k, keep in CASES])
def test_files_and_reconstruction(coded, i):
    from rgbac import encode_rgba_near
    delta, keep = coded["delta"], CASES[i][2]
    x = coded["images"][i]
    blob, rec = coded["twin"][i]
    rec = torch.from_numpy(rec).to(x.device)
    alone = encode_rgba_near([x], delta, keep_hidden=keep)[0]
    assert alone == coded["blobs"][i] == coded["rev"][i]
    assert alone == blob
    assert torch.equal(coded["outs"][i], rec) and torch.equal(coded["recon"][i], rec)
    out = coded["outs"][i]
    vis = torch.ones_like(x[..., 3], dtype=torch.bool) if keep else x[..., 3] != 0
    assert torch.equal(out[..., 3], x[..., 3])
    worst = int((out[..., :3].int() - x[..., :3].int()).abs()[vis].max()) if vis.any() else 0
    print(f"delta {delta} {CASES[i]}: {len(alone)} bytes, max error {worst}")
    assert worst <= delta
    assert not out[..., :3][~vis].any()


def test_mixed_files_in_one_decode(device):
    from rgbac import decode_rgba_near, encode_rgba_near, encode_rgba_near_host
    im = image(17, 33, "soft", 7)
    x = torch.from_numpy(im).to(device)
    jobs = [(d, keep) for d in DELTAS for keep in (False, True)]
    blobs = [encode_rgba_near([x], d, keep_hidden=keep)[0] for d, keep in jobs]
    outs = decode_rgba_near(blobs[::-1])[::-1]
    for (d, keep), out in zip(jobs, outs):
        assert torch.equal(out.cpu(), torch.from_numpy(encode_rgba_near_host(im, d, keep)[1]))
