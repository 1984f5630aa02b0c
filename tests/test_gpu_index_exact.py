"""GPU: version 4 RGAL files, transform="palette" with index_model="neighbour"
(csrc/index_exact.hip, rgbac/indexexact.py).  The reference is the input itself, the byte-level
reference the numpy twin, which test_index_exact_host.py holds against the format.

* the sizes of test_gpu_rgba_palette.py (17 x 33 and 17 x 1030 end in blocks one and six pixels
  wide: no NE anywhere in the first) crossed with one colour, two colours alternating per pixel,
  a dither, 256 colours, 257 colours (the adaptive bytes) and 16 colours under hard alpha with
  and without keep_hidden: coded in one ragged call per flag, alone and in reversed order, equal
  bytes every way and equal to the twin's, decoded exactly; the index plane alone through
  encode_index_planes / decode_index_planes;
* version 1, 2, 3 and 4 files decode together in one call;
* a literal past the palette reports code 3 and writes the pixel 0.
"""
import numpy as np
import pytest
import torch

from test_gpu_rgba_palette import SIZES
from test_index_exact_host import BAYER
from test_rgba_palette_host import canonical, image

pytestmark = pytest.mark.gpu

KINDS = [("one", False), ("alt", False), ("dither", False), ("r256", False), ("c257", False),
         ("hard", False), ("hard", True)]
CASES = [(s, k, keep) for k, keep in KINDS for s in SIZES]


def _image(h, w, kind, seed):
    if kind not in ("alt", "dither"):
        return image(h, w, kind, seed)
    yy, xx = np.mgrid[:h, :w]
    im = np.full((h, w, 4), 255, dtype=np.uint8)
    level = (yy + xx) % 2 if kind == "alt" else \
        (7.0 * (xx + 2 * yy) / (w + 2 * h) + (BAYER[yy % 4, xx % 4] + 0.5) / 16).astype(int)
    im[..., :3] = np.random.default_rng(seed).integers(0, 256, (8, 3))[level]
    return im


def _want(host, keep):
    return torch.from_numpy(canonical(host, keep).view(np.uint8).reshape(host.shape))


@pytest.fixture(scope="module")
def coded(device):
    """Every case coded in one ragged call per flag value, and again in reversed order; all
    files decoded in one call."""
    from rgbac import decode_rgba_lossless, encode_rgba_lossless
    host = [_image(h, w, k, i) for i, ((h, w), k, _) in enumerate(CASES)]
    images = [torch.from_numpy(im).to(device) for im in host]
    blobs, rev = [None] * len(CASES), [None] * len(CASES)
    for keep in (False, True):
        ks = [i for i, c in enumerate(CASES) if c[2] == keep]
        for out, order in ((blobs, ks), (rev, ks[::-1])):
            files = encode_rgba_lossless([images[i] for i in order], keep, transform="palette",
                                         index_model="neighbour")
            for i, b in zip(order, files):
                out[i] = b
    return {"host": host, "images": images, "blobs": blobs, "rev": rev,
            "outs": decode_rgba_lossless(blobs)}


@pytest.mark.parametrize("i", range(len(CASES)),
                         ids=[f"{h}x{w}-{k}{'-keep' * keep}" for (h, w), k, keep in CASES])
def test_files_are_the_twins_and_exact(coded, i):
    from rgbac import (decode_index_planes, decode_rgba_lossless, encode_index_planes,
                       encode_rgba_lossless, encode_rgba_lossless_host, parse_rgba_lossless)
    from rgbac.indexexact import encode_index_plane_host
    (h, w), kind, keep = CASES[i]
    x, host = coded["images"][i], coded["host"][i]
    alone = encode_rgba_lossless([x], keep, transform="palette", index_model="neighbour")[0]
    assert alone == coded["blobs"][i] == coded["rev"][i]
    assert alone == encode_rgba_lossless_host(host, keep, "palette", "neighbour")
    want = _want(host, keep)
    assert torch.equal(coded["outs"][i].cpu(), want)
    assert torch.equal(decode_rgba_lossless([alone])[0].cpu(), want)
    if kind == "c257" and h * w > 256:
        assert alone[4] == 2 and alone == encode_rgba_lossless([x], keep, transform="adaptive")[0]
        return
    f = parse_rgba_lossless(alone)
    assert alone[4] == 4 and f["index_model"] == "neighbour"
    pal = f["palette"]
    order = np.argsort(pal)
    index = order[np.searchsorted(pal[order], canonical(host, keep))].astype(np.uint8)
    blob = encode_index_planes([torch.from_numpy(index).to(x.device)], [pal.size])[0]
    assert blob == alone[28 + 4 * pal.size:] == encode_index_plane_host(index, pal.size)
    assert torch.equal(decode_index_planes([blob])[0].cpu(), torch.from_numpy(index))


def test_four_versions_decode_together(coded):
    from rgbac import decode_rgba_lossless, encode_rgba_lossless
    i, j = CASES.index(((17, 33), "dither", False)), CASES.index(((17, 1030), "hard", True))
    x, y = coded["images"][i], coded["images"][j]
    files = [coded["blobs"][j], encode_rgba_lossless([x])[0],
             encode_rgba_lossless([y], True, transform="palette")[0], coded["blobs"][i],
             encode_rgba_lossless([x], transform="adaptive")[0]]
    assert [f[4] for f in files] == [4, 1, 3, 4, 2]
    for out, k in zip(decode_rgba_lossless(files), [j, i, j, i, i]):
        assert torch.equal(out.cpu(), _want(coded["host"][k], CASES[k][2]))


def test_literal_past_the_palette_is_corrupt(coded, device):
    """The parser cannot see such a literal; the unmap kernel does not trust the plane.  The
    file is built by coding the altered plane with the host coder."""
    from rgbac import indexexact as ix, rgbalossless as rl
    i = CASES.index(((17, 33), "alt", False))
    f = rl.parse_rgba_lossless(coded["blobs"][i])
    px = canonical(coded["host"][i], False)
    index = (px == f["palette"][1]).astype(np.uint8)
    assert f["palette"].size == 2 and (f["palette"][index] == px).all()
    index[9, 20] = 2                                              # n is 2: an escape and a literal
    bad = rl.build_rgba_palette(17, 33, False, f["palette"],
                                ix.encode_index_plane_host(index, 2), neighbour=True)
    with pytest.raises(RuntimeError, match="error 3"):
        rl.decode_rgba_lossless([bad])
    out = torch.full((17, 33, 4), 0x5A, dtype=torch.uint8, device=device)
    err = torch.zeros(1, dtype=torch.int32, device=device)
    rl._decode_palette([rl.parse_rgba_lossless(bad)], [(out.data_ptr(), 17, 33, out.stride(0))],
                       device, err)
    assert int(err.item()) == 3
    want = _want(coded["host"][i], False)
    want[9, 20] = 0
    assert torch.equal(out.cpu(), want)
