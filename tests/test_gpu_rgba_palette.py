"""GPU: palette mode of the lossless RGBA files (csrc/color_palette.hip, rgbac/rgbalossless.py,
transform="palette").  The reference is the input itself, the byte-level reference the numpy
twin, whose files test_rgba_palette_host.py holds against the format.

* the cross of sizes (one pixel, a partial block, one block, several blocks, five collect
  workgroups) and contents, the images of one keep_hidden value coded in one ragged call, alone
  and in reversed order: equal bytes every way, equal to the twin's, decoded exactly;
* 257 colours, the last one at the last pixel only, fall back to the adaptive bytes, and so do
  workgroups with 256 colours each that differ between them ("wide");
* views with longer rows and a base that is not 16-byte aligned give the dense image's bytes;
* version 1, 2 and 3 files decode together in one call;
* an index plane that points past the palette reports code 3 and writes the pixel 0.
"""
import numpy as np
import pytest
import torch

from test_rgba_palette_host import KINDS, canonical, image

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 7), (16, 16), (17, 33), (17, 1030)]
CASES = [(s, k, keep) for keep, kinds in ((False, KINDS), (True, ["soft", "hard"]))
         for s in SIZES for k in kinds]


def _expected(i, host):
    return torch.from_numpy(canonical(host[i], CASES[i][2]).view(np.uint8).reshape(host[i].shape))


@pytest.fixture(scope="module")
def coded(device):
    """Every case coded in one ragged call per flag value, and again in reversed order; all
    files decoded in one call."""
    from rgbac import decode_rgba_lossless, encode_rgba_lossless
    host = [image(h, w, k, i) for i, ((h, w), k, _) in enumerate(CASES)]
    images = [torch.from_numpy(im).to(device) for im in host]
    blobs, rev = [None] * len(CASES), [None] * len(CASES)
    for keep in (False, True):
        ks = [i for i, c in enumerate(CASES) if c[2] == keep]
        for out, order in ((blobs, ks), (rev, ks[::-1])):
            files = encode_rgba_lossless([images[i] for i in order], keep, transform="palette")
            for i, b in zip(order, files):
                out[i] = b
    return {"host": host, "images": images, "blobs": blobs, "rev": rev,
            "outs": decode_rgba_lossless(blobs)}


@pytest.mark.parametrize("i", range(len(CASES)),
                         ids=[f"{h}x{w}-{k}{'-keep' * keep}" for (h, w), k, keep in CASES])
def test_round_trip_exact(coded, i):
    from rgbac import decode_rgba_lossless, encode_rgba_lossless, encode_rgba_lossless_host
    (h, w), kind, keep = CASES[i]
    x = coded["images"][i]
    alone = encode_rgba_lossless([x], keep, transform="palette")[0]
    assert alone == coded["blobs"][i] == coded["rev"][i]
    assert alone == encode_rgba_lossless_host(coded["host"][i], keep, transform="palette")
    falls_back = h * w > {"c257": 256, "wide": 4096}.get(kind, h * w)
    assert alone[4] == (2 if falls_back else 3)
    if falls_back:
        assert alone == encode_rgba_lossless([x], keep, transform="adaptive")[0]
    want = _expected(i, coded["host"])
    assert torch.equal(coded["outs"][i].cpu(), want)
    assert torch.equal(decode_rgba_lossless([alone])[0].cpu(), want)


@pytest.mark.parametrize("h,w", [(17, 33), (1, 37)], ids=["longer-rows", "flat-unaligned"])
def test_views_are_read_in_place(device, h, w):
    """Rows of a larger buffer go pixel by pixel; one row is flat but starts off a 16-byte line."""
    from rgbac import decode_rgba_lossless, encode_rgba_lossless, encode_rgba_lossless_host
    x = image(h, w, "soft", 1)
    big = torch.full((h + 2, w + 5, 4), 77, dtype=torch.uint8, device=device)
    y = big[1:1 + h, 1:1 + w]
    y.copy_(torch.from_numpy(x))
    assert y.data_ptr() % 16 and y.stride(0) != 4 * w
    blob = encode_rgba_lossless([y], transform="palette")[0]
    assert blob[4] == 3 and blob == encode_rgba_lossless_host(x, transform="palette")
    want = torch.from_numpy(canonical(x, False).view(np.uint8).reshape(x.shape))
    assert torch.equal(decode_rgba_lossless([blob])[0].cpu(), want)


def test_three_versions_decode_together(coded):
    from rgbac import decode_rgba_lossless, encode_rgba_lossless
    i, j = CASES.index(((17, 33), "soft", False)), CASES.index(((17, 1030), "hard", True))
    x, y = coded["images"][i], coded["images"][j]
    files = [coded["blobs"][j], encode_rgba_lossless([x])[0], coded["blobs"][i],
             encode_rgba_lossless([y], True, transform="adaptive")[0],
             coded["blobs"][CASES.index(((17, 1030), "c257", False))]]
    assert [f[4] for f in files] == [3, 1, 3, 2, 2]
    outs = decode_rgba_lossless(files)
    for out, k in zip(outs, [j, i, i, j, CASES.index(((17, 1030), "c257", False))]):
        assert torch.equal(out.cpu(), _expected(k, coded["host"]))


def test_index_past_the_palette_is_corrupt(coded, device):
    """The parser cannot see such an index; the kernel does not trust the plane.  The file is
    built by coding the altered plane with the host coder."""
    from rgbac import alphaexact as ax, rgbalossless as rl
    i = CASES.index(((17, 33), "two", False))
    f = rl.parse_rgba_lossless(coded["blobs"][i])
    index = np.searchsorted(f["palette"], canonical(coded["host"][i], False)).astype(np.uint8)
    assert (f["palette"][index] == canonical(coded["host"][i], False)).all()
    index[9, 20] = 2                                              # n is 2
    bad = rl.build_rgba_palette(17, 33, False, f["palette"], ax.encode_alpha_plane_host(index))
    with pytest.raises(RuntimeError, match="error 3"):
        rl.decode_rgba_lossless([bad])
    out = torch.full((17, 33, 4), 0x5A, dtype=torch.uint8, device=device)
    err = torch.zeros(1, dtype=torch.int32, device=device)
    rl._decode_palette([rl.parse_rgba_lossless(bad)], [(out.data_ptr(), 17, 33, out.stride(0))],
                       device, err)
    assert int(err.item()) == 3
    want = _expected(i, coded["host"])
    want[9, 20] = 0
    assert torch.equal(out.cpu(), want)
