"""GPU: lossless RGBA files with the colour transform chosen per block (csrc/color_adapt.hip,
rgbac/rgbalossless.py, transform="adaptive").  The reference is the input itself, the byte-level
reference the numpy twin of the coder, whose files test_rgba_adapt_host.py decodes with a plain
loop over the model.

* the cross of sizes and contents, the images of one keep_hidden value coded in one ragged call,
  alone and in reversed order: equal bytes every way, equal to the twin's, decoded exactly
  (hidden RGB zeroed without keep_hidden);
* version 1 and version 2 files of both flag values decode together in one call;
* the adaptive file of the opaque ramps at (17, 1030) is smaller than the green one;
* a class word the format forbids leaves its block alone and reports code 3.
"""
import pytest
import torch

from test_rgba_adapt_host import KINDS, image

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 7), (16, 16), (17, 33), (17, 1030)]
CASES = [(s, k, keep) for keep, kinds in ((False, KINDS), (True, ["soft"])) for s in SIZES
         for k in kinds]


def _expected(im, keep_hidden):
    out = im.clone()
    if not keep_hidden:
        out[..., :3][im[..., 3] == 0] = 0
    return out


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
            files = encode_rgba_lossless([images[i] for i in order], keep, transform="adaptive")
            for i, b in zip(order, files):
                out[i] = b
    return {"host": host, "images": images, "blobs": blobs, "rev": rev,
            "outs": decode_rgba_lossless(blobs)}


@pytest.mark.parametrize("i", range(len(CASES)),
                         ids=[f"{h}x{w}-{k}{'-keep' * keep}" for (h, w), k, keep in CASES])
def test_round_trip_exact(coded, i):
    from rgbac import decode_rgba_lossless, encode_rgba_lossless, encode_rgba_lossless_host
    x, keep = coded["images"][i], CASES[i][2]
    alone = encode_rgba_lossless([x], keep, transform="adaptive")[0]
    assert alone == coded["blobs"][i] == coded["rev"][i]
    assert alone == encode_rgba_lossless_host(coded["host"][i], keep, transform="adaptive")
    assert torch.equal(coded["outs"][i], _expected(x, keep))
    assert torch.equal(decode_rgba_lossless([alone])[0], _expected(x, keep))


def test_versions_and_flags_decode_together(coded):
    from rgbac import decode_rgba_lossless, encode_rgba_lossless
    i, j = CASES.index(((17, 33), "soft", False)), CASES.index(((17, 33), "soft", True))
    x, y = coded["images"][i], coded["images"][j]
    files = [coded["blobs"][j], encode_rgba_lossless([x])[0], coded["blobs"][i],
             encode_rgba_lossless([y], keep_hidden=True)[0]]
    assert [f[4] for f in files] == [2, 1, 2, 1]
    outs = decode_rgba_lossless(files)
    for out, (im, keep) in zip(outs, [(y, True), (x, False), (x, False), (y, True)]):
        assert torch.equal(out, _expected(im, keep))


def test_adaptive_is_smaller_on_opaque_ramps(coded):
    from rgbac import encode_rgba_lossless
    i = CASES.index(((17, 1030), "ramps", False))
    green = encode_rgba_lossless([coded["images"][i]])[0]
    print(f"opaque ramps 17x1030: green {len(green)} bytes, adaptive {len(coded['blobs'][i])}")
    assert len(coded["blobs"][i]) < len(green)


@pytest.mark.parametrize("word", [0x40, 0x80, 1 | 0x10, 1 | 0x20])
def test_forbidden_class_word_touches_nothing(coded, device, word):
    """The parser never lets such a word through; the kernel does not trust the parser."""
    from rgbac import rgbalossless as rl
    i = CASES.index(((17, 33), "ramps", False))
    f = rl.parse_rgba_lossless(coded["blobs"][i])
    f["cls"] = f["cls"].copy()
    f["cls"][1] = word if word & 1 else int(f["cls"][1]) | word
    out = coded["images"][i].clone()
    out[..., :3] = 0x5A
    err = torch.zeros(1, dtype=torch.int32, device=device)
    rl._decode_colour([f], [(out.data_ptr(), 17, 33, out.stride(0))], False, device, err, True)
    assert int(err.item()) == 3
    assert (out[:16, 16:32, :3] == 0x5A).all()                    # block 1 is as it was
    want = coded["outs"][i].clone()
    want[:16, 16:32, :3] = 0x5A
    assert torch.equal(out, want)
