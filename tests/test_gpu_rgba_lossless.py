"""GPU: lossless RGBA files (csrc/color_exact.hip, rgbac/rgbalossless.py).  The reference is the
input itself, the byte-level reference the numpy twin of the coder, and the model the plain
loop of test_rgba_lossless_host.py.

* the cross of sizes and contents, coded in one ragged call, alone and in reversed order: equal
  bytes every way, equal to the host twin's, decoded exactly (hidden RGB zeroed);
* keep_hidden, colour under alpha 0, strided views;
* the stream is the chunked rANS format's and no larger than the model's code length;
* corrupt payloads and a foreign alpha section raise through the error word.
"""
import struct

import pytest
import torch

from test_rgba_lossless_host import check_stream, image, loop_model

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 7), (16, 16), (17, 33), (17, 1030)]
KINDS = ["flat", "grey", "noise", "disc", "soft", "checker", "last_pixel", "wrap"]
CASES = [(s, k) for s in SIZES for k in KINDS]


def _expected(im, keep_hidden=False):
    out = im.clone()
    if not keep_hidden:
        out[..., :3][im[..., 3] == 0] = 0
    return out


@pytest.fixture(scope="module")
def coded(device):
    """Every case coded in one ragged call, and again in reversed order; decoded in one call."""
    from rgbac import decode_rgba_lossless, encode_rgba_lossless
    host = [image(h, w, k, i) for i, ((h, w), k) in enumerate(CASES)]
    images = [torch.from_numpy(im).to(device) for im in host]
    blobs = encode_rgba_lossless(images)
    rev = encode_rgba_lossless(images[::-1])[::-1]
    return {"host": host, "images": images, "blobs": blobs, "rev": rev,
            "outs": decode_rgba_lossless(blobs)}


@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{h}x{w}-{k}" for (h, w), k in CASES])
def test_round_trip_exact(coded, i):
    from rgbac import (decode_rgba_lossless, encode_rgba_lossless, encode_rgba_lossless_host,
                       parse_rgba_lossless)
    x = coded["images"][i]
    alone = encode_rgba_lossless([x])[0]
    assert alone == coded["blobs"][i] == coded["rev"][i]
    assert alone == encode_rgba_lossless_host(coded["host"][i])
    assert torch.equal(coded["outs"][i], _expected(x))
    assert torch.equal(decode_rgba_lossless([alone])[0], _expected(x))
    f = parse_rgba_lossless(alone)
    if CASES[i][1] == "flat":
        assert not f["counts"].any() and not f["payload"].size
    if CASES[i][1] == "grey":
        assert not f["counts"][:, 1:].any() and (f["cls"] & 12 == 12).all()


def test_keep_hidden_and_hidden_colour(coded, device):
    from rgbac import decode_rgba_lossless, encode_rgba_lossless
    i = CASES.index(((17, 33), "disc"))
    x = coded["images"][i]
    assert (x[..., 3] == 0).any() and x[..., :3][x[..., 3] == 0].any()
    kept = encode_rgba_lossless([x], keep_hidden=True)[0]
    both = decode_rgba_lossless([kept, coded["blobs"][i]])        # the two flags in one call
    assert torch.equal(both[0], x) and torch.equal(both[1], _expected(x))
    other = x.clone()
    other[..., :3][x[..., 3] == 0] ^= 0x5A                        # differs only under alpha 0
    assert encode_rgba_lossless([other])[0] == coded["blobs"][i]
    assert encode_rgba_lossless([other], keep_hidden=True)[0] != kept


def test_strided_view(device):
    from rgbac import decode_rgba_lossless, encode_rgba_lossless
    big = torch.from_numpy(image(50, 60, "disc", 5)).to(device)
    view = big[2:2 + 33, 3:3 + 40]
    blobs = encode_rgba_lossless([view, big])
    assert blobs == encode_rgba_lossless([view.contiguous(), big])
    assert torch.equal(decode_rgba_lossless(blobs)[0], _expected(view))


@pytest.mark.parametrize("kind,keep", [("disc", False), ("checker", False), ("soft", True)])
def test_stream_is_the_chunked_format(coded, kind, keep):
    from rgbac import encode_rgba_lossless, parse_rgba_lossless
    i = CASES.index(((17, 33), kind))
    blob = encode_rgba_lossless([coded["images"][i]], keep_hidden=True)[0] if keep else coded["blobs"][i]
    f = parse_rgba_lossless(blob)
    words, chunks = loop_model(coded["host"][i], keep)
    assert (f["cls"] == words).all()
    bound = check_stream(f, chunks)
    print(f"{CASES[i]}: payload {4 * f['payload'].size} bytes, bound {bound}")
    assert 4 * f["payload"].size <= bound


def test_corrupt_streams_raise(coded, device):
    from rgbac import decode_rgba_lossless, encode_rgba_lossless
    from rgbac import rgbalossless as rl
    good = coded["blobs"][CASES.index(((17, 33), "noise"))]
    bad = bytearray(good)
    bad[-3] ^= 0x10                                               # a flipped payload word
    with pytest.raises(RuntimeError, match="RGAL file decode: error"):
        decode_rgba_lossless([bytes(bad)])
    # the alpha section of another mask of the same size: class words and visibility disagree
    i = CASES.index(((17, 33), "disc"))
    other = coded["images"][i].clone()
    assert not other[16, :, 3].any()
    other[16, :16, 3] = 255                   # block (1, 0) becomes visible, no other block moves
    a, b = coded["blobs"][i], encode_rgba_lossless([other])[0]
    cut = [rl.HEADER_BYTES + struct.unpack_from("<I", x, 16)[0] for x in (a, b)]
    swapped = rl.build_rgba_lossless(17, 33, False, b[rl.HEADER_BYTES:cut[1]], a[cut[0]:])
    rl.parse_rgba_lossless(swapped)                               # sound as far as the host can see
    with pytest.raises(RuntimeError, match="RGAL file decode: error 3"):
        decode_rgba_lossless([swapped])
    assert torch.equal(decode_rgba_lossless([a])[0], coded["outs"][i])
