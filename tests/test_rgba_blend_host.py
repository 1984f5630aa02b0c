"""CPU: the host half of the composite-bounded near-lossless RGBA files (rgbac/rgbanear.py with
bound="composite"): the arithmetic facts the format rests on, by brute
force; the numpy twin keeps the guarantee and its files pass the parser; an opaque image codes as
under the pixel bound; a soft alpha makes the file smaller; the parser rejects what it promises
to."""
import struct

import numpy as np
import pytest

from test_rgba_near_host import KINDS, image

DELTAS = [1, 3, 16]


def test_facts_of_the_model():
    """For every tolerance e that occurs (e(a) = min(255, 255 delta // a)) and all P, C in
    0..255: |C^ - C| <= e with the clamp, Q(C^ - P) = q, |q| <= (255 + e) // (2 e + 1) <= 85; for
    every delta and a: a |C^ - C| <= 255 delta; and n // step = (n * ceil(2^18 / step)) >> 18
    for every n <= 255 + e."""
    from rgbac import rgbanear as rn
    a = np.arange(1, 256)
    P, C = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    worst = {}
    for e in sorted({int(e) for d in range(1, 17) for e in rn.tolerance(a, d, True)}):
        step = 2 * e + 1

        def Q(x):
            return np.sign(x) * ((np.abs(x) + e) // step)
        q = Q(C - P)
        rec = np.clip(P + q * step, 0, 255)
        worst[e] = int(np.abs(rec - C).max())
        assert worst[e] <= e
        assert (Q(rec - P) == q).all()
        assert np.abs(q).max() <= (255 + e) // step <= 85
        n = np.arange(255 + e + 1)
        assert ((n * -(-2 ** 18 // step)) >> 18 == n // step).all()
    assert len(worst) == 191
    for d in range(1, 17):
        e = rn.tolerance(a, d, True)
        assert e[-1] == d and (e >= d).all() and (rn.tolerance(a, d, False) == d).all()
        assert (a * np.asarray([worst[int(x)] for x in e]) <= 255 * d).all()
        assert rn.max_quantised(d) >= ((255 + e) // (2 * e + 1)).max()


@pytest.mark.parametrize("delta", DELTAS)
@pytest.mark.parametrize("kind", KINDS)
def test_twin_keeps_the_composite_bound_and_parses(kind, delta):
    from rgbac import rgbanear as rn
    im = image(17, 33, kind, 3)
    blob, rec = rn.encode_rgba_near_host(im, delta, bound="composite")
    vis = im[..., 3] != 0
    assert (rec[..., 3] == im[..., 3]).all()
    err = np.abs(rec[..., :3].astype(int) - im[..., :3])
    assert (im[..., 3].astype(int)[..., None] * err <= 255 * delta)[vis].all()
    assert not rec[..., :3][~vis].any()
    f = rn.parse_rgba_near(blob)
    assert (f["h"], f["w"], f["delta"], f["keep_hidden"], f["bound"]) == \
        (17, 33, delta, False, "composite")
    assert (f["cls"] == rn.settle_host(im, delta, bound="composite")[1]).all()
    assert rn.parse_rgba_near(rn.encode_rgba_near_host(im, delta)[0])["bound"] == "pixel"


@pytest.mark.parametrize("delta", DELTAS)
def test_opaque_image_codes_as_under_the_pixel_bound(delta):
    from rgbac import rgbanear as rn
    im = image(17, 33, "ramp", 3)
    im[..., :3] ^= image(17, 33, "noise", 4)[..., :3] & 7
    (pb, prec), (cb, crec) = (rn.encode_rgba_near_host(im, delta, bound=b) for b in rn.BOUNDS)
    assert (prec == crec).all()
    assert struct.unpack_from("<HH", pb, 4) == (1, 0) and struct.unpack_from("<HH", cb, 4) == (2, 2)
    assert pb[:4] == cb[:4] and pb[8:] == cb[8:]


@pytest.mark.parametrize("delta", DELTAS)
def test_soft_alpha_makes_the_file_smaller(delta):
    """A 96 x 128 noisy colour ramp under a radial soft disc of alpha: tables and class words
    cost the same under both bounds, the symbols less under the composite bound."""
    from rgbac import rgbanear as rn
    g = np.random.default_rng(5)
    yy, xx = np.mgrid[:96, :128]
    im = np.empty((96, 128, 4), dtype=np.uint8)
    im[..., :3] = np.clip((2 * xx + yy)[..., None] % 256 + g.integers(-12, 13, (96, 128, 3)), 0, 255)
    im[..., 3] = np.clip(300 - 5 * np.hypot(yy - 48, xx - 64), 0, 255)
    pixel, composite = (len(rn.encode_rgba_near_host(im, delta, bound=b)[0]) for b in rn.BOUNDS)
    print(f"delta {delta}: pixel bound {pixel} bytes, composite bound {composite} bytes")
    assert composite < pixel


def _header(b, version, flags):
    return b[:4] + struct.pack("<HH", version, flags) + b[8:]


REJECTS = {
    "composite_flag_in_version_1": (lambda p, c: _header(p, 1, 2), "do not fit version 1"),
    "version_2_without_the_flag": (lambda p, c: _header(c, 2, 0), "do not fit version 2"),
    "version_2_with_keep_hidden": (lambda p, c: _header(c, 2, 3), "keep_hidden under"),
    "unknown_version": (lambda p, c: _header(c, 3, 2), "unsupported version 3"),
}


@pytest.mark.parametrize("name", sorted(REJECTS))
def test_parser_rejects(name):
    from rgbac import rgbanear as rn
    im = image(17, 33, "soft", 3)
    blobs = [rn.encode_rgba_near_host(im, 3, bound=b)[0] for b in rn.BOUNDS]
    for b in blobs:
        rn.parse_rgba_near(b)
    damage, pattern = REJECTS[name]
    with pytest.raises(RuntimeError, match=pattern):
        rn.parse_rgba_near(damage(*blobs))


def test_bound_argument():
    import rgbac
    from rgbac import rgbanear as rn
    im = image(5, 7, "soft")
    for fn, arg in ((rgbac.encode_rgba_near, [im]), (rgbac.encode_rgba_near_host, im),
                    (rn.settle_host, im)):
        with pytest.raises(ValueError, match="keep_hidden has no meaning"):
            fn(arg, 2, keep_hidden=True, bound="composite")
        with pytest.raises(ValueError, match="bound must be one of"):
            fn(arg, 2, bound="visible")
