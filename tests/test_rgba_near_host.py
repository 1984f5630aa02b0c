"""CPU: the host half of the near-lossless RGBA files (rgbac/rgbanear.py): the numpy twin keeps
the guarantee of DESIGN.md section 28, its files pass the parser, and the parser rejects what it
promises to."""
import struct

import numpy as np
import pytest

KINDS = ["noise", "checker", "ramp", "flat", "soft"]


def image(h, w, kind, seed=0):
    """(h, w, 4) uint8 test images; each ``kind`` reaches one mechanism of the coder."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    im = np.empty((h, w, 4), dtype=np.uint8)
    im[..., 3] = 255
    if kind == "noise":                          # clamping at 0 and 255, the largest |q|
        im[..., :3] = g.integers(0, 256, (h, w, 3))
    elif kind == "checker":                      # saturated chroma: the clamp of G^ + p
        im[..., :3] = np.where(((yy + xx) % 2 == 0)[..., None], (255, 0, 255), (0, 255, 0))
    elif kind == "ramp":                         # R spans <= 2 in a block, G <= 30, B up to 75
        im[..., :3] = np.stack([xx // 8 % 256, (xx + yy) % 256, (2 * xx + 3 * yy) % 256], axis=-1)
    elif kind == "flat":                         # no chunk at all
        im[..., :3] = (10, 200, 77)
    else:                                        # soft alpha with holes over textured colour
        assert kind == "soft"
        im[..., :3] = np.clip((2 * xx + yy)[..., None] % 256 + g.integers(-20, 21, (h, w, 3)), 0, 255)
        im[..., 3] = np.clip(((xx * 37 + yy * 11) % 64) * 5 - 40, 0, 255)
        im[:16, 16:32, 3] = 0                    # a hidden block
        im[16:, :16, 3] = 0
        im[16:, 3:4, 3] = 9                      # a block with a single visible pixel
    return im


@pytest.mark.parametrize("delta", [1, 3, 16])
@pytest.mark.parametrize("kind,keep", [(k, False) for k in KINDS] + [("soft", True)])
def test_twin_keeps_the_bound_and_parses(kind, keep, delta):
    from rgbac import rgbanear as rn
    im = image(17, 33, kind, 3)
    blob, rec = rn.encode_rgba_near_host(im, delta, keep)
    vis = np.ones((17, 33), dtype=bool) if keep else im[..., 3] != 0
    assert (rec[..., 3] == im[..., 3]).all()
    assert np.abs(rec[..., :3].astype(int) - im[..., :3])[vis].max() <= delta
    assert not rec[..., :3][~vis].any()
    f = rn.parse_rgba_near(blob)
    assert (f["h"], f["w"], f["delta"], f["keep_hidden"]) == (17, 33, delta, keep)
    assert (f["cls"] == rn.settle_host(im, delta, keep)[1]).all()
    assert (f["counts"] > 0).sum() == rn.rl._chunk_mask(f["cls"]).sum()
    if kind == "flat":
        assert not f["payload"].size
    if kind == "ramp":                           # R constant at every delta, G only at 16
        seen = f["cls"] != 1
        assert (f["cls"][seen] & 4).all() and bool(f["cls"][0] & 2) == (delta == 16)


def _patched(b, off, fmt, value):
    out = bytearray(b)
    struct.pack_into(fmt, out, off, value)
    return bytes(out)


def _table_symbol(b):
    """The file with one frequency of table 0 moved to symbol 100 (q = 100: no such error)."""
    from rgbac import rgbanear as rn
    f = rn.parse_rgba_near(b)
    freqs = f["freqs"].copy()
    s = np.flatnonzero(freqs[0])[1]
    freqs[0, 100], freqs[0, s] = freqs[0, s], 0
    alpha = b[rn.HEADER_BYTES:rn.HEADER_BYTES + struct.unpack_from("<I", b, 20)[0]]
    return rn.build_rgba_near(17, 33, 16, False, alpha, rn.rl.build_colour(
        freqs, f["cls"], f["counts"][f["counts"] > 0], f["payload"]))


REJECTS = {
    "magic": (lambda b: b"RGAL" + b[4:], "bad magic"),
    "delta_0": (lambda b: _patched(b, 8, "<B", 0), "max_error 0"),
    "delta_17": (lambda b: _patched(b, 8, "<B", 17), "max_error 17"),
    "reserved": (lambda b: _patched(b, 10, "<B", 1), "reserved"),
    "truncated": (lambda b: b[:-4], "RGAN file: truncated"),
    "table_symbol": (_table_symbol, "outside the range"),
}


@pytest.mark.parametrize("name", sorted(REJECTS))
def test_parser_rejects(name):
    from rgbac import rgbanear as rn
    blob = rn.encode_rgba_near_host(image(17, 33, "soft", 3), 16)[0]
    rn.parse_rgba_near(blob)
    damage, pattern = REJECTS[name]
    with pytest.raises(RuntimeError, match=pattern):
        rn.parse_rgba_near(damage(blob))


@pytest.mark.parametrize("bad", [0, 17, -1, 1.5, True, None])
def test_max_error_range(bad):
    import rgbac
    im = image(5, 7, "noise")
    for fn, arg in ((rgbac.encode_rgba_near, [im]), (rgbac.encode_rgba_near_host, im)):
        with pytest.raises(ValueError, match="encode_rgba_lossless" if bad == 0 else "1..16"):
            fn(arg, bad)


def test_no_cpu_path():
    import rgbac
    im = image(5, 7, "noise")
    for fn, args in ((rgbac.encode_rgba_near, ([im], 2)),
                     (rgbac.decode_rgba_near, ([rgbac.encode_rgba_near_host(im, 2)[0]],))):
        with pytest.raises(RuntimeError, match="GPU"):
            fn(*args, device="cpu")
