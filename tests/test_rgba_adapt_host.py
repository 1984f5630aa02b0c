"""CPU: lossless RGBA files with the colour transform chosen per block (rgbac/rgbalossless.py,
transform="adaptive").  The numpy twin's version 2 files go through the
parser and a pixel-by-pixel decoder of the model written here; the choice rule is checked on
blocks built for each of its branches; the parser's new rejections each from a one-field
corruption."""
import struct

import numpy as np
import pytest

KINDS = ["ramps", "luma", "mixed", "rconst", "grey", "soft"]


def image(h, w, kind, seed=0):
    """(h, w, 4) uint8 test images; ``kind`` names the colour content."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    ramps = np.stack([3 * xx + yy, 255 - 2 * yy - xx // 3, 7 * yy + 5 * (xx // 2) + 40], axis=-1)
    luma = g.integers(116, 141, (h, w, 1)) + g.integers(-2, 3, (h, w, 3))
    rgb = {"ramps": ramps, "soft": ramps, "luma": luma,
           "mixed": np.where((xx < w // 2)[..., None], ramps, luma),
           "rconst": np.concatenate([np.full((h, w, 1), 77), luma[..., 1:]], axis=-1),
           "grey": np.repeat(ramps[..., :1], 3, axis=-1)}[kind]
    im = np.empty((h, w, 4), dtype=np.uint8)
    im[..., :3] = rgb % 256
    im[..., 3] = 255
    if kind == "soft":      # a soft disc; below row 16 one one-pixel block, the rest hidden
        disc = np.sqrt((yy + 0.5 - h / 2) ** 2 + (xx + 0.5 - w / 2) ** 2)
        im[..., 3] = np.clip((max(h, w) / 2.2 - disc) / 3.0, 0, 1) * 255
        im[16:, :, 3] = 0
        im[16:, :1, 3] = 9
    return im


def decode_model(blob, alpha):
    """A version 2 file and the alpha plane it was coded beside -> (h, w, 3) colour, by the rules
    of DESIGN.md sections 26 and 30, one pixel and one rANS step at a time."""
    from rgbac import rgbalossless as rl
    f = rl.parse_rgba_lossless(blob)
    h, w = f["h"], f["w"]
    vis = np.ones((h, w), dtype=bool) if f["keep_hidden"] else alpha != 0
    starts = np.cumsum(f["freqs"], axis=1) - f["freqs"]
    words, at = [int(x) for x in f["payload"]], 0
    out = np.zeros((h, w, 3), dtype=np.int64)
    blocks = [(r, c) for r in range(0, h, 16) for c in range(0, w, 16)]
    for (r0, c0), cw, counts in zip(blocks, f["cls"].tolist(), f["counts"]):
        if cw & 1:
            continue
        px = [(r, c) for r in range(r0, min(r0 + 16, h)) for c in range(c0, min(c0 + 16, w))
              if vis[r, c]]
        slots = np.zeros((h, w, 3), dtype=np.int64)           # only this block's part is used
        for s in range(3):
            if (cw >> (1 + s)) & 1:
                for r, c in px:
                    slots[r, c, s] = (cw >> (8 + 8 * s)) & 255
                continue
            kind = s + 2 if s and cw & (8 << s) else s
            x, end = words[at] | words[at + 1] << 32, at + int(counts[s])
            at += 2
            for r, c in px:
                eL, eU = c > c0 and vis[r, c - 1], r > r0 and vis[r - 1, c]
                eD = c > c0 and r > r0 and vis[r - 1, c - 1]
                L, U, D = slots[r, c - 1, s], slots[r - 1, c, s], slots[r - 1, c - 1, s]
                if eL and eU:
                    D = D if eD else L
                    lo, hi = min(L, U), max(L, U)
                    pred = lo if D >= hi else hi if D <= lo else L + U - D
                    d = max(L, U, D) - min(L, U, D)
                    k = 0 if d == 0 else 1 if d <= 8 else 2 if d <= 64 else 3
                elif eL or eU or eD:
                    pred, k = (L if eL else U if eU else D), 0
                else:
                    pred, k = 0, 4
                t = 5 * kind + k
                cum = x & 0xFFFF
                sym = int(np.searchsorted(starts[t], cum, side="right")) - 1
                while f["freqs"][t, sym] == 0:
                    sym -= 1
                x = int(f["freqs"][t, sym]) * (x >> 16) + cum - int(starts[t, sym])
                if x < 1 << 31:
                    x, at = x << 32 | words[at], at + 1
                slots[r, c, s] = (pred + sym) & 255
            assert x == 1 << 31 and at == end
        for r, c in px:
            y, s1, s2 = slots[r, c]
            out[r, c] = (s1 if cw & 16 else s1 + y - 128, y, s2 if cw & 32 else s2 + y - 128)
    assert at == len(words)
    return (out & 255).astype(np.uint8)


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_twin_round_trips(kind, keep):
    from rgbac import rgbalossless as rl
    im = image(17, 33, kind, 3)
    blob = rl.encode_rgba_lossless_host(im, keep, transform="adaptive")
    f = rl.parse_rgba_lossless(blob)
    assert (f["transform"], f["keep_hidden"], f["freqs"].shape) == ("adaptive", keep, (25, 256))
    assert struct.unpack_from("<HH", blob, 4) == (2, 2 | keep)
    want = im[..., :3].copy()
    if not keep:
        want[im[..., 3] == 0] = 0
    assert (decode_model(blob, im[..., 3]) == want).all()
    coded = f["cls"][f["cls"] != 1]
    if kind == "ramps":
        assert (coded[:2] & 48 == 48).all()                  # the whole blocks: plain wins twice
    if kind == "luma":
        assert (coded & 48 == 0).all()
    if kind == "mixed":
        assert {0, 48} <= set((coded & 48).tolist())


def _block(r, g, b):
    im = np.full((16, 16, 4), 255, dtype=np.uint8)
    im[..., 0], im[..., 1], im[..., 2] = r, g, b
    return im


def test_choice_rule_branches():
    from rgbac import rgbalossless as rl
    yy, xx = np.mgrid[:16, :16]
    noise = np.random.default_rng(1).integers(0, 256, (16, 16))

    def word(im):
        return int(rl.parse_rgba_lossless(
            rl.encode_rgba_lossless_host(im, transform="adaptive"))["cls"][0])

    # grey: both differences are constant (128); Y is coded
    assert word(_block(noise, noise, noise)) == 12 | 128 << 16 | 128 << 24
    # R constant over a varying G: the red slot is plain and constant; B = G: Cb constant
    assert word(_block(77, noise, noise)) == 16 | 12 | 77 << 16 | 128 << 24
    # G constant at 128: Cr = R and Cb = B, the costs tie, the difference is chosen
    assert word(_block(noise, 128, noise[::-1])) == 2 | 128 << 8
    # unrelated ramps: plain wins in both slots, nothing is constant
    assert word(_block(3 * xx, 255 - 7 * yy, 5 * yy + xx)) == 48


@pytest.fixture(scope="module")
def files():
    from rgbac import rgbalossless as rl
    im = image(17, 33, "soft", 3)
    return (im, rl.encode_rgba_lossless_host(im),
            rl.encode_rgba_lossless_host(im, transform="adaptive"))


def _class_table_at(blob):
    from rgbac import rgbalossless as rl
    f = rl.parse_rgba_lossless(blob)
    tables = sum(2 + (512 if n > rl.SPARSE_MAX else 3 * n)
                 for n in (int((r > 0).sum()) for r in f["freqs"]))
    return rl.HEADER_BYTES + struct.unpack_from("<I", blob, 16)[0] + 8 + tables, f["cls"]


@pytest.mark.parametrize("name", ["adaptive_flag_in_v1", "v2_without_flag", "reserved_class_bits",
                                  "plain_bits_in_v1", "plain_bits_hidden"])
def test_parser_rejects(files, name):
    from rgbac import rgbalossless as rl
    im, v1, v2 = files

    def patched(b, off, fmt, value):
        out = bytearray(b)
        struct.pack_into(fmt, out, off, value)
        return bytes(out)

    at1, cls1 = _class_table_at(v1)
    at2, cls2 = _class_table_at(v2)
    assert cls1[0] & 0xF1 == 0 and cls2[0] & 1 == 0 and cls2[2] == 1   # coded, coded, hidden
    bad, pattern = {
        "adaptive_flag_in_v1": (patched(v1, 6, "<H", 2), "unknown flags"),
        "v2_without_flag": (patched(v2, 6, "<H", 0), "unsupported version 2"),
        "reserved_class_bits": (patched(v2, at2, "<I", int(cls2[0]) | 0x40), "reserved bits"),
        "plain_bits_in_v1": (patched(v1, at1, "<I", int(cls1[0]) | 0x10), "reserved bits"),
        "plain_bits_hidden": (patched(v2, at2 + 8, "<I", 1 | 0x20), "hidden block's word"),
    }[name]
    with pytest.raises(RuntimeError, match=pattern):
        rl.parse_rgba_lossless(bad)


def test_green_is_the_default_and_unchanged(files):
    from rgbac import rgbalossless as rl
    im, v1, v2 = files
    assert rl.encode_rgba_lossless_host(im, transform="green") == v1 != v2
    assert rl.parse_rgba_lossless(v1)["transform"] == "green"
    for fn in (rl.encode_rgba_lossless_host, rl.encode_rgba_lossless):
        with pytest.raises(ValueError, match="transform"):
            fn(im, transform="blue")


def test_adaptive_is_smaller_on_opaque_ramps():
    """The issue's size condition, on the twin: opaque unrelated ramps at (17, 1030)."""
    from rgbac import rgbalossless as rl
    im = image(17, 1030, "ramps")
    green, adaptive = (len(rl.encode_rgba_lossless_host(im, transform=t)) for t in rl.TRANSFORMS)
    print(f"opaque ramps 17x1030: green {green} bytes, adaptive {adaptive}")
    assert adaptive < green
