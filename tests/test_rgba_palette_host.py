"""CPU: palette mode of the lossless RGBA files (rgbac/rgbalossless.py, transform="palette",
DESIGN.md section 31).  The numpy twin's version 3 files are checked against the format's words:
the palette is the image's canonical pixels in key order (sorted here as plain tuples), the index
plane is the plane coder's blob of their positions; 256 colours fit and 257 do not; hidden
pixels count as colours only with keep_hidden; the parser's rejections each from one corruption;
the other transforms write the bytes they wrote before."""
import hashlib
import struct

import numpy as np
import pytest

KINDS = ["one", "two", "r256", "a256", "c257", "wide", "soft", "hard"]


def image(h, w, kind, seed=0):
    """(h, w, 4) uint8 test images; ``kind`` names the colour content."""
    yy, xx = np.mgrid[:h, :w]
    i = yy * w + xx
    im = np.empty((h, w, 4), dtype=np.uint8)
    im[...] = (10, 20, 30, 255)
    if kind == "two":
        im[(xx // 3 + yy) % 2 == 1] = (200, 20, 30, 255)
    elif kind in ("r256", "c257", "wide"):          # 256 colours that differ only in R
        im[..., 0] = i % 256
        if kind == "c257":
            im[-1, -1, 1] = 21                      # the 257th, at the last pixel only
        if kind == "wide":                          # 256 more in every 4,096 pixels
            im[..., 1] = i // 4096
    elif kind == "a256":                            # ... only in alpha, 0 among them
        im[..., 3] = i % 256
    elif kind in ("soft", "hard"):                  # 16 colours, also under alpha 0
        pal = np.random.default_rng(seed).integers(0, 256, (16, 3))
        im[..., :3] = pal[(xx // 3 + 2 * (yy // 2)) % 16]
        disc = np.sqrt((yy + 0.5 - h / 2) ** 2 + (xx + 0.5 - w / 2) ** 2)
        a = np.clip((max(h, w) / 2.2 - disc) / 3.0, 0, 1)
        im[..., 3] = (a if kind == "soft" else a > 0.5) * 255
    return im


def canonical(im, keep_hidden):
    px = im.view("<u4")[..., 0].astype(np.uint32)
    return px if keep_hidden else np.where(im[..., 3] == 0, np.uint32(0), px)


def _key(v):
    return v >> 24, ((v & 255) + 2 * (v >> 8 & 255) + (v >> 16 & 255)) >> 2, v


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_twin_file_is_the_format(kind, keep):
    from rgbac import alphaexact as ax, rgbalossless as rl
    im = image(17, 33, kind, 3)
    blob = rl.encode_rgba_lossless_host(im, keep, transform="palette")
    px = canonical(im, keep)
    want = sorted(set(px.reshape(-1).tolist()), key=_key)
    if kind == "c257":
        assert len(want) == 257
        assert blob == rl.encode_rgba_lossless_host(im, keep, transform="adaptive")
        return
    assert len(want) == {"one": 1, "two": 2, "r256": 256, "a256": 256}.get(kind, len(want))
    f = rl.parse_rgba_lossless(blob)
    assert (f["transform"], f["keep_hidden"], f["h"], f["w"]) == ("palette", keep, 17, 33)
    assert struct.unpack_from("<HHIIII", blob, 4) == (3, 4 | keep, 17, 33, 0, len(blob) - 24)
    assert f["palette"].tolist() == want
    index = np.vectorize({v: k for k, v in enumerate(want)}.get)(px).astype(np.uint8)
    assert blob[28 + 4 * len(want):] == ax.encode_alpha_plane_host(index)
    assert (f["palette"][index] == px).all()


def test_hidden_colours_count_only_with_keep_hidden():
    from rgbac import rgbalossless as rl
    im = image(17, 33, "hard", 3)
    hidden = im[im[..., 3] == 0]
    assert len({tuple(p) for p in hidden.tolist()}) > 1             # differing hidden colours
    n = {keep: rl.parse_rgba_lossless(rl.encode_rgba_lossless_host(im, keep, "palette"))["palette"]
         for keep in (False, True)}
    assert (n[False] >> 24 == 0).sum() == 1 and n[False][0] == 0
    assert (n[True] >> 24 == 0).sum() > 1 and n[True].size > n[False].size


@pytest.fixture(scope="module")
def files():
    from rgbac import rgbalossless as rl
    im = image(17, 33, "two")
    return im, rl.encode_rgba_lossless_host(im, transform="palette"), \
        rl.encode_rgba_lossless_host(im, transform="adaptive")


@pytest.mark.parametrize("name", ["n_zero", "n_257", "order", "equal_entries", "hidden_colour",
                                  "plane_size", "alpha_section", "lengths", "plane_over_long",
                                  "reserved_flag", "v3_without_flag", "palette_flag_in_v2"])
def test_parser_rejects(files, name):
    from rgbac import alphaexact as ax, rgbalossless as rl
    im, v3, v2 = files

    def patched(b, off, fmt, *values):
        out = bytearray(b)
        struct.pack_into(fmt, out, off, *values)
        return bytes(out)

    f = rl.parse_rgba_lossless(v3)
    p0, p1 = f["palette"].tolist()
    other = ax.encode_alpha_plane_host(np.zeros((17, 32), dtype=np.uint8))
    bad, pattern = {
        "n_zero": (patched(v3, 24, "<I", 0), "palette of 0"),
        "n_257": (patched(v3, 24, "<I", 257), "palette of 257"),
        "order": (patched(v3, 28, "<II", p1, p0), "not strictly ascending"),
        "equal_entries": (patched(v3, 28, "<II", p0, p0), "not strictly ascending"),
        "hidden_colour": (patched(v3, 28, "<I", 0x00000001), "hidden palette entry"),
        "plane_size": (rl.build_rgba_palette(17, 33, False, f["palette"], other), "index plane is"),
        "alpha_section": (patched(v3, 16, "<II", 4, len(v3) - 28), "no alpha section"),
        "lengths": (patched(v3, 20, "<I", len(v3) - 23), "truncated"),
        "plane_over_long": (patched(v3 + b"\0", 20, "<I", len(v3) - 23), "over-long"),
        "reserved_flag": (patched(v3, 6, "<H", 4 | 8), "unknown flags"),
        "v3_without_flag": (patched(v3, 6, "<H", 0), "unsupported version 3"),
        "palette_flag_in_v2": (patched(v2, 6, "<H", 2 | 4), "unknown flags"),
    }[name]
    with pytest.raises(RuntimeError, match=pattern):
        rl.parse_rgba_lossless(bad)


def test_other_transforms_write_what_they_wrote():
    """The digests are of the twin's files before palette mode existed."""
    from rgbac import rgbalossless as rl
    im = image(17, 33, "soft", 3)
    got = {t: hashlib.sha256(rl.encode_rgba_lossless_host(im, transform=t)).hexdigest()[:16]
           for t in ("green", "adaptive")}
    assert got == {"green": "ee0c4d37a37811e6", "adaptive": "fea6ad6d7eed2de4"}
    assert rl.encode_rgba_lossless_host(im) == rl.encode_rgba_lossless_host(im, transform="green")
    assert rl.TRANSFORM_NAMES == ("green", "adaptive", "palette")
    with pytest.raises(ValueError, match="transform"):
        rl.encode_rgba_lossless_host(im, transform="index")


def test_palette_file_is_smaller_on_16_colours():
    """The issue's size condition: a smooth field quantised to 16 levels over a seeded random
    palette, opaque, 125 x 170."""
    from rgbac import rgbalossless as rl
    yy, xx = np.mgrid[:125, :170]
    field = np.sin(xx / 23.0) + np.cos(yy / 17.0) + 0.01 * xx
    level = ((field - field.min()) / (np.ptp(field) + 1e-9) * 16).astype(np.int64).clip(0, 15)
    im = np.full((125, 170, 4), 255, dtype=np.uint8)
    im[..., :3] = np.random.default_rng(5).integers(0, 256, (16, 3))[level]
    v3, v2 = (len(rl.encode_rgba_lossless_host(im, transform=t)) for t in ("palette", "adaptive"))
    print(f"16 colours 125x170: version 3 {v3} bytes, version 2 {v2}")
    assert v3 < v2
