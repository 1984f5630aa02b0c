"""CPU: the neighbour-match coder of palette index planes (rgbac/indexexact.py, DESIGN.md section
32) and the version 4 RGAL files built on it.  The numpy twin is the model's definition, so it is
held against the format's words here: symbols and contexts of a plane worked out by hand, every
chunk decodable by the host chunk decoder of rgbac.ans, the twin's own pixel-by-pixel decoder
returning the plane; the parser's rejections each from one corruption; version 4 smaller than
version 3 where the issue says so; ``index_model="plane"`` writing version 3's bytes."""
import struct

import numpy as np
import pytest

SIZES = [(1, 1), (1, 40), (40, 1), (17, 33), (16, 16)]
KINDS = ["constant", "checker", "dither", "all256", "noise5"]
BAYER = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]])


def plane(h, w, kind):
    yy, xx = np.mgrid[:h, :w]
    if kind == "constant":
        p = np.full((h, w), 7)
    elif kind == "checker":
        p = (yy + xx) % 2
    elif kind == "dither":                    # a ramp over 4 positions, 4 x 4 ordered dither
        p = (3.0 * (xx + yy) / max(h + w - 2, 1) + (BAYER[yy % 4, xx % 4] + 0.5) / 16).astype(int)
    elif kind == "all256":                    # every position once in the 16 x 16 plane
        p = np.random.default_rng(1).permutation(256)[(yy * w + xx) % 256]
    else:
        p = np.random.default_rng(2).integers(0, 5, (h, w))
    return p.astype(np.uint8)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("h,w", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_twin_round_trip_and_chunks(h, w, kind):
    from rgbac import ans, indexexact as ix
    p = plane(h, w, kind)
    blob = ix.encode_index_plane_host(p, 256)
    assert (ix.decode_index_plane_host(blob) == p).all()
    f = ix.parse_index_planes(blob)
    keep = np.flatnonzero(f["cls"] == 0)
    if (p == p.flat[0]).all() or not keep.size:
        assert not f["payload"].size and not f["freqs"].any()
        return
    sym, ctx = ix.model_symbols(p)
    parts = [ix._stream(ix._blocks(p)[k], ix._blocks(sym)[k], ix._blocks(ctx)[k]) for k in keep]
    s, t = (np.concatenate([x[i] for x in parts]) for i in (0, 1))
    counts = np.bincount(np.where(t < 64, t * 5 + s, 320 + s), minlength=576)
    from rgbac.alphaexact import normalise_counts
    rule = [ix.normalise_match(counts[5 * k:5 * k + 5]) for k in range(64)]
    assert (f["freqs"] == np.concatenate(rule + [normalise_counts(counts[320:])])).all()
    container = (ans._header(512, np.array([x[0].size for x in parts])).tobytes()
                 + f["counts"][keep].astype("<u4").tobytes() + f["payload"].astype("<u4").tobytes())
    assert (ans.decode_chunked_host(container, t, ix.host_tables(f["freqs"])) == s).all()


def test_model_symbols_by_hand():
    """3 x 4, one block.  (0, 1): N takes W's value and is dropped as its duplicate; (1, 0) and
    (2, 0): W takes N's value; (1, 1): NE ranks 1 because N and NW repeat W; (1, 3) and (2, 3):
    no NE at the right edge, so NW ranks 2 in (2, 3); (0, 2), (0, 3), (1, 3), (2, 0), (2, 2):
    escapes."""
    from rgbac import indexexact as ix
    sym, ctx = ix.model_symbols(np.array([[1, 1, 2, 3], [1, 2, 2, 5], [4, 2, 1, 2]], np.uint8))
    assert sym.tolist() == [[-1, 0, 4, 4], [0, 1, 0, 4], [4, 1, 4, 2]]
    assert ctx.tolist() == [[64, 1, 17, 1], [5, 11, 1, 24], [33, 4, 43, 0]]
    # the same plane as the right edge of a wider one: its blocks do not see one another
    wide = np.zeros((3, 20), dtype=np.uint8)
    wide[:, 16:] = [[1, 1, 2, 3], [1, 2, 2, 5], [4, 2, 1, 2]]
    s2, c2 = ix.model_symbols(wide)
    assert (s2[:, 16:] == sym).all() and (c2[:, 16:] == ctx).all()


def _patched(b, off, fmt, *values):
    out = bytearray(b)
    struct.pack_into(fmt, out, off, *values)
    return bytes(out)


def _first_table(blob):
    """-> offset of the first match table that lists symbols (its u16 count)."""
    pos = 28
    while not struct.unpack_from("<H", blob, pos)[0]:
        pos += 2
    return pos


@pytest.mark.parametrize("name", ["magic", "symbol_5", "not_fixed_point", "word_count",
                                  "bit3_in_v3", "v4_without_bit3", "truncated", "over_long"])
def test_parser_rejects(name):
    from rgbac import indexexact as ix, rgbalossless as rl
    p = plane(17, 33, "noise5")
    blob = ix.encode_index_plane_host(p, 5)
    f = ix.parse_index_planes(blob)
    im = np.full((17, 33, 4), 255, dtype=np.uint8)
    im[..., 0] = p
    v4 = rl.encode_rgba_lossless_host(im, transform="palette", index_model="neighbour")
    v3 = rl.encode_rgba_lossless_host(im, transform="palette")
    assert v4[24 + 4 + 4 * 5:] == blob and rl.parse_rgba_lossless(v4)["index_model"] == "neighbour"
    t = _first_table(blob)
    k = struct.unpack_from("<H", blob, t)[0]
    chunk_table = len(blob) - 4 * f["payload"].size - 2 * int((f["cls"] == 0).sum())
    parse, bad, pattern = {
        "magic": (ix.parse_index_planes, _patched(blob, 0, "<4s", b"RGAP"), "bad magic"),
        "symbol_5": (ix.parse_index_planes, _patched(blob, t + 2 + 3 * (k - 1), "<B", 5),
                     "lists symbol 5"),
        # one frequency off by one: the rule's tables sum to 2^16
        "not_fixed_point": (ix.parse_index_planes,
                            _patched(blob, t + 3, "<H", struct.unpack_from("<H", blob, t + 3)[0] + 1),
                            "sums to 65537"),
        "word_count": (ix.parse_index_planes, _patched(blob, chunk_table, "<H", 256 + 4),
                       "impossible for its block"),
        "bit3_in_v3": (rl.parse_rgba_lossless, _patched(v3, 6, "<H", 4 | 8), "unknown flags"),
        "v4_without_bit3": (rl.parse_rgba_lossless, _patched(v4, 6, "<H", 4),
                            "unsupported version 4"),
        "truncated": (ix.parse_index_planes, blob[:-1], "truncated"),
        "over_long": (ix.parse_index_planes, blob + b"\0", "over-long"),
    }[name]
    with pytest.raises(RuntimeError, match=pattern):
        parse(bad)


def test_version_4_is_smaller_and_plane_writes_version_3():
    """The issue's size condition on the 125 x 170 16-level field of
    test_palette_file_is_smaller_on_16_colours and on its 4 x 4 dither, and the existing bytes."""
    from rgbac import rgbalossless as rl
    yy, xx = np.mgrid[:125, :170]
    field = np.sin(xx / 23.0) + np.cos(yy / 17.0) + 0.01 * xx
    level = (field - field.min()) / (np.ptp(field) + 1e-9) * 16
    pal = np.random.default_rng(5).integers(0, 256, (16, 3))
    for name, lv in (("flat", level), ("dither", level + (BAYER[yy % 4, xx % 4] + 0.5) / 16 - 0.5)):
        im = np.full((125, 170, 4), 255, dtype=np.uint8)
        im[..., :3] = pal[lv.astype(np.int64).clip(0, 15)]
        v3 = rl.encode_rgba_lossless_host(im, transform="palette")
        v4 = rl.encode_rgba_lossless_host(im, transform="palette", index_model="neighbour")
        print(f"16 colours 125x170 {name}: version 4 {len(v4)} bytes, version 3 {len(v3)}, "
              f"ratio {len(v4) / len(v3):.3f}")
        assert v4[4] == 4 and v3[4] == 3 and len(v4) < len(v3)
        assert v3 == rl.encode_rgba_lossless_host(im, transform="palette", index_model="plane")
    for t in ("green", "adaptive"):           # the keyword is looked at under "palette" only
        assert rl.encode_rgba_lossless_host(im, transform=t, index_model="neighbour") == \
            rl.encode_rgba_lossless_host(im, transform=t)
    with pytest.raises(ValueError, match="index_model"):
        rl.encode_rgba_lossless_host(im, transform="palette", index_model="match")
