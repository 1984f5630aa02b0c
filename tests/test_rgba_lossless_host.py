"""CPU: the host half of the lossless RGBA files (rgbac/rgbalossless.py): what the numpy twin of
the coder writes is the model of DESIGN.md section 26 computed here pixel by pixel, the parser
accepts it, and rejects every malformation it promises to, each from a one-field corruption."""
import struct

import numpy as np
import pytest


def image(h, w, kind, seed=0):
    """(h, w, 4) uint8 test images; ``kind`` names the content (see the GPU test's cross)."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    im = np.empty((h, w, 4), dtype=np.uint8)
    im[..., :3] = g.integers(0, 256, (h, w, 3))
    im[..., 3] = 255
    disc = (yy + 0.5 - h / 2) ** 2 + (xx + 0.5 - w / 2) ** 2
    if kind == "flat":
        im[..., :3] = (10, 200, 77)
    elif kind == "grey":
        im[..., :3] = ((xx * 255 // max(w - 1, 1) + yy) % 256)[..., None]
    elif kind == "disc":
        im[..., 3] = np.where(disc < (min(h, w) / 3) ** 2, 255, 0)
    elif kind == "soft":
        im[..., :3] = np.stack([xx + yy, 2 * xx + 40, 255 - yy], axis=-1) % 256
        im[..., 3] = np.clip((min(h, w) / 2.2 - np.sqrt(disc)) / 3.0, 0, 1) * 255
    elif kind == "checker":
        im[..., 3] = np.where((yy + xx) % 2 == 0, 200, 0)
    elif kind == "last_pixel":
        im[..., 3] = 0
        im[-1, -1, 3] = 9
    elif kind == "wrap":                                  # R - G and B - G wrap mod 256
        im[..., :3] = np.where((xx % 2 == 0)[..., None], (255, 0, 7), (9, 255, 0))
    else:
        assert kind == "noise"
    return im


def loop_model(img, keep_hidden=False):
    """-> (class words, [(symbols, table indexes) of every chunk in file order]), pixel by pixel
    from the rules of DESIGN.md section 26."""
    a = img.astype(np.int64)
    h, w = a.shape[:2]

    def vis(r, c):
        return keep_hidden or a[r, c, 3] != 0

    def val(r, c, ch):
        return (a[r, c, 1], (a[r, c, 0] - a[r, c, 1] + 128) & 255,
                (a[r, c, 2] - a[r, c, 1] + 128) & 255)[ch]

    words, chunks = [], []
    for r0 in range(0, h, 16):
        for c0 in range(0, w, 16):
            px = [(r, c) for r in range(r0, min(r0 + 16, h)) for c in range(c0, min(c0 + 16, w))
                  if vis(r, c)]
            word = 0 if px else 1
            for ch in range(3 if px else 0):
                vals = [val(r, c, ch) for r, c in px]
                if len(set(vals)) == 1:
                    word |= (2 << ch) | (vals[0] << (8 + 8 * ch))
                    continue
                s, t = [], []
                for (r, c), v in zip(px, vals):
                    eL, eU = c > c0 and vis(r, c - 1), r > r0 and vis(r - 1, c)
                    eD = c > c0 and r > r0 and vis(r - 1, c - 1)
                    if eL and eU:
                        L, U = val(r, c - 1, ch), val(r - 1, c, ch)
                        D = val(r - 1, c - 1, ch) if eD else L
                        pred = (min(L, U) if D >= max(L, U) else max(L, U) if D <= min(L, U)
                                else L + U - D)
                        d = max(L, U, D) - min(L, U, D)
                        k = 0 if d == 0 else 1 if d <= 8 else 2 if d <= 64 else 3
                    elif eL or eU or eD:
                        pred = (val(r, c - 1, ch) if eL else val(r - 1, c, ch) if eU
                                else val(r - 1, c - 1, ch))
                        k = 0
                    else:
                        pred, k = 0, 4
                    s.append((v - pred) & 255)
                    t.append(5 * ch + k)
                chunks.append((np.array(s), np.array(t)))
            words.append(word)
    return np.array(words, dtype=np.uint32), chunks


def check_stream(f, chunks):
    """A parsed file against the loop model's chunks: the tables are the normalised histograms,
    every chunk decodes with the host chunk decoder to the model's symbols.  -> the model's code
    length under the file's tables, in bytes, plus 8 bytes of flush per chunk."""
    from rgbac import ans
    from rgbac import rgbalossless as rl
    assert (f["counts"] > 0).sum() == len(chunks) > 0
    s, t = (np.concatenate([c[i] for c in chunks]) for i in (0, 1))
    for k in range(rl.NTAB):
        assert (f["freqs"][k] == rl.normalise_counts(np.bincount(s[t == k], minlength=256))).all()
    seg = np.array([c[0].size for c in chunks])
    counts = f["counts"][f["counts"] > 0]
    container = (ans._header(256, seg).tobytes() + counts.astype("<u4").tobytes()
                 + f["payload"].astype("<u4").tobytes())
    assert (ans.decode_chunked_host(container, t, rl.host_tables(f["freqs"])) == s).all()
    return sum(int(np.ceil(-np.log2(f["freqs"][c[1], c[0]] / 65536.0).sum() / 8)) + 8
               for c in chunks)


@pytest.fixture(scope="module")
def blob():
    from rgbac import rgbalossless as rl
    im = image(17, 33, "disc", 3)
    return im, rl.encode_rgba_lossless_host(im)


@pytest.mark.parametrize("kind", ["disc", "checker", "grey"])
def test_host_twin_is_the_model(kind):
    from rgbac import rgbalossless as rl
    im = image(17, 33, kind, 3)
    f = rl.parse_rgba_lossless(rl.encode_rgba_lossless_host(im))
    words, chunks = loop_model(im)
    assert (f["h"], f["w"], f["keep_hidden"]) == (17, 33, False)
    assert (f["cls"] == words).all()
    assert 4 * f["payload"].size <= check_stream(f, chunks)
    if kind == "grey":                                   # Cr = Cb = 128 everywhere: Y chunks only
        assert not f["counts"][:, 1:].any() and (words[words != 1] & 12 == 12).all()


def _patched(b, off, fmt, value):
    out = bytearray(b)
    struct.pack_into(fmt, out, off, value)
    return bytes(out)


def _cases(im, b):
    from rgbac import rgbalossless as rl
    f = rl.parse_rgba_lossless(b)
    alpha_len = struct.unpack_from("<I", b, 16)[0]
    col = rl.HEADER_BYTES + alpha_len
    tables = sum(2 + (512 if n > rl.SPARSE_MAX else 3 * n)
                 for n in (int((r > 0).sum()) for r in f["freqs"]))
    cls_at = col + 8 + tables
    cnt_at = cls_at + 4 * f["cls"].size
    assert f["cls"][0] & 15 == 0 and f["cls"][2] == 1    # a coded block, a hidden block
    other = rl.encode_rgba_lossless_host(image(17, 32, "disc", 3))
    other_alpha = other[rl.HEADER_BYTES:rl.HEADER_BYTES + struct.unpack_from("<I", other, 16)[0]]
    return {
        "magic": (b"RGAX" + b[4:], "bad magic"),
        "version": (_patched(b, 4, "<H", 2), "unsupported version"),
        "flags": (_patched(b, 6, "<H", 2), "unknown flags"),
        "size": (_patched(b, 8, "<I", 0), "bad size"),
        "header_cut": (b[:10], "truncated"),
        "truncated": (b[:-4], "truncated"),
        "over_long": (b + b"\0", "over-long"),
        "sections_disagree": (_patched(_patched(b, 16, "<I", alpha_len + 4), 20, "<I",
                                       len(b) - col - 4), "alpha planes: over-long"),
        "colour_length": (_patched(b, 20, "<I", len(b) - col - 4)[:-4], "truncated in the payload"),
        "alpha_size": (rl.build_rgba_lossless(17, 33, False, other_alpha, b[col:]),
                       "alpha plane is 17x32"),
        "table": (_patched(b, col + 8 + 3, "<H", struct.unpack_from("<H", b, col + 8 + 3)[0] + 1),
                  "sums to"),
        "table_order": (_patched(b, col + 8 + 3, "<H", 0), "without a frequency"),
        "reserved_bits": (_patched(b, cls_at, "<I", 0x10), "reserved bits"),
        "hidden_word": (_patched(b, cls_at + 8, "<I", 1 | 5 << 8), "hidden block's word"),
        "value_byte": (_patched(b, cls_at, "<I", 7 << 16), "clear constant flag"),
        "chunk_count": (_patched(b, col, "<I", int((f["counts"] > 0).sum()) + 1), "implies"),
        "class_implies": (_patched(b, cls_at, "<I", 1), "implies"),
        "word_count_low": (_patched(b, cnt_at, "<H", 1), "word count is impossible"),
        "word_count_high": (_patched(b, cnt_at, "<H", 132), "word count is impossible"),
        "payload_sum": (_patched(b, col + 4, "<I", f["payload"].size + 1), "sums to"),
    }


CASE_NAMES = ["magic", "version", "flags", "size", "header_cut", "truncated", "over_long",
              "sections_disagree", "colour_length", "alpha_size", "table", "table_order",
              "reserved_bits", "hidden_word", "value_byte", "chunk_count", "class_implies",
              "word_count_low", "word_count_high", "payload_sum"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_parser_rejects(blob, name):
    from rgbac import rgbalossless as rl
    cases = _cases(*blob)
    assert sorted(cases) == sorted(CASE_NAMES)
    bad, pattern = cases[name]
    with pytest.raises(RuntimeError, match=pattern):
        rl.parse_rgba_lossless(bad)


def test_no_cpu_path(blob):
    import rgbac
    for fn, arg in ((rgbac.encode_rgba_lossless, [blob[0]]), (rgbac.decode_rgba_lossless, [blob[1]])):
        with pytest.raises(RuntimeError, match="GPU"):
            fn(arg, device="cpu")
