"""CPU: the host half of the lossless alpha coder and of the RGAX files (rgbac/alphaexact.py,
rgbac/rgbaexact.py): the table rule's numpy twin, the blob built by the CPU twin of the coder
and every rejection the two parsers promise, each from a one-field corruption."""
import struct

import numpy as np
import pytest

from test_rgba_file_host import _container


def _counts(kind):
    g = np.random.default_rng(3)
    c = np.zeros(256, dtype=np.int64)
    if kind == "one":
        c[255] = 40                                   # its companion wraps to symbol 0
    elif kind == "tie":
        c[[9, 4, 200]] = 5
    elif kind == "flat":
        c[:] = 3
    elif kind == "rare":                              # 255 symbols bumped up to 1
        c[:] = 1
        c[77] = 1 << 28
    elif kind == "noise":
        c = g.integers(0, 1000, 256)
    return c


@pytest.mark.parametrize("kind", ["empty", "one", "tie", "flat", "rare", "noise"])
def test_normalise_twin(kind):
    from rgbac.alphaexact import normalise_counts
    c = _counts(kind)
    f = normalise_counts(c)
    if kind == "empty":
        assert not f.any()
        return
    assert f.sum() == 1 << 16 and (f[c > 0] >= 1).all() and f.max() < 1 << 16
    assert (normalise_counts(f) == f).all() and (normalise_counts(c.copy()) == f).all()
    if kind == "one":
        assert f[255] == 65535 and f[0] == 1 and np.count_nonzero(f) == 2
    else:
        assert not f[c == 0].any()
    if kind == "tie":                                 # the remainder goes to the lowest symbol
        assert f[4] == 21846 and f[9] == f[200] == 21845
    if kind == "rare":
        assert (np.delete(f, 77) == 1).all()


@pytest.fixture(scope="module")
def blob():
    from rgbac.alphaexact import encode_alpha_plane_host
    g = np.random.default_rng(1)
    a = np.full((20, 40), 9, dtype=np.uint8)          # blocks: coded, coded, constant / ...
    a[:, :28] = g.integers(0, 256, (20, 28))
    a[16:, :16] = 200
    return a, encode_alpha_plane_host(a)


def test_blob_round_trip(blob):
    from rgbac import alphaexact as ax
    from rgbac import ans
    a, b = blob
    f = ax.parse_alpha_planes(b)
    assert (f["h"], f["w"]) == a.shape
    assert f["cls"].tolist() == [0, 0, 1 | 9 << 8, 1 | 200 << 8, 0, 1 | 9 << 8]
    sym, ctx = ax.model_symbols(a)
    keep = np.flatnonzero(f["cls"] == 0)
    s = np.concatenate([ax._blocks(sym)[k] for k in keep])
    c = np.concatenate([ax._blocks(ctx)[k] for k in keep])
    seg = np.array([ax._blocks(sym)[k].size for k in keep])
    container = (ans._header(256, seg).tobytes() + f["counts"][keep].astype("<u4").tobytes()
                 + f["payload"].astype("<u4").tobytes())
    assert (ans.decode_chunked_host(container, c, ax.host_tables(f["freqs"])) == s).all()
    flat = ax.encode_alpha_plane_host(np.full((3, 70), 5, dtype=np.uint8))
    assert len(flat) == ax.HEADER_BYTES + 5 * 2 + 5 * 2 and not ax.parse_alpha_planes(flat)["payload"].size
    # the device table: exclusive sums and the last symbol of every context
    tab = ax.device_table(f["freqs"])
    assert tab.size == 1288 and tab[0] == 0 and tab[1] == f["freqs"][0, 0]
    assert tab[1280:1285].view(np.int16).tolist() == [int(np.flatnonzero(r)[-1]) if r.any() else -1
                                                      for r in f["freqs"]]


def _patched(b, off, fmt, value):
    out = bytearray(b)
    struct.pack_into(fmt, out, off, value)
    return bytes(out)


def test_alpha_parser_rejections(blob):
    from rgbac import alphaexact as ax
    a, b = blob
    f = ax.parse_alpha_planes(b)
    H = ax.HEADER_BYTES
    tables = sum(2 + (512 if n > ax.SPARSE_MAX else 3 * n)
                 for n in (int((r > 0).sum()) for r in f["freqs"]))
    cls_at = H + tables
    cases = [
        (b"XGAP" + b[4:], "bad magic"),
        (_patched(b, 4, "<H", 2), "unsupported version"),
        (_patched(b, 6, "<H", 8), "block size"),
        (_patched(b, 8, "<I", 0), "bad size"),
        (b[:10], "truncated"),
        (b[:-4], "truncated"),
        (b + b"\0", "over-long"),
        (_patched(b, H + 3, "<H", struct.unpack_from("<H", b, H + 3)[0] + 1), "sums to"),
        (_patched(b, H + 3, "<H", 0), "without a frequency"),
        (_patched(b, H, "<H", 1), "lists 1 symbols"),
        (_patched(b, 8, "<I", 40), "truncated|class|chunk"),      # another plane's block count
        (_patched(b, cls_at, "<H", 1), "coded blocks, the header"),
        (_patched(b, cls_at, "<H", 2), "unknown block class"),
        (_patched(b, cls_at + 12, "<H", 1), "word count is impossible"),
        (_patched(b, 20, "<I", f["payload"].size + 1), "sums to|truncated"),
    ]
    for bad, pattern in cases:
        with pytest.raises(RuntimeError, match=pattern):
            ax.parse_alpha_planes(bad)
    for fn, arg in ((ax.encode_alpha_planes, [a]), (ax.decode_alpha_planes, [b])):
        with pytest.raises(RuntimeError, match="GPU"):
            fn(arg, device="cpu")


def test_rgax_parser(blob):
    from rgbac import anysize, rgbaexact as rx, rgbafile as rf
    info = rf.CodecInfo(0x0BADF00D, False, 192, 10, 8)
    h, w = blob[0].shape
    z, y = (_container(s, 64, 3 + i) for i, s in enumerate(rf._segments(info, *anysize.padded_size(h, w))))
    good = rx.build_rgba_exact(h, w, 64, "mixed", info, [blob[1], z, y])
    f = rx.parse_rgba_exact(good, info)
    assert (f["h"], f["w"], f["chunk"], f["opaque"], f["transparent"]) == (h, w, 64, False, False)
    assert f["alpha"]["payload"].size and f["rgb_y"].K == 64
    opaque = rx.build_rgba_exact(h, w, 64, "opaque", info, [b"", z, y])
    assert rx.parse_rgba_exact(opaque, info)["alpha"] is None
    blank = rx.build_rgba_exact(h, w, 64, "transparent", info, [b""] * 3)
    assert len(blank) == rx.HEADER_BYTES and rx.parse_rgba_exact(blank, info)["transparent"]
    A = rx.HEADER_BYTES
    cases = [
        (b"RGAF" + good[4:], "bad magic"),
        (_patched(good, 4, "<H", 2), "unsupported version"),
        (_patched(good, 6, "<H", 2), "unknown flags"),
        (_patched(good, 6, "<H", 9), "unknown flags"),
        (good[:20], "truncated"),
        (good[:-4], "truncated"),
        (good + b"\0\0\0\0", "over-long"),
        (_patched(good, 6, "<H", 1), "do not allow"),            # opaque, yet an alpha blob
        (_patched(opaque, 6, "<H", 0), "ask for is empty"),
        (_patched(good, 6, "<H", 4), "bf16"),
        (_patched(good, 20, "<I", 1), "other weights"),
        (_patched(good, 8, "<I", 21), "alpha plane is|alpha planes"),
        (_patched(good, 16, "<I", 32), "needs"),
        (_patched(good, A, "<I", 0), "alpha planes: bad magic"),
        (_patched(good, A + len(blob[1]), "<I", 0), "chunked stream: bad magic"),
    ]
    for bad, pattern in cases:
        with pytest.raises(RuntimeError, match=pattern):
            rx.parse_rgba_exact(bad, info)
