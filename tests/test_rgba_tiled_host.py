"""CPU: the host half of tiled RGBA files (rgbac/tiling.py, rgbac/rgbatile.py).

* tile_grid: the three properties the format rests on, exhaustively over small axes, and the
  refusals;
* the blend weights and the numpy twin of the blend kernel (blend_tiles_host);
* the tiled file: build -> parse round trip, every rejection the parser promises, tiled_info;
* region -> tile selection.
"""
import struct

import numpy as np
import pytest

from rans_chunk_cases import _gauss_symbols, gauss

TILES = (64, 128, 256)


def _overlaps(tile):
    return sorted({0, 2, 16, 32, tile // 2})


# ------------------------------------------------------------------ geometry
def test_tile_axis_properties_exhaustive():
    from rgbac.tiling import tile_axis
    for tile in TILES:
        for overlap in _overlaps(tile):
            S = tile - overlap
            for n in range(1, 601):
                ax = tile_axis(n, tile, overlap)
                k = ax.k
                assert k == max(1, -(-(n - overlap) // S)) and len(ax.origins) == k
                assert ax.origins == [i * S for i in range(k)]
                assert ax.extents == [min(tile, n - o) for o in ax.origins]
                # every pixel is covered by one or two tiles
                cover = np.zeros(n, dtype=np.int64)
                for o, e in zip(ax.origins, ax.extents):
                    assert e >= 1 and o + e <= n
                    cover[o:o + e] += 1
                assert cover.min() >= 1 and cover.max() <= 2, (n, tile, overlap)
                # neighbours overlap by exactly `overlap` pixels, the last pair included
                for i in range(k - 1):
                    assert ax.origins[i] + ax.extents[i] - ax.origins[i + 1] == overlap
                assert int((cover == 2).sum()) == (k - 1) * overlap
                # the last tile's extent
                if k > 1:
                    assert overlap < ax.extents[-1] <= tile, (n, tile, overlap)
                else:
                    assert ax.extents == [n]


def test_tile_grid_numbering_and_canvases():
    from rgbac import anysize
    from rgbac.tiling import tile_grid, tile_rect
    g = tile_grid(200, 300, 128, 16)
    assert (g.ky, g.kx) == (2, 3)
    assert [tile_rect(g, t) for t in range(6)] == [
        (0, 0, 128, 128), (0, 112, 128, 128), (0, 224, 128, 76),
        (112, 0, 88, 128), (112, 112, 88, 128), (112, 224, 88, 76)]
    for h, w in ((1, 1), (256, 256), (257, 1000), (4096, 4096), (500, 375)):
        g = tile_grid(h, w)
        assert (g.tile, g.overlap) == (256, 32)
        canvases = {anysize.padded_size(*tile_rect(g, t)[2:]) for t in range(g.ky * g.kx)}
        assert len(canvases) <= 4
        if g.ky > 1 and g.kx > 1:
            assert (256, 256) in canvases


@pytest.mark.parametrize("args", [(10, 10, 0, 0), (10, 10, 100, 0), (10, 10, -64, 0),
                                  (10, 10, 96, 0), (10, 10, 128, 65), (10, 10, 128, -1),
                                  (0, 10, 128, 16), (10, 0, 128, 16), (10, -3, 128, 16)])
def test_tile_grid_refuses(args):
    from rgbac.tiling import tile_grid
    with pytest.raises(ValueError):
        tile_grid(*args)


# ------------------------------------------------------------------ weights and the twin
def test_blend_weights():
    from rgbac.tiling import axis_weights, tile_axis
    for n, tile, overlap in ((300, 128, 16), (300, 128, 64), (200, 128, 0), (77, 64, 2),
                             (600, 256, 32)):
        ax = tile_axis(n, tile, overlap)
        seen = {}
        for i, (o, e) in enumerate(zip(ax.origins, ax.extents)):
            w = axis_weights(ax, i, overlap, o, o + e)
            assert w.dtype == np.float32 and w.shape == (e,)
            for p, v in zip(range(o, o + e), w):
                seen.setdefault(p, []).append(v)
        for p in range(n):
            ws = seen[p]
            if len(ws) == 1:
                assert ws[0] == np.float32(1.0) and ws[0].tobytes() == np.float32(1).tobytes()
            else:
                j = min(p // (tile - overlap), ax.k - 1)
                r = (np.float32(p - ax.origins[j]) + np.float32(0.5)) / np.float32(overlap)
                assert ws[1] == r and ws[0] == np.float32(1.0) - r
                assert 0 < ws[0] < 1 and 0 < ws[1] < 1
        # a window of a tile gets the same weights as the whole tile
        if ax.k > 1:
            o, e = ax.origins[1], ax.extents[1]
            whole = axis_weights(ax, 1, overlap, o, o + e)
            assert np.array_equal(axis_weights(ax, 1, overlap, o + 3, o + e - 1), whole[3:e - 1])


def _planes(grid, value=None, alpha=None, seed=0):
    """{t: (x_hat, alpha)} on each tile's own canvas, NaN outside the tile's rectangle."""
    from rgbac.anysize import padded_size
    from rgbac.tiling import tile_rect
    rng = np.random.default_rng(seed)
    out = {}
    for t in range(grid.ky * grid.kx):
        _, _, ey, ex = tile_rect(grid, t)
        hp, wp = padded_size(ey, ex)
        x = np.full((3, hp, wp), np.nan, dtype=np.float32)
        a = np.full((hp, wp), np.nan, dtype=np.float32)
        x[:, :ey, :ex] = rng.random((3, ey, ex), dtype=np.float32) if value is None else value
        a[:ey, :ex] = rng.random((ey, ex), dtype=np.float32) if alpha is None else alpha
        out[t] = (x, a)
    return out


def test_blend_host_constant_planes():
    from rgbac.tiling import blend_tiles_host, quant_u8, tile_grid
    for overlap in (0, 16, 64):
        g = tile_grid(200, 300, 128, overlap)
        for v, a in ((0.25, 1.0), (0.6, 0.4), (1.0, 1.0 / 3)):
            out = blend_tiles_host(g, _planes(g, np.float32(v), np.float32(a)))
            assert out.shape == (200, 300, 4)
            # the weights of a pixel sum to 1 within an ulp or two: the byte is the constant's
            # unless the constant sits on a rounding tie (these do not)
            assert (out[..., :3] == quant_u8(np.float32(v))).all()
            assert (out[..., 3] == quant_u8(np.float32(a))).all()


def test_blend_host_single_tile_passes_through():
    from rgbac.tiling import blend_tiles_host, quant_u8, tile_grid
    g = tile_grid(100, 77, 128, 16)
    assert (g.ky, g.kx) == (1, 1)
    pl = _planes(g, seed=3)
    x, a = pl[0]
    a[:100, :77] = a[:100, :77] * 1.2 - 0.1                # some alpha <= 0 too
    out = blend_tiles_host(g, pl)
    want_a = quant_u8(a[:100, :77])
    assert np.array_equal(out[..., 3], want_a)
    for c in range(3):
        assert np.array_equal(out[..., c], np.where(want_a > 0, quant_u8(x[c, :100, :77]), 0))
    assert (want_a == 0).any() and (want_a > 0).any()
    # without an alpha plane the tile is opaque
    out = blend_tiles_host(g, {0: (x, None)})
    assert (out[..., 3] == 255).all() and np.array_equal(out[..., 0], quant_u8(x[0, :100, :77]))
    # and a region of it is the crop
    full = blend_tiles_host(g, pl)
    assert np.array_equal(blend_tiles_host(g, pl, (10, 20, 30, 40)), full[10:40, 20:60])


def test_blend_host_colour_comes_from_the_tile_with_alpha():
    from rgbac.tiling import blend_tiles_host, quant_u8, tile_grid
    g = tile_grid(128, 240, 128, 16)                        # 1 x 2 tiles, columns 112..127 shared
    assert (g.ky, g.kx) == (1, 2)
    pl = _planes(g, seed=5)
    pl[0] = (np.full_like(pl[0][0], 0.9), np.zeros_like(pl[0][1]))       # alpha 0: no colour
    pl[1] = (np.full_like(pl[1][0], 0.2), np.ones_like(pl[1][1]))
    out = blend_tiles_host(g, pl)
    seam = out[:, 112:128]
    assert (seam[..., :3] == quant_u8(np.float32(0.2))).all()            # not a mix with 0.9
    r = (np.arange(16, dtype=np.float32) + np.float32(0.5)) / np.float32(16)
    assert np.array_equal(seam[0, :, 3], quant_u8(r))                    # alpha does fade
    assert (out[:, :112] == 0).all() and (out[:, 128:, 3] == 255).all()
    # a missing (transparent / not decoded) tile behaves as alpha 0
    out2 = blend_tiles_host(g, {1: pl[1]})
    assert np.array_equal(out2, out)


# ------------------------------------------------------------------ region -> tiles
def test_region_tiles():
    from rgbac.tiling import check_region, region_tiles, tile_grid
    g = tile_grid(200, 300, 128, 16)
    assert region_tiles(g) == [0, 1, 2, 3, 4, 5]
    assert region_tiles(g, (100, 105, 50, 130)) == [0, 1, 2, 3, 4, 5]
    assert region_tiles(g, (0, 0, 112, 112)) == [0]
    assert region_tiles(g, (0, 0, 113, 112)) == [0, 3]
    assert region_tiles(g, (127, 127, 1, 1)) == [0, 1, 3, 4]
    assert region_tiles(g, (128, 240, 72, 60)) == [5]
    assert region_tiles(g, (199, 0, 1, 300)) == [3, 4, 5]
    assert check_region(g, None) == (0, 0, 200, 300)
    for bad in ((-1, 0, 5, 5), (0, 0, 201, 5), (0, 295, 5, 6), (0, 0, 0, 5), (200, 0, 1, 1)):
        with pytest.raises(ValueError):
            region_tiles(g, bad)
    # brute force: a tile is selected exactly when its rectangle meets the region
    from rgbac.tiling import tile_rect
    rng = np.random.default_rng(1)
    g = tile_grid(333, 150, 64, 32)
    for _ in range(200):
        y0, x0 = int(rng.integers(0, 333)), int(rng.integers(0, 150))
        hr, wr = int(rng.integers(1, 334 - y0)), int(rng.integers(1, 151 - x0))
        want = []
        for t in range(g.ky * g.kx):
            oy, ox, ey, ex = tile_rect(g, t)
            if oy < y0 + hr and oy + ey > y0 and ox < x0 + wr and ox + ex > x0:
                want.append(t)
        assert region_tiles(g, (y0, x0, hr, wr)) == want


# ------------------------------------------------------------------ the file
@pytest.fixture(scope="module")
def infos():
    from rgbac.rgbafile import CodecInfo
    return (CodecInfo(0x1234ABCD, False, 192, 5, 16), CodecInfo(0x0BADF00D, False, 192, 10, 8))


def _container(seg_lengths, chunk, seed):
    from rgbac.ans import encode_chunked_host
    sym, idx = _gauss_symbols(int(sum(seg_lengths)), seed)
    return encode_chunked_host(sym, idx, gauss().tables, seg_lengths, chunk)


KINDS6 = ["transparent", "mixed", "opaque", "mixed", "mixed", "opaque"]


def _file(infos, h=100, w=200, tile=64, overlap=16, chunk=64, kinds=KINDS6):
    """A valid tiled file of host-coded containers, one kind per tile (100 x 150 at tile 64 and
    overlap 16 is a 2 x 3 grid), and the sections it was built from."""
    from rgbac import anysize, rgbafile as rf, rgbatile as rt_, tiling
    g = tiling.tile_grid(h, w, tile, overlap)
    assert g.ky * g.kx == len(kinds)
    secs = []
    for t, kind in enumerate(kinds):
        if kind == "transparent":
            secs.append(None)
            continue
        hp, wp = anysize.padded_size(*tiling.tile_rect(g, t)[2:])
        az, ay = rf._segments(infos[0], hp, wp)
        rz, ry = rf._segments(infos[1], hp, wp)
        s = [b"", b""] if kind == "opaque" else [_container(az, chunk, 10 * t + 1),
                                                 _container(ay, chunk, 10 * t + 2)]
        secs.append(s + [_container(rz, chunk, 10 * t + 3), _container(ry, chunk, 10 * t + 4)])
    return rt_.build_rgba_tiled(h, w, tile, overlap, chunk, infos[0], infos[1], secs), secs


@pytest.fixture(scope="module")
def tiled(infos):
    return _file(infos, 100, 150)


def test_tiled_round_trip_and_info(infos, tiled):
    from rgbac import rgbatile as rt_
    blob, secs = tiled
    assert rt_.HEADER_BYTES == 40 and blob[:4] == b"RGAT"
    table = 40 + 16 * 6
    assert len(blob) == table + sum(len(s) for ss in secs if ss for s in ss)
    f = rt_.parse_rgba_tiled(blob, *infos)
    assert (f["h"], f["w"], f["tile"], f["overlap"], f["chunk"]) == (100, 150, 64, 16, 64)
    assert (f["grid"].ky, f["grid"].kx) == (2, 3) and f["kinds"] == KINDS6
    assert sorted(f["tiles"]) == list(range(6)) and f["tiles"][0] is None
    pos = table
    for t, ss in enumerate(secs):
        rec = f["tiles"][t]
        if ss is None:
            assert f["lengths"][t].tolist() == [0, 0, 0, 0]
            continue
        assert rec["opaque"] == (KINDS6[t] == "opaque") and rec["chunk"] == 64
        assert (rec["h"], rec["w"]) == ((64, 52)[t // 3], (64, 64, 54)[t % 3])
        assert rec["canvas"] == (64, 64)
        for name, s, off in zip(rt_.SECTIONS, ss, f["offsets"][t].tolist()):
            assert off == pos and blob[off:off + len(s)] == s
            assert (rec[name] is None) == (not s)
            pos += len(s)
        assert rec["rgb_y"].seg_lengths.tolist() == [8 * 64] * 10
    # only the tiles asked for are parsed
    part = rt_.parse_rgba_tiled(blob, *infos, tiles=[4, 0])
    assert sorted(part["tiles"]) == [0, 4] and part["tiles"][4]["rgb_z"].K == 64
    # an all-opaque / transparent file is accepted whatever the alpha codec at hand
    ob, _ = _file(infos, 100, 150, kinds=["opaque", "transparent"] * 3)
    rt_.parse_rgba_tiled(ob, infos[0]._replace(crc=1, bf16=True), infos[1])
    info = rt_.tiled_info(blob)
    assert info["grid"] == (2, 3) and info["kinds"] == KINDS6 and info["bytes"] == len(blob)
    assert (info["h"], info["w"], info["tile"], info["overlap"], info["chunk"]) == (100, 150, 64, 16, 64)
    assert info["header_bytes"] == table
    assert info["tile_bytes"] == [tuple(len(s) for s in ss) if ss else (0, 0, 0, 0) for ss in secs]
    assert info["rects"][5] == (48, 96, 52, 54)
    # a fully transparent image: header and table only
    tb = rt_.build_rgba_tiled(100, 150, 64, 16, 64, infos[0], infos[1], [None] * 6)
    assert len(tb) == table and rt_.tiled_info(tb)["kinds"] == ["transparent"] * 6
    assert all(v is None for v in rt_.parse_rgba_tiled(tb, *infos)["tiles"].values())


def test_tiled_parser_rejections(infos, tiled):
    from rgbac import rgbatile as rt_
    from rgbac.rgbafile import FLAG_ALPHA_BF16, FLAG_RGB_BF16
    blob, secs = tiled
    T = 40                                                    # the table's start

    def rejects(bad, pattern, a=infos[0], r=infos[1]):
        with pytest.raises(RuntimeError, match=pattern):
            rt_.parse_rgba_tiled(bytes(bad), a, r)

    def patched(off, fmt, value, base=blob):
        b = bytearray(base)
        struct.pack_into(fmt, b, off, value)
        return b

    flip = bytearray(blob)
    flip[0] ^= 1
    rejects(flip, "bad magic")
    rejects(b"RGAF" + blob[4:], "bad magic")
    rejects(patched(4, "<H", 2), "unsupported version")
    rejects(patched(6, "<H", 1), "unknown flags")            # RGAF's opaque bit means nothing here
    rejects(patched(6, "<H", 8), "unknown flags")
    rejects(blob[:20], "truncated")                          # inside the header
    rejects(blob[:T + 20], "truncated inside the tile table")
    rejects(blob[:-4], "truncated")                          # inside the last section
    rejects(blob + b"\0\0\0\0", "over-long")
    rejects(patched(8, "<I", 0), "bad size")
    rejects(patched(24, "<I", 0), "chunk size 0")
    # tile / overlap that tile_grid refuses
    rejects(patched(16, "<I", 0), "bad tile geometry")
    rejects(patched(16, "<I", 96), "bad tile geometry")
    rejects(patched(20, "<I", 33), "bad tile geometry")
    # a tile count that is not the grid's, and sizes whose grid is another one
    rejects(patched(36, "<I", 5), "tiles in the header")
    rejects(patched(12, "<I", 300), "tiles in the header")
    rejects(patched(8, "<I", 64), "tiles in the header")
    # a size with the same grid but another canvas for the last tile (128 x 38 -> 128 x 118):
    # its containers' segments are not the ones that canvas implies
    wide, _ = _file(infos, 100, 150, tile=128, kinds=["opaque", "opaque"])
    rt_.parse_rgba_tiled(wide, *infos)
    rejects(patched(12, "<I", 230, base=wide), "needs")
    # lengths that are none of the three kinds
    (l_ay,) = struct.unpack_from("<I", blob, T + 16 * 1 + 4)
    rejects(patched(T + 16 * 1 + 4, "<I", 0), "over-long")
    b = bytearray(blob)
    struct.pack_into("<I", b, T + 16 * 1 + 0, struct.unpack_from("<I", blob, T + 16)[0] + l_ay)
    struct.pack_into("<I", b, T + 16 * 1 + 4, 0)             # the sum fits, the kind does not exist
    rejects(b, "neither transparent, opaque nor mixed")
    # one length off by a word; two traded against each other
    (l2,) = struct.unpack_from("<I", blob, T + 16 * 2 + 8)
    (l3,) = struct.unpack_from("<I", blob, T + 16 * 2 + 12)
    rejects(patched(T + 16 * 2 + 8, "<I", l2 + 4), "section lengths say")
    b = patched(T + 16 * 2 + 8, "<I", l2 + 4)
    struct.pack_into("<I", b, T + 16 * 2 + 12, l3 - 4)
    rejects(b, "chunked stream|segments|needs")
    # the chunk size field disagrees with the containers'
    rejects(patched(24, "<I", 128), "needs")
    # a segment count changed inside a container (tile 1's alpha z, its own header word 3)
    b = bytearray(blob)
    struct.pack_into("<I", b, T + 16 * 6 + 12, 2)
    rejects(b, "chunked stream|needs")
    # CRC and dtype against the models given
    rejects(patched(28, "<I", 0x1234ABCC), "alpha codec's CDF tables differ")
    rejects(patched(32, "<I", 0), "RGB codec's CDF tables differ")
    rejects(blob, "RGB codec's CDF tables differ", r=infos[1]._replace(crc=5))
    rejects(patched(6, "<H", FLAG_ALPHA_BF16), "alpha codec in bf16")
    rejects(patched(6, "<H", FLAG_RGB_BF16), "RGB codec in bf16")
    rejects(blob, "RGB codec in fp32", r=infos[1]._replace(bf16=True))
    # tiled_info needs no models but refuses the same broken headers
    with pytest.raises(RuntimeError, match="bad magic"):
        rt_.tiled_info(bytes(flip))
    with pytest.raises(RuntimeError, match="truncated"):
        rt_.tiled_info(blob[:-1])


# ------------------------------------------------------------------ the C entry points
_P = 4096                                                     # non-null, never dereferenced
_GOOD = {"rgbac_rgba_alpha_class": [2, _P, _P, _P, None],
         "rgbac_rgba_blend_tiles": [2, _P, 6, _P, 1000, None]}


@pytest.mark.parametrize("name,idx,value,msg", [
    ("rgbac_rgba_alpha_class", 0, 0, "batch"),
    ("rgbac_rgba_alpha_class", 0, 65536, "batch"),
    ("rgbac_rgba_alpha_class", 1, None, "null pointer"),
    ("rgbac_rgba_alpha_class", 2, None, "null pointer"),
    ("rgbac_rgba_alpha_class", 3, None, "null pointer"),
    ("rgbac_rgba_blend_tiles", 0, 0, "output count"),
    ("rgbac_rgba_blend_tiles", 0, 65536, "output count"),
    ("rgbac_rgba_blend_tiles", 1, None, "null descriptor"),
    ("rgbac_rgba_blend_tiles", 2, 0, "tile count"),
    ("rgbac_rgba_blend_tiles", 3, None, "null descriptor"),
    ("rgbac_rgba_blend_tiles", 4, 0, "max_pixels"),
])
def test_argument_errors_are_reported_without_launching(name, idx, value, msg):
    from rgbac import _lib
    args = list(_GOOD[name])
    args[idx] = value
    with pytest.raises(RuntimeError, match=f"{name} failed.*{msg}"):
        _lib.call(name, *args)


@pytest.mark.parametrize("pyname,cname,size", [("TileDesc", "rgbac_tile_desc", 40),
                                               ("BlendDesc", "rgbac_blend_desc", 56)])
def test_descriptor_layouts_match_c(tmp_path, pyname, cname, size):
    """Compile a probe against include/rgbac.h with gcc and compare offsets with ctypes."""
    import ctypes
    import os
    import subprocess
    from rgbac import _lib
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                          "include", "rgbac.h")
    cls = getattr(_lib, pyname)
    fields = [f for f, _ in cls._fields_]
    src = tmp_path / "probe.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"',
             'int main(void){', f'printf("%zu\\n", sizeof({cname}));']
    lines += [f'printf("%zu\\n", offsetof({cname}, {f}));' for f in fields]
    lines += ['return 0;}']
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-O0", str(src), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True,
                                           text=True).stdout.split()]
    assert vals[0] == ctypes.sizeof(cls) == size
    for f, off in zip(fields, vals[1:]):
        assert getattr(cls, f).offset == off, f
