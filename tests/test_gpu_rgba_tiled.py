"""GPU: tiled RGBA files (rgbac/rgbatile.py) and the two kernels under them.

* rgbac_rgba_alpha_class against torch on the same bytes, class 1 against rgbac_rgba_opaque;
* rgbac_rgba_blend_tiles against its numpy twin (rgbac.tiling.blend_tiles_host), byte for byte:
  smaller edge tiles, the overlap limit, planted rounding ties, NaN outside every tile's
  rectangle (nothing there is read), a pre-filled output (nothing outside is written);
* the file codec: a tile's sections are encode_rgba's of that crop; a file decodes alone, in any
  batch, in any order and with any max_batch to the same bytes; a region decode is the crop of
  the full decode and decodes only what it touches; the full decode is the twin's blend of the
  decoded planes; errors.

The nets are the benchmark's (random init, latent gain 20, update() called), as in
test_gpu_rgba_file.py.
"""
import struct

import numpy as np
import pytest
import torch

from test_gpu_rgba_file import _rgba

pytestmark = pytest.mark.gpu

TILE, OVERLAP = 128, 16
REGION = (100, 105, 50, 130)


# ------------------------------------------------------------------ rgbac_rgba_alpha_class
def test_alpha_class_against_torch(device):
    from rgbac import anysize
    images = []
    for s, (h, w) in enumerate([(1, 1), (5, 7), (64, 64), (70, 129)]):
        for kind in ("opaque", "zero", "last254", "first1"):
            im = _rgba(h, w, "zero" if kind in ("zero", "first1") else "opaque", 40 + s)
            if kind == "last254":
                im[h - 1, w - 1, 3] = 254
            if kind == "first1":
                im[0, 0, 3] = 1
            images.append(im)
    # strided views of larger buffers whose outside pixels would change the answer
    big = _rgba(80, 140, "opaque", 50).to(device)
    big[2, 5:134, 3] = 0
    big[3:73, 4, 3] = 7
    big[73, 133, 3] = 0
    images.append(big[3:3 + 70, 5:5 + 129])                  # opaque inside
    zero = _rgba(80, 140, "zero", 51).to(device)
    zero[3:73, 134, 3] = 255
    zero[73, 5:134, 3] = 1
    images.append(zero[3:3 + 70, 5:5 + 129])                 # transparent inside
    mixed = zero.clone()
    mixed[3 + 69, 5 + 128, 3] = 9                            # the view's last pixel
    images.append(mixed[3:3 + 70, 5:5 + 129])

    def want(im):
        a = torch.as_tensor(im)[..., 3]
        return 1 if bool((a == 255).all()) else 2 if bool((a == 0).all()) else 0
    expect = [want(im) for im in images]
    assert expect[:8] == [1, 2, 0, 0, 1, 2, 0, 0] and expect[-3:] == [1, 2, 0]
    # a 1 x 1 image: "last254" and "first1" are the one pixel
    cls = anysize.alpha_class(images, device=device)
    assert cls.dtype == torch.int32 and cls.cpu().tolist() == expect
    flags = anysize.opaque_flags(images, device=device)
    assert torch.equal((cls == 1).to(torch.int32), flags)


# ------------------------------------------------------------------ rgbac_rgba_blend_tiles
def _ties():
    """Every rounding tie (k + 0.5) / 255 of the quantiser with its two fp32 neighbours."""
    t = (np.arange(255, dtype=np.float32) + np.float32(0.5)) / np.float32(255)
    return np.concatenate([t, np.nextafter(t, np.float32(-1)), np.nextafter(t, np.float32(2))])


def _blend_planes(grid, seed):
    from rgbac.anysize import padded_size
    from rgbac.tiling import tile_rect
    rng = np.random.default_rng(seed)
    ties = _ties()
    planes = {}
    for t in range(grid.ky * grid.kx):
        _, _, ey, ex = tile_rect(grid, t)
        hp, wp = padded_size(ey, ex)
        x = np.full((4, hp, wp), np.nan, dtype=np.float32)    # 3 colour planes + alpha
        v = (rng.random((4, ey, ex), dtype=np.float32) * np.float32(1.2) - np.float32(0.1))
        for c in range(4):
            at = rng.choice(ey * ex, size=ties.size, replace=False)
            v[c].reshape(-1)[at] = ties
        x[:, :ey, :ex] = v
        planes[t] = (x[:3].copy(), x[3].copy())
    return planes


@pytest.mark.parametrize("overlap", [0, 16, 64])
def test_blend_tiles_kernel_exact(device, overlap):
    """Image 200 x 300 at tile 128: 2 x 3 tiles at overlap 0 and 16, 3 x 4 at the limit 64, the
    last row and column smaller; the tile at grid (1, 1) is null (transparent), tile 2 has no
    alpha plane (opaque).  Two outputs in one launch -- the whole image and a region that
    crosses overlaps on both axes -- each into the middle of a pre-filled buffer."""
    from rgbac import _lib
    from rgbac.tiling import blend_tiles_host, tile_grid, tile_rect
    g = tile_grid(200, 300, TILE, overlap)
    assert (g.ky, g.kx) == ((3, 4) if overlap == 64 else (2, 3))
    n = g.ky * g.kx
    host = _blend_planes(g, 7 + overlap)
    host[2] = (host[2][0], None)
    host[g.kx + 1] = None
    rects = [(0, 0, 200, 300), REGION]
    want = [blend_tiles_host(g, host, r) for r in rects]
    # the overlaps do blend, and not every pixel is trivial
    assert want[0][..., 3].min() == 0 and want[0][..., 3].max() == 255

    dev_planes, tdesc = {}, (_lib.TileDesc * (2 * n))()
    for rep in range(2):                                     # each output has its own table slice
        for t in range(n):
            oy, ox, ey, ex = tile_rect(g, t)
            if host[t] is None:
                tdesc[n * rep + t] = _lib.TileDesc(None, None, 0, 0, oy, ox, ey, ex)
                continue
            x, a = host[t]
            xd = torch.from_numpy(x).to(device)
            ad = None if a is None else torch.from_numpy(a).to(device)
            dev_planes[(rep, t)] = (xd, ad)
            tdesc[n * rep + t] = _lib.TileDesc(xd.data_ptr(), _lib.ptr(ad), x.shape[1], x.shape[2],
                                               oy, ox, ey, ex)
    PAD, FILL = 3, 0xAB
    bufs, odesc = [], (_lib.BlendDesc * 2)()
    for k, (y0, x0, hr, wr) in enumerate(rects):
        buf = torch.full((hr + 2 * PAD, wr + 2 * PAD, 4), FILL, dtype=torch.uint8, device=device)
        bufs.append(buf)
        first = buf.data_ptr() + PAD * buf.stride(0) + PAD * 4
        odesc[k] = _lib.BlendDesc(_lib.ImageDesc(first, hr, wr, buf.stride(0)), n * k, g.ky, g.kx,
                                  g.tile, g.overlap, y0, x0, 0)
    td = torch.frombuffer(bytearray(bytes(tdesc)), dtype=torch.uint8).to(device)
    od = torch.frombuffer(bytearray(bytes(odesc)), dtype=torch.uint8).to(device)
    _lib.call("rgbac_rgba_blend_tiles", 2, od.data_ptr(), 2 * n, td.data_ptr(), 200 * 300,
              _lib.stream_ptr(device))
    torch.cuda.synchronize()
    for k, (y0, x0, hr, wr) in enumerate(rects):
        got = bufs[k].cpu().numpy()
        inner = got[PAD:PAD + hr, PAD:PAD + wr]
        bad = np.argwhere((inner != want[k]).any(axis=2))
        assert bad.size == 0, (overlap, k, len(bad), bad[:5].tolist())
        frame = got.copy()
        frame[PAD:PAD + hr, PAD:PAD + wr] = FILL
        assert (frame == FILL).all(), (overlap, k, "a byte outside the rectangle was written")
    # the region is the crop of the whole image
    y0, x0, hr, wr = REGION
    assert np.array_equal(want[1], want[0][y0:y0 + hr, x0:x0 + wr])


def test_blend_single_tile_is_unpack(device):
    """A pixel covered by one tile gets the bytes rgbac_rgba_unpack writes for that tile."""
    from rgbac import anysize, rgbatile
    from rgbac.tiling import tile_grid
    g = tile_grid(100, 77, TILE, OVERLAP)
    x, a = _blend_planes(g, 3)[0]
    xd = torch.nan_to_num(torch.from_numpy(x)).to(device)
    ad = torch.nan_to_num(torch.from_numpy(a)).to(device)
    for alpha in (ad, None):
        got = rgbatile.blend_tiles(g, {0: (xd, alpha)})
        ref = anysize.unpack_rgba(xd[None], None if alpha is None else alpha[None, None], [(100, 77)])
        assert torch.equal(got, ref[0])


# ------------------------------------------------------------------ the file codec
@pytest.fixture(scope="module")
def nets(device):
    from bench import mask_net, rgb_net
    masknet, net = mask_net(), rgb_net()
    masknet.update()
    net.update()
    return masknet.to(device), net.to(device)


def _images():
    a = _rgba(200, 300, "ramp", 21)
    yy, xx = torch.meshgrid(torch.arange(200), torch.arange(300), indexing="ij")
    alpha = a[..., 3].clone()
    alpha[(yy < 128) & (xx < 128)] = 0                       # tile (0, 0) is transparent
    alpha[(yy >= 112) & (xx >= 224)] = 255                   # tile (1, 2) is opaque
    a[..., 3] = alpha
    return [a, _rgba(128, 128, "opaque", 22), _rgba(100, 77, "ramp", 23)]


def _sections(blob):
    """{t: [four section bytes]} of a tiled file, read off the table."""
    from rgbac.rgbatile import _parse_head
    head = _parse_head(blob)
    return {t: [blob[o:o + n] for o, n in zip(head["offsets"][t].tolist(), head["lengths"][t].tolist())]
            for t in range(len(head["kinds"]))}


def _file_sections(blob):
    lens = struct.unpack_from("<4I", blob, 28)
    out, pos = [], 44
    for n in lens:
        out.append(blob[pos:pos + n])
        pos += n
    return out


@pytest.fixture(scope="module")
def shared(nets):
    from rgbac.rgbatile import decode_rgba_tiled, encode_rgba_tiled
    masknet, net = nets
    images = _images()
    enc = []
    files = encode_rgba_tiled(masknet, net, images, tile=TILE, overlap=OVERLAP, debug=enc)
    dbg = []
    outs = decode_rgba_tiled(masknet, net, files, debug=dbg)
    torch.cuda.synchronize()
    return {"images": images, "files": files, "enc": enc, "outs": outs, "dbg": dbg}


def test_tile_sections_are_encode_rgba_of_the_crop(shared, nets):
    from rgbac.rgbafile import encode_rgba
    from rgbac.rgbatile import tiled_info
    masknet, net = nets
    images, files = shared["images"], shared["files"]
    info = tiled_info(files[0])
    assert info["grid"] == (2, 3)
    assert info["kinds"] == ["transparent", "mixed", "mixed", "mixed", "mixed", "opaque"]
    assert shared["enc"][0]["cls"] == [2, 0, 0, 0, 0, 1]
    assert info["tile_bytes"][0] == (0, 0, 0, 0)
    assert info["tile_bytes"][5][:2] == (0, 0) and all(info["tile_bytes"][5][2:])
    assert tiled_info(files[1])["kinds"] == ["opaque"] and tiled_info(files[2])["kinds"] == ["mixed"]
    crops, where = [], []
    for k, blob in enumerate(files):
        inf = tiled_info(blob)
        for t, (oy, ox, ey, ex) in enumerate(inf["rects"]):
            if inf["kinds"][t] != "transparent":
                crops.append(images[k][oy:oy + ey, ox:ox + ex])
                where.append((k, t))
    assert len(crops) == 7
    singles = encode_rgba(masknet, net, crops)
    secs = [_sections(b) for b in files]
    nonzero = 0
    for (k, t), one in zip(where, singles):
        assert secs[k][t] == _file_sections(one), (k, t)
        nonzero += sum(map(len, secs[k][t]))
    assert sum(map(len, files)) == nonzero + sum(tiled_info(b)["header_bytes"] for b in files)
    y = torch.cat([r["rgb"]["y"].reshape(-1) for e in shared["enc"] for r in e["tiles"].values()])
    assert (y != 0).float().mean().item() > 0.10, "the latents are (nearly) all zero"


def test_single_tile_images_decode_as_rgba_files(shared, nets):
    from rgbac.rgbafile import decode_rgba, encode_rgba
    masknet, net = nets
    ref = decode_rgba(masknet, net, encode_rgba(masknet, net, shared["images"][1:]))
    for k in (1, 2):
        assert shared["outs"][k].shape == shared["images"][k].shape
        assert torch.equal(shared["outs"][k], ref[k - 1]), k
    assert bool((shared["outs"][1][..., 3] == 255).all())


def test_alone_together_reversed_and_max_batch(shared, nets):
    from rgbac.rgbatile import decode_rgba_tiled
    masknet, net = nets
    files, outs = shared["files"], shared["outs"]
    assert [tuple(o.shape) for o in outs] == [(200, 300, 4), (128, 128, 4), (100, 77, 4)]
    for k, blob in enumerate(files):
        assert torch.equal(decode_rgba_tiled(masknet, net, [blob])[0], outs[k]), k
    rev = decode_rgba_tiled(masknet, net, files[::-1])
    for k in range(3):
        assert torch.equal(rev[2 - k], outs[k]), k
    small = decode_rgba_tiled(masknet, net, files, max_batch=2)
    for k in range(3):
        assert torch.equal(small[k], outs[k]), k


def test_max_batch_does_not_change_the_files(shared, nets):
    from rgbac.rgbatile import encode_rgba_tiled
    masknet, net = nets
    again = encode_rgba_tiled(masknet, net, shared["images"][::-1], tile=TILE, overlap=OVERLAP,
                              max_batch=2)
    assert again[::-1] == shared["files"]


def test_region_decode_is_the_crop(shared, nets):
    from rgbac.rgbatile import decode_rgba_tiled
    masknet, net = nets
    full = shared["outs"][0]
    regions = [REGION, (150, 240, 40, 60), (10, 10, 50, 50), None]
    dbg = []
    got = decode_rgba_tiled(masknet, net, [shared["files"][0]] * 3 + [shared["files"][2]],
                            regions=regions, debug=dbg)
    for out, (y0, x0, hr, wr) in zip(got[:3], regions[:3]):
        assert out.shape == (hr, wr, 4)
        assert torch.equal(out, full[y0:y0 + hr, x0:x0 + wr]), (y0, x0, hr, wr)
    assert torch.equal(got[3], shared["outs"][2])
    assert dbg[0]["tiles"] == [1, 2, 3, 4, 5]                # all touch it; tile 0 stores nothing
    assert dbg[1]["tiles"] == [5] and sorted(dbg[1]["planes"]) == [5]
    assert dbg[2]["tiles"] == [] and not dbg[2]["planes"]    # inside the transparent tile
    assert not bool(got[2].any())
    assert bool(full[REGION[0]:, REGION[1]:].any())
    for bad in ((0, 0, 201, 10), (-1, 0, 5, 5), (0, 290, 5, 11), (0, 0, 0, 1)):
        with pytest.raises(ValueError):
            decode_rgba_tiled(masknet, net, shared["files"][:1], regions=[bad])


def test_full_decode_is_the_host_blend_of_the_planes(shared):
    from rgbac.tiling import blend_tiles_host
    d = shared["dbg"][0]
    assert d["tiles"] == [1, 2, 3, 4, 5] and d["planes"][5][1] is None
    planes = {t: (x.cpu().numpy(), None if a is None else a.cpu().numpy())
              for t, (x, a) in d["planes"].items()}
    want = blend_tiles_host(d["grid"], planes)
    got = shared["outs"][0].cpu().numpy()
    assert np.array_equal(got, want)
    assert not got[:112, :112].any()                         # only the transparent tile there
    assert (got[128:, 240:, 3] == 255).all()                 # only the opaque tile there


def test_fully_transparent_image(nets, device):
    from rgbac.rgbatile import decode_rgba_tiled, encode_rgba_tiled, tiled_info
    masknet, net = nets
    im = _rgba(130, 200, "zero", 31)
    (blob,) = encode_rgba_tiled(masknet, net, [im], tile=TILE, overlap=OVERLAP)
    info = tiled_info(blob)
    assert info["grid"] == (2, 2) and info["kinds"] == ["transparent"] * 4
    assert len(blob) == 40 + 16 * 4
    dbg = []
    (out,) = decode_rgba_tiled(masknet, net, [blob], debug=dbg)
    assert out.shape == (130, 200, 4) and not bool(out.any()) and dbg[0]["tiles"] == []


def test_errors(shared, nets):
    """A flipped word of one tile's RGB y payload is reported through the rANS error word (the
    word is chosen with the CPU twin of the decoder core, on slice 0, as test_gpu_rgba_file.py
    does); a broken header raises before any launch."""
    from rgbac import ans
    from rgbac.rgbafile import codec_info
    from rgbac.rgbatile import _parse_head, decode_rgba_tiled, parse_rgba_tiled
    masknet, net = nets
    blob = shared["files"][0]
    t = 3
    head = _parse_head(blob)
    lay = parse_rgba_tiled(blob, codec_info(masknet), codec_info(net), tiles=[t])["tiles"][t]["rgb_y"]
    sec = int(head["offsets"][t][3])
    n = int(head["lengths"][t][3])
    body = 4 + lay.seg_lengths.size + lay.counts.size         # words before the payload
    idx = shared["enc"][0]["tiles"][t]["rgb"]["idx"].cpu().numpy().reshape(-1)
    tab = net.gaussian_conditional.tables()
    words = np.frombuffer(blob[sec:sec + n], dtype="<u4")
    found = None
    for k in range(int(lay.counts[:int(lay.first[1])].sum())):
        bad = words.copy()
        bad[body + k] ^= 0xFFFFFFFF
        try:
            ans.decode_chunked_host(bad.tobytes(), idx, tab)
        except RuntimeError:
            found = k
            break
    assert found is not None, "no flipped word of slice 0 is noticed by the decoder core"
    broken = bytearray(blob)
    off = sec + 4 * (body + found)
    broken[off:off + 4] = bytes(b ^ 0xFF for b in broken[off:off + 4])
    with pytest.raises(RuntimeError, match="tiled RGBA file decode: error"):
        decode_rgba_tiled(masknet, net, [shared["files"][1], bytes(broken)])
    # a region that does not touch the broken tile still decodes
    out = decode_rgba_tiled(masknet, net, [bytes(broken)], regions=[(150, 240, 40, 60)])[0]
    assert torch.equal(out, shared["outs"][0][150:190, 240:300])
    # header errors: before any launch
    torch.cuda.synchronize()
    for patch, pattern in (((0, b"RGAF"), "bad magic"), ((36, struct.pack("<I", 5)), "tiles in the header"),
                           ((32, struct.pack("<I", 1)), "RGB codec's CDF tables differ")):
        b = bytearray(blob)
        b[patch[0]:patch[0] + len(patch[1])] = patch[1]
        with pytest.raises(RuntimeError, match=pattern):
            decode_rgba_tiled(masknet, net, [shared["files"][2], bytes(b)])
    with pytest.raises(RuntimeError, match="truncated"):
        decode_rgba_tiled(masknet, net, [blob[:-8]])


def test_bf16_round_trip(nets):
    """bf16: the round trip runs and the sizes are right; a tile's decoded symbols, CDF indexes
    and y_hat are identical decoded alone (a region that touches only it) and in the batch, and
    equal the encoder's -- what decodability rests on.  Whether the RGBA bytes are identical too
    is printed, not asserted (the synthesis in bf16 may depend on the batch)."""
    from rgbac.rgbatile import decode_rgba_tiled, encode_rgba_tiled
    masknet, net = nets
    masknet.set_compute_dtype(torch.bfloat16)
    net.set_compute_dtype(torch.bfloat16)
    try:
        images = _images()
        enc, dbg, alone = [], [], []
        files = encode_rgba_tiled(masknet, net, images, tile=TILE, overlap=OVERLAP, debug=enc)
        outs = decode_rgba_tiled(masknet, net, files, debug=dbg)
        part = decode_rgba_tiled(masknet, net, files[:1], regions=[(150, 240, 40, 60)], debug=alone)
        torch.cuda.synchronize()
    finally:
        masknet.set_compute_dtype(torch.float32)
        net.set_compute_dtype(torch.float32)
    assert [tuple(o.shape) for o in outs] == [tuple(im.shape) for im in images]
    assert struct.unpack_from("<H", files[0], 6)[0] == 2 | 4
    assert alone[0]["tiles"] == [5]
    for k, e in enumerate(enc):
        for t, rec in e["tiles"].items():
            for codec in ("rgb", "alpha"):
                if rec[codec] is None:
                    assert dbg[k]["records"][t][codec] is None
                    continue
                for key in ("z", "y", "idx", "YH"):
                    assert torch.equal(dbg[k]["records"][t][codec][key], rec[codec][key]), (k, t, codec, key)
    for key in ("z", "y", "idx", "YH"):
        assert torch.equal(alone[0]["records"][5]["rgb"][key], dbg[0]["records"][5]["rgb"][key]), key
    same = bool(torch.equal(part[0], outs[0][150:190, 240:300]))
    print(f"rgba-tiled bf16: the region's RGBA bytes equal the crop of the full decode: {same}")
