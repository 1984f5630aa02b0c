"""Tiled RGBA files: an image coded as a grid of fixed-size, overlapping tiles (DESIGN.md
section 23).  Every tile is an image of the RGBA file codec (rgbac.rgbafile, section 21): the
same chain, the same four chunked containers, its own canvas round_up(e_y, 64) x round_up(e_x, 64).

* Interior tiles of every image share the tile x tile canvas, so the tiles of a whole call --
  images of any mix of sizes -- form at most a handful of batches (``encode_rgba`` /
  ``decode_rgba`` need one pass per distinct canvas).
* Opacity is decided per tile (rgbac_rgba_alpha_class, one launch and one read for all tiles of
  all images): a fully transparent tile stores nothing, a fully opaque one carries no alpha
  stream.
* A region decodes from the tiles that touch it.  Under ``rt.fixed_tiles(per_image=True)`` a
  tile's decode does not depend on what it is batched with, so in fp32 a region decode is
  byte-identical to the same crop of the full decode.
* Decoded tiles are put together by rgbac_rgba_blend_tiles: a linear cross-fade over each
  overlap, alpha-aware (rgbac.tiling.blend_tiles_host states the rule), one launch for all the
  images and regions of a call.

File layout (little-endian): a 40-byte header (magic "RGAT", version, flags, H, W, tile,
overlap, chunk K, the two CDF-table CRCs, the tile count), a table of four u32 section byte
lengths per tile (alpha z, alpha y, RGB z, RGB y) in row-major tile order, then the sections of
all tiles back to back in table order.  All four lengths zero: a transparent tile; the alpha
lengths zero: an opaque tile; all non-zero: a mixed tile.  GPU only, except parse_rgba_tiled,
build_rgba_tiled and tiled_info.
"""
import collections
import struct

import numpy as np
import torch

from . import _lib, anysize, tiling
from .ans import ChunkedLayout, _raise_code
from .rgbafile import (FLAG_ALPHA_BF16, FLAG_RGB_BF16, SECTIONS, _decode_group, _encode_group,
                       _models, _segments, codec_info)

MAGIC = b"RGAT"
VERSION = 1
_HEADER = struct.Struct("<4sHHIIIIIIII")
HEADER_BYTES = _HEADER.size          # 40
KINDS = ("transparent", "opaque", "mixed")
_MAX_OUTPUTS = 65535                 # outputs per blend launch (the grid's y dimension)


def build_rgba_tiled(h, w, tile, overlap, chunk, alpha, rgb, tile_sections):
    """Header + table + sections -> bytes.  alpha / rgb: CodecInfo; tile_sections: per tile in
    row-major order its four containers' bytes in SECTIONS order (the alpha ones empty for an
    opaque tile), or None for a transparent tile."""
    grid = tiling.tile_grid(h, w, tile, overlap)
    tile_sections = list(tile_sections)
    if len(tile_sections) != grid.ky * grid.kx:
        raise ValueError(f"a {h}x{w} image has {grid.ky}x{grid.kx} tiles, got "
                         f"{len(tile_sections)} section sets")
    flags = (FLAG_ALPHA_BF16 if alpha.bf16 else 0) | (FLAG_RGB_BF16 if rgb.bf16 else 0)
    head = _HEADER.pack(MAGIC, VERSION, flags, grid.h, grid.w, grid.tile, grid.overlap, int(chunk),
                        alpha.crc, rgb.crc, grid.ky * grid.kx)
    lens, body = [], []
    for secs in tile_sections:
        secs = [b""] * 4 if secs is None else [bytes(s) for s in secs]
        if len(secs) != 4:
            raise ValueError("a tile has four sections")
        lens += [len(s) for s in secs]
        body += secs
    return head + struct.pack(f"<{len(lens)}I", *lens) + b"".join(body)


def _parse_head(blob):
    """Header and tile table, no models: everything that can be said without the codecs."""
    if len(blob) < HEADER_BYTES:
        raise RuntimeError(f"tiled RGBA file: truncated ({len(blob)} bytes, the header has "
                           f"{HEADER_BYTES})")
    magic, version, flags, h, w, tile, overlap, chunk, crc_a, crc_r, count = \
        _HEADER.unpack_from(blob)
    if magic != MAGIC:
        raise RuntimeError("tiled RGBA file: bad magic (not a tiled RGBA file)")
    if version != VERSION:
        raise RuntimeError(f"tiled RGBA file: unsupported version {version}")
    if flags & ~(FLAG_ALPHA_BF16 | FLAG_RGB_BF16):
        raise RuntimeError(f"tiled RGBA file: unknown flags {flags:#x}")
    if h < 1 or w < 1 or h >= 1 << 24 or w >= 1 << 24 or chunk < 1 or chunk >= 1 << 31:
        raise RuntimeError(f"tiled RGBA file: bad size {h}x{w} or chunk size {chunk}")
    if tile >= 1 << 24:
        raise RuntimeError(f"tiled RGBA file: bad tile size {tile}")
    try:
        grid = tiling.tile_grid(h, w, tile, overlap)
    except ValueError as e:
        raise RuntimeError(f"tiled RGBA file: bad tile geometry ({e})") from None
    if count != grid.ky * grid.kx:
        raise RuntimeError(f"tiled RGBA file: {count} tiles in the header, a {h}x{w} image with "
                           f"tile {tile} and overlap {overlap} has {grid.ky}x{grid.kx}")
    body = HEADER_BYTES + 16 * count
    if len(blob) < body:
        raise RuntimeError(f"tiled RGBA file: truncated inside the tile table ({len(blob)} "
                           f"bytes, header and table have {body})")
    lens = np.frombuffer(blob, dtype="<u4", count=4 * count, offset=HEADER_BYTES)
    lens = lens.astype(np.int64).reshape(count, 4)
    total = body + int(lens.sum())
    if total != len(blob):
        kind = "truncated" if len(blob) < total else "over-long"
        raise RuntimeError(f"tiled RGBA file: {kind}: the section lengths say {total} bytes, "
                           f"the file has {len(blob)}")
    kinds = []
    for t, (az, ay, rz, ry) in enumerate(lens.tolist()):
        if not (az or ay or rz or ry):
            kinds.append("transparent")
        elif not (az or ay) and rz and ry:
            kinds.append("opaque")
        elif az and ay and rz and ry:
            kinds.append("mixed")
        else:
            raise RuntimeError(f"tiled RGBA file: tile {t} has section lengths "
                               f"{[az, ay, rz, ry]}: neither transparent, opaque nor mixed")
    ends = body + np.cumsum(lens.reshape(-1))
    offsets = (ends - lens.reshape(-1)).reshape(count, 4)
    return {"h": h, "w": w, "tile": tile, "overlap": overlap, "chunk": chunk, "flags": flags,
            "crc": (crc_a, crc_r), "grid": grid, "kinds": kinds, "lengths": lens,
            "offsets": offsets}


def parse_rgba_tiled(blob, alpha, rgb, tiles=None):
    """bytes -> {"h", "w", "tile", "overlap", "chunk", "grid", "kinds", "lengths", "offsets",
    "tiles": {t: parsed tile}}: a parsed tile is None for a transparent one, else what
    rgbafile.parse_rgba_file returns for a file ({"h", "w", "canvas", "chunk", "opaque",
    SECTIONS...: ChunkedLayout or None}).  ``tiles``: the tiles whose containers are parsed
    (None: all) -- offsets follow from the table, so the others are not touched.
    Pure host code; raises RuntimeError on anything wrong: bad magic, version or flags, a
    truncated or over-long file, a tile size / overlap tile_grid refuses, a tile count that is
    not the grid's, section lengths that are none of the three kinds, a container whose chunk
    size or segment lengths are not what the tile's canvas implies, and a CRC or dtype that
    disagrees with the codecs given (alpha / rgb: CodecInfo; the alpha codec's are looked at
    only when some tile is mixed)."""
    blob = bytes(blob)
    head = _parse_head(blob)
    flags, (crc_a, crc_r) = head["flags"], head["crc"]
    checks = [("RGB", rgb, crc_r, bool(flags & FLAG_RGB_BF16))]
    if "mixed" in head["kinds"]:
        checks.append(("alpha", alpha, crc_a, bool(flags & FLAG_ALPHA_BF16)))
    for name, info, crc, bf16 in checks:
        if bf16 != info.bf16:
            raise RuntimeError(f"tiled RGBA file: coded with the {name} codec in "
                               f"{'bf16' if bf16 else 'fp32'}, the model given runs in "
                               f"{'bf16' if info.bf16 else 'fp32'} (compute dtype)")
        if crc != info.crc:
            raise RuntimeError(f"tiled RGBA file: the {name} codec's CDF tables differ from the "
                               f"encoder's (CRC {info.crc:#010x}, the file says {crc:#010x}): "
                               "other weights")
    grid, chunk = head["grid"], head["chunk"]
    count = grid.ky * grid.kx
    wanted = range(count) if tiles is None else sorted({int(t) for t in tiles})
    out = {k: head[k] for k in ("h", "w", "tile", "overlap", "chunk", "grid", "kinds", "lengths",
                                "offsets")}
    out["tiles"] = {}
    for t in wanted:
        if not 0 <= t < count:
            raise ValueError(f"tiled RGBA file: no tile {t} in a {grid.ky}x{grid.kx} grid")
        if head["kinds"][t] == "transparent":
            out["tiles"][t] = None
            continue
        _, _, ey, ex = tiling.tile_rect(grid, t)
        hp, wp = anysize.padded_size(ey, ex)
        rec = {"h": ey, "w": ex, "canvas": (hp, wp), "chunk": chunk,
               "opaque": head["kinds"][t] == "opaque"}
        want = dict(zip(SECTIONS, _segments(alpha, hp, wp) + _segments(rgb, hp, wp)))
        for name, pos, n in zip(SECTIONS, head["offsets"][t].tolist(), head["lengths"][t].tolist()):
            lay = None
            if n:
                lay = ChunkedLayout(blob[pos:pos + n])
                if lay.K != chunk or lay.seg_lengths.tolist() != want[name]:
                    raise RuntimeError(
                        f"tiled RGBA file: tile {t} section {name} has chunk size {lay.K} and "
                        f"segments {lay.seg_lengths.tolist()}; a {ey}x{ex} tile needs {chunk} "
                        f"and {want[name]}")
            rec[name] = lay
        out["tiles"][t] = rec
    return out


def tiled_info(blob):
    """Host only, no models: {"h", "w", "tile", "overlap", "chunk", "grid": (ky, kx), "kinds":
    per tile "transparent" / "opaque" / "mixed", "tile_bytes": per tile its four section byte
    counts, "rects": per tile (oy, ox, ey, ex), "header_bytes": header + table, "bytes"}."""
    blob = bytes(blob)
    head = _parse_head(blob)
    grid = head["grid"]
    n = grid.ky * grid.kx
    return {"h": head["h"], "w": head["w"], "tile": head["tile"], "overlap": head["overlap"],
            "chunk": head["chunk"], "grid": (grid.ky, grid.kx), "kinds": list(head["kinds"]),
            "tile_bytes": [tuple(r) for r in head["lengths"].tolist()],
            "rects": [tiling.tile_rect(grid, t) for t in range(n)],
            "header_bytes": HEADER_BYTES + 16 * n, "bytes": len(blob)}


def _upload(arr, dev):
    """A ctypes array of descriptors -> device bytes (one copy)."""
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)


def _batch_limit(max_batch, who):
    max_batch = int(max_batch)
    if max_batch < 1:
        raise ValueError(f"{who}: max_batch must be at least 1")
    return max_batch


@torch.no_grad()
def encode_rgba_tiled(masknet, net, images, tile=tiling.TILE, overlap=tiling.OVERLAP, chunk=256,
                      max_batch=64, debug=None):
    """images: what anysize.pack_rgba takes -> list[bytes], one tiled file per image.  The tiles
    are views into the sources (pointer offset + row stride, no crop copies); one
    rgbac_rgba_alpha_class launch and one read classify all tiles of all images; transparent
    tiles are dropped, the others grouped by canvas across the whole call and coded in passes
    of at most ``max_batch`` tiles through encode_rgba's group body.  ``debug``: a list that
    receives, per image, {"grid", "cls": the class per tile, "tiles": {t: encode_rgba's debug
    record of that tile}}."""
    dev = _models(masknet, net)
    chunk = int(chunk)
    if chunk <= 0 or chunk >= 1 << 31:
        raise ValueError("chunk size must be a positive 32-bit number")
    max_batch = _batch_limit(max_batch, "encode_rgba_tiled")
    tiling.tile_grid(1, 1, tile, overlap)                    # bad tile / overlap: raise first
    dev, sizes, entries, keep = anysize._sources(images, dev, "encode_rgba_tiled")
    grids = [tiling.tile_grid(h, w, tile, overlap) for h, w in sizes]
    owner, t_sizes, t_entries = [], [], []
    for k, (grid, (ptr, _, _, stride)) in enumerate(zip(grids, entries)):
        for t in range(grid.ky * grid.kx):
            oy, ox, ey, ex = tiling.tile_rect(grid, t)
            owner.append((k, t))
            t_sizes.append((ey, ex))
            t_entries.append((ptr + oy * stride + 4 * ox, ey, ex, stride))
    cls_dev = anysize._alpha_class(dev, t_entries)
    cls = cls_dev.cpu().tolist()      # the one read: which sections, which tiles enter masknet
    info_a, info_r = codec_info(masknet), codec_info(net)
    groups = collections.OrderedDict()
    for i, c in enumerate(cls):
        if c != 2:
            groups.setdefault(anysize.padded_size(*t_sizes[i]), []).append(i)
    sections = [[None] * (g.ky * g.kx) for g in grids]
    records = [{} for _ in grids]
    for members in groups.values():
        for lo in range(0, len(members), max_batch):
            part = members[lo:lo + max_batch]
            opaque_dev = (cls_dev[torch.tensor(part, device=dev)] == 1).to(torch.int32).contiguous()
            coded = _encode_group(masknet, net, dev, [t_sizes[i] for i in part],
                                  [t_entries[i] for i in part], [cls[i] == 1 for i in part],
                                  opaque_dev, chunk, debug is not None)
            for i, (secs, dbg) in zip(part, coded):
                k, t = owner[i]
                sections[k][t] = secs
                records[k][t] = dbg
    files = [build_rgba_tiled(h, w, tile, overlap, chunk, info_a, info_r, sections[k])
             for k, (h, w) in enumerate(sizes)]
    if debug is not None:
        pos = 0
        debug[:] = []
        for k, g in enumerate(grids):
            n = g.ky * g.kx
            debug.append({"grid": g, "cls": cls[pos:pos + n], "tiles": records[k]})
            pos += n
    return files


def _blend(dev, grids, rects, planes):
    """One rgbac_rgba_blend_tiles launch: grids[k] / rects[k] = (y0, x0, hr, wr) per output,
    planes[k] = {t: (x_hat (3,hp,wp) fp32 tensor, alpha (hp,wp) fp32 tensor or None)} for the
    tiles that exist.  -> list of (hr, wr, 4) uint8 tensors."""
    outs, args = _blend_tables(dev, grids, rects, planes)
    _lib.call("rgbac_rgba_blend_tiles", *args[:5], _lib.stream_ptr(dev))
    return outs


def _blend_tables(dev, grids, rects, planes):
    """The outputs and the uploaded descriptor tables of one blend launch: (outs, (nout, outs
    table pointer, ntiles, tile table pointer, max_pixels, the two tables kept alive))."""
    if len(grids) > _MAX_OUTPUTS:
        raise ValueError(f"at most {_MAX_OUTPUTS} images per call, got {len(grids)}")
    ntiles = sum(g.ky * g.kx for g in grids)
    flat = torch.empty(sum(4 * hr * wr for _, _, hr, wr in rects), dtype=torch.uint8, device=dev)
    tdesc = (_lib.TileDesc * ntiles)()
    odesc = (_lib.BlendDesc * len(grids))()
    outs, tile0, off = [], 0, 0
    for k, (g, (y0, x0, hr, wr)) in enumerate(zip(grids, rects)):
        for t in range(g.ky * g.kx):
            oy, ox, ey, ex = tiling.tile_rect(g, t)
            got = planes[k].get(t)
            if got is None:
                tdesc[tile0 + t] = _lib.TileDesc(None, None, 0, 0, oy, ox, ey, ex)
                continue
            x_hat, alpha = got
            hp, wp = int(x_hat.shape[1]), int(x_hat.shape[2])
            if (x_hat.dtype != torch.float32 or not x_hat.is_contiguous() or x_hat.shape[0] != 3
                    or ey > hp or ex > wp):
                raise ValueError(f"tile {t}: x_hat must be a contiguous (3, hp, wp) fp32 tensor "
                                 f"that holds the {ey}x{ex} tile, got {tuple(x_hat.shape)}")
            if alpha is not None and (alpha.dtype != torch.float32 or not alpha.is_contiguous()
                                      or tuple(alpha.shape) != (hp, wp)):
                raise ValueError(f"tile {t}: alpha must be a contiguous ({hp}, {wp}) fp32 tensor")
            tdesc[tile0 + t] = _lib.TileDesc(x_hat.data_ptr(), _lib.ptr(alpha), hp, wp, oy, ox,
                                             ey, ex)
        outs.append(flat[off:off + 4 * hr * wr].view(hr, wr, 4))
        odesc[k] = _lib.BlendDesc(_lib.ImageDesc(flat.data_ptr() + off, hr, wr, 4 * wr), tile0,
                                  g.ky, g.kx, g.tile, g.overlap, y0, x0, 0)
        tile0 += g.ky * g.kx
        off += 4 * hr * wr
    td, od = _upload(tdesc, dev), _upload(odesc, dev)
    return outs, (len(grids), od.data_ptr(), ntiles, td.data_ptr(),
                  max(hr * wr for _, _, hr, wr in rects), (od, td))


def blend_tiles(grid, planes, region=None):
    """The device twin of tiling.blend_tiles_host for one image: planes = {t: (x_hat, alpha or
    None)} GPU tensors -> (hr, wr, 4) uint8 GPU tensor."""
    dev = next(iter(v[0] for v in planes.values() if v is not None)).device
    return _blend(dev, [grid], [tiling.check_region(grid, region)], [planes])[0]


@torch.no_grad()
def decode_rgba_tiled(masknet, net, blobs, regions=None, max_batch=64, debug=None):
    """blobs: files from encode_rgba_tiled, any number, any order -> list of (h, w, 4) uint8 GPU
    tensors.  regions[k]: None for the whole image or (y0, x0, h, w) inside it (ValueError
    otherwise); only the tiles that intersect it are decoded.  Every header, table and needed
    container is validated on the host before any launch (RuntimeError).  The tiles of all files
    are grouped by (canvas, chunk) and decoded in passes of at most ``max_batch`` through
    decode_rgba's group body; one blend launch writes all outputs; the one error word of all
    rANS launches is read once at the end.  ``debug``: a list that receives, per file,
    {"grid", "region", "tiles": the decoded tiles' indices, "planes": {t: (x_hat (3,hp,wp),
    alpha (hp,wp) or None) fp32}, "records": {t: decode_rgba's debug record of that tile}}."""
    dev = _models(masknet, net)
    blobs = list(blobs)
    if not blobs:
        raise ValueError("decode_rgba_tiled: no files")
    max_batch = _batch_limit(max_batch, "decode_rgba_tiled")
    regions = [None] * len(blobs) if regions is None else list(regions)
    if len(regions) != len(blobs):
        raise ValueError(f"decode_rgba_tiled: {len(regions)} regions for {len(blobs)} files")
    info_a, info_r = codec_info(masknet), codec_info(net)
    parsed, rects = [], []
    for blob, region in zip(blobs, regions):
        blob = bytes(blob)
        grid = _parse_head(blob)["grid"]
        rects.append(tiling.check_region(grid, region))
        parsed.append(parse_rgba_tiled(blob, info_a, info_r, tiles=tiling.region_tiles(grid, region)))
    groups = collections.OrderedDict()
    for k, f in enumerate(parsed):
        for t, rec in f["tiles"].items():
            if rec is not None:
                groups.setdefault(rec["canvas"] + (rec["chunk"],), []).append((k, t))
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    planes = [{} for _ in blobs]
    records = [{} for _ in blobs]
    for (hp, wp, _), members in groups.items():
        for lo in range(0, len(members), max_batch):
            part = members[lo:lo + max_batch]
            fs = [parsed[k]["tiles"][t] for k, t in part]
            x_hat, alpha, dbgs = _decode_group(masknet, net, fs, hp, wp, dev, err,
                                               debug is not None)
            for j, (k, t) in enumerate(part):
                planes[k][t] = (x_hat[j], None if fs[j]["opaque"] else alpha[j, 0])
                if debug is not None:
                    records[k][t] = dbgs[j]
    outs = _blend(dev, [f["grid"] for f in parsed], rects, planes)
    if debug is not None:
        debug[:] = [{"grid": f["grid"], "region": rects[k], "tiles": sorted(planes[k]),
                     "planes": {t: (x.clone(), None if a is None else a.clone())
                                for t, (x, a) in planes[k].items()},
                     "records": records[k]} for k, f in enumerate(parsed)]
    _raise_code("tiled RGBA file decode", int(err.item()))
    return outs
