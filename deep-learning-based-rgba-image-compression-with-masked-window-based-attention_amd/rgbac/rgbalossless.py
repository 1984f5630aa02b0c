"""Lossless RGBA files (``RGAL``): exact alpha beside exact colour, both coded on the device.

``encode_rgba_lossless`` takes a ragged batch of packed uint8 RGBA images and returns one
self-contained file per image; ``decode_rgba_lossless`` takes any list of files in any order and
returns the images bit for bit, except that a pixel nobody can see (alpha 0) comes back with
R = G = B = 0 unless the file was written with ``keep_hidden``.  No model is involved.  GPU only:
a CPU device or a missing library raises.

The alpha plane is an ``RGAP`` blob of rgbac.alphaexact, unchanged.  The colour is coded by
csrc/color_exact.hip: subtract-green (Y = G, Cr = (R - G + 128) & 255, Cb = (B - G + 128) & 255),
MED prediction inside 16 x 16 blocks over the neighbours that are visible, 15 static tables per
image (channel * 5 + context), one rANS chunk per block and channel that is not constant.  Model,
format and launches: DESIGN.md section 26.

``transform="adaptive"`` (csrc/color_adapt.hip) lets every block choose, for
red and for blue on their own, between the difference from green and the plain channel, whichever
the model codes in fewer bits: five planes Y, Cr, Cb, R, B with 25 tables (kind * 5 + context),
class word bit 4 / 5 = the red / blue slot holds the plain channel.  Such files are version 2;
``transform="green"``, the default, writes what it always wrote.

``transform="palette"`` (csrc/color_palette.hip) writes an image that has
at most 256 distinct pixels as a version 3 file: its palette and one plane of palette positions,
an ``RGAP`` blob like the alpha plane.  Every other image of the call is written as
``transform="adaptive"`` writes it.  A pixel is its little-endian dword (R low, A high), 0 where
alpha is 0 unless ``keep_hidden``; the palette is ascending by (A, (R + 2 G + B) >> 2, dword).

``index_model="neighbour"`` (csrc/index_exact.hip) codes that plane of
positions as labels instead: which neighbour a pixel equals, an ``RGAI`` blob of
rgbac.indexexact.  Such files are version 4; ``index_model="plane"``, the default, writes what
palette mode always wrote.

File, little-endian:
    "RGAL", u16 version (1; 2 adaptive; 3 palette; 4 palette, neighbour model), u16 flags (bit 0: keep_hidden; bit 1:
    adaptive, set in every version 2 file and in no other; bit 2: palette, likewise for version
    3), u32 h, u32 w, u32 alpha bytes, u32 colour bytes; the
    RGAP blob; the colour section: u32 chunks, u32 payload words; 15 tables (25 in version 2) in
    the RGAP table form, channel-major (kind-major); one u32 class word per block, row-major (bit
    0 hidden, bits 1-3 channel Y / Cr / Cb constant, version 2: bits 4 / 5 plain R / B, bits
    8-15 / 16-23 / 24-31 the constants); one u16 word count per chunk (block-major, Y, Cr, Cb);
    the payload, u32 words.
    Version 3: alpha bytes is 0 and there is no alpha blob (the alpha lies in the palette); the
    colour section is u32 n in 1..256, n palette dwords, the RGAP blob of the (h, w) index plane.
    Version 4: as version 3 with flags bit 2 and bit 3 (the neighbour model) always set, and the
    RGAI blob of the index plane, whose n is the palette's, in the RGAP blob's place.
"""
import struct

import numpy as np
import torch

from . import _lib, alphaexact, anysize, indexexact
from .alphaexact import BLOCK, MAX_SIDE, SPARSE_MAX, TOTAL, block_grid, normalise_counts
from .ans import _raise_code, _upload

MAGIC = b"RGAL"
VERSION = 1
VERSION_ADAPTIVE = 2
FLAG_KEEP_HIDDEN = 1
VERSION_PALETTE = 3
FLAG_ADAPTIVE = 2
FLAG_PALETTE = 4
VERSION_NEIGHBOUR = 4                 # palette mode, the index plane as an RGAI blob
FLAG_NEIGHBOUR = 8
INDEX_MODELS = ("plane", "neighbour")
TRANSFORMS = ("green", "adaptive")    # the colour transforms any image can be written with
TRANSFORM_NAMES = TRANSFORMS + ("palette",)   # every value of ``transform``, by version - 1
PALETTE_MAX = _lib.PALETTE_MAX        # colours of a version 3 file
NCH = _lib.COLOR_CHANNELS
NCTX = alphaexact.NCTX
NTAB = NCH * NCTX                     # 15 tables: channel * 5 + context
NKIND = _lib.COLOR_ADAPT_KINDS        # adaptive: the planes Y, Cr, Cb, R, B
NTAB_ADAPTIVE = NKIND * NCTX          # 25 tables: kind * 5 + context
PLAIN_R, PLAIN_B = 16, 32             # class word, adaptive: the red / blue slot holds R / B
_HEADER = struct.Struct("<4sHHIIII")
HEADER_BYTES = _HEADER.size           # 24
_HIDDEN = 1                           # the class word of a block without a visible pixel


def _chunk_mask(cls):
    """class words (N,) -> bool (N, 3): block k has a chunk for channel c."""
    cls = np.asarray(cls).astype(np.int64)
    return ((cls[:, None] & 1) == 0) & (((cls[:, None] >> (1 + np.arange(NCH))) & 1) == 0)


def device_table(freqs):
    """(15, 256) frequencies -> the uint16[3856] table the kernels stage in LDS: exclusive sums
    mod 2^16, the last symbol with a frequency per table (-1: empty), one zero.  (25, 256), the
    adaptive transform's, -> uint16[6426] in the same form."""
    f = np.asarray(freqs, dtype=np.int64).reshape(-1, 256)
    ntab = f.shape[0]
    tab = np.zeros(ntab * 257 + 1, dtype=np.uint16)
    tab[:ntab * 256] = ((np.cumsum(f, axis=1) - f) & 0xFFFF).reshape(-1)
    for c in range(ntab):
        nz = np.flatnonzero(f[c])
        tab[ntab * 256 + c] = np.int16(nz[-1] if nz.size else -1).view(np.uint16)
    return tab


def host_tables(freqs):
    """(15, 256) or (25, 256) frequencies -> the rgbac.ans.CdfTables the host chunk coder takes
    (rows of 258 entries, as alphaexact.host_tables)."""
    from .ans import CdfTables
    f = np.asarray(freqs, dtype=np.int64).reshape(-1, 256)
    ntab = f.shape[0]
    cdfs = np.zeros((ntab, 258), dtype=np.int32)
    cdfs[:, 1:257] = np.cumsum(f, axis=1)
    cdfs[:, 257] = cdfs[:, 256]
    return CdfTables(cdfs, [258] * ntab, [0] * ntab)


def build_colour(freqs, cls, counts, payload):
    """The pieces of one image's colour section -> bytes.  freqs (15 or 25, 256); cls: the blocks'
    class words; counts: the chunks' word counts in chunk order; payload: their words."""
    counts = np.asarray(counts)
    return b"".join(
        [struct.pack("<II", counts.size, len(payload))]
        + [alphaexact._pack_table(np.asarray(f, dtype=np.int64)) for f in freqs]
        + [np.asarray(cls).astype("<u4").tobytes(), counts.astype("<u2").tobytes(),
           np.asarray(payload).astype("<u4").tobytes()])


def build_rgba_lossless(h, w, keep_hidden, alpha, colour, adaptive=False):
    flags = (FLAG_KEEP_HIDDEN if keep_hidden else 0) | (FLAG_ADAPTIVE if adaptive else 0)
    return _HEADER.pack(MAGIC, VERSION_ADAPTIVE if adaptive else VERSION, flags, h, w,
                        len(alpha), len(colour)) + alpha + colour


def build_rgba_palette(h, w, keep_hidden, palette, plane, neighbour=False):
    """One version 3 file from its palette (canonical dwords in the format's order) and the RGAP
    blob of its index plane; ``neighbour``: a version 4 file, ``plane`` the RGAI blob."""
    colour = struct.pack("<I", len(palette)) + np.asarray(palette).astype("<u4").tobytes() + plane
    flags = FLAG_PALETTE | (FLAG_KEEP_HIDDEN if keep_hidden else 0)
    if neighbour:
        return _HEADER.pack(MAGIC, VERSION_NEIGHBOUR, flags | FLAG_NEIGHBOUR, h, w, 0,
                            len(colour)) + colour
    return _HEADER.pack(MAGIC, VERSION_PALETTE, flags, h, w, 0, len(colour)) + colour


def palette_key(dwords):
    """Canonical pixel dwords -> the uint64 keys a palette is ascending by:
    A << 40 | ((R + 2 G + B) >> 2) << 32 | dword."""
    v = np.asarray(dwords).astype(np.uint64)
    luma = ((v & 255) + 2 * ((v >> 8) & 255) + ((v >> 16) & 255)) >> 2
    return ((v >> 24) << 40) | (luma << 32) | v


def _transform(transform, who):
    if transform not in TRANSFORM_NAMES:
        raise ValueError(f"{who}: transform must be one of {TRANSFORM_NAMES}, got {transform!r}")
    return transform


def _index_model(index_model, who):
    if index_model not in INDEX_MODELS:
        raise ValueError(f"{who}: index_model must be one of {INDEX_MODELS}, got {index_model!r}")
    return index_model == "neighbour"


def _parse_palette(blob, flags, h, w, alpha_len, bad):
    """The rest of parse_rgba_lossless for a version 3 or 4 file (header and total length
    checked)."""
    neighbour = bool(flags & FLAG_NEIGHBOUR)
    if alpha_len:
        raise bad(f"a version {3 + neighbour} file has no alpha section, the header says "
                  f"{alpha_len} bytes")
    sec = blob[HEADER_BYTES:]
    if len(sec) < 4:
        raise bad("the colour section is truncated in the palette")
    n = struct.unpack_from("<I", sec)[0]
    if not 1 <= n <= PALETTE_MAX:
        raise bad(f"a palette of {n} colours")
    if len(sec) < 4 + 4 * n:
        raise bad("the colour section is truncated in the palette")
    palette = np.frombuffer(sec, dtype="<u4", count=n, offset=4).astype(np.uint32)
    if (np.diff(palette_key(palette).astype(np.int64)) <= 0).any():
        raise bad("the palette is not strictly ascending")
    if not flags & FLAG_KEEP_HIDDEN and ((palette >> 24 == 0) & (palette != 0)).any():
        raise bad("a hidden palette entry with a colour, without keep_hidden")
    if neighbour:
        plane = indexexact.parse_index_planes(sec[4 + 4 * n:])
        if plane["n"] != n:
            raise bad(f"the index plane is of {plane['n']} positions, the palette has {n}")
    else:
        plane = alphaexact.parse_alpha_planes(sec[4 + 4 * n:])
    if (plane["h"], plane["w"]) != (h, w):
        raise bad(f"the index plane is {plane['h']}x{plane['w']}, the image {h}x{w}")
    out = {"h": h, "w": w, "keep_hidden": bool(flags & FLAG_KEEP_HIDDEN), "transform": "palette",
           "palette": palette, "plane": plane}
    if neighbour:
        out["index_model"] = "neighbour"
    return out


def parse_rgba_lossless(blob):
    """bytes -> {"h", "w", "keep_hidden", "transform" ("green": version 1, "adaptive": version
    2, "palette": version 3), and for a version 3 file "palette": uint32 canonical pixels, "plane":
    the parsed RGAP blob of the index plane; for the others "alpha": the parsed RGAP blob, "freqs" (15, 256) int64, (25, 256) if adaptive, "cls"
    uint32 per block, "counts" int32 (blocks, 3) (0 where there is no chunk), "payload"
    uint32}.  Pure host code; raises RuntimeError on anything wrong: bad magic, version, flags or
    size (flags bit 1 belongs to version 2, which always has it; class bits 4 and 5 to version 2,
    bits 6 and 7 to none); truncation or over-length; section lengths that disagree; an alpha
    blob that
    parse_alpha_planes rejects or of another size; tables that are not fixed points of
    normalise_counts; class words with reserved bits set, a hidden word that is not 1 or a value
    byte under a clear flag; a chunk table whose length is not what the class words imply; word
    counts outside [2, block pixels / 2 + 3] or that do not sum to the payload.  Version 3: flags
    other than bit 2 (always) and bit 0; an alpha section; a palette of 0 or more than 256
    colours, not strictly ascending in its key, or, without keep_hidden, with an entry of alpha
    0 that is not 0; an index plane parse_alpha_planes rejects or of another size.  Version 4: as
    version 3 with "index_model": "neighbour" and "plane" the parsed RGAI blob; flags without bits
    2 and 3 (bit 3 belongs to version 4 alone); an index plane parse_index_planes rejects, of
    another size or of another n than the palette's."""
    blob = bytes(blob)

    def bad(msg):
        return RuntimeError(f"RGAL file: {msg}")

    if len(blob) < HEADER_BYTES:
        raise bad(f"truncated ({len(blob)} bytes, the header has {HEADER_BYTES})")
    magic, version, flags, h, w, alpha_len, colour_len = _HEADER.unpack_from(blob)
    if magic != MAGIC:
        raise bad("bad magic (not an RGAL file)")
    if version not in (VERSION, VERSION_ADAPTIVE, VERSION_PALETTE, VERSION_NEIGHBOUR):
        raise bad(f"unsupported version {version}")
    if version == VERSION_NEIGHBOUR and flags & 12 != FLAG_PALETTE | FLAG_NEIGHBOUR:
        raise bad(f"unsupported version {version} with flags {flags:#x} (a version 4 file has "
                  "bits 2 and 3, the palette and the neighbour model)")
    adaptive = version == VERSION_ADAPTIVE
    if adaptive and not flags & FLAG_ADAPTIVE:
        raise bad(f"unsupported version {version} with flags {flags:#x} (a version 2 file has "
                  "bit 1, the adaptive transform)")
    if version == VERSION_PALETTE and not flags & FLAG_PALETTE:
        raise bad(f"unsupported version {version} with flags {flags:#x} (a version 3 file has "
                  "bit 2, the palette)")
    own = {VERSION: 0, VERSION_ADAPTIVE: FLAG_ADAPTIVE, VERSION_PALETTE: FLAG_PALETTE,
           VERSION_NEIGHBOUR: FLAG_PALETTE | FLAG_NEIGHBOUR}[version]
    if flags & ~(FLAG_KEEP_HIDDEN | own):
        raise bad(f"unknown flags {flags:#x} in a version {version} file")
    ntab = NTAB_ADAPTIVE if adaptive else NTAB
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise bad(f"bad size {h}x{w}")
    total = HEADER_BYTES + alpha_len + colour_len
    if total != len(blob):
        raise bad(f"{'truncated' if len(blob) < total else 'over-long'}: the section lengths say "
                  f"{total} bytes, the file has {len(blob)}")
    if version in (VERSION_PALETTE, VERSION_NEIGHBOUR):
        return _parse_palette(blob, flags, h, w, alpha_len, bad)
    alpha = alphaexact.parse_alpha_planes(blob[HEADER_BYTES:HEADER_BYTES + alpha_len])
    if (alpha["h"], alpha["w"]) != (h, w):
        raise bad(f"the alpha plane is {alpha['h']}x{alpha['w']}, the image {h}x{w}")
    sec = blob[HEADER_BYTES + alpha_len:]
    pos = 0

    def take(n, what):
        nonlocal pos
        if pos + n > len(sec):
            raise bad(f"the colour section is truncated in the {what}")
        pos += n
        return sec[pos - n:pos]

    nchunks, nwords = struct.unpack("<II", take(8, "header"))
    freqs = np.zeros((ntab, 256), dtype=np.int64)
    for c in range(ntab):
        n = struct.unpack("<H", take(2, "tables"))[0]
        if n > 256 or n == 1:
            raise bad(f"table {c} lists {n} symbols")
        if n > SPARSE_MAX:
            freqs[c] = np.frombuffer(take(512, "tables"), dtype="<u2")
            if int((freqs[c] > 0).sum()) != n:
                raise bad(f"table {c}: the symbol count disagrees with its frequencies")
        elif n:
            rec = np.frombuffer(take(3 * n, "tables"), dtype=np.dtype([("s", "u1"), ("f", "<u2")]))
            if (np.diff(rec["s"].astype(np.int64)) <= 0).any() or (rec["f"] == 0).any():
                raise bad(f"table {c}: symbols out of order or without a frequency")
            freqs[c, rec["s"]] = rec["f"]
        if n and int(freqs[c].sum()) != TOTAL:
            raise bad(f"table {c} sums to {int(freqs[c].sum())}, not 2^16")
        if (normalise_counts(freqs[c]) != freqs[c]).any():
            raise bad(f"table {c} is not a normalised table")
    npix = block_grid(h, w)[2]
    cls = np.frombuffer(take(4 * npix.size, "class table"), dtype="<u4").astype(np.uint32)
    if (cls & (0xC0 if adaptive else 0xF0)).any():
        raise bad("class table: reserved bits set")
    if ((cls & 1) & (cls != _HIDDEN)).any():
        raise bad("class table: a hidden block's word is not 1")
    const = ((cls[:, None].astype(np.int64) >> (1 + np.arange(NCH))) & 1) == 1
    value = (cls[:, None].astype(np.int64) >> (8 + 8 * np.arange(NCH))) & 255
    if (value[~const] != 0).any():
        raise bad("class table: a value under a clear constant flag")
    has = _chunk_mask(cls)
    if int(has.sum()) != nchunks:
        raise bad(f"the class table implies {int(has.sum())} chunks, the chunk table has "
                  f"{nchunks}")
    cnt = np.frombuffer(take(2 * nchunks, "chunk table"), dtype="<u2").astype(np.int64)
    # a chunk holds its two state words and at most 16 bits per symbol
    if (cnt < 2).any() or (cnt > np.broadcast_to(npix[:, None], has.shape)[has] // 2 + 3).any():
        raise bad("chunk table: a chunk's word count is impossible for its block")
    if int(cnt.sum()) != nwords:
        raise bad(f"the chunk table sums to {int(cnt.sum())} words, the section says {nwords}")
    payload = np.frombuffer(take(4 * nwords, "payload"), dtype="<u4").astype(np.uint32)
    if pos != len(sec):
        raise bad(f"the colour section is over-long: {len(sec) - pos} bytes after the payload")
    counts = np.zeros(has.shape, dtype=np.int32)
    counts[has] = cnt
    return {"h": h, "w": w, "keep_hidden": bool(flags & FLAG_KEEP_HIDDEN),
            "transform": TRANSFORMS[adaptive], "alpha": alpha, "freqs": freqs, "cls": cls,
            "counts": counts, "payload": payload}


# ---- the CPU twin: the model in numpy, the chunks by the host chunk coder (rgbac.ans)
def _shift(a, dy, dx):
    """a moved down / right by (dy, dx) along its last two axes, zeros coming in."""
    out = np.zeros_like(a)
    h, w = a.shape[-2:]
    out[..., dy:, dx:] = a[..., :h - dy, :w - dx]
    return out


def model_symbols(image, keep_hidden=False, adaptive=False):
    """(h, w, 4) uint8 -> (symbols (3, h, w), contexts (3, h, w), visible (h, w)): the model of
    DESIGN.md section 26 for every pixel of the planes Y, Cr, Cb, each inside its own 16 x 16
    block; entries of hidden pixels mean nothing.  ``adaptive``: (5, h, w), the planes Y, Cr, Cb,
    R, B of DESIGN.md section 30."""
    a = np.asarray(image).astype(np.int64)
    h, w = a.shape[:2]
    vis = np.ones((h, w), dtype=bool) if keep_hidden else a[..., 3] != 0
    g = a[..., 1]
    v = np.stack([g, (a[..., 0] - g + 128) & 255, (a[..., 2] - g + 128) & 255]
                 + ([a[..., 0], a[..., 2]] if adaptive else []))
    inr = np.broadcast_to((np.arange(h) % BLOCK != 0)[:, None], (h, w))
    inc = np.broadcast_to((np.arange(w) % BLOCK != 0)[None, :], (h, w))
    eL, eU, eD = _shift(vis, 0, 1) & inc, _shift(vis, 1, 0) & inr, _shift(vis, 1, 1) & inr & inc
    L, U, D = _shift(v, 0, 1), _shift(v, 1, 0), _shift(v, 1, 1)
    D = np.where(eD, D, L)
    lo, hi = np.minimum(L, U), np.maximum(L, U)
    med = np.where(D >= hi, lo, np.where(D <= lo, hi, L + U - D))
    d = np.maximum(hi, D) - np.minimum(lo, D)
    bins = (d > 0).astype(np.int64) + (d > 8) + (d > 64)
    one = np.where(eL, L, np.where(eU, U, _shift(v, 1, 1)))
    both, some = eL & eU, eL | eU | eD
    pred = np.where(both, med, np.where(some, one, 0))
    ctx = np.where(both, bins, np.where(some, 0, 4))
    return ((v - pred) & 255).astype(np.int32), ctx.astype(np.int32), vis


def encode_rgba_lossless_host(image, keep_hidden=False, transform="green", index_model="plane"):
    """encode_rgba_lossless for one image on the CPU: the kernels' byte-level reference (not a
    fallback; the device path never calls it)."""
    from .ans import encode_table_host
    transform = _transform(transform, "encode_rgba_lossless_host")
    neighbour = transform == "palette" and _index_model(index_model, "encode_rgba_lossless_host")
    a = np.ascontiguousarray(np.asarray(image, dtype=np.uint8))
    if a.ndim != 3 or a.shape[2] != 4 or a.size == 0 or max(a.shape[:2]) > MAX_SIDE:
        raise ValueError(f"encode_rgba_lossless_host: expected (H, W, 4) uint8 RGBA, got {a.shape}")
    h, w = a.shape[:2]
    if transform == "palette":
        px = a.view("<u4")[..., 0].astype(np.uint32)
        if not keep_hidden:
            px = np.where(a[..., 3] == 0, np.uint32(0), px)
        colours, index = np.unique(px, return_inverse=True)          # ascending by dword
        if colours.size <= PALETTE_MAX:
            order = np.argsort(palette_key(colours))
            rank = np.empty(colours.size, dtype=np.uint8)
            rank[order] = np.arange(colours.size)
            plane = rank[index.reshape(h, w)]
            plane = (indexexact.encode_index_plane_host(plane, colours.size) if neighbour
                     else alphaexact.encode_alpha_plane_host(plane))
            return build_rgba_palette(h, w, keep_hidden, colours[order], plane, neighbour)
    adaptive = transform != "green"
    sym, ctx, vis = model_symbols(a, keep_hidden, adaptive)
    g = a[..., 1].astype(np.int64)
    planes = [g, (a[..., 0] - g + 128) & 255, (a[..., 2] - g + 128) & 255,
              a[..., 0].astype(np.int64), a[..., 2].astype(np.int64)]
    cost = np.minimum(sym, 256 - sym)
    ntab = NTAB_ADAPTIVE if adaptive else NTAB
    cls, s, t, lens = [], [], [], []
    blocks = [(r, c) for r in range(0, h, BLOCK) for c in range(0, w, BLOCK)]
    for r, c in blocks:
        at = (slice(r, r + BLOCK), slice(c, c + BLOCK))
        m = vis[at]
        if not m.any():
            cls.append(_HIDDEN)
            continue
        word = 0
        for ch in range(NCH):
            kind = ch                                    # the plane this slot holds
            if adaptive and ch:
                d, p = planes[ch][at][m], planes[ch + 2][at][m]
                if (d != d[0]).any() and ((p == p[0]).all()
                                          or cost[ch + 2][at][m].sum() < cost[ch][at][m].sum()):
                    kind = ch + 2
                    word |= (PLAIN_R, PLAIN_B)[ch - 1]
            vals = planes[kind][at][m]                   # raster order
            if (vals == vals[0]).all():
                word |= (2 << ch) | (int(vals[0]) << (8 + 8 * ch))
            else:
                s.append(sym[kind][at][m])
                t.append(ctx[kind][at][m] + NCTX * kind)
                lens.append(vals.size)
        cls.append(word)
    freqs = np.zeros((ntab, 256), dtype=np.int64)
    counts, payload = np.zeros(0, np.int32), np.zeros(0, np.uint32)
    if lens:
        s, t, lens = np.concatenate(s), np.concatenate(t), np.asarray(lens, dtype=np.int64)
        for k in range(ntab):
            freqs[k] = normalise_counts(np.bincount(s[t == k], minlength=256))
        table = np.stack([np.cumsum(lens) - lens, lens])
        words = encode_table_host(s, t, host_tables(freqs), table, BLOCK * BLOCK)
        counts, payload = words[:lens.size], words[lens.size:].view(np.uint32)
    return build_rgba_lossless(h, w, keep_hidden, alphaexact.encode_alpha_plane_host(a[..., 3]),
                               build_colour(freqs, np.asarray(cls, dtype=np.uint32), counts,
                                            payload), adaptive)


# ---- launches
def _alpha_entries(entries):
    """RGBA descriptor entries -> the same rectangles' alpha bytes, 4 bytes apart."""
    return [(ptr + 3, h, w, stride) for ptr, h, w, stride in entries]


def _args(wk, keep_hidden, grouped):
    """The leading arguments of the rgbac_color_exact_* and rgbac_color_adapt_* calls from
    alphaexact's geometry."""
    head = (wk.B, wk._descs.data_ptr(), int(keep_hidden))
    mid = (wk.ngroups, wk._groups.data_ptr()) if grouped else ()
    return head + mid + (wk._base.data_ptr(), wk.N)


def _encode_colour(dev, sizes, entries, keep_hidden, adaptive=False):
    """The five launches over a ragged batch (classify, histogram, normalise, sizes, encode) and
    the two host reads -> one colour section per image.  ``adaptive``: the same five of
    csrc/color_adapt.hip, where choose stands for classify and an image has 25 tables."""
    fn = "rgbac_color_adapt_" if adaptive else "rgbac_color_exact_"
    ntab = NTAB_ADAPTIVE if adaptive else NTAB
    wk = alphaexact._Work(sizes, entries, 4, dev)
    B, N, nf = wk.B, wk.N, ntab * 256
    meta = torch.empty((1 + NCH) * N + B * nf, dtype=torch.int32, device=dev)
    cls, counts, freqs = meta[:N], meta[N:(1 + NCH) * N], meta[(1 + NCH) * N:]
    partials = torch.empty(B * _lib.COLOR_HIST_BLOCKS * nf, dtype=torch.int32, device=dev)
    tables = torch.empty(B * (_lib.COLOR_ADAPT_TABLE_U16 if adaptive else _lib.COLOR_TABLE_U16),
                         dtype=torch.int16, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    plain, grouped = _args(wk, keep_hidden, False), _args(wk, keep_hidden, True)
    _lib.call(fn + ("choose" if adaptive else "classify"), *grouped, cls.data_ptr(), wk.stream)
    _lib.call(fn + "tables", *plain, cls.data_ptr(), partials.data_ptr(),
              freqs.data_ptr(), tables.data_ptr(), wk.stream)
    _lib.call(fn + "sizes", *grouped, cls.data_ptr(), tables.data_ptr(),
              counts.data_ptr(), err.data_ptr(), wk.stream)
    ends = torch.cumsum(counts, 0, dtype=torch.int64)
    host = meta.cpu().numpy()                                       # the sizes: one read
    h_cls = host[:N].view(np.uint32)
    h_counts = host[N:(1 + NCH) * N].reshape(N, NCH)
    h_freqs = host[(1 + NCH) * N:].reshape(B, ntab, 256)
    cut = np.concatenate([[0], np.cumsum(h_counts.sum(axis=1, dtype=np.int64))])
    total = int(cut[-1])
    words = torch.empty(total + 1, dtype=torch.int32, device=dev)
    if total:
        _lib.call(fn + "encode", *grouped, cls.data_ptr(), tables.data_ptr(),
                  counts.data_ptr(), ends.data_ptr(), words.data_ptr(), total, err.data_ptr(),
                  wk.stream)
    words[total:].copy_(err)
    words = words.cpu().numpy()                                     # the words: one copy
    _raise_code("encode_rgba_lossless", int(words[total]))
    out = []
    for b in range(B):
        lo, hi = int(wk.base[b]), int(wk.base[b + 1])
        c = h_cls[lo:hi]
        out.append(build_colour(h_freqs[b], c, h_counts[lo:hi][_chunk_mask(c)],
                                words[int(cut[lo]):int(cut[hi])].view(np.uint32)))
    return out


def _slices(sizes):
    return max(-(-h * w // _lib.PALETTE_SLICE) for h, w in sizes)


def _planes(sizes, dev):
    """One dense uint8 index plane per image, 16-byte aligned -> (the buffer, the planes as
    views, their descriptor entries)."""
    cut = np.concatenate([[0], np.cumsum([-(-h * w // 16) * 16 for h, w in sizes])])
    flat = torch.empty(int(cut[-1]), dtype=torch.uint8, device=dev)
    views = [flat[int(cut[i]):int(cut[i]) + h * w].view(h, w) for i, (h, w) in enumerate(sizes)]
    return flat, views, [(v.data_ptr(), h, w, w) for v, (h, w) in zip(views, sizes)]


def _encode_palette(dev, sizes, entries, keep_hidden, neighbour=False):
    """The three launches over a ragged batch (collect, order, map), one read-back of every
    image's overflow word, colour count and palette, then the plane coder over the index planes
    of the images that have a palette -> per image (palette uint32, RGAP blob), or None where
    the image has more than 256 colours.  ``neighbour``: the index coder and RGAI blobs."""
    B, stream = len(sizes), _lib.stream_ptr(dev)
    descs = anysize._upload_descs(entries, dev)
    flat, views, pentries = _planes(sizes, dev)
    pdescs = anysize._upload_descs(pentries, dev)
    state = torch.zeros(B * _lib.PALETTE_STATE_U32, dtype=torch.int32, device=dev)
    result = torch.zeros(B * _lib.PALETTE_RESULT_U32 + 1, dtype=torch.int32, device=dev)
    err = result[-1:]
    _lib.call("rgbac_color_palette_collect", B, descs.data_ptr(), int(keep_hidden),
              _slices(sizes), state.data_ptr(), err.data_ptr(), stream)
    _lib.call("rgbac_color_palette_order", B, state.data_ptr(), result.data_ptr(), stream)
    _lib.call("rgbac_color_palette_map", B, descs.data_ptr(), pdescs.data_ptr(),
              int(keep_hidden), _slices(sizes), result.data_ptr(), err.data_ptr(), stream)
    host = result.cpu().numpy()                                     # the one read-back
    _raise_code("encode_rgba_lossless (palette)", int(host[-1]))
    host = host[:-1].view(np.uint32).reshape(B, _lib.PALETTE_RESULT_U32)
    ks = [k for k in range(B) if not host[k, 0]]
    out = [None] * B
    if ks:
        if neighbour:
            blobs = indexexact._encode(dev, [sizes[k] for k in ks], [pentries[k] for k in ks],
                                       [int(host[k, 1]) for k in ks])
        else:
            blobs = alphaexact._encode(dev, [sizes[k] for k in ks], [pentries[k] for k in ks], 1)
        for k, blob in zip(ks, blobs):
            out[k] = (host[k, 2:2 + int(host[k, 1])].copy(), blob)
    return out


def encode_rgba_lossless(images, keep_hidden=False, transform="green", index_model="plane",
                         device="cuda"):
    """images: a list of (h, w, 4) uint8 RGBA images of any sizes; GPU tensors are read in place,
    views into larger buffers included -> list[bytes], one RGAL file per image.  A hidden pixel
    (alpha 0) decodes to R = G = B = 0 and its colour bytes do not reach the file;
    ``keep_hidden`` codes every pixel's colour.  ``transform``: "green" subtracts green from red
    and blue everywhere (version 1 files); "adaptive" lets each block keep red or blue plain
    where that codes shorter (version 2 files, smaller where the channels do not move together);
    "palette" writes an image of at most 256 distinct pixels as its palette and one plane of
    palette positions (version 3 files) and every other image as "adaptive" does.
    ``index_model``, looked at under "palette" only: "plane" codes the positions with the alpha
    plane coder; "neighbour" codes which neighbour a pixel equals (version 4 files, smaller on
    flat and dithered images: DESIGN.md section 32).
    A file does not depend on the images coded with it."""
    transform = _transform(transform, "encode_rgba_lossless")
    neighbour = transform == "palette" and _index_model(index_model, "encode_rgba_lossless")
    adaptive = transform != "green"
    dev = anysize._gpu_device(device)
    _lib.load()
    dev, sizes, entries, keep = anysize._sources(images, dev, "encode_rgba_lossless")
    if max(max(s) for s in sizes) > MAX_SIDE:
        raise ValueError(f"encode_rgba_lossless: an image side is at most {MAX_SIDE}")
    keep_hidden = bool(keep_hidden)
    files = [None] * len(sizes)
    if transform == "palette":
        for k, found in enumerate(_encode_palette(dev, sizes, entries, keep_hidden, neighbour)):
            if found:
                files[k] = build_rgba_palette(*sizes[k], keep_hidden, *found, neighbour)
    ks = [k for k, f in enumerate(files) if f is None]
    if ks:
        sizes, entries = [sizes[k] for k in ks], [entries[k] for k in ks]
        alpha = alphaexact._encode(dev, sizes, _alpha_entries(entries), 4)
        colour = _encode_colour(dev, sizes, entries, keep_hidden, adaptive)
        for k, (h, w), a, c in zip(ks, sizes, alpha, colour):
            files[k] = build_rgba_lossless(h, w, keep_hidden, a, c, adaptive)
    return files


def _decode_colour(parsed, entries, keep_hidden, dev, err, adaptive=False):
    """One launch for parsed files that share ``keep_hidden`` and the transform onto the images
    ``entries`` describe (their alpha bytes in place); errors land in ``err``."""
    sizes = [(f["h"], f["w"]) for f in parsed]
    wk = alphaexact._Work(sizes, entries, 4, dev)
    counts = np.concatenate([f["counts"].reshape(-1) for f in parsed])
    pbase = np.concatenate([[0], np.cumsum([f["payload"].size for f in parsed])])
    off = np.concatenate([pbase[i] + np.cumsum(f["counts"].reshape(-1), dtype=np.int64)
                          - f["counts"].reshape(-1) for i, f in enumerate(parsed)])
    payload = np.concatenate([f["payload"] for f in parsed] + [np.zeros(1, dtype=np.uint32)])
    cls = np.concatenate([f["cls"] for f in parsed])
    ints = _upload(np.concatenate([cls.view(np.int32), counts, payload.view(np.int32)])
                   .astype(np.int32), dev)
    off = _upload(off.astype(np.int64), dev)
    tables = _upload(np.concatenate([device_table(f["freqs"]) for f in parsed]).view(np.int16),
                     dev)
    N = wk.N
    _lib.call("rgbac_color_adapt_decode" if adaptive else "rgbac_color_exact_decode",
              *_args(wk, keep_hidden, True), ints[:N].data_ptr(),
              tables.data_ptr(), off.data_ptr(), ints[N:(1 + NCH) * N].data_ptr(),
              ints[(1 + NCH) * N:].data_ptr(), int(pbase[-1]), err.data_ptr(), wk.stream)


def _decode_palette(parsed, entries, dev, err):
    """Version 3 and 4 files onto the images ``entries`` describe: one plane-decoder launch per
    index model present into index planes of their own, one unmap launch behind them on the same
    stream."""
    sizes = [(f["h"], f["w"]) for f in parsed]
    flat, views, pentries = _planes(sizes, dev)
    ks = [k for k, f in enumerate(parsed) if "index_model" not in f]
    if ks:
        alphaexact._decode([parsed[k]["plane"] for k in ks], [pentries[k] for k in ks], 1, dev,
                           err)
    ks = [k for k, f in enumerate(parsed) if f.get("index_model") == "neighbour"]
    if ks:
        indexexact._decode([parsed[k]["plane"] for k in ks], [pentries[k] for k in ks], dev, err)
    palettes = np.zeros((len(parsed), PALETTE_MAX), dtype=np.uint32)
    for k, f in enumerate(parsed):
        palettes[k, :f["palette"].size] = f["palette"]
    palettes = _upload(palettes.view(np.int32), dev)
    counts = _upload(np.array([f["palette"].size for f in parsed], dtype=np.int32), dev)
    descs, pdescs = anysize._upload_descs(entries, dev), anysize._upload_descs(pentries, dev)
    _lib.call("rgbac_color_palette_unmap", len(parsed), descs.data_ptr(), pdescs.data_ptr(),
              _slices(sizes), palettes.data_ptr(), counts.data_ptr(), err.data_ptr(),
              _lib.stream_ptr(dev))


def decode_rgba_lossless(blobs, device="cuda"):
    """blobs: files from encode_rgba_lossless, any number, any order, every transform -> list of
    (h, w, 4) uint8 GPU tensors in the same order.  Every file is parsed and validated on the
    host before any launch (RuntimeError); one plane-decoder launch puts all alpha planes into
    the outputs' alpha bytes, one colour launch per (version, keep_hidden) present fills in
    R, G, B on the same stream; version 3 files have a plane-decoder launch for their index
    planes and one launch that writes whole pixels from them; the one error word is read once at
    the end."""
    blobs = list(blobs)
    if not blobs:
        raise ValueError("decode_rgba_lossless: no files")
    parsed = [parse_rgba_lossless(b) for b in blobs]
    dev = anysize._gpu_device(device)
    _lib.load()
    outs = [torch.empty((f["h"], f["w"], 4), dtype=torch.uint8, device=dev) for f in parsed]
    dev = outs[0].device
    entries = [(t.data_ptr(), f["h"], f["w"], t.stride(0)) for t, f in zip(outs, parsed)]
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ks = [k for k, f in enumerate(parsed) if f["transform"] == "palette"]
    if ks:
        _decode_palette([parsed[k] for k in ks], [entries[k] for k in ks], dev, err)
    ks = [k for k, f in enumerate(parsed) if f["transform"] != "palette"]
    if ks:
        alphaexact._decode([parsed[k]["alpha"] for k in ks],
                           _alpha_entries([entries[k] for k in ks]), 4, dev, err)
    for adaptive in (False, True):
        for flag in (False, True):
            ks = [k for k, f in enumerate(parsed)
                  if (f["transform"], f["keep_hidden"]) == (TRANSFORMS[adaptive], flag)]
            if ks:
                _decode_colour([parsed[k] for k in ks], [entries[k] for k in ks], flag, dev, err,
                               adaptive)
    _raise_code("RGAL file decode", int(err.item()))
    return outs
