"""Palette index planes: the device-side neighbour-match rANS coder (csrc/index_exact.hip).

``encode_index_planes`` takes a ragged batch of uint8 planes of palette positions and the number
of positions each may use, and returns one self-contained ``RGAI`` blob per plane;
``decode_index_planes`` takes any list of blobs and returns the planes, bit for bit.  GPU only: a
CPU device or a missing library raises.

A position is a label, so nothing predicts its value.  A plane is cut into 16 x 16 blocks that
decode alone; a block of equal bytes stores its value, every other block is one chunk of the
chunked rANS format (rgbac.ans).  A pixel of a chunk is the rank of the
neighbour it equals among W, N, NE, NW inside its block (duplicates dropped), or an escape and
the position itself; the context is how the neighbours equal one another.  ``model_symbols`` is
the model's definition; format, table rule and launches: DESIGN.md section 32.

Blob, little-endian:
    "RGAI", u16 version (1), u16 block size (16), u32 h, u32 w, u32 n = positions of the palette
    (1..256), u32 coded blocks, u32 payload words; 64 match tables over the symbols 0..4, each
    u16 count, then count x (u8 symbol, u16 frequency), symbols ascending; the literal table in
    the RGAP table form; one u16 per block and one u16 word count per coded block as in RGAP; the
    payload, u32 words, the chunks back to back.
A plane of constant blocks only has empty tables, no chunk table and no payload.  A literal is
stored whatever its value: n binds the reader of the plane, not the coder.
"""
import struct

import numpy as np
import torch

from . import _lib
from .alphaexact import (BLOCK, MAX_SIDE, SPARSE_MAX, TOTAL, _blocks, _pack_table, _views, _Work,
                         block_grid, normalise_counts)
from .ans import _raise_code, _upload
from .anysize import _gpu_device

MAGIC = b"RGAI"
VERSION = 1
NCTX = _lib.INDEX_CONTEXTS            # 64 match tables; table 64 is the literals'
NSYM = _lib.INDEX_SYMBOLS             # ranks 0..3 and the escape
ESCAPE = NSYM - 1
NMATCH = NCTX * NSYM
NBINS = _lib.INDEX_TABLE_U16          # 320 match frequencies, then 256 literal ones
CHUNK = 2 * BLOCK * BLOCK             # a block holds up to two symbols per pixel
_HEADER = struct.Struct("<4sHHIIIII")
HEADER_BYTES = _HEADER.size           # 28
_REC = np.dtype([("s", "u1"), ("f", "<u2")])


def normalise_match(counts):
    """alphaexact.normalise_counts over the alphabet 0..4: 5 counts -> int64 frequencies; a table
    with one symbol puts its spare frequency 1 on (top + 1) % 5."""
    f = normalise_counts(np.concatenate([np.asarray(counts, dtype=np.int64).reshape(NSYM),
                                         np.zeros(256 - NSYM, dtype=np.int64)]))
    if f[NSYM]:                                              # the spare of a lone escape
        f[0], f[NSYM] = f[NSYM], 0
    return f[:NSYM]


def _normalise(counts):
    """(576,) counts -> (576,) frequencies: normalise_match for the 64 match tables at once,
    normalise_counts for the literals."""
    c = np.asarray(counts, dtype=np.int64).reshape(NBINS)
    m = c[:NMATCH].reshape(NCTX, NSYM)
    total = m.sum(axis=1)
    f = np.where(m > 0, np.maximum(1, (m << 16) // np.maximum(total, 1)[:, None]), 0)
    rows, top = np.arange(NCTX), np.argmax(m, axis=1)       # the first of equal maxima
    one = (m > 0).sum(axis=1) == 1
    f[rows, top] += np.where(one | (total == 0), 0, TOTAL - f.sum(axis=1))
    f[rows[one], top[one]] = TOTAL - 1
    f[rows[one], (top[one] + 1) % NSYM] = 1
    return np.concatenate([f.reshape(-1), normalise_counts(c[NMATCH:])])


def device_table(freqs):
    """(576,) frequencies -> the uint16[576] table the kernels stage in LDS: every table's
    exclusive sums mod 2^16."""
    f = np.asarray(freqs, dtype=np.int64).reshape(NBINS)
    m, lit = f[:NMATCH].reshape(NCTX, NSYM), f[NMATCH:]
    return (np.concatenate([(np.cumsum(m, axis=1) - m).reshape(-1), np.cumsum(lit) - lit])
            & 0xFFFF).astype(np.uint16)


def host_tables(freqs):
    """(576,) frequencies -> the rgbac.ans.CdfTables of the 65 tables for the host chunk coder
    (rows of 258 entries, as alphaexact.host_tables; row 64 is the literal table)."""
    from .ans import CdfTables
    f = np.asarray(freqs, dtype=np.int64).reshape(NBINS)
    rows = np.zeros((NCTX + 1, 256), dtype=np.int64)
    rows[:NCTX, :NSYM], rows[NCTX] = f[:NMATCH].reshape(NCTX, NSYM), f[NMATCH:]
    cdfs = np.zeros((NCTX + 1, 258), dtype=np.int32)
    cdfs[:, 1:257] = np.cumsum(rows, axis=1)
    cdfs[:, 257] = cdfs[:, 256]
    return CdfTables(cdfs, [258] * (NCTX + 1), [0] * (NCTX + 1))


def build_index_planes(h, w, n, freqs, cls, counts, payload):
    """The pieces of one plane -> bytes.  freqs (576,); cls: the blocks' class words; counts: the
    coded blocks' word counts; payload: their words (uint32)."""
    cls, f = np.asarray(cls), np.asarray(freqs, dtype=np.int64).reshape(NBINS)
    return b"".join(
        [_HEADER.pack(MAGIC, VERSION, BLOCK, h, w, n, int(((cls & 3) == 0).sum()), len(payload))]
        + [_pack_table(f[k * NSYM:(k + 1) * NSYM]) for k in range(NCTX)]
        + [_pack_table(f[NMATCH:]), cls.astype("<u2").tobytes(),
           np.asarray(counts).astype("<u2").tobytes(), np.asarray(payload).astype("<u4").tobytes()])


def parse_index_planes(blob):
    """bytes -> {"h", "w", "n", "freqs" (576,) int64, "cls" int32 per block, "counts" int32 per
    block (0 for a constant one), "payload" uint32}.  Pure host code; raises RuntimeError on
    anything wrong: bad magic, version, block size, plane size or n outside 1..256; a truncated or
    over-long blob; a table that lists one symbol, a symbol outside its alphabet, out of order or
    without a frequency, that does not sum to 2^16 or is not a fixed point of its rule; coded
    blocks without a literal table, or tables in a plane of constant blocks; a class table or
    chunk table whose counts are not the ones (h, w) implies; word counts outside [2, block
    pixels + 3] or that do not sum to the payload."""
    blob = bytes(blob)

    def bad(msg):
        return RuntimeError(f"index planes: {msg}")

    if len(blob) < HEADER_BYTES:
        raise bad(f"truncated ({len(blob)} bytes, the header has {HEADER_BYTES})")
    magic, version, block, h, w, n, ncoded, nwords = _HEADER.unpack_from(blob)
    if magic != MAGIC:
        raise bad("bad magic (not an index-plane blob)")
    if version != VERSION:
        raise bad(f"unsupported version {version}")
    if block != BLOCK:
        raise bad(f"unsupported block size {block}")
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise bad(f"bad size {h}x{w}")
    if not 1 <= n <= 256:
        raise bad(f"a palette of {n} positions")
    pos = HEADER_BYTES

    def take(k, what):
        nonlocal pos
        if pos + k > len(blob):
            raise bad(f"truncated in the {what}")
        pos += k
        return blob[pos - k:pos]

    freqs = np.zeros(NBINS, dtype=np.int64)
    for c in range(NCTX + 1):
        size = NSYM if c < NCTX else 256
        f = freqs[c * NSYM:c * NSYM + size]                  # a view
        k = struct.unpack("<H", take(2, "tables"))[0]
        if k > size or k == 1:
            raise bad(f"table {c} lists {k} symbols")
        if k > SPARSE_MAX:
            f[:] = np.frombuffer(take(512, "tables"), dtype="<u2")
            if int((f > 0).sum()) != k:
                raise bad(f"table {c}: the symbol count disagrees with its frequencies")
        elif k:
            rec = np.frombuffer(take(3 * k, "tables"), dtype=_REC)
            if (np.diff(rec["s"].astype(np.int64)) <= 0).any() or (rec["f"] == 0).any():
                raise bad(f"table {c}: symbols out of order or without a frequency")
            if int(rec["s"][-1]) >= size:
                raise bad(f"table {c} lists symbol {int(rec['s'][-1])}, its alphabet has {size}")
            f[rec["s"]] = rec["f"]
        if k and int(f.sum()) != TOTAL:
            raise bad(f"table {c} sums to {int(f.sum())}, not 2^16")
    off = np.flatnonzero(_normalise(freqs) != freqs)
    if off.size:
        raise bad(f"table {min(int(off[0]) // NSYM, NCTX)} is not a normalised table")
    nblk = block_grid(h, w)[2]
    cls = np.frombuffer(take(2 * nblk.size, "class table"), dtype="<u2").astype(np.int32)
    coded = cls == 0
    if ((cls & 0xFC) != 0).any() or (((cls & 3) != 1) & ~coded).any():
        raise bad("class table: unknown block class")
    if int(coded.sum()) != ncoded:
        raise bad(f"the class table has {int(coded.sum())} coded blocks, the header says {ncoded}")
    if ncoded and not (freqs[NMATCH:].any() and freqs[:NMATCH].any()):
        raise bad("coded blocks without the tables every coded block needs")
    if not ncoded and (freqs.any() or nwords):
        raise bad("a plane of constant blocks has tables or a payload")
    cnt = np.frombuffer(take(2 * ncoded, "chunk table"), dtype="<u2").astype(np.int64)
    # a chunk holds its two state words and at most two symbols of 16 bits per pixel
    if (cnt < 2).any() or (cnt > nblk[coded] + 3).any():
        raise bad("chunk table: a chunk's word count is impossible for its block")
    if int(cnt.sum()) != nwords:
        raise bad(f"the chunk table sums to {int(cnt.sum())} words, the header says {nwords}")
    payload = np.frombuffer(take(4 * nwords, "payload"), dtype="<u4").astype(np.uint32)
    if pos != len(blob):
        raise bad(f"over-long: {len(blob) - pos} bytes after the payload")
    counts = np.zeros(nblk.size, dtype=np.int32)
    counts[coded] = cnt
    return {"h": h, "w": w, "n": n, "freqs": freqs, "cls": cls, "counts": counts,
            "payload": payload}


# ---- the CPU twin: the model in numpy, the chunks by the host chunk coder (rgbac.ans)
def model_symbols(plane):
    """(h, w) uint8 -> (symbols, contexts), int32 (h, w): the model of DESIGN.md section 32 for
    every pixel, each inside its own 16 x 16 block.  A symbol is the rank 0..3 of the candidate
    the pixel equals or 4, the escape; the first pixel of a block has symbol -1 and context 64:
    it is a literal without a match symbol."""
    a = np.asarray(plane).astype(np.int64)
    h, w = a.shape
    r = np.broadcast_to((np.arange(h) % BLOCK)[:, None], (h, w))
    c = np.broadcast_to((np.arange(w) % BLOCK)[None, :], (h, w))

    def at(dy, dx, inside, absent):
        """The pixel dy rows up and dx columns to the left where ``inside``, else ``absent``."""
        return np.where(inside, np.roll(a, (dy, dx), axis=(0, 1)), absent)

    left, up = at(0, 1, c >= 1, -1), at(1, 0, r >= 1, -1)
    W, N = np.where(c >= 1, left, up), np.where(r >= 1, up, left)
    NW = at(1, 1, (r >= 1) & (c >= 1), -1)
    NE = at(1, -1, (r >= 1) & (c + 1 < BLOCK) & (np.arange(w)[None, :] + 1 < w), -2)
    ctx = ((W == N) * 1 | (N == NW) * 2 | (N == NE) * 4 | (W == NW) * 8
           | (left == at(0, 2, c >= 2, -3)) * 16 | (up == at(2, 0, r >= 2, -3)) * 32)
    keep = [np.ones((h, w), dtype=bool), N != W, (NE >= 0) & (NE != W) & (NE != N),
            (NW >= 0) & (NW != W) & (NW != N) & (NW != NE)]
    sym = np.full((h, w), ESCAPE, dtype=np.int64)
    rank = np.zeros((h, w), dtype=np.int64)
    for cand, k in zip((W, N, NE, NW), keep):
        sym = np.where(k & (a == cand), rank, sym)
        rank = rank + k
    first = (r == 0) & (c == 0)
    return np.where(first, -1, sym).astype(np.int32), np.where(first, NCTX, ctx).astype(np.int32)


def _stream(p, sym, ctx):
    """One block's pixels, symbols and contexts in raster order -> (symbols, tables) in decode
    order: per pixel the match symbol, then the literal where there is one."""
    s = np.stack([sym, p.astype(np.int32)], axis=1)
    t = np.stack([ctx, np.full(ctx.shape, NCTX, dtype=np.int32)], axis=1)
    use = np.stack([sym >= 0, (sym == ESCAPE) | (sym < 0)], axis=1)
    return s[use], t[use]


def encode_index_plane_host(plane, n=256):
    """encode_index_planes for one plane on the CPU: the kernels' byte-level reference (not a
    fallback; the device path never calls it)."""
    from .ans import encode_table_host
    a = np.ascontiguousarray(np.asarray(plane, dtype=np.uint8))
    if a.ndim != 2 or a.size == 0 or max(a.shape) > MAX_SIDE:
        raise ValueError(f"encode_index_plane_host: expected an (H, W) uint8 plane, got {a.shape}")
    if not 1 <= int(n) <= 256:
        raise ValueError(f"encode_index_plane_host: n must be in 1..256, got {n}")
    sym, ctx = model_symbols(a)
    blocks = _blocks(a)
    cls = np.array([1 | (int(b[0]) << 8) if (b == b[0]).all() else 0 for b in blocks],
                   dtype=np.int32)
    coded = np.flatnonzero(cls == 0)
    if not coded.size:
        return build_index_planes(*a.shape, int(n), np.zeros(NBINS, dtype=np.int64), cls, [], [])
    bs, bc = _blocks(sym), _blocks(ctx)
    streams = [_stream(blocks[k], bs[k], bc[k]) for k in coded]
    s = np.concatenate([x[0] for x in streams])
    t = np.concatenate([x[1] for x in streams])
    freqs = _normalise(np.bincount(np.where(t < NCTX, t * NSYM + s, NMATCH + s),
                                   minlength=NBINS))
    lens = np.array([x[0].size for x in streams], dtype=np.int64)
    table = np.stack([np.cumsum(lens) - lens, lens])
    words = encode_table_host(s, t, host_tables(freqs), table, CHUNK)
    return build_index_planes(*a.shape, int(n), freqs, cls, words[:coded.size],
                              words[coded.size:].view(np.uint32))


def _decode_block_host(words, bh, bw, freqs):
    """One chunk -> its (bh, bw) block: the model and the rANS state machine of csrc/rans_chunk.h
    pixel by pixel, in plain Python.  Raises RuntimeError on a chunk that is not sound."""
    f = np.asarray(freqs, dtype=np.int64).reshape(NBINS)
    ends = [np.cumsum(f[k * NSYM:(k + 1) * NSYM]) for k in range(NCTX)] + [np.cumsum(f[NMATCH:])]
    words = [int(x) for x in words]
    if len(words) < 2:
        raise RuntimeError("index planes: a chunk without its state words")
    state, nread = words[0] | (words[1] << 32), 2

    def pop(table):
        nonlocal state, nread
        cum = state & 0xFFFF
        if not ends[table][-1]:
            raise RuntimeError("index planes: a symbol in an empty table")
        s = int(np.searchsorted(ends[table], cum, side="right"))
        freq = int(ends[table][s]) - (int(ends[table][s - 1]) if s else 0)
        state = freq * (state >> 16) + cum - (int(ends[table][s]) - freq)
        if state < 1 << 31:
            if nread >= len(words):
                raise RuntimeError("index planes: a chunk ends before its symbols")
            state, nread = (state << 32) | words[nread], nread + 1
        return s

    out = np.zeros((bh, bw), dtype=np.int64)
    for r in range(bh):
        for c in range(bw):
            if r == 0 and c == 0:
                out[0, 0] = pop(NCTX)
                continue
            W = out[r, c - 1] if c else out[r - 1, c]
            N = out[r - 1, c] if r else out[r, c - 1]
            NW = out[r - 1, c - 1] if r and c else -1
            NE = out[r - 1, c + 1] if r and c + 1 < bw else -2
            ctx = ((W == N) | (N == NW) << 1 | (N == NE) << 2 | (W == NW) << 3
                   | (c >= 2 and out[r, c - 1] == out[r, c - 2]) << 4
                   | (r >= 2 and out[r - 1, c] == out[r - 2, c]) << 5)
            kept = []
            for cand in (W, N, NE, NW):
                if cand >= 0 and cand not in kept:
                    kept.append(cand)
            sym = pop(int(ctx))
            if sym != ESCAPE and sym >= len(kept):
                raise RuntimeError("index planes: a rank past the pixel's candidates")
            out[r, c] = pop(NCTX) if sym == ESCAPE else kept[sym]
    if state != 1 << 31 or nread != len(words):
        raise RuntimeError("index planes: a chunk does not end where its coder began")
    return out.astype(np.uint8)


def decode_index_plane_host(blob):
    """One blob -> the (h, w) uint8 plane, on the CPU, pixel by pixel (small planes only)."""
    f = parse_index_planes(blob)
    h, w = f["h"], f["w"]
    out = np.zeros((h, w), dtype=np.uint8)
    off = np.cumsum(f["counts"]) - f["counts"]
    k = 0
    for r in range(0, h, BLOCK):
        for c in range(0, w, BLOCK):
            bh, bw = min(BLOCK, h - r), min(BLOCK, w - c)
            if f["cls"][k] & 3:
                out[r:r + bh, c:c + bw] = f["cls"][k] >> 8
            else:
                out[r:r + bh, c:c + bw] = _decode_block_host(
                    f["payload"][off[k]:off[k] + f["counts"][k]], bh, bw, f["freqs"])
            k += 1
    return out


# ---- launches
def _check_counts(counts, nplanes, who):
    ns = [int(n) for n in counts]
    if len(ns) != nplanes or not all(1 <= n <= 256 for n in ns):
        raise ValueError(f"{who}: counts must hold one n in 1..256 per plane, got {ns}")
    return ns


def _encode(dev, sizes, entries, ns):
    """The five launches over a ragged batch (the plane coder's classify, then histogram,
    normalise, sizes, encode) and the two host reads: the sizes (class words, word counts,
    frequencies), then the words."""
    wk = _Work(sizes, entries, 1, dev)
    B, N = wk.B, wk.N
    meta = torch.empty(2 * N + B * NBINS, dtype=torch.int32, device=dev)
    cls, counts, freqs = meta[:N], meta[N:2 * N], meta[2 * N:]
    partials = torch.empty(B * _lib.INDEX_HIST_BLOCKS * NBINS, dtype=torch.int32, device=dev)
    tables = torch.empty(B * NBINS, dtype=torch.int16, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    plain = (B, wk._descs.data_ptr(), wk._base.data_ptr(), N)
    grouped = (B, wk._descs.data_ptr(), wk.ngroups, wk._groups.data_ptr(), wk._base.data_ptr(), N)
    _lib.call("rgbac_alpha_exact_classify", *wk.grouped(), cls.data_ptr(), wk.stream)
    _lib.call("rgbac_index_exact_tables", *plain, cls.data_ptr(), partials.data_ptr(),
              freqs.data_ptr(), tables.data_ptr(), wk.stream)
    _lib.call("rgbac_index_exact_sizes", *grouped, cls.data_ptr(), tables.data_ptr(),
              counts.data_ptr(), err.data_ptr(), wk.stream)
    ends = torch.cumsum(counts, 0, dtype=torch.int64)
    host = meta.cpu().numpy()                                       # the sizes: one read
    h_cls, h_counts, h_freqs = host[:N], host[N:2 * N], host[2 * N:].reshape(B, NBINS)
    cut = np.concatenate([[0], np.cumsum(h_counts.astype(np.int64))])
    total = int(cut[-1])
    words = torch.empty(total + 1, dtype=torch.int32, device=dev)
    if total:
        _lib.call("rgbac_index_exact_encode", *grouped, cls.data_ptr(), tables.data_ptr(),
                  counts.data_ptr(), ends.data_ptr(), words.data_ptr(), total, err.data_ptr(),
                  wk.stream)
    words[total:].copy_(err)
    words = words.cpu().numpy()                                     # the words: one copy
    _raise_code("encode_index_planes", int(words[total]))
    blobs = []
    for b, (h, w) in enumerate(sizes):
        lo, hi = int(wk.base[b]), int(wk.base[b + 1])
        c = h_cls[lo:hi]
        blobs.append(build_index_planes(h, w, ns[b], h_freqs[b], c, h_counts[lo:hi][c == 0],
                                        words[int(cut[lo]):int(cut[hi])].view(np.uint32)))
    return blobs


def _decode(parsed, entries, dev, err):
    """One launch for parsed blobs onto the planes ``entries`` describe; nothing is read back,
    errors land in ``err``."""
    sizes = [(f["h"], f["w"]) for f in parsed]
    wk = _Work(sizes, entries, 1, dev)
    counts = np.concatenate([f["counts"] for f in parsed])
    pbase = np.concatenate([[0], np.cumsum([f["payload"].size for f in parsed])])
    off = np.concatenate([pbase[i] + np.cumsum(f["counts"], dtype=np.int64) - f["counts"]
                          for i, f in enumerate(parsed)]).astype(np.int64)
    payload = np.concatenate([f["payload"] for f in parsed] + [np.zeros(1, dtype=np.uint32)])
    ints = _upload(np.concatenate([np.concatenate([f["cls"] for f in parsed]), counts,
                                   payload.view(np.int32)]).astype(np.int32), dev)
    off = _upload(off, dev)
    tables = _upload(np.concatenate([device_table(f["freqs"]) for f in parsed]).view(np.int16),
                     dev)
    N = wk.N
    _lib.call("rgbac_index_exact_decode", wk.B, wk._descs.data_ptr(), wk.ngroups,
              wk._groups.data_ptr(), wk._base.data_ptr(), N, ints[:N].data_ptr(),
              tables.data_ptr(), off.data_ptr(), ints[N:2 * N].data_ptr(),
              ints[2 * N:].data_ptr(), int(pbase[-1]), err.data_ptr(), wk.stream)


def encode_index_planes(planes, counts, device="cuda"):
    """planes: a list of (h, w) uint8 planes of palette positions of any sizes; GPU tensors are
    read in place, views with longer rows included; counts: each plane's n, the positions its
    palette has -> list[bytes], one blob per plane.  A blob does not depend on the planes coded
    with it."""
    dev = _gpu_device(device)
    _lib.load()
    planes = list(planes)
    if any(isinstance(p, torch.Tensor) and p.dim() != 2 for p in planes):
        raise ValueError("encode_index_planes: expected (H, W) uint8 planes")
    sizes, entries, ps, keep = _views(planes, dev, "encode_index_planes")
    if ps != 1:                                                     # pixels 4 bytes apart
        keep = [t.contiguous() for t in keep]
        entries = [(t.data_ptr(), h, w, t.stride(0)) for t, (h, w) in zip(keep, sizes)]
    return _encode(dev, sizes, entries, _check_counts(counts, len(sizes), "encode_index_planes"))


def decode_index_planes(blobs, device="cuda"):
    """blobs from encode_index_planes, any number, any order -> list of (h, w) uint8 GPU tensors.
    Every blob is parsed and validated on the host before the one launch; a corrupt payload
    raises through the rANS error word."""
    blobs = list(blobs)
    if not blobs:
        raise ValueError("decode_index_planes: no blobs")
    parsed = [parse_index_planes(b) for b in blobs]
    dev = _gpu_device(device)
    _lib.load()
    cut = np.concatenate([[0], np.cumsum([-(-f["h"] * f["w"] // 16) * 16 for f in parsed])])
    flat = torch.empty(int(cut[-1]), dtype=torch.uint8, device=dev)
    out = [flat[int(cut[i]):int(cut[i]) + f["h"] * f["w"]].view(f["h"], f["w"])
           for i, f in enumerate(parsed)]
    err = torch.zeros(1, dtype=torch.int32, device=flat.device)
    _decode(parsed, [(t.data_ptr(), f["h"], f["w"], f["w"]) for t, f in zip(out, parsed)],
            flat.device, err)
    _raise_code("index plane decode", int(err.item()))
    return out
