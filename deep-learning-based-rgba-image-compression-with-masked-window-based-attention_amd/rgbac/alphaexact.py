"""Lossless alpha planes: the device-side predictive rANS plane coder (csrc/alpha_exact.hip).

``encode_alpha_planes`` takes a ragged batch of uint8 planes -- (h, w) tensors, views into
larger buffers included, or (h, w, 4) RGBA whose alpha bytes are coded where they lie -- and
returns one self-contained ``RGAP`` blob per plane; ``decode_alpha_planes`` takes any list of
blobs and returns the planes, bit for bit.  No model is involved.  GPU only: a CPU device or a
missing library raises.

A plane is cut into 16 x 16 blocks; a block of equal bytes stores its value, every other block
is one chunk of the chunked rANS format (rgbac.ans) coded with the
plane's own five static tables.  Model, table rule and launches: DESIGN.md section 24.

Blob, little-endian:
    "RGAP", u16 version (1), u16 block size (16), u32 h, u32 w, u32 coded blocks, u32 payload
    words; five tables, each u16 n = symbols with a frequency, then n <= 170: n x (u8 symbol,
    u16 frequency), symbols ascending; n > 170: 256 x u16 frequency; one u16 per block, row-major:
    bits 0-1 class (0 coded, 1 constant), bits 8-15 the constant's value; one u16 word count per
    coded block, in block order; the payload, u32 words, the chunks back to back.
A plane of constant blocks only has empty tables, no chunk table and no payload.
"""
import struct

import numpy as np
import torch

from . import _lib
from .ans import _raise_code, _upload
from .anysize import _gpu_device, _upload_descs

MAGIC = b"RGAP"
VERSION = 1
BLOCK = _lib.ALPHA_BLOCK
NCTX = _lib.ALPHA_CONTEXTS
SPARSE_MAX = 170                      # 3 n < 512: the sparse form is the shorter one
MAX_SIDE = 32767
_HEADER = struct.Struct("<4sHHIIII")
HEADER_BYTES = _HEADER.size           # 24
TOTAL = 1 << 16


def normalise_counts(counts):
    """The coder's table rule (the numpy twin of alpha_normalise_kernel): 256 counts -> int64
    frequencies.  All zero for an empty context; otherwise f[s] = 0 where the count is 0, else
    max(1, floor(count * 2^16 / total)); ``top`` is the symbol with the largest count, the lowest
    such symbol on a tie; a context with one symbol gets f[top] = 65535 and f[(top + 1) & 255] =
    1, any other gets the remainder 2^16 - sum(f) added to f[top].  The sum is exactly 2^16,
    every symbol that occurs has a frequency >= 1 and none reaches 2^16.  A valid table is a
    fixed point of the rule, which is how the parser checks one."""
    c = np.asarray(counts, dtype=np.int64).reshape(256)
    if (c < 0).any():
        raise ValueError("normalise_counts: negative count")
    f = np.zeros(256, dtype=np.int64)
    total = int(c.sum())
    if total == 0:
        return f
    occurs = c > 0
    f[occurs] = np.maximum(1, (c[occurs] << 16) // total)
    top = int(np.argmax(c))                         # the first of equal maxima
    if int(occurs.sum()) == 1:
        f[top], f[(top + 1) & 255] = TOTAL - 1, 1
    else:
        f[top] += TOTAL - int(f.sum())
    return f


def device_table(freqs):
    """(5, 256) frequencies -> the uint16[1288] table the kernels stage in LDS: exclusive sums
    mod 2^16, the last symbol with a frequency per context (-1: empty), 3 zeros."""
    f = np.asarray(freqs, dtype=np.int64).reshape(NCTX, 256)
    tab = np.zeros(_lib.ALPHA_TABLE_U16, dtype=np.uint16)
    tab[:NCTX * 256] = ((np.cumsum(f, axis=1) - f) & 0xFFFF).reshape(-1)
    for c in range(NCTX):
        nz = np.flatnonzero(f[c])
        tab[NCTX * 256 + c] = np.int16(nz[-1] if nz.size else -1).view(np.uint16)
    return tab


def block_grid(h, w):
    """-> (block rows, block columns, int64 pixel count of every block, row-major)."""
    by, bx = -(-h // BLOCK), -(-w // BLOCK)
    bh = np.minimum(BLOCK, h - BLOCK * np.arange(by, dtype=np.int64))
    bw = np.minimum(BLOCK, w - BLOCK * np.arange(bx, dtype=np.int64))
    return by, bx, (bh[:, None] * bw[None, :]).reshape(-1)


def _pack_table(f):
    nz = np.flatnonzero(f)
    head = struct.pack("<H", nz.size)
    if nz.size > SPARSE_MAX:
        return head + f.astype("<u2").tobytes()
    rec = np.zeros(nz.size, dtype=np.dtype([("s", "u1"), ("f", "<u2")]))
    rec["s"], rec["f"] = nz, f[nz]
    return head + rec.tobytes()


def build_alpha_planes(h, w, freqs, cls, counts, payload):
    """The pieces of one plane -> bytes.  freqs (5, 256); cls: the blocks' class words; counts:
    the coded blocks' word counts; payload: their words (uint32)."""
    cls = np.asarray(cls)
    return b"".join(
        [_HEADER.pack(MAGIC, VERSION, BLOCK, h, w, int(((cls & 3) == 0).sum()), len(payload))]
        + [_pack_table(np.asarray(f, dtype=np.int64)) for f in freqs]
        + [cls.astype("<u2").tobytes(), np.asarray(counts).astype("<u2").tobytes(),
           np.asarray(payload).astype("<u4").tobytes()])


def parse_alpha_planes(blob):
    """bytes -> {"h", "w", "freqs" (5, 256) int64, "cls" int32 per block, "counts" int32 per
    block (0 for a constant one), "payload" uint32}.  Pure host code; raises RuntimeError on
    anything wrong: bad magic, version, block size or plane size; a truncated or over-long blob;
    a table that does not sum to 2^16, lists a symbol without a frequency or out of order, or is
    not a fixed point of normalise_counts; tables a plane with coded blocks cannot have (context
    0 or 4 empty) or a constant plane must not have; a class table or chunk table whose counts
    are not the ones (h, w) implies; word counts impossible for their blocks or that do not sum
    to the payload."""
    blob = bytes(blob)

    def bad(msg):
        return RuntimeError(f"alpha planes: {msg}")

    if len(blob) < HEADER_BYTES:
        raise bad(f"truncated ({len(blob)} bytes, the header has {HEADER_BYTES})")
    magic, version, block, h, w, ncoded, nwords = _HEADER.unpack_from(blob)
    if magic != MAGIC:
        raise bad("bad magic (not an alpha-plane blob)")
    if version != VERSION:
        raise bad(f"unsupported version {version}")
    if block != BLOCK:
        raise bad(f"unsupported block size {block}")
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise bad(f"bad size {h}x{w}")
    pos = HEADER_BYTES

    def take(n, what):
        nonlocal pos
        if pos + n > len(blob):
            raise bad(f"truncated in the {what}")
        pos += n
        return blob[pos - n:pos]

    freqs = np.zeros((NCTX, 256), dtype=np.int64)
    for c in range(NCTX):
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
    nblk = block_grid(h, w)[2]
    cls = np.frombuffer(take(2 * nblk.size, "class table"), dtype="<u2").astype(np.int32)
    coded = cls == 0
    if ((cls & 0xFC) != 0).any() or (((cls & 3) != 1) & ~coded).any():
        raise bad("class table: unknown block class")
    if int(coded.sum()) != ncoded:
        raise bad(f"the class table has {int(coded.sum())} coded blocks, the header says {ncoded}")
    used = freqs.sum(axis=1) > 0
    if ncoded and not (used[0] and used[4]):
        raise bad("coded blocks without the tables every coded block needs")
    if not ncoded and (used.any() or nwords):
        raise bad("a plane of constant blocks has tables or a payload")
    cnt = np.frombuffer(take(2 * ncoded, "chunk table"), dtype="<u2").astype(np.int64)
    # a chunk holds its two state words and at most 16 bits per symbol
    if (cnt < 2).any() or (cnt > nblk[coded] // 2 + 3).any():
        raise bad("chunk table: a chunk's word count is impossible for its block")
    if int(cnt.sum()) != nwords:
        raise bad(f"the chunk table sums to {int(cnt.sum())} words, the header says {nwords}")
    payload = np.frombuffer(take(4 * nwords, "payload"), dtype="<u4").astype(np.uint32)
    if pos != len(blob):
        raise bad(f"over-long: {len(blob) - pos} bytes after the payload")
    counts = np.zeros(nblk.size, dtype=np.int32)
    counts[coded] = cnt
    return {"h": h, "w": w, "freqs": freqs, "cls": cls, "counts": counts, "payload": payload}


# ---- the CPU twin: the model in numpy, the chunks by the host chunk coder (rgbac.ans)
def model_symbols(plane):
    """(h, w) uint8 -> (symbols, contexts), int32 (h, w): the model of DESIGN.md section 24 for
    every pixel, each inside its own 16 x 16 block."""
    a = np.asarray(plane).astype(np.int64)
    h, w = a.shape
    r0 = np.broadcast_to((np.arange(h) % BLOCK == 0)[:, None], (h, w))
    c0 = np.broadcast_to((np.arange(w) % BLOCK == 0)[None, :], (h, w))
    L, U = np.roll(a, 1, axis=1), np.roll(a, 1, axis=0)
    D = np.roll(U, 1, axis=1)
    # one neighbour only: it stands for all three
    L, U, D = np.where(c0, U, L), np.where(r0, L, U), np.where(r0, L, np.where(c0, U, D))
    lo, hi = np.minimum(L, U), np.maximum(L, U)
    pred = np.where(D >= hi, lo, np.where(D <= lo, hi, L + U - D))
    d = np.maximum(hi, D) - np.minimum(lo, D)
    ctx = (d > 0).astype(np.int64) + (d > 8) + (d > 64)
    first = r0 & c0
    pred, ctx = np.where(first, 0, pred), np.where(first, 4, ctx)
    return ((a - pred) & 255).astype(np.int32), ctx.astype(np.int32)


def _blocks(arr):
    """(h, w) array -> its 16 x 16 blocks, row-major, each flattened in raster order."""
    h, w = arr.shape
    return [arr[r:r + BLOCK, c:c + BLOCK].reshape(-1)
            for r in range(0, h, BLOCK) for c in range(0, w, BLOCK)]


def host_tables(freqs):
    """(5, 256) frequencies -> rgbac.ans.CdfTables the host chunk coder takes: rows of 258
    entries (the 256 symbols, then an escape symbol of frequency 0 that is never coded)."""
    from .ans import CdfTables
    f = np.asarray(freqs, dtype=np.int64).reshape(NCTX, 256)
    cdfs = np.zeros((NCTX, 258), dtype=np.int32)
    cdfs[:, 1:257] = np.cumsum(f, axis=1)
    cdfs[:, 257] = cdfs[:, 256]
    return CdfTables(cdfs, [258] * NCTX, [0] * NCTX)


def encode_alpha_plane_host(plane):
    """encode_alpha_planes for one plane on the CPU: the kernels' byte-level reference (not a
    fallback; the device path never calls it)."""
    from .ans import encode_table_host
    a = np.ascontiguousarray(np.asarray(plane, dtype=np.uint8))
    if a.ndim != 2 or a.size == 0 or max(a.shape) > MAX_SIDE:
        raise ValueError(f"encode_alpha_plane_host: expected an (H, W) uint8 plane, got {a.shape}")
    sym, ctx = model_symbols(a)
    blocks = _blocks(a)
    cls = np.array([1 | (int(b[0]) << 8) if (b == b[0]).all() else 0 for b in blocks],
                   dtype=np.int32)
    coded = np.flatnonzero(cls == 0)
    freqs = np.zeros((NCTX, 256), dtype=np.int64)
    if not coded.size:
        return build_alpha_planes(*a.shape, freqs, cls, [], [])
    s = np.concatenate([_blocks(sym)[k] for k in coded])
    c = np.concatenate([_blocks(ctx)[k] for k in coded])
    for k in range(NCTX):
        freqs[k] = normalise_counts(np.bincount(s[c == k], minlength=256))
    lens = np.array([blocks[k].size for k in coded], dtype=np.int64)
    table = np.stack([np.cumsum(lens) - lens, lens])
    words = encode_table_host(s, c, host_tables(freqs), table, BLOCK * BLOCK)
    return build_alpha_planes(*a.shape, freqs, cls, words[:coded.size],
                              words[coded.size:].view(np.uint32))


# ---- launches
def _views(planes, dev, who, writable=False):
    """planes -> (sizes, descriptor entries, pixel stride, the device tensors behind them).
    (h, w) uint8 or, for reading, (h, w, 4) RGBA; rows are used in place when the pixels of a
    row are 1 or 4 bytes apart, anything else is made dense (an output must be usable as is)."""
    ts = []
    for p in planes:
        t = p if isinstance(p, torch.Tensor) else torch.as_tensor(p)
        if not writable and t.dim() == 3 and t.shape[2] == 4:
            t = t[..., 3]
        if t.dtype != torch.uint8 or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"{who}: expected (H, W) uint8 planes"
                             f"{'' if writable else ' or (H, W, 4) uint8 RGBA'}, got "
                             f"{tuple(t.shape)} {t.dtype}")
        if max(t.shape) > MAX_SIDE:
            raise ValueError(f"{who}: a plane side is at most {MAX_SIDE}, got {tuple(t.shape)}")
        if writable and (t.device.type != "cuda" or t.device != dev):
            raise RuntimeError(f"{who}: outputs must be GPU tensors on {dev} (there is no CPU "
                               f"path), got {t.device}")
        ts.append(t.to(dev, non_blocking=True))
    if not ts:
        raise ValueError(f"{who}: empty batch")

    def stride_of(t):
        return 1 if t.shape[1] == 1 or t.stride(1) == 1 else (4 if t.stride(1) == 4 else 0)

    ps = {stride_of(t) for t in ts}
    if len(ps) > 1 or 0 in ps:
        if writable:
            raise ValueError(f"{who}: outputs must all have pixels 1 byte apart, or all 4")
        ts = [t if stride_of(t) == 1 else t.contiguous() for t in ts]
        ps = {1}
    sizes = [(int(t.shape[0]), int(t.shape[1])) for t in ts]
    return sizes, [(t.data_ptr(), h, w, t.stride(0)) for t, (h, w) in zip(ts, sizes)], ps.pop(), ts


class _Work:
    """The launch geometry of a ragged batch: block counts, each plane's first entry of the
    per-block arrays, and the groups of 64 blocks the coding workgroups serve."""

    def __init__(self, sizes, entries, pixel_stride, dev):
        self.B, self.ps = len(sizes), pixel_stride
        self.nblk = [by * bx for by, bx, _ in (block_grid(h, w) for h, w in sizes)]
        self.base = np.concatenate([[0], np.cumsum(self.nblk)]).astype(np.int64)
        self.N = int(self.base[-1])
        if self.B > 65535 or self.N >= 1 << 31:
            raise ValueError("alpha planes: at most 65535 planes and 2^31 blocks per call")
        groups = np.array([(b, k) for b, n in enumerate(self.nblk)
                           for k in range(0, n, _lib.ALPHA_GROUP)], dtype=np.int32)
        self.ngroups = groups.shape[0]
        self._groups = _upload(groups, dev)
        self._base = _upload(self.base[:-1].astype(np.int32), dev)
        self._descs = _upload_descs(entries, dev)
        self.stream = _lib.stream_ptr(dev)

    def plain(self):
        return (self.B, self._descs.data_ptr(), self.ps, self._base.data_ptr(), self.N)

    def grouped(self):
        return (self.B, self._descs.data_ptr(), self.ps, self.ngroups, self._groups.data_ptr(),
                self._base.data_ptr(), self.N)


def _encode(dev, sizes, entries, pixel_stride):
    """The five launches over a ragged batch (classify, histogram, normalise, sizes, encode) and
    the two host reads: the sizes (class words, word counts, tables), then the words."""
    wk = _Work(sizes, entries, pixel_stride, dev)
    B, N, nf = wk.B, wk.N, NCTX * 256
    meta = torch.empty(2 * N + B * nf, dtype=torch.int32, device=dev)
    cls, counts, freqs = meta[:N], meta[N:2 * N], meta[2 * N:]
    partials = torch.empty(B * _lib.ALPHA_HIST_BLOCKS * nf, dtype=torch.int32, device=dev)
    tables = torch.empty(B * _lib.ALPHA_TABLE_U16, dtype=torch.int16, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call("rgbac_alpha_exact_classify", *wk.grouped(), cls.data_ptr(), wk.stream)
    _lib.call("rgbac_alpha_exact_tables", *wk.plain(), cls.data_ptr(), partials.data_ptr(),
              freqs.data_ptr(), tables.data_ptr(), wk.stream)
    _lib.call("rgbac_alpha_exact_sizes", *wk.grouped(), cls.data_ptr(), tables.data_ptr(),
              counts.data_ptr(), err.data_ptr(), wk.stream)
    ends = torch.cumsum(counts, 0, dtype=torch.int64)
    host = meta.cpu().numpy()                                       # the sizes: one read
    h_cls, h_counts, h_freqs = host[:N], host[N:2 * N], host[2 * N:].reshape(B, NCTX, 256)
    cut = np.concatenate([[0], np.cumsum(h_counts.astype(np.int64))])
    total = int(cut[-1])
    words = torch.empty(total + 1, dtype=torch.int32, device=dev)
    if total:
        _lib.call("rgbac_alpha_exact_encode", *wk.grouped(), cls.data_ptr(), tables.data_ptr(),
                  counts.data_ptr(), ends.data_ptr(), words.data_ptr(), total, err.data_ptr(),
                  wk.stream)
    words[total:].copy_(err)
    words = words.cpu().numpy()                                     # the words: one copy
    _raise_code("encode_alpha_planes", int(words[total]))
    blobs = []
    for b, (h, w) in enumerate(sizes):
        lo, hi = int(wk.base[b]), int(wk.base[b + 1])
        c = h_cls[lo:hi]
        blobs.append(build_alpha_planes(h, w, h_freqs[b], c, h_counts[lo:hi][c == 0],
                                        words[int(cut[lo]):int(cut[hi])].view(np.uint32)))
    return blobs


def _decode(parsed, entries, pixel_stride, dev, err):
    """One launch for parsed blobs onto the planes ``entries`` describe; nothing is read back,
    errors land in ``err``."""
    _decode_job(parsed, entries, pixel_stride, dev, err)()


def _decode_job(parsed, entries, pixel_stride, dev, err):
    """Uploads the merged tables of parsed blobs (class words, word counts and offsets, payloads
    back to back, the LDS tables) -> a function that queues the one decode launch."""
    sizes = [(f["h"], f["w"]) for f in parsed]
    wk = _Work(sizes, entries, pixel_stride, dev)
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
    args = wk.grouped() + (ints[:N].data_ptr(), tables.data_ptr(), off.data_ptr(),
                           ints[N:2 * N].data_ptr(), ints[2 * N:].data_ptr(), int(pbase[-1]),
                           err.data_ptr())

    def launch():
        _lib.call("rgbac_alpha_exact_decode", *args, _lib.stream_ptr(dev))
    launch.keep = (wk, ints, off, tables)          # the device arrays behind the pointers
    return launch


def encode_alpha_planes(images, device="cuda"):
    """images: a list of uint8 planes of any sizes -- (h, w), or (h, w, 4) RGBA whose alpha is
    taken; GPU tensors are read in place, views into larger buffers included -> list[bytes], one
    blob per plane.  A plane's blob does not depend on the planes coded with it."""
    dev = _gpu_device(device)
    _lib.load()
    sizes, entries, ps, keep = _views(list(images), dev, "encode_alpha_planes")
    return _encode(dev, sizes, entries, ps)


def decode_alpha_planes(blobs, out=None, device="cuda"):
    """blobs from encode_alpha_planes, any number, any order -> list of (h, w) uint8 GPU
    tensors.  Every blob is parsed and validated on the host before the one launch.  ``out``:
    a list of GPU uint8 (h, w) tensors to decode into (views into larger buffers included;
    nothing around them is written).  A corrupt payload raises through the rANS error word."""
    blobs = list(blobs)
    if not blobs:
        raise ValueError("decode_alpha_planes: no blobs")
    parsed = [parse_alpha_planes(b) for b in blobs]
    sizes = [(f["h"], f["w"]) for f in parsed]
    if out is None:
        dev = _gpu_device(device)
        flat = torch.empty(sum(h * w for h, w in sizes), dtype=torch.uint8, device=dev)
        dev = flat.device
        cut = np.concatenate([[0], np.cumsum([h * w for h, w in sizes])])
        out = [flat[int(cut[i]):int(cut[i + 1])].view(h, w) for i, (h, w) in enumerate(sizes)]
    else:
        out = list(out)
        if len(out) != len(blobs) or not all(isinstance(t, torch.Tensor) for t in out):
            raise ValueError("decode_alpha_planes: out must be one tensor per blob")
        dev = _gpu_device(out[0].device)
    _lib.load()
    got, entries, ps, keep = _views(out, dev, "decode_alpha_planes", writable=True)
    if got != sizes:
        raise ValueError(f"decode_alpha_planes: the blobs hold planes {sizes}, out has {got}")
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    _decode(parsed, entries, ps, dev, err)
    _raise_code("alpha plane decode", int(err.item()))
    return out
