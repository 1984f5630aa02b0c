"""compressai.ans / compressai._CXX surface over the host rANS coder of librgbac_hip.so.

The reference imports ``BufferedRansEncoder`` and ``RansDecoder`` from compressai.ans
(models/AutoEncoderRGB_Journal.py:5, AutoEncoderMask_Journal.py:6) and uses them at
AutoEncoderRGB_Journal.py:334,367-368 (encode) and :387-388,401 (decode); compressai's
entropy models use ``RansEncoder.encode_with_indexes`` / ``RansDecoder.decode_with_indexes``
and ``_CXX.pmf_to_quantized_cdf``.  Same class / method names and argument meaning; the
coder itself is csrc/rans.cpp (C ABI in include/rgbac.h), byte-compatible with compressai's.
Arguments may be Python lists (as the reference passes them) or numpy / torch int tensors.

Below that surface: the opt-in chunked stream format and its device-side coder
(``encode_chunked``, ``ChunkedDecoder``, ``DeviceCdfTables`` over csrc/rans_dev.hip; the CPU
twins ``encode_chunked_host`` / ``decode_chunked_host``), used by compress / decompress with
coder="device".
"""
import ctypes

import numpy as np
import torch

from . import _lib


def _i32(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x, dtype=np.int32).reshape(-1))


class CdfTables:
    """(cdfs, cdf_lengths, offsets) packed once for the C ABI: cdfs as [ncdf][stride] int32."""

    def __init__(self, cdfs, cdf_lengths, offsets):
        if isinstance(cdfs, torch.Tensor):
            tab = cdfs.detach().cpu().numpy().astype(np.int32)
        elif isinstance(cdfs, np.ndarray):
            tab = cdfs.astype(np.int32)
        else:
            rows = [list(r) for r in cdfs]
            width = max(len(r) for r in rows)
            tab = np.zeros((len(rows), width), dtype=np.int32)
            for i, r in enumerate(rows):
                tab[i, :len(r)] = r
        self.cdfs = np.ascontiguousarray(tab.reshape(tab.shape[0], -1))
        self.sizes = _i32(cdf_lengths)
        self.offsets = _i32(offsets)
        n = self.cdfs.shape[0]
        if self.sizes.size != n or self.offsets.size != n:
            raise ValueError("cdfs, cdf_lengths and offsets disagree on the number of tables")

    @classmethod
    def of(cls, cdfs, cdf_lengths=None, offsets=None):
        return cdfs if isinstance(cdfs, CdfTables) else cls(cdfs, cdf_lengths, offsets)

    def args(self):
        return (self.cdfs.ctypes.data, int(self.cdfs.shape[1]), self.sizes.ctypes.data,
                self.offsets.ctypes.data, int(self.cdfs.shape[0]))


def pmf_to_quantized_cdf(pmf, precision=16):
    """compressai._CXX.pmf_to_quantized_cdf -> list of len(pmf)+1 ints."""
    p = np.ascontiguousarray(np.asarray(
        pmf.detach().cpu() if isinstance(pmf, torch.Tensor) else pmf, dtype=np.float32).reshape(-1))
    out = np.zeros(p.size + 1, dtype=np.uint32)
    _lib.call("rgbac_pmf_to_quantized_cdf", p.ctypes.data, int(p.size), int(precision),
              out.ctypes.data)
    return out.astype(np.int64).tolist()


class BufferedRansEncoder:
    """Buffers (symbol, table) records across encode_with_indexes calls; flush() -> bytes."""

    def __init__(self):
        lib = _lib.load()
        self._h = ctypes.c_void_p()
        _lib.call("rgbac_rans_encoder_create", ctypes.byref(self._h))
        self._destroy = lib.rgbac_rans_encoder_destroy

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._destroy(h)
            self._h = None

    def encode_with_indexes(self, symbols, indexes, cdfs, cdf_lengths=None, offsets=None):
        s, i = _i32(symbols), _i32(indexes)
        if s.size != i.size:
            raise ValueError("symbols and indexes differ in length")
        tab = CdfTables.of(cdfs, cdf_lengths, offsets)
        _lib.call("rgbac_rans_encoder_put", self._h, s.ctypes.data, i.ctypes.data, int(s.size),
                  *tab.args())

    def flush(self):
        cap = int(_lib.load().rgbac_rans_encoder_bound(self._h))
        buf = np.empty(max(cap, 8), dtype=np.uint8)
        nb = ctypes.c_int64(0)
        _lib.call("rgbac_rans_encoder_flush", self._h, buf.ctypes.data, int(buf.size),
                  ctypes.byref(nb))
        return buf[:nb.value].tobytes()


class RansEncoder:
    """One-shot encoder: encode_with_indexes(...) -> bytes."""

    def encode_with_indexes(self, symbols, indexes, cdfs, cdf_lengths=None, offsets=None):
        enc = BufferedRansEncoder()
        enc.encode_with_indexes(symbols, indexes, cdfs, cdf_lengths, offsets)
        return enc.flush()


class RansDecoder:
    """set_stream(bytes) + decode_stream(indexes, ...) (stateful, across slices), or the
    one-shot decode_with_indexes(bytes, indexes, ...).  Returns a list of ints, like compressai;
    ``decode_stream_np`` returns the int32 array without the list conversion."""

    def __init__(self):
        _lib.load()
        self._st = _lib.RansDecoderState()
        self._buf = None

    def set_stream(self, encoded):
        self._buf = np.frombuffer(bytes(encoded), dtype=np.uint8).copy()
        _lib.call("rgbac_rans_decoder_init", ctypes.byref(self._st), self._buf.ctypes.data,
                  int(self._buf.size))

    def decode_stream_np(self, indexes, cdfs, cdf_lengths=None, offsets=None):
        if self._buf is None:
            raise RuntimeError("RansDecoder: set_stream() first")
        i = _i32(indexes)
        out = np.empty(i.size, dtype=np.int32)
        tab = CdfTables.of(cdfs, cdf_lengths, offsets)
        _lib.call("rgbac_rans_decode", ctypes.byref(self._st), i.ctypes.data, int(i.size),
                  *tab.args(), out.ctypes.data)
        return out

    def decode_stream(self, indexes, cdfs, cdf_lengths=None, offsets=None):
        return self.decode_stream_np(indexes, cdfs, cdf_lengths, offsets).tolist()

    def decode_with_indexes(self, encoded, indexes, cdfs, cdf_lengths=None, offsets=None):
        self.set_stream(encoded)
        return self.decode_stream(indexes, cdfs, cdf_lengths, offsets)


# ---------------------------------------------------------------------------------------------
# Chunked stream format: the device-side coder (csrc/rans_dev.hip) and its host twin.
#
# The symbol sequence of a container is ``nseg`` segments; every segment is cut into chunks of
# K symbols (its last chunk may be short) and every chunk is an independent rANS stream, coded
# by one GPU lane.  Container, little-endian u32 words:
#     magic, version (1), K, nseg, nseg symbol counts,
#     then for every chunk in segment order its word count, then the chunks' words.
# The bytes of a chunk are exactly ``RansEncoder().encode_with_indexes(sym[chunk], idx[chunk],
# tables)``, so the size is fixed by the format: header + 4 bytes per chunk of count table +
# each chunk's own 8-byte final state and tail word, i.e. at most 12 bytes per chunk over one
# long stream.  K trades rate against parallelism: a smaller K costs up to 12 bytes more per K
# symbols and gives n / K lanes; the 655,360 y symbols of eight 256 x 256 images are 640 lanes
# at K = 1024 (<= 0.1 bit per symbol of overhead) and 2,560 lanes at K = 256 (<= 0.4 bit).
CHUNK_MAGIC = 0x43524752            # b"RGRC"
CHUNK_VERSION = 1
CHUNK_ERRORS = {1: "read past the end of a chunk", 2: "CDF index out of range",
                3: "corrupt stream or CDF table", 4: "corrupt bypass length",
                5: "chunk table or offsets out of range"}


def _chunk_table(seg_lengths, chunk):
    """-> (seg_lengths int64, per-segment first chunk (nseg + 1), table int64 (2, nchunks):
    row 0 each chunk's first symbol in the container's sequence, row 1 its length)."""
    seg = np.asarray(list(seg_lengths), dtype=np.int64).reshape(-1)
    chunk = int(chunk)
    if chunk <= 0 or chunk >= 1 << 31:
        raise ValueError("chunk size must be a positive 32-bit number")
    if seg.size == 0 or (seg <= 0).any():
        raise ValueError("a container needs at least one segment, each of at least one symbol")
    per = (seg + chunk - 1) // chunk
    first = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    base = np.concatenate([[0], np.cumsum(seg)[:-1]]).astype(np.int64)
    which = np.repeat(np.arange(seg.size), per)
    k = np.arange(int(first[-1]), dtype=np.int64) - first[which]
    tab = np.empty((2, int(first[-1])), dtype=np.int64)
    tab[0] = base[which] + k * chunk
    tab[1] = np.minimum(chunk, seg[which] - k * chunk)
    return seg, first, tab


def _header(chunk, seg):
    return np.concatenate([[CHUNK_MAGIC, CHUNK_VERSION, int(chunk), seg.size], seg]).astype("<u4")


def _raise_code(what, code):
    if code:
        raise RuntimeError(f"{what}: error {code} ({CHUNK_ERRORS.get(code, 'unknown')})")


class ChunkedLayout:
    """A parsed and validated container: K, seg_lengths, counts (words per chunk), offsets
    (first word of each chunk in the payload), payload (uint32), first (per-segment first
    chunk) and table (see _chunk_table).  Anything wrong raises RuntimeError."""

    def __init__(self, blob):
        blob = bytes(blob)
        if len(blob) % 4 != 0 or len(blob) < 20:
            raise RuntimeError("chunked stream: length must be whole 32-bit words, >= 20 bytes")
        w = np.frombuffer(blob, dtype="<u4")
        if int(w[0]) != CHUNK_MAGIC:
            raise RuntimeError("chunked stream: bad magic (not a chunked container)")
        if int(w[1]) != CHUNK_VERSION:
            raise RuntimeError(f"chunked stream: unsupported version {int(w[1])}")
        K, nseg = int(w[2]), int(w[3])
        if K <= 0 or K >= 1 << 31 or nseg <= 0 or 4 + nseg > w.size:
            raise RuntimeError("chunked stream: bad chunk size or segment count")
        seg = w[4:4 + nseg].astype(np.int64)
        if (seg <= 0).any():
            raise RuntimeError("chunked stream: empty segment")
        self.K = K
        self.seg_lengths, self.first, self.table = _chunk_table(seg, K)
        nchunks = int(self.first[-1])
        body = 4 + nseg
        if body + nchunks > w.size:
            raise RuntimeError("chunked stream: the chunk count disagrees with the segment "
                               "lengths (count table longer than the stream)")
        self.counts = w[body:body + nchunks].astype(np.int64)
        self.payload = np.ascontiguousarray(w[body + nchunks:]).astype(np.uint32)
        # every chunk holds its two state words and at most 10 words per symbol
        if (self.counts < 2).any() or (self.counts > 10 * self.table[1] + 2).any():
            raise RuntimeError("chunked stream: the chunk count disagrees with the segment "
                               "lengths (a chunk's word count is impossible for its length)")
        total = int(self.counts.sum())
        if total != self.payload.size:
            raise RuntimeError(f"chunked stream: the counts sum to {total} words, the payload "
                               f"has {self.payload.size}")
        if total == 0:
            raise RuntimeError("chunked stream: empty payload")
        self.offsets = (np.cumsum(self.counts) - self.counts).astype(np.int64)
        self.seg_base = np.concatenate([[0], np.cumsum(self.seg_lengths)]).astype(np.int64)

    def chunk_bytes(self, c):
        o, n = int(self.offsets[c]), int(self.counts[c])
        return self.payload[o:o + n].astype("<u4").tobytes()


class DeviceCdfTables:
    """The (cdfs, lengths, offsets) triple resident on a device, for the chunked kernels;
    built from (and validated like) a CdfTables."""

    def __init__(self, tables, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("DeviceCdfTables needs a GPU device (there is no CPU path)")
        tab = CdfTables.of(tables)
        stride = int(tab.cdfs.shape[1])
        if stride < 3 or (tab.sizes < 3).any() or (tab.sizes > stride).any():
            raise ValueError("CDF length out of range")
        self.device = device
        self.stride, self.ncdf = stride, int(tab.cdfs.shape[0])
        self.cdfs = torch.from_numpy(tab.cdfs).to(device)
        self.sizes = torch.from_numpy(tab.sizes).to(device)
        self.offsets = torch.from_numpy(tab.offsets).to(device)

    def args(self):
        return (self.cdfs.data_ptr(), self.stride, self.sizes.data_ptr(),
                self.offsets.data_ptr(), self.ncdf)


def _dev_i32(t, what):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise RuntimeError(f"{what} must be a GPU tensor (the device coder has no CPU path; "
                           "use encode_chunked_host / decode_chunked_host)")
    if t.dtype != torch.int32:
        raise TypeError(f"{what} must be int32")
    return t.contiguous().view(-1)


def _upload(arr, device):
    """Host array -> device without stalling the host on queued GPU work."""
    return torch.from_numpy(arr).pin_memory().to(device, non_blocking=True)


def _encode_tables(prep, chunk):
    """prep: [(symbols, indexes, DeviceCdfTables, table int64 (2, nchunks)), ...], checked device
    tensors on one device -> per job one host int32 array: the chunks' word counts, then their
    words, in table order.  One sizes and one encode launch per job; all jobs share the host
    reads: the sizes (a few bytes), then one device->host copy of everything."""
    dev = prep[0][0].device
    stream = _lib.stream_ptr(dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    queued = []
    for sym, idx, tab, table in prep:
        nch = table.shape[1]
        tdev = _upload(np.ascontiguousarray(table), dev)
        counts = torch.empty(nch, dtype=torch.int32, device=dev)
        head = (sym.data_ptr(), idx.data_ptr(), int(sym.numel()), 0, tdev[0].data_ptr(),
                tdev[1].data_ptr(), nch, int(chunk)) + tab.args()
        _lib.call("rgbac_rans_chunk_sizes", *head, counts.data_ptr(), err.data_ptr(), stream)
        ends = torch.cumsum(counts, 0, dtype=torch.int64)
        queued.append((head, counts, ends, tdev))
    totals = torch.stack([q[2][-1] for q in queued]).cpu().tolist()   # the sizes: one read
    # one buffer: per job its count table then its words; the error word last
    spans, pos = [], 0
    for (head, counts, ends, _), total in zip(queued, totals):
        spans.append((pos, counts.numel(), int(total)))
        pos += counts.numel() + int(total)
    out = torch.empty(pos + 1, dtype=torch.int32, device=dev)
    for (head, counts, ends, _), (p, nch, total) in zip(queued, spans):
        out[p:p + nch].copy_(counts)
        _lib.call("rgbac_rans_chunk_encode", *head, counts.data_ptr(), ends.data_ptr(),
                  out[p + nch:].data_ptr(), total, err.data_ptr(), stream)
    out[pos:].copy_(err)
    host = out.cpu().numpy()                                          # the bytes: one copy
    _raise_code("encode_chunked", int(host[pos]))
    return [host[p:p + nch + total] for p, nch, total in spans]


def _check_job(sym, idx, tab, dev):
    sym, idx = _dev_i32(sym, "symbols"), _dev_i32(idx, "indexes")
    if not isinstance(tab, DeviceCdfTables):
        raise TypeError("encode_chunked needs DeviceCdfTables")
    if dev is None:
        dev = sym.device
    if idx.device != dev or sym.device != dev or tab.device != dev:
        raise RuntimeError("symbols, indexes and tables must live on one device")
    if sym.numel() != idx.numel():
        raise ValueError("symbols and indexes disagree on the symbol count")
    return sym, idx, dev


def encode_chunked_many(jobs, chunk):
    """jobs: [(symbols, indexes, DeviceCdfTables, seg_lengths), ...] -> [bytes, ...], one
    container per job.  All jobs share the host reads: the containers' sizes (a few bytes),
    then one device->host copy of all finished containers."""
    if not jobs:
        return []
    prep, segs = [], []
    dev = None
    for sym, idx, tab, seg_lengths in jobs:
        sym, idx, dev = _check_job(sym, idx, tab, dev)
        seg, _, table = _chunk_table(seg_lengths, chunk)
        if sym.numel() != int(seg.sum()):
            raise ValueError("symbols, indexes and seg_lengths disagree on the symbol count")
        prep.append((sym, idx, tab, table))
        segs.append(seg)
    return [_header(chunk, seg).tobytes() + words.astype("<i4").tobytes()
            for seg, words in zip(segs, _encode_tables(prep, chunk))]


def encode_chunked(symbols, indexes, tables, seg_lengths, chunk=256):
    """Device int32 symbols / indexes (sum(seg_lengths) each, segments back to back) -> the
    container's bytes.  Two kernel passes (sizes, then encode into the scanned offsets); the
    host reads the total size, then copies the finished bytes once."""
    return encode_chunked_many([(symbols, indexes, tables, seg_lengths)], chunk)[0]


class ChunkedDecoder:
    """Decodes one container on the device.  The header is parsed and validated on the host
    (RuntimeError before any launch); payload, offsets, counts and the chunk table are uploaded
    once.  ``decode_segments`` only queues a kernel; ``check()`` reads the error word.  Several
    decoders may share one error word (``err``)."""

    def __init__(self, blob, device, err=None):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("ChunkedDecoder needs a GPU device (there is no CPU path; "
                               "use decode_chunked_host)")
        lay = ChunkedLayout(blob)
        self.layout, self.device = lay, device
        self.K, self.seg_lengths = lay.K, lay.seg_lengths.tolist()
        self._payload = torch.from_numpy(lay.payload.view(np.int32)).to(device)
        meta = np.stack([lay.offsets, lay.table[0], lay.table[1]])
        self._meta = torch.from_numpy(meta).to(device)               # int64 (3, nchunks)
        self._counts = torch.from_numpy(lay.counts.astype(np.int32)).to(device)
        self._err = err if err is not None else torch.zeros(1, dtype=torch.int32, device=device)

    def decode_segments(self, lo, hi, indexes, tables, out=None):
        """Symbols of segments lo..hi-1 (device int32, flat) from their CDF indexes; no sync."""
        lay = self.layout
        if not 0 <= lo < hi <= len(self.seg_lengths):
            raise ValueError("segment range")
        idx = _dev_i32(indexes, "indexes")
        if not isinstance(tables, DeviceCdfTables):
            raise TypeError("decode_segments needs DeviceCdfTables")
        base, nsym = int(lay.seg_base[lo]), int(lay.seg_base[hi] - lay.seg_base[lo])
        if idx.numel() != nsym:
            raise RuntimeError(f"chunked stream: segments {lo}..{hi - 1} hold {nsym} symbols, "
                               f"{idx.numel()} indexes given")
        if out is None:
            out = torch.empty(nsym, dtype=torch.int32, device=self.device)
        elif (out.dtype != torch.int32 or out.device != idx.device or out.numel() != nsym
              or not out.is_contiguous()):
            raise ValueError("out must be a contiguous device int32 tensor of the segments' size")
        c0, c1 = int(lay.first[lo]), int(lay.first[hi])
        m = self._meta
        _lib.call("rgbac_rans_chunk_decode", self._payload.data_ptr(), int(self._payload.numel()),
                  m[0, c0:].data_ptr(), self._counts[c0:].data_ptr(), idx.data_ptr(), nsym, base,
                  m[1, c0:].data_ptr(), m[2, c0:].data_ptr(), c1 - c0, self.K, *tables.args(),
                  out.data_ptr(), self._err.data_ptr(), _lib.stream_ptr(self.device))
        return out

    def check(self):
        """Reads the error word (a sync); raises RuntimeError naming the first error code."""
        _raise_code("chunked stream decode", int(self._err.item()))


def encode_chunked_host(symbols, indexes, tables, seg_lengths, chunk=256,
                        cdf_lengths=None, offsets=None):
    """encode_chunked on the CPU (the same coder core in a loop over chunks): for tests and
    for writing streams without a GPU.  The device path never calls it."""
    s, i = _i32(symbols), _i32(indexes)
    tab = CdfTables.of(tables, cdf_lengths, offsets)
    seg, _, table = _chunk_table(seg_lengths, chunk)
    if s.size != i.size or s.size != int(seg.sum()):
        raise ValueError("symbols, indexes and seg_lengths disagree on the symbol count")
    return (_header(chunk, seg).tobytes()
            + encode_table_host(s, i, tab, table, chunk).astype("<i4").tobytes())


def decode_chunked_host(blob, indexes, tables, cdf_lengths=None, offsets=None):
    """Decodes a whole container on the CPU -> int32 array of all segments' symbols."""
    lay = ChunkedLayout(blob)
    i = _i32(indexes)
    tab = CdfTables.of(tables, cdf_lengths, offsets)
    nsym = int(lay.seg_base[-1])
    if i.size != nsym:
        raise RuntimeError(f"chunked stream: the container holds {nsym} symbols, "
                           f"{i.size} indexes given")
    out = np.empty(nsym, dtype=np.int32)
    counts = lay.counts.astype(np.int32)
    err = ctypes.c_int32(0)
    _lib.call("rgbac_rans_chunk_decode_host", lay.payload.ctypes.data, int(lay.payload.size),
              lay.offsets.ctypes.data, counts.ctypes.data, i.ctypes.data, nsym, 0,
              lay.table[0].ctypes.data, lay.table[1].ctypes.data, int(lay.first[-1]), lay.K,
              *tab.args(), out.ctypes.data, ctypes.byref(err))
    _raise_code("chunked stream decode", err.value)
    return out


# ---------------------------------------------------------------------------------------------
# Per-image containers from one batched pass (rgbac.rgbafile).  The chunk kernels address any
# ranges of the flat symbol sequence they are given, so B images that share their segment
# lengths are coded by one launch through one table ordered image-major, then segment, then
# chunk; the host cuts the counts and the words into B containers, each byte for byte what
# coding that image alone gives.  Decoding merges the files' tables the other way.  All of it
# is host arithmetic on numpy arrays: the same functions drive the kernels and their *_host
# twins.
def image_major_table(seg_starts, seg_lengths, chunk):
    """seg_starts int64 (B, nseg): where segment s of image b begins in the flat sequence the
    coder is handed.  -> (table int64 (2, B * nch): each chunk's first symbol and length, image
    b's nch chunks at [b * nch, (b + 1) * nch) in container order; nch)."""
    seg, first, tab = _chunk_table(seg_lengths, chunk)
    starts = np.asarray(seg_starts, dtype=np.int64).reshape(-1, seg.size)
    base = np.concatenate([[0], np.cumsum(seg)[:-1]]).astype(np.int64)
    which = np.repeat(np.arange(seg.size), np.diff(first))
    local = tab[0] - base[which]                        # a chunk's offset inside its segment
    nch = int(first[-1])
    table = np.empty((2, starts.shape[0] * nch), dtype=np.int64)
    table[0] = (starts[:, which] + local[None, :]).reshape(-1)
    table[1] = np.tile(tab[1], starts.shape[0])
    return table, nch


def split_containers(words, nimages, seg_lengths, chunk):
    """words: what one image-major pass wrote (every chunk's word count, then the chunks'
    words back to back, in image_major_table order) -> [bytes, ...]: one container per image."""
    seg, first, _ = _chunk_table(seg_lengths, chunk)
    nch = int(first[-1])
    words = np.asarray(words)
    counts = words[:nimages * nch].astype(np.int64)
    payload = words[nimages * nch:]
    if int(counts.sum()) != payload.size:
        raise ValueError("split_containers: the counts do not sum to the payload's length")
    cut = np.concatenate([[0], np.cumsum(counts.reshape(nimages, nch).sum(axis=1))])
    head = _header(chunk, seg).tobytes()
    return [head + counts[b * nch:(b + 1) * nch].astype("<u4").tobytes()
            + payload[int(cut[b]):int(cut[b + 1])].astype("<u4").tobytes()
            for b in range(nimages)]


def merged_decode_tables(layouts, seg_starts):
    """layouts: one ChunkedLayout per file, all with the same seg_lengths; seg_starts int64
    (B, nseg): where segment s of file b lands in the flat output.  -> (payload uint32: the
    files' payloads back to back, meta int64 (3, nseg-major chunks): word offset into that
    payload, first symbol, length; counts int32; first int64 (nseg + 1): segment s of ALL files
    is meta[:, first[s]:first[s + 1]], file-major inside)."""
    l0 = layouts[0]
    nseg, B = l0.seg_lengths.size, len(layouts)
    for lay in layouts:
        if lay.seg_lengths.size != nseg or (lay.seg_lengths != l0.seg_lengths).any():
            raise RuntimeError("chunked stream: the files of a group disagree on their segments")
    starts = np.asarray(seg_starts, dtype=np.int64).reshape(B, nseg)
    pbase = np.concatenate([[0], np.cumsum([lay.payload.size for lay in layouts])]).astype(np.int64)
    meta, counts, first = [], [], [0]
    for s in range(nseg):
        for b, lay in enumerate(layouts):
            c0, c1 = int(lay.first[s]), int(lay.first[s + 1])
            meta.append(np.stack([pbase[b] + lay.offsets[c0:c1],
                                  starts[b, s] + lay.table[0, c0:c1] - lay.seg_base[s],
                                  lay.table[1, c0:c1]]))
            counts.append(lay.counts[c0:c1])
        first.append(first[-1] + sum(int(lay.first[s + 1] - lay.first[s]) for lay in layouts))
    payload = np.concatenate([lay.payload for lay in layouts]).astype(np.uint32)
    return (payload, np.ascontiguousarray(np.concatenate(meta, axis=1)),
            np.concatenate(counts).astype(np.int32), np.asarray(first, dtype=np.int64))


def _span(seg_starts, seg_lengths, lo, hi):
    """(first symbol, symbol count) of the flat range that segments lo..hi-1 of all files cover."""
    st = np.asarray(seg_starts, dtype=np.int64)[:, lo:hi]
    base = int(st.min())
    return base, int((st + np.asarray(seg_lengths, dtype=np.int64)[None, lo:hi]).max()) - base


def encode_table_host(symbols, indexes, tables, table, chunk, cdf_lengths=None, offsets=None):
    """The CPU twin of one sizes + encode pass through an arbitrary chunk table (int64
    (2, nchunks)) -> int32 array: the counts, then the words (what split_containers takes)."""
    s, i = _i32(symbols), _i32(indexes)
    tab = CdfTables.of(tables, cdf_lengths, offsets)
    table = np.ascontiguousarray(table, dtype=np.int64)
    nch = table.shape[1]
    counts = np.zeros(nch, dtype=np.int32)
    total, err = ctypes.c_int64(0), ctypes.c_int32(0)
    head = (s.ctypes.data, i.ctypes.data, int(s.size), 0, table[0].ctypes.data,
            table[1].ctypes.data, nch, int(chunk)) + tab.args()
    _lib.call("rgbac_rans_chunk_encode_host", *head, counts.ctypes.data, None, 0,
              ctypes.byref(total), ctypes.byref(err))
    _raise_code("encode_chunked_host", err.value)
    payload = np.zeros(total.value, dtype=np.uint32)
    _lib.call("rgbac_rans_chunk_encode_host", *head, counts.ctypes.data, payload.ctypes.data,
              int(payload.size), ctypes.byref(total), ctypes.byref(err))
    _raise_code("encode_chunked_host", err.value)
    return np.concatenate([counts, payload.view(np.int32)])


def decode_merged_host(layouts, seg_starts, indexes, tables, cdf_lengths=None, offsets=None):
    """The CPU twin of MergedChunkedDecoder: decodes all segments of all files into one flat
    int32 array laid out by seg_starts (``indexes`` in the same layout)."""
    payload, meta, counts, first = merged_decode_tables(layouts, seg_starts)
    i = _i32(indexes)
    tab = CdfTables.of(tables, cdf_lengths, offsets)
    base, nsym = _span(seg_starts, layouts[0].seg_lengths, 0, layouts[0].seg_lengths.size)
    if base != 0 or i.size != nsym:
        raise RuntimeError(f"chunked stream: the files hold symbols {base}..{base + nsym}, "
                           f"{i.size} indexes given")
    out = np.zeros(nsym, dtype=np.int32)
    err = ctypes.c_int32(0)
    K = max(lay.K for lay in layouts)
    _lib.call("rgbac_rans_chunk_decode_host", payload.ctypes.data, int(payload.size),
              meta[0].ctypes.data, counts.ctypes.data, i.ctypes.data, nsym, 0,
              meta[1].ctypes.data, meta[2].ctypes.data, int(first[-1]), K, *tab.args(),
              out.ctypes.data, ctypes.byref(err))
    _raise_code("chunked stream decode", err.value)
    return out


def encode_image_major(jobs, chunk):
    """jobs: [(symbols, indexes, DeviceCdfTables, seg_starts (B, nseg), seg_lengths), ...] ->
    per job its B containers.  One sizes and one encode launch per job for all B images, the
    host reads shared by all jobs (encode_chunked_many's two)."""
    prep, cuts = [], []
    dev = None
    for sym, idx, tab, seg_starts, seg_lengths in jobs:
        sym, idx, dev = _check_job(sym, idx, tab, dev)
        table, _ = image_major_table(seg_starts, seg_lengths, chunk)
        prep.append((sym, idx, tab, table))
        cuts.append((np.asarray(seg_starts).reshape(-1, len(seg_lengths)).shape[0], seg_lengths))
    return [split_containers(words, B, seg, chunk)
            for (B, seg), words in zip(cuts, _encode_tables(prep, chunk))]


class MergedChunkedDecoder:
    """Decodes a group of containers that share their segment lengths as ONE launch per
    segment range: the payloads are uploaded back to back with merged offset / start / length
    tables (merged_decode_tables).  The interface latent_code expects of ``y_chunked``
    (decode_segments, check); ``layouts`` are parsed, validated ChunkedLayouts."""

    def __init__(self, layouts, seg_starts, device, err=None):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("MergedChunkedDecoder needs a GPU device (there is no CPU path; "
                               "use decode_merged_host)")
        payload, meta, counts, first = merged_decode_tables(layouts, seg_starts)
        self.device, self.K = device, max(lay.K for lay in layouts)
        self.seg_lengths = layouts[0].seg_lengths
        self._starts = np.asarray(seg_starts, dtype=np.int64).reshape(len(layouts), -1)
        self._first = first
        self._payload = _upload(payload.view(np.int32), device)
        self._meta = _upload(meta, device)
        self._counts = _upload(counts, device)
        self._err = err if err is not None else torch.zeros(1, dtype=torch.int32, device=device)

    def decode_segments(self, lo, hi, indexes, tables, out=None):
        """Segments lo..hi-1 of every file (device int32, the flat range they cover); no sync."""
        if not 0 <= lo < hi <= self.seg_lengths.size:
            raise ValueError("segment range")
        idx = _dev_i32(indexes, "indexes")
        if not isinstance(tables, DeviceCdfTables):
            raise TypeError("decode_segments needs DeviceCdfTables")
        base, nsym = _span(self._starts, self.seg_lengths, lo, hi)
        if idx.numel() != nsym:
            raise RuntimeError(f"chunked stream: segments {lo}..{hi - 1} cover {nsym} symbols, "
                               f"{idx.numel()} indexes given")
        if out is None:
            out = torch.empty(nsym, dtype=torch.int32, device=self.device)
        elif (out.dtype != torch.int32 or out.device != idx.device or out.numel() != nsym
              or not out.is_contiguous()):
            raise ValueError("out must be a contiguous device int32 tensor of the segments' size")
        c0, c1 = int(self._first[lo]), int(self._first[hi])
        m = self._meta
        _lib.call("rgbac_rans_chunk_decode", self._payload.data_ptr(), int(self._payload.numel()),
                  m[0, c0:].data_ptr(), self._counts[c0:].data_ptr(), idx.data_ptr(), nsym, base,
                  m[1, c0:].data_ptr(), m[2, c0:].data_ptr(), c1 - c0, self.K, *tables.args(),
                  out.data_ptr(), self._err.data_ptr(), _lib.stream_ptr(self.device))
        return out

    def check(self):
        _raise_code("chunked stream decode", int(self._err.item()))
