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


# ---------------------------------------------------------------------------------------------
# Lanes stream format: the lane-interleaved device coder (csrc/rans_lanes.hip) and its host twin
# (DESIGN.md section 25).
#
# A segment is cut into groups of at most W * K symbols (W lanes, K steps); symbol j of a group
# belongs to lane j % W at step j / W.  A lane is a 32-bit rANS state with byte renormalisation;
# the W lanes of a group share one byte stream ordered by the decoder's reads.  Container,
# little-endian u32:
#     magic, version (1), W, K, nseg, nseg symbol counts (0 allowed),
#     then for every group in segment order its byte count, then the groups' bytes (W final
#     states, then the stream), zero-padded to a multiple of 4.
# The size is fixed by the format: 20 + 4 * nseg bytes of header and 4 * W + 4 bytes per group
# over the ideal code length (plus at most 0.0113 bit per record of state granularity), i.e.
# 68 bytes per 8,192 symbols at W = 16, K = 512 where the chunked format pays 12 per 256.
LANES_MAGIC = 0x4C524752            # b"RGRL"
LANES_VERSION = 1
LANES_WIDTHS = (8, 16, 32, 64)
LANES_DEFAULT = (64, 256)           # (lanes, steps): the fastest of tools/lanes_bench.py's sweep
LANES_LDS_ENTRIES = 24576           # RGBAC_LANES_LDS_ENTRIES: larger tables stay in global memory


def _check_lanes(lanes, steps):
    lanes, steps = int(lanes), int(steps)
    if lanes not in LANES_WIDTHS:
        raise ValueError(f"lanes must be one of {LANES_WIDTHS}, got {lanes}")
    if steps <= 0 or steps > 1 << 24:
        raise ValueError("steps must be in 1 .. 2^24")
    return lanes, steps


def _group_table(seg_lengths, lanes, steps):
    """-> (seg_lengths int64, per-segment first group (nseg + 1), table int64 (2, ngroups): each
    group's first symbol in the container's sequence and its length).  Segments may be empty."""
    seg = np.asarray(list(seg_lengths), dtype=np.int64).reshape(-1)
    lanes, steps = _check_lanes(lanes, steps)
    if seg.size == 0 or (seg < 0).any() or (seg >= 1 << 32).any():
        raise ValueError("a container needs at least one segment of 0 .. 2^32 - 1 symbols")
    G = lanes * steps
    per = (seg + G - 1) // G
    first = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    base = np.concatenate([[0], np.cumsum(seg)[:-1]]).astype(np.int64)
    which = np.repeat(np.arange(seg.size), per)
    k = np.arange(int(first[-1]), dtype=np.int64) - first[which]
    tab = np.empty((2, int(first[-1])), dtype=np.int64)
    tab[0] = base[which] + k * G
    tab[1] = np.minimum(G, seg[which] - k * G)
    return seg, first, tab


def _lanes_header(lanes, steps, seg):
    return np.concatenate([[LANES_MAGIC, LANES_VERSION, lanes, steps, seg.size],
                           seg]).astype("<u4").tobytes()


def _lanes_blob(lanes, steps, seg, counts, payload):
    body = np.asarray(payload, dtype=np.uint8).tobytes()
    return (_lanes_header(lanes, steps, seg) + np.asarray(counts).astype("<u4").tobytes()
            + body + b"\0" * (-len(body) % 4))


class LanesLayout:
    """A parsed and validated lanes container: W, K, seg_lengths, counts (bytes per group),
    offsets (first byte of each group in the payload), payload (uint8, a multiple of 4 long),
    first (per-segment first group) and table (see _group_table).  Anything wrong raises
    RuntimeError."""

    def __init__(self, blob):
        blob = bytes(blob)
        if len(blob) % 4 != 0 or len(blob) < 24:
            raise RuntimeError("lanes stream: length must be whole 32-bit words, >= 24 bytes")
        w = np.frombuffer(blob, dtype="<u4")
        if int(w[0]) != LANES_MAGIC:
            raise RuntimeError("lanes stream: bad magic (not a lanes container)")
        if int(w[1]) != LANES_VERSION:
            raise RuntimeError(f"lanes stream: unsupported version {int(w[1])}")
        W, K, nseg = int(w[2]), int(w[3]), int(w[4])
        if W not in LANES_WIDTHS or K <= 0 or K > 1 << 24:
            raise RuntimeError(f"lanes stream: bad lane count {W} or step count {K}")
        if nseg <= 0 or 5 + nseg > w.size:
            raise RuntimeError("lanes stream: bad segment count (truncated header)")
        self.W, self.K = W, K
        body = 5 + nseg
        # the group count the header implies, checked against the blob before any table of
        # that size is built
        ngroups = int(((w[5:body].astype(np.int64) + W * K - 1) // (W * K)).sum())
        if body + ngroups > w.size:
            raise RuntimeError("lanes stream: the group count disagrees with the segment "
                               "lengths (count table longer than the stream)")
        self.seg_lengths, self.first, self.table = _group_table(w[5:body], W, K)
        self.counts = w[body:body + ngroups].astype(np.int64)
        # every group holds its W states and at most 11 bytes per symbol
        if (self.counts < 4 * W).any() or (self.counts > 4 * W + 11 * self.table[1]).any():
            raise RuntimeError("lanes stream: a group's byte count is impossible for its length")
        total = int(self.counts.sum())
        payload = np.frombuffer(blob, dtype=np.uint8)[4 * (body + ngroups):]
        if payload.size != total + (-total % 4):
            raise RuntimeError(f"lanes stream: the counts sum to {total} bytes, the payload "
                               f"has {payload.size} (truncated or over-long)")
        if payload[total:].any():
            raise RuntimeError("lanes stream: non-zero padding")
        self.payload = np.array(payload)
        self.nbytes = total
        self.offsets = (np.cumsum(self.counts) - self.counts).astype(np.int64)
        self.seg_base = np.concatenate([[0], np.cumsum(self.seg_lengths)]).astype(np.int64)

    def group_bytes(self, g):
        o, n = int(self.offsets[g]), int(self.counts[g])
        return self.payload[o:o + n].tobytes()


def _encode_groups(prep, lanes, steps):
    """prep: [(symbols, indexes, DeviceCdfTables, table int64 (2, ngroups)), ...] on one device
    -> per job (counts int32, bytes uint8) in table order.  One sizes and one encode launch per
    job; all jobs share two host reads (the sizes, then every finished byte)."""
    dev = prep[0][0].device
    stream = _lib.stream_ptr(dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    queued = []
    for sym, idx, tab, table in prep:
        ng = table.shape[1]
        if ng == 0:
            queued.append(None)
            continue
        tdev = _upload(np.ascontiguousarray(table), dev)
        counts = torch.empty(ng, dtype=torch.int32, device=dev)
        head = (sym.data_ptr(), idx.data_ptr(), int(sym.numel()), 0, tdev[0].data_ptr(),
                tdev[1].data_ptr(), ng, lanes, steps) + tab.args()
        _lib.call("rgbac_rans_lanes_sizes", *head, counts.data_ptr(), err.data_ptr(), stream)
        queued.append((head, counts, torch.cumsum(counts, 0, dtype=torch.int64), tdev))
    live = [q for q in queued if q is not None]
    totals = iter(torch.stack([q[2][-1] for q in live]).cpu().tolist() if live else [])
    # one buffer: per job its counts then its bytes (4-byte aligned); the error word last
    spans, pos = [], 0
    for q in queued:
        ng, total = (q[1].numel(), int(next(totals))) if q is not None else (0, 0)
        spans.append((pos, ng, total))
        pos += 4 * ng + total + (-total % 4)
    out = torch.zeros(pos + 4, dtype=torch.uint8, device=dev)
    for q, (p, ng, total) in zip(queued, spans):
        if q is None:
            continue
        head, counts, ends, _ = q
        out[p:p + 4 * ng].copy_(counts.view(torch.uint8))
        _lib.call("rgbac_rans_lanes_encode", *head, counts.data_ptr(), ends.data_ptr(),
                  out[p + 4 * ng:].data_ptr(), total, err.data_ptr(), stream)
    out[pos:].copy_(err.view(torch.uint8))
    host = out.cpu().numpy()
    _raise_code("encode_lanes", int(host[pos:].view(np.int32)[0]))
    return [(host[p:p + 4 * ng].view(np.int32), host[p + 4 * ng:p + 4 * ng + total])
            for p, ng, total in spans]


def encode_lanes_many(jobs, lanes=LANES_DEFAULT[0], steps=LANES_DEFAULT[1]):
    """jobs: [(symbols, indexes, DeviceCdfTables, seg_lengths), ...] -> [bytes, ...], one lanes
    container per job, all jobs sharing the two host reads."""
    if not jobs:
        return []
    lanes, steps = _check_lanes(lanes, steps)
    prep, segs = [], []
    dev = None
    for sym, idx, tab, seg_lengths in jobs:
        sym, idx, dev = _check_job(sym, idx, tab, dev)
        seg, _, table = _group_table(seg_lengths, lanes, steps)
        if sym.numel() != int(seg.sum()):
            raise ValueError("symbols, indexes and seg_lengths disagree on the symbol count")
        prep.append((sym, idx, tab, table))
        segs.append(seg)
    return [_lanes_blob(lanes, steps, seg, counts, payload)
            for seg, (counts, payload) in zip(segs, _encode_groups(prep, lanes, steps))]


def encode_lanes(symbols, indexes, tables, seg_lengths, lanes=LANES_DEFAULT[0],
                 steps=LANES_DEFAULT[1]):
    """Device int32 symbols / indexes (sum(seg_lengths) each, segments back to back) -> the
    lanes container's bytes: a sizes pass, a scan, an encode pass into the scanned offsets."""
    return encode_lanes_many([(symbols, indexes, tables, seg_lengths)], lanes, steps)[0]


def _lanes_decode_launch(payload, meta, counts, g0, g1, idx, nsym, base, W, K, tables, out,
                         err, device):
    """Queues the decode of groups g0..g1-1 of (payload, meta, counts) into out; no sync."""
    if not isinstance(tables, DeviceCdfTables):
        raise TypeError("decode_segments needs DeviceCdfTables")
    if idx.numel() != nsym:
        raise RuntimeError(f"lanes stream: the segments cover {nsym} symbols, "
                           f"{idx.numel()} indexes given")
    if out is None:
        out = torch.empty(nsym, dtype=torch.int32, device=device)
    elif (out.dtype != torch.int32 or out.device != idx.device or out.numel() != nsym
          or not out.is_contiguous()):
        raise ValueError("out must be a contiguous device int32 tensor of the segments' size")
    if g1 > g0:
        _lib.call("rgbac_rans_lanes_decode", payload.data_ptr(), int(payload.numel()),
                  meta[0, g0:].data_ptr(), counts[g0:].data_ptr(), idx.data_ptr(), nsym, base,
                  meta[1, g0:].data_ptr(), meta[2, g0:].data_ptr(), g1 - g0, W, K,
                  *tables.args(), out.data_ptr(), err.data_ptr(), _lib.stream_ptr(device))
    return out


class LanesDecoder:
    """Decodes one lanes container on the device; the surface of ChunkedDecoder: the header is
    parsed and validated on the host, ``decode_segments`` only queues a kernel, ``check()``
    reads the error word, which several decoders may share (``err``)."""

    def __init__(self, blob, device, err=None):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("LanesDecoder needs a GPU device (there is no CPU path; "
                               "use decode_lanes_host)")
        lay = blob if isinstance(blob, LanesLayout) else LanesLayout(blob)
        self.layout, self.device = lay, device
        self.W, self.K, self.seg_lengths = lay.W, lay.K, lay.seg_lengths.tolist()
        self._payload = _upload(lay.payload if lay.payload.size else np.zeros(4, np.uint8), device)
        self._meta = _upload(np.stack([lay.offsets, lay.table[0], lay.table[1]]), device)
        self._counts = _upload(lay.counts.astype(np.int32), device)
        self._err = err if err is not None else torch.zeros(1, dtype=torch.int32, device=device)

    def decode_segments(self, lo, hi, indexes, tables, out=None):
        """Symbols of segments lo..hi-1 (device int32, flat) from their CDF indexes; no sync."""
        lay = self.layout
        if not 0 <= lo < hi <= len(self.seg_lengths):
            raise ValueError("segment range")
        base, nsym = int(lay.seg_base[lo]), int(lay.seg_base[hi] - lay.seg_base[lo])
        return _lanes_decode_launch(self._payload, self._meta, self._counts, int(lay.first[lo]),
                                    int(lay.first[hi]), _dev_i32(indexes, "indexes"), nsym, base,
                                    self.W, self.K, tables, out, self._err, self.device)

    def check(self):
        """Reads the error word (a sync); raises RuntimeError naming the first error code."""
        _raise_code("lanes stream decode", int(self._err.item()))


def _host_groups(s, i, tab, table, lanes, steps):
    """The CPU twin of one sizes + encode pass through a group table -> (counts, bytes)."""
    table = np.ascontiguousarray(table, dtype=np.int64)
    ng = table.shape[1]
    counts = np.zeros(ng, dtype=np.int32)
    if ng == 0:
        return counts, np.zeros(0, dtype=np.uint8)
    total, err = ctypes.c_int64(0), ctypes.c_int32(0)
    head = (s.ctypes.data, i.ctypes.data, int(s.size), 0, table[0].ctypes.data,
            table[1].ctypes.data, ng, lanes, steps) + tab.args()
    _lib.call("rgbac_rans_lanes_encode_host", *head, counts.ctypes.data, None, 0,
              ctypes.byref(total), ctypes.byref(err))
    _raise_code("encode_lanes_host", err.value)
    payload = np.zeros(total.value, dtype=np.uint8)
    _lib.call("rgbac_rans_lanes_encode_host", *head, counts.ctypes.data, payload.ctypes.data,
              int(payload.size), ctypes.byref(total), ctypes.byref(err))
    _raise_code("encode_lanes_host", err.value)
    return counts, payload


def encode_lanes_host(symbols, indexes, tables, seg_lengths, lanes=LANES_DEFAULT[0],
                      steps=LANES_DEFAULT[1], cdf_lengths=None, offsets=None):
    """encode_lanes on the CPU (the same lane functions in loops over the lanes): for tests and
    for writing streams without a GPU.  The device path never calls it."""
    s, i = _i32(symbols), _i32(indexes)
    tab = CdfTables.of(tables, cdf_lengths, offsets)
    lanes, steps = _check_lanes(lanes, steps)
    seg, _, table = _group_table(seg_lengths, lanes, steps)
    if s.size != i.size or s.size != int(seg.sum()):
        raise ValueError("symbols, indexes and seg_lengths disagree on the symbol count")
    return _lanes_blob(lanes, steps, seg, *_host_groups(s, i, tab, table, lanes, steps))


def _decode_groups_host(payload, meta, counts, W, K, i, tab, nsym):
    out = np.zeros(nsym, dtype=np.int32)
    if meta.shape[1] == 0:
        return out
    err = ctypes.c_int32(0)
    meta = np.ascontiguousarray(meta, dtype=np.int64)
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    _lib.call("rgbac_rans_lanes_decode_host", payload.ctypes.data, int(payload.size),
              meta[0].ctypes.data, counts.ctypes.data, i.ctypes.data, nsym, 0,
              meta[1].ctypes.data, meta[2].ctypes.data, meta.shape[1], W, K, *tab.args(),
              out.ctypes.data, ctypes.byref(err))
    _raise_code("lanes stream decode", err.value)
    return out


def decode_lanes_host(blob, indexes, tables, cdf_lengths=None, offsets=None):
    """Decodes a whole lanes container on the CPU -> int32 array of all segments' symbols."""
    lay = blob if isinstance(blob, LanesLayout) else LanesLayout(blob)
    i = _i32(indexes)
    nsym = int(lay.seg_base[-1])
    if i.size != nsym:
        raise RuntimeError(f"lanes stream: the container holds {nsym} symbols, "
                           f"{i.size} indexes given")
    return _decode_groups_host(lay.payload, np.stack([lay.offsets, lay.table[0], lay.table[1]]),
                               lay.counts, lay.W, lay.K, i,
                               CdfTables.of(tables, cdf_lengths, offsets), nsym)


# Per-image lanes containers from one batched pass, as for the chunked format above: one group
# table ordered image-major for encoding, the files' tables merged slice-major for decoding.
def lanes_image_major_table(seg_starts, seg_lengths, lanes, steps):
    """seg_starts int64 (B, nseg) -> (table int64 (2, B * ng), image b's ng groups at
    [b * ng, (b + 1) * ng) in container order; ng)."""
    seg, first, tab = _group_table(seg_lengths, lanes, steps)
    starts = np.asarray(seg_starts, dtype=np.int64).reshape(-1, seg.size)
    base = np.concatenate([[0], np.cumsum(seg)[:-1]]).astype(np.int64)
    which = np.repeat(np.arange(seg.size), np.diff(first))
    local = tab[0] - base[which]
    ng = int(first[-1])
    table = np.empty((2, starts.shape[0] * ng), dtype=np.int64)
    table[0] = (starts[:, which] + local[None, :]).reshape(-1)
    table[1] = np.tile(tab[1], starts.shape[0])
    return table, ng


def split_lanes_containers(counts, payload, nimages, seg_lengths, lanes, steps):
    """What one image-major pass wrote (every group's byte count; the groups' bytes back to
    back) -> [bytes, ...]: one container per image."""
    seg, first, _ = _group_table(seg_lengths, lanes, steps)
    ng = int(first[-1])
    counts = np.asarray(counts).astype(np.int64)
    if counts.size != nimages * ng or int(counts.sum()) != len(payload):
        raise ValueError("split_lanes_containers: the counts do not match the payload")
    cut = np.concatenate([[0], np.cumsum(counts.reshape(nimages, ng).sum(axis=1))])
    return [_lanes_blob(lanes, steps, seg, counts[b * ng:(b + 1) * ng],
                        payload[int(cut[b]):int(cut[b + 1])]) for b in range(nimages)]


def merged_lanes_tables(layouts, seg_starts):
    """layouts: one LanesLayout per file, all with the same W, K and seg_lengths; seg_starts
    int64 (B, nseg).  -> (payload uint8: the files' group bytes back to back, padded to 4; meta
    int64 (3, groups): byte offset, first symbol, length; counts int32; first int64 (nseg + 1):
    segment s of ALL files is meta[:, first[s]:first[s + 1]], file-major inside)."""
    l0 = layouts[0]
    nseg, B = l0.seg_lengths.size, len(layouts)
    for lay in layouts:
        if (lay.W, lay.K) != (l0.W, l0.K) or lay.seg_lengths.size != nseg \
                or (lay.seg_lengths != l0.seg_lengths).any():
            raise RuntimeError("lanes stream: the files of a group disagree on their layout")
    starts = np.asarray(seg_starts, dtype=np.int64).reshape(B, nseg)
    pbase = np.concatenate([[0], np.cumsum([lay.nbytes for lay in layouts])]).astype(np.int64)
    meta, counts, first = [np.zeros((3, 0), dtype=np.int64)], [np.zeros(0, dtype=np.int64)], [0]
    for s in range(nseg):
        for b, lay in enumerate(layouts):
            g0, g1 = int(lay.first[s]), int(lay.first[s + 1])
            meta.append(np.stack([pbase[b] + lay.offsets[g0:g1],
                                  starts[b, s] + lay.table[0, g0:g1] - lay.seg_base[s],
                                  lay.table[1, g0:g1]]))
            counts.append(lay.counts[g0:g1])
        first.append(first[-1] + sum(int(lay.first[s + 1] - lay.first[s]) for lay in layouts))
    payload = np.concatenate([lay.payload[:lay.nbytes] for lay in layouts]
                             + [np.zeros(4 + (-int(pbase[-1]) % 4), dtype=np.uint8)])
    return (payload[:payload.size - payload.size % 4].copy(),
            np.ascontiguousarray(np.concatenate(meta, axis=1)),
            np.concatenate(counts).astype(np.int32), np.asarray(first, dtype=np.int64))


def encode_groups_host(symbols, indexes, tables, table, lanes, steps, cdf_lengths=None,
                       offsets=None):
    """The CPU twin of one sizes + encode pass through an arbitrary group table -> (counts int32,
    bytes uint8): what split_lanes_containers takes."""
    lanes, steps = _check_lanes(lanes, steps)
    return _host_groups(_i32(symbols), _i32(indexes), CdfTables.of(tables, cdf_lengths, offsets),
                        table, lanes, steps)


def decode_merged_lanes_host(layouts, seg_starts, indexes, tables, cdf_lengths=None,
                             offsets=None):
    """The CPU twin of MergedLanesDecoder: all segments of all files into one flat int32 array
    laid out by seg_starts (``indexes`` in the same layout)."""
    payload, meta, counts, _ = merged_lanes_tables(layouts, seg_starts)
    i = _i32(indexes)
    base, nsym = _span(seg_starts, layouts[0].seg_lengths, 0, layouts[0].seg_lengths.size)
    if base != 0 or i.size != nsym:
        raise RuntimeError(f"lanes stream: the files hold symbols {base}..{base + nsym}, "
                           f"{i.size} indexes given")
    return _decode_groups_host(payload, meta, counts, layouts[0].W, layouts[0].K, i,
                               CdfTables.of(tables, cdf_lengths, offsets), nsym)


def encode_lanes_image_major(jobs, lanes=LANES_DEFAULT[0], steps=LANES_DEFAULT[1]):
    """jobs: [(symbols, indexes, DeviceCdfTables, seg_starts (B, nseg), seg_lengths), ...] ->
    per job its B containers; one sizes and one encode launch per job for all B images."""
    lanes, steps = _check_lanes(lanes, steps)
    prep, cuts = [], []
    dev = None
    for sym, idx, tab, seg_starts, seg_lengths in jobs:
        sym, idx, dev = _check_job(sym, idx, tab, dev)
        table, _ = lanes_image_major_table(seg_starts, seg_lengths, lanes, steps)
        prep.append((sym, idx, tab, table))
        cuts.append((np.asarray(seg_starts).reshape(-1, len(seg_lengths)).shape[0], seg_lengths))
    return [split_lanes_containers(counts, payload, B, seg, lanes, steps)
            for (B, seg), (counts, payload) in zip(cuts, _encode_groups(prep, lanes, steps))]


class MergedLanesDecoder:
    """Decodes a group of lanes containers that share their layout as ONE launch per segment
    range (merged_lanes_tables); the interface latent_code expects of ``y_chunked``."""

    def __init__(self, layouts, seg_starts, device, err=None):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("MergedLanesDecoder needs a GPU device (there is no CPU path; "
                               "use decode_merged_lanes_host)")
        payload, meta, counts, first = merged_lanes_tables(layouts, seg_starts)
        self.device, self.W, self.K = device, layouts[0].W, layouts[0].K
        self.seg_lengths = layouts[0].seg_lengths
        self._starts = np.asarray(seg_starts, dtype=np.int64).reshape(len(layouts), -1)
        self._first = first
        self._payload = _upload(payload, device)
        self._meta = _upload(meta, device)
        self._counts = _upload(counts, device)
        self._err = err if err is not None else torch.zeros(1, dtype=torch.int32, device=device)

    def decode_segments(self, lo, hi, indexes, tables, out=None):
        """Segments lo..hi-1 of every file (device int32, the flat range they cover); no sync."""
        if not 0 <= lo < hi <= self.seg_lengths.size:
            raise ValueError("segment range")
        base, nsym = _span(self._starts, self.seg_lengths, lo, hi)
        return _lanes_decode_launch(self._payload, self._meta, self._counts,
                                    int(self._first[lo]), int(self._first[hi]),
                                    _dev_i32(indexes, "indexes"), nsym, base, self.W, self.K,
                                    tables, out, self._err, self.device)

    def check(self):
        _raise_code("lanes stream decode", int(self._err.item()))
