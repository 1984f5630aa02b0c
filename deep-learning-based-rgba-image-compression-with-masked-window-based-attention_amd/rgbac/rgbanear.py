"""Near-lossless RGBA files (``RGAN``): exact alpha beside colour with a bounded error, both coded
on the device.

``encode_rgba_near`` takes a ragged batch of packed uint8 RGBA images and a bound ``max_error``
(delta, 1..16) and returns one self-contained file per image; ``decode_rgba_near`` takes any list
of files in any order.  The alpha comes back bit for bit, every colour byte of a visible pixel
within +-delta, and a pixel nobody can see (alpha 0) with R = G = B = 0 unless the file was
written with ``keep_hidden``.  No model is involved.  GPU only: a CPU device or a missing library
raises.

The alpha plane is an ``RGAP`` blob of rgbac.alphaexact, unchanged.  The colour is coded by
csrc/color_near.hip: planes G, R, B; MED prediction inside 16 x 16 blocks over the RECONSTRUCTED
visible neighbours, chroma relative to the reconstructed green; the prediction error quantised
with step 2 delta + 1; 15 static tables per image (channel * 5 + context); one rANS chunk per
block and channel that is not constant within 2 delta.  Model, format and launches: DESIGN.md
section 28.

``bound="composite"`` (csrc/color_blend.hip) bounds what people see, not the
stored byte: the composite of every pixel over ANY background comes back within +-delta.  A pixel
of alpha a may then be off by e(a) = min(255, 255 delta // a), which is delta where a = 255 and
grows as the pixel fades: soft edges, shadows and glass cost fewer bytes.  Such a file has version
2 and flags bit 1; ``keep_hidden`` has no meaning under it.

File, little-endian:
    "RGAN", u16 version (1; 2 under the composite bound), u16 flags (bit 0: keep_hidden, bit 1:
    composite bound, version 2 only and never with bit 0), u8 delta, 3 zero bytes, u32 h, u32 w,
    u32 alpha bytes, u32 colour bytes; the RGAP blob; the colour section in the layout of an RGAL
    file's (rgbac.rgbalossless): u32 chunks, u32 payload words, 15 tables, one u32 class word per
    block (bit 0 hidden, bits 1-3 channel G / R / B constant, bits 8-15 / 16-23 / 24-31 the
    constants), one u16 word count per chunk (block-major, G, R, B), the payload.
"""
import struct

import numpy as np
import torch

from . import _lib, alphaexact, anysize
from . import rgbalossless as rl
from .alphaexact import BLOCK, MAX_SIDE, normalise_counts
from .ans import _raise_code, _upload

MAGIC = b"RGAN"
VERSION = 1
VERSION_COMPOSITE = 2                 # the bound is on the composite: flags bit 1, never bit 0
FLAG_COMPOSITE = 2
BOUNDS = ("pixel", "composite")
MAX_ERROR = _lib.NEAR_MAX_ERROR
NCH, NCTX, NTAB = rl.NCH, rl.NCTX, rl.NTAB
_HEADER = struct.Struct("<4sHHB3sIIII")
HEADER_BYTES = _HEADER.size           # 28
_HIDDEN = 1                           # the class word of a block without a visible pixel


def _delta(max_error, who):
    if isinstance(max_error, bool) or not isinstance(max_error, (int, np.integer)) \
            or not 1 <= max_error <= MAX_ERROR:
        hint = " (for 0 use encode_rgba_lossless)" if max_error == 0 else ""
        raise ValueError(f"{who}: max_error must be an int in 1..{MAX_ERROR}, got "
                         f"{max_error!r}{hint}")
    return int(max_error)


def _composite(bound, keep_hidden, who):
    """Is ``bound`` the composite bound?"""
    if bound not in BOUNDS:
        raise ValueError(f"{who}: bound must be one of {BOUNDS}, got {bound!r}")
    if bound == "composite" and keep_hidden:
        raise ValueError(f"{who}: keep_hidden has no meaning under bound='composite' (a hidden "
                         "pixel adds nothing to any composite)")
    return bound == "composite"


def max_quantised(delta):
    """The largest |q| a file of this delta can hold (a tolerance e >= delta only lowers it)."""
    return (255 + delta) // (2 * delta + 1)


def tolerance(alpha, delta, composite):
    """Per-pixel tolerance e of the colour bytes: delta, or under the composite bound
    min(255, 255 delta // a) (255 where a = 0: such a pixel is hidden and never coded)."""
    a = np.asarray(alpha).astype(np.int64)
    if not composite:
        return np.full(a.shape, delta, dtype=np.int64)
    return np.where(a > 0, np.minimum(255, 255 * delta // np.maximum(a, 1)), 255)


def build_rgba_near(h, w, delta, keep_hidden, alpha, colour, composite=False):
    flags = (rl.FLAG_KEEP_HIDDEN if keep_hidden else 0) | (FLAG_COMPOSITE if composite else 0)
    return _HEADER.pack(MAGIC, VERSION_COMPOSITE if composite else VERSION, flags, delta,
                        b"\0\0\0", h, w, len(alpha), len(colour)) + alpha + colour


def parse_rgba_near(blob):
    """bytes -> parse_rgba_lossless's dictionary plus "delta" and "bound" ("pixel" or
    "composite").  Pure host code; raises RuntimeError on anything wrong.  After its own header
    (magic, version 1 or 2, delta in 1..16, zero reserved bytes; flags bit 1, the composite bound,
    set in a version 2 file, where bit 0 must be clear, and in no other) an RGAN file is laid out
    as an RGAL file, so the rest is parse_rgba_lossless's work and every one of its rejections
    holds here.  On top of them: no table may give a
    frequency to a symbol whose |q| exceeds (255 + delta) div (2 delta + 1) -- except the
    companion symbol of frequency 1 that the table rule adds to a one-symbol context, which no
    stream ever codes."""
    blob = bytes(blob)

    def bad(msg):
        return RuntimeError(f"RGAN file: {msg}")

    if len(blob) < HEADER_BYTES:
        raise bad(f"truncated ({len(blob)} bytes, the header has {HEADER_BYTES})")
    magic, version, flags, delta, reserved, h, w, alpha_len, colour_len = _HEADER.unpack_from(blob)
    if magic != MAGIC:
        raise bad("bad magic (not an RGAN file)")
    if version not in (VERSION, VERSION_COMPOSITE):
        raise bad(f"unsupported version {version}")
    composite = version == VERSION_COMPOSITE
    if bool(flags & FLAG_COMPOSITE) != composite:
        raise bad(f"flags {flags:#x} do not fit version {version} (bit 1, the composite bound, "
                  "belongs to version 2 alone)")
    if composite and flags & rl.FLAG_KEEP_HIDDEN:
        raise bad("keep_hidden under the composite bound")
    flags &= ~FLAG_COMPOSITE
    if not 1 <= delta <= MAX_ERROR:
        raise bad(f"max_error {delta} is outside 1..{MAX_ERROR}")
    if reserved != b"\0\0\0":
        raise bad("reserved header bytes are not zero")
    try:
        f = rl.parse_rgba_lossless(rl._HEADER.pack(rl.MAGIC, rl.VERSION, flags, h, w, alpha_len,
                                                   colour_len) + blob[HEADER_BYTES:])
    except RuntimeError as e:
        raise RuntimeError(str(e).replace("RGAL file", "RGAN file", 1)) from None
    del f["transform"]                                      # an RGAN file has no such choice
    q = np.arange(256)
    outside = np.minimum(q, 256 - q) > max_quantised(delta)
    for c in range(NTAB):
        nz = np.flatnonzero(f["freqs"][c])
        if nz.size == 2 and f["freqs"][c].max() == alphaexact.TOTAL - 1:
            nz = nz[f["freqs"][c][nz] > 1]                  # the one symbol that occurs
        if outside[nz].any():
            raise bad(f"table {c} has a symbol outside the range of max_error {delta}")
    f["delta"] = delta
    f["bound"] = BOUNDS[composite]
    return f


# ---- the CPU twin: the closed loop in numpy, all blocks of the image at once, one block
# position after the other; the chunks by the host chunk coder (rgbac.ans)
def _model(eL, eU, eD, L, U, D):
    """section 26's prediction and context over arrays of neighbour plane values."""
    D = np.where(eD, D, L)
    lo, hi = np.minimum(L, U), np.maximum(L, U)
    med = np.where(D >= hi, lo, np.where(D <= lo, hi, L + U - D))
    d = np.maximum(hi, D) - np.minimum(lo, D)
    bins = (d > 0).astype(np.int64) + (d > 8) + (d > 64)
    both, some = eL & eU, eL | eU | eD
    one = np.where(eL, L, np.where(eU, U, D))
    return np.where(both, med, np.where(some, one, 0)), np.where(both, bins, np.where(some, 0, 4))


def settle_host(image, delta, keep_hidden=False, bound="pixel"):
    """(h, w, 4) uint8 -> (recon (h, w, 4) uint8, class words (blocks,) uint32, symbols
    (blocks, 3, 16, 16), contexts likewise, visible (blocks, 16, 16)): the model of DESIGN.md
    section 28, and of section 29 for ``bound="composite"`` (with every tolerance equal to delta
    the two are one).  Symbols of hidden pixels and of constant channels mean nothing."""
    composite = _composite(bound, keep_hidden, "settle_host")
    a = np.asarray(image).astype(np.int64)
    h, w = a.shape[:2]
    by, bx = -(-h // BLOCK), -(-w // BLOCK)
    pad = np.zeros((by * BLOCK, bx * BLOCK, 4), dtype=np.int64)
    pad[:h, :w] = a
    inside = np.zeros(pad.shape[:2], dtype=bool)
    inside[:h, :w] = True

    def blocks(x):                                        # (H, W, ...) -> (blocks, 16, 16, ...)
        x = x.reshape((by, BLOCK, bx, BLOCK) + x.shape[2:])
        return np.moveaxis(x, 2, 1).reshape((by * bx, BLOCK, BLOCK) + x.shape[4:])

    V = blocks(inside & (True if keep_hidden else pad[..., 3] != 0))
    S = blocks(pad[..., [1, 0, 2]])                       # G, R, B
    E = blocks(tolerance(pad[..., 3], delta, composite))  # per pixel; the step is 2 E + 1
    lo = np.where(V[..., None], S - E[..., None], -512).max(axis=(1, 2))
    hi = np.where(V[..., None], S + E[..., None], 512).min(axis=(1, 2))
    seen = V.any(axis=(1, 2))
    const = seen[:, None] & (lo <= hi)                    # at E = delta: max - min <= 2 delta
    value = np.clip((lo + hi) >> 1, 0, 255)               # at E = delta: (min + max) >> 1
    cls = np.where(seen, (const * (2 << np.arange(NCH))).sum(axis=1)
                   + (const * value << (8 + 8 * np.arange(NCH))).sum(axis=1), _HIDDEN)
    rec = np.zeros_like(S)
    sym = np.zeros((S.shape[0], NCH, BLOCK, BLOCK), dtype=np.int64)
    ctx = np.zeros_like(sym)
    no = np.zeros(S.shape[0], dtype=bool)
    for r in range(BLOCK):
        for c in range(BLOCK):
            eL = V[:, r, c - 1] if c else no
            eU = V[:, r - 1, c] if r else no
            eD = V[:, r - 1, c - 1] if r and c else no
            for ch in range(NCH):
                def plane(rr, cc):
                    return rec[:, rr, cc, ch] - (rec[:, rr, cc, 0] if ch else 0)
                p, k = _model(eL, eU, eD, plane(r, c - 1), plane(r - 1, c), plane(r - 1, c - 1))
                P = np.clip(rec[:, r, c, 0] + p, 0, 255) if ch else p
                e, step = S[:, r, c, ch] - P, 2 * E[:, r, c] + 1
                q = np.sign(e) * ((np.abs(e) + E[:, r, c]) // step)
                rec[:, r, c, ch] = np.where(const[:, ch], value[:, ch],
                                            np.clip(P + q * step, 0, 255))
                sym[:, ch, r, c], ctx[:, ch, r, c] = q & 255, k
    rec *= V[..., None]
    out = np.moveaxis(rec[..., [1, 0, 2]].reshape(by, bx, BLOCK, BLOCK, 3), 1, 2)
    recon = np.asarray(image).copy()
    recon[..., :3] = out.reshape(by * BLOCK, bx * BLOCK, 3)[:h, :w]
    return recon, cls.astype(np.uint32), sym, ctx, V


def encode_rgba_near_host(image, max_error, keep_hidden=False, bound="pixel"):
    """encode_rgba_near for one image on the CPU -> (bytes, the decoded image as (h, w, 4) uint8):
    the kernels' byte-level reference (not a fallback; the device path never calls it)."""
    from .ans import encode_table_host
    delta = _delta(max_error, "encode_rgba_near_host")
    composite = _composite(bound, keep_hidden, "encode_rgba_near_host")
    a = np.ascontiguousarray(np.asarray(image, dtype=np.uint8))
    if a.ndim != 3 or a.shape[2] != 4 or a.size == 0 or max(a.shape[:2]) > MAX_SIDE:
        raise ValueError(f"encode_rgba_near_host: expected (H, W, 4) uint8 RGBA, got {a.shape}")
    h, w = a.shape[:2]
    recon, cls, sym, ctx, V = settle_host(a, delta, keep_hidden, bound)
    has = rl._chunk_mask(cls)
    s = [sym[k, ch][V[k]] for k, ch in zip(*np.nonzero(has))]           # raster order
    t = [ctx[k, ch][V[k]] + NCTX * ch for k, ch in zip(*np.nonzero(has))]
    freqs = np.zeros((NTAB, 256), dtype=np.int64)
    counts, payload = np.zeros(0, np.int32), np.zeros(0, np.uint32)
    if s:
        lens = np.asarray([x.size for x in s], dtype=np.int64)
        s, t = np.concatenate(s), np.concatenate(t)
        for k in range(NTAB):
            freqs[k] = normalise_counts(np.bincount(s[t == k], minlength=256))
        table = np.stack([np.cumsum(lens) - lens, lens])
        words = encode_table_host(s.astype(np.int32), t.astype(np.int32), rl.host_tables(freqs),
                                  table, BLOCK * BLOCK)
        counts, payload = words[:lens.size], words[lens.size:].view(np.uint32)
    blob = build_rgba_near(h, w, delta, keep_hidden,
                           alphaexact.encode_alpha_plane_host(a[..., 3]),
                           rl.build_colour(freqs, cls, counts, payload), composite)
    return blob, recon


# ---- launches
def _modes(deltas, keeps, composites, dev):
    """The kernels' per-image mode words: delta, bit 8 keep_hidden, bit 9 the composite bound
    (csrc/color_blend.hip alone knows that bit)."""
    return _upload(np.asarray([d | (_lib.NEAR_KEEP_HIDDEN if k else 0)
                               | (_lib.BLEND_COMPOSITE if c else 0)
                               for d, k, c in zip(deltas, keeps, composites)], dtype=np.int32), dev)


def _args(wk, descs, modes, grouped):
    """The leading arguments of the rgbac_color_near_* and rgbac_color_blend_* calls from
    alphaexact's geometry."""
    mid = (wk.ngroups, wk._groups.data_ptr()) if grouped else ()
    return (wk.B, descs.data_ptr(), modes.data_ptr()) + mid + (wk._base.data_ptr(), wk.N)


def _encode_colour(dev, sizes, entries, delta, keep_hidden, composite):
    """The six launches over a ragged batch (settle, histogram, normalise, sizes, encode) and
    the two host reads -> (one colour section per image, the settled images).  ``composite``
    takes them through csrc/color_blend.hip, otherwise they are csrc/color_near.hip's."""
    fn = "rgbac_color_blend_" if composite else "rgbac_color_near_"
    wk = alphaexact._Work(sizes, entries, 4, dev)
    B, N, nf = wk.B, wk.N, NTAB * 256
    cut_px = np.concatenate([[0], np.cumsum([h * w for h, w in sizes])])
    flat = torch.empty((int(cut_px[-1]), 4), dtype=torch.uint8, device=dev)
    recon = [flat[int(cut_px[i]):int(cut_px[i + 1])].view(h, w, 4)
             for i, (h, w) in enumerate(sizes)]
    settled = anysize._upload_descs([(t.data_ptr(), h, w, 4 * w)
                                     for t, (h, w) in zip(recon, sizes)], dev)
    modes = _modes([delta] * B, [keep_hidden] * B, [composite] * B, dev)
    meta = torch.empty((1 + NCH) * N + B * nf, dtype=torch.int32, device=dev)
    cls, counts, freqs = meta[:N], meta[N:(1 + NCH) * N], meta[(1 + NCH) * N:]
    partials = torch.empty(B * _lib.COLOR_HIST_BLOCKS * nf, dtype=torch.int32, device=dev)
    tables = torch.empty(B * _lib.COLOR_TABLE_U16, dtype=torch.int16, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    plain, grouped = _args(wk, settled, modes, False), _args(wk, settled, modes, True)
    _lib.call(fn + "settle", B, wk._descs.data_ptr(), *grouped[1:], cls.data_ptr(),
              err.data_ptr(), wk.stream)
    _lib.call(fn + "tables", *plain, cls.data_ptr(), partials.data_ptr(),
              freqs.data_ptr(), tables.data_ptr(), wk.stream)
    _lib.call(fn + "sizes", *grouped, cls.data_ptr(), tables.data_ptr(),
              counts.data_ptr(), err.data_ptr(), wk.stream)
    ends = torch.cumsum(counts, 0, dtype=torch.int64)
    host = meta.cpu().numpy()                                       # the sizes: one read
    h_cls = host[:N].view(np.uint32)
    h_counts = host[N:(1 + NCH) * N].reshape(N, NCH)
    h_freqs = host[(1 + NCH) * N:].reshape(B, NTAB, 256)
    cut = np.concatenate([[0], np.cumsum(h_counts.sum(axis=1, dtype=np.int64))])
    total = int(cut[-1])
    words = torch.empty(total + 1, dtype=torch.int32, device=dev)
    if total:
        _lib.call(fn + "encode", *grouped, cls.data_ptr(), tables.data_ptr(),
                  counts.data_ptr(), ends.data_ptr(), words.data_ptr(), total, err.data_ptr(),
                  wk.stream)
    words[total:].copy_(err)
    words = words.cpu().numpy()                                     # the words: one copy
    _raise_code("encode_rgba_near", int(words[total]))
    out = []
    for b in range(B):
        lo, hi = int(wk.base[b]), int(wk.base[b + 1])
        c = h_cls[lo:hi]
        out.append(rl.build_colour(h_freqs[b], c, h_counts[lo:hi][rl._chunk_mask(c)],
                                   words[int(cut[lo]):int(cut[hi])].view(np.uint32)))
    return out, recon


def encode_rgba_near(images, max_error, keep_hidden=False, return_recon=False, device="cuda",
                     bound="pixel"):
    """images: a list of (h, w, 4) uint8 RGBA images of any sizes; GPU tensors are read in place,
    views into larger buffers included -> list[bytes], one RGAN file per image; with
    ``return_recon`` also the list of decoded images, (h, w, 4) uint8 GPU tensors (the encoder
    builds them before it can form a symbol).  ``max_error``: an int delta in 1..16, the bound on
    every colour byte of a visible pixel.  A hidden pixel (alpha 0) decodes to R = G = B = 0 and
    its colour does not reach the file; ``keep_hidden`` codes every pixel's colour.
    ``bound="composite"`` bounds the composite (a C + (255 - a) B) / 255 over any background B by
    ``max_error`` instead of the colour byte: a pixel of alpha a may be off by
    min(255, 255 max_error // a).  It writes version 2 files and excludes ``keep_hidden``.  A
    file does not depend on the images coded with it."""
    delta = _delta(max_error, "encode_rgba_near")
    composite = _composite(bound, keep_hidden, "encode_rgba_near")
    dev = anysize._gpu_device(device)
    _lib.load()
    dev, sizes, entries, keep = anysize._sources(images, dev, "encode_rgba_near")
    if max(max(s) for s in sizes) > MAX_SIDE:
        raise ValueError(f"encode_rgba_near: an image side is at most {MAX_SIDE}")
    keep_hidden = bool(keep_hidden)
    alpha = alphaexact._encode(dev, sizes, rl._alpha_entries(entries), 4)
    colour, recon = _encode_colour(dev, sizes, entries, delta, keep_hidden, composite)
    blobs = [build_rgba_near(h, w, delta, keep_hidden, a, c, composite)
             for (h, w), a, c in zip(sizes, alpha, colour)]
    return (blobs, recon) if return_recon else blobs


def decode_rgba_near(blobs, device="cuda"):
    """blobs: files from encode_rgba_near, any number, any order, any mix of max_error,
    keep_hidden and bound -> list of (h, w, 4) uint8 GPU tensors in the same order.  A list with
    a composite-bound file in it goes through csrc/color_blend.hip as a whole (its other files
    get a flat tolerance table there), any other list through csrc/color_near.hip.  Every file is parsed
    and validated on the host before any launch (RuntimeError); one plane-decoder launch puts all
    alpha planes into the outputs' alpha bytes, one colour launch fills in R, G, B on the same
    stream; the one error word is read once at the end."""
    blobs = list(blobs)
    if not blobs:
        raise ValueError("decode_rgba_near: no files")
    parsed = [parse_rgba_near(b) for b in blobs]
    dev = anysize._gpu_device(device)
    _lib.load()
    outs = [torch.empty((f["h"], f["w"], 4), dtype=torch.uint8, device=dev) for f in parsed]
    dev = outs[0].device
    entries = [(t.data_ptr(), f["h"], f["w"], t.stride(0)) for t, f in zip(outs, parsed)]
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    alphaexact._decode([f["alpha"] for f in parsed], rl._alpha_entries(entries), 4, dev, err)
    wk = alphaexact._Work([(f["h"], f["w"]) for f in parsed], entries, 4, dev)
    composite = [f["bound"] == "composite" for f in parsed]
    modes = _modes([f["delta"] for f in parsed], [f["keep_hidden"] for f in parsed], composite,
                   dev)
    counts = np.concatenate([f["counts"].reshape(-1) for f in parsed])
    pbase = np.concatenate([[0], np.cumsum([f["payload"].size for f in parsed])])
    off = np.concatenate([pbase[i] + np.cumsum(f["counts"].reshape(-1), dtype=np.int64)
                          - f["counts"].reshape(-1) for i, f in enumerate(parsed)])
    payload = np.concatenate([f["payload"] for f in parsed] + [np.zeros(1, dtype=np.uint32)])
    cls = np.concatenate([f["cls"] for f in parsed])
    ints = _upload(np.concatenate([cls.view(np.int32), counts, payload.view(np.int32)])
                   .astype(np.int32), dev)
    off = _upload(off.astype(np.int64), dev)
    tables = _upload(np.concatenate([rl.device_table(f["freqs"]) for f in parsed])
                     .view(np.int16), dev)
    N = wk.N
    _lib.call("rgbac_color_blend_decode" if any(composite) else "rgbac_color_near_decode",
              *_args(wk, wk._descs, modes, True), ints[:N].data_ptr(), tables.data_ptr(), off.data_ptr(), ints[N:(1 + NCH) * N].data_ptr(),
              ints[(1 + NCH) * N:].data_ptr(), int(pbase[-1]), err.data_ptr(), wk.stream)
    _raise_code("RGAN file decode", int(err.item()))
    return outs
