"""Self-contained RGBA files: one bitstream per image, decodable alone or in any batch.

``encode_rgba`` runs the alpha -> RGB chain of the evaluation pass (rgbac.rgba.rgba_forward,
reference trainRGB.py:282-306) on the bitstream path and returns one ``bytes`` object per image;
``decode_rgba`` takes any list of such files, in any order, and returns the images.  GPU only.

* Per-image opacity decides everything an image needs (rgbac_rgba_opaque, one read of B flags):
  an opaque image is padded by replication, never enters the alpha codec and carries no alpha
  sections (trainRGB.py:299-302); any other image is padded transparent and carries both.
* Every image is coded on ITS OWN canvas, round_up(h, 64) x round_up(w, 64) -- the decoder
  knows nothing else -- so a call groups its images by canvas and runs each group as a batch.
* One batched pass per group writes per-image containers (rgbac.ans.encode_image_major: one
  sizes and one encode launch per CDF-table set for all images); decoding merges the files'
  chunk tables and issues one rANS launch per slice wave for the whole group
  (MergedChunkedDecoder), with one error word read once at the very end.
* Both chains run under ``rt.fixed_tiles(per_image=True)``: every conv's (tile, split-K) -- and
  with it the order of every fp32 sum -- depends on one image's geometry only, so mu / sigma,
  the reconstructed alpha and the pixels do not depend on which files are decoded together.

File layout (little-endian; DESIGN.md section 21 has it byte by byte): a 44-byte header
(magic "RGAF", version, flags, h, w, chunk K, CRC32 of each codec's quantised CDF tables, four
section byte lengths) and the four sections alpha z, alpha y, RGB z, RGB y, each a chunked
container exactly as rgbac.ans.ChunkedLayout parses it (the alpha ones empty when opaque).
"""
import collections
import struct
import zlib

import numpy as np
import torch

from . import anysize
from . import runtime as rt
from .ans import ChunkedLayout, MergedChunkedDecoder, _raise_code, encode_image_major
from .layers.SupplyMask import mask_pyramid
from .rgba import recon_alpha

MAGIC = b"RGAF"
VERSION = 1
FLAG_OPAQUE, FLAG_ALPHA_BF16, FLAG_RGB_BF16 = 1, 2, 4
_HEADER = struct.Struct("<4sHHIIIII4I")
HEADER_BYTES = _HEADER.size          # 44
SECTIONS = ("alpha_z", "alpha_y", "rgb_z", "rgb_y")

# what a decoder must share with the encoder, per codec: the CRC32 of its CDF tables, its
# compute dtype, and the latent geometry that fixes every container's segment lengths
CodecInfo = collections.namedtuple("CodecInfo", "crc bf16 z_channels num_slices slice_channels")


def tables_crc(model):
    """CRC32 (zlib) over the model's quantised CDF tables as the coder reads them: int32
    little-endian cdfs, lengths, offsets of the Gaussian conditional, then of the bottleneck."""
    crc = 0
    for em in (model.gaussian_conditional, model.entropy_bottleneck):
        tab = em.tables()
        for arr in (tab.cdfs, tab.sizes, tab.offsets):
            crc = zlib.crc32(np.ascontiguousarray(arr).astype("<i4").tobytes(), crc)
    return crc & 0xFFFFFFFF


def codec_info(model):
    return CodecInfo(tables_crc(model), model.compute_dtype == torch.bfloat16,
                     model.entropy_bottleneck.channels, model.num_slices,
                     model.M // model.num_slices)


def _segments(info, hp, wp):
    """(z segment lengths, y segment lengths) of one image on an hp x wp canvas."""
    zh, zw = hp // 64, wp // 64
    return ([info.z_channels * zh * zw],
            [info.slice_channels * (8 * zh) * (8 * zw)] * info.num_slices)


def build_rgba_file(h, w, chunk, opaque, alpha, rgb, sections):
    """Header + sections -> bytes.  alpha / rgb: CodecInfo; sections: the four containers'
    bytes in SECTIONS order (the alpha ones empty when opaque)."""
    flags = ((FLAG_OPAQUE if opaque else 0) | (FLAG_ALPHA_BF16 if alpha.bf16 else 0) |
             (FLAG_RGB_BF16 if rgb.bf16 else 0))
    sections = [bytes(s) for s in sections]
    if len(sections) != 4:
        raise ValueError("an RGBA file has four sections")
    head = _HEADER.pack(MAGIC, VERSION, flags, int(h), int(w), int(chunk), alpha.crc, rgb.crc,
                        *[len(s) for s in sections])
    return head + b"".join(sections)


def parse_rgba_file(blob, alpha, rgb):
    """bytes -> {"h", "w", "canvas", "chunk", "opaque", SECTIONS...: ChunkedLayout or None}.
    Pure host code; raises RuntimeError on anything wrong: bad magic or version, a truncated
    or over-long file, section lengths that disagree with the file length, a container whose
    chunk size or segment lengths are not the ones (h, w) implies, and a CRC or dtype that
    disagrees with the codecs given (alpha / rgb: CodecInfo of the decoder's models; the alpha
    codec's are not looked at for an opaque file)."""
    blob = bytes(blob)
    if len(blob) < HEADER_BYTES:
        raise RuntimeError(f"RGBA file: truncated ({len(blob)} bytes, the header has "
                           f"{HEADER_BYTES})")
    magic, version, flags, h, w, chunk, crc_a, crc_r, *lens = _HEADER.unpack_from(blob)
    if magic != MAGIC:
        raise RuntimeError("RGBA file: bad magic (not an RGBA file)")
    if version != VERSION:
        raise RuntimeError(f"RGBA file: unsupported version {version}")
    if flags & ~(FLAG_OPAQUE | FLAG_ALPHA_BF16 | FLAG_RGB_BF16):
        raise RuntimeError(f"RGBA file: unknown flags {flags:#x}")
    if h < 1 or w < 1 or h >= 1 << 24 or w >= 1 << 24 or chunk < 1 or chunk >= 1 << 31:
        raise RuntimeError(f"RGBA file: bad size {h}x{w} or chunk size {chunk}")
    opaque = bool(flags & FLAG_OPAQUE)
    total = HEADER_BYTES + sum(lens)
    if total != len(blob):
        kind = "truncated" if len(blob) < total else "over-long"
        raise RuntimeError(f"RGBA file: {kind}: the section lengths say {total} bytes, the "
                           f"file has {len(blob)}")
    if opaque and (lens[0] or lens[1]):
        raise RuntimeError("RGBA file: an opaque file must have empty alpha sections")
    if (not opaque and not (lens[0] and lens[1])) or not (lens[2] and lens[3]):
        raise RuntimeError("RGBA file: a section the flags ask for is empty")
    checks = [("RGB", rgb, crc_r, bool(flags & FLAG_RGB_BF16))]
    if not opaque:
        checks.append(("alpha", alpha, crc_a, bool(flags & FLAG_ALPHA_BF16)))
    for name, info, crc, bf16 in checks:
        if bf16 != info.bf16:
            raise RuntimeError(f"RGBA file: coded with the {name} codec in "
                               f"{'bf16' if bf16 else 'fp32'}, the model given runs in "
                               f"{'bf16' if info.bf16 else 'fp32'} (compute dtype)")
        if crc != info.crc:
            raise RuntimeError(f"RGBA file: the {name} codec's CDF tables differ from the "
                               f"encoder's (CRC {info.crc:#010x}, the file says {crc:#010x}): "
                               "other weights")
    hp, wp = anysize.padded_size(h, w)
    out = {"h": h, "w": w, "canvas": (hp, wp), "chunk": chunk, "opaque": opaque}
    want = dict(zip(SECTIONS, _segments(alpha, hp, wp) + _segments(rgb, hp, wp)))
    pos = HEADER_BYTES
    for name, n in zip(SECTIONS, lens):
        lay = None
        if n:
            lay = ChunkedLayout(blob[pos:pos + n])
            if lay.K != chunk or lay.seg_lengths.tolist() != want[name]:
                raise RuntimeError(f"RGBA file: section {name} has chunk size {lay.K} and "
                                   f"segments {lay.seg_lengths.tolist()}; a {h}x{w} image needs "
                                   f"{chunk} and {want[name]}")
        out[name] = lay
        pos += n
    return out


# ---- the per-image container jobs of one batch's latents
def _starts(B, nseg, m):
    """Where segment s of image b begins in a (nseg, B, m) symbol tensor."""
    return (np.arange(nseg, dtype=np.int64)[None, :] * B + np.arange(B, dtype=np.int64)[:, None]) * m


def _z_indexes(C, hw, B, dev):
    one = torch.arange(C, dtype=torch.int32, device=dev).view(C, 1).expand(C, hw).reshape(-1)
    return one.repeat(B)


def _latent_jobs(model, z_sym, y_sym, y_idx):
    """encode_image_major jobs (z, then y) for latent_code's symbols of a batch."""
    dev = z_sym.device
    B, C, zh, zw = z_sym.shape
    ns, n = y_sym.shape
    mz, m = C * zh * zw, n // B
    return [(z_sym, _z_indexes(C, zh * zw, B, dev), model.entropy_bottleneck.device_tables(dev),
             _starts(B, 1, mz), [mz]),
            (y_sym, y_idx, model.gaussian_conditional.device_tables(dev), _starts(B, ns, m),
             [m] * ns)]


def _decode_latents(model, z_lays, y_lays, hp, wp, dev, err):
    """The files' z / y containers of one group -> latent_code's (YH, z_sym, y_sym, y_idx): one
    rANS launch for all z, one per slice wave for all y, nothing read back."""
    from .models._codec import latent_code
    info = codec_info(model)
    B, zh, zw = len(z_lays), hp // 64, wp // 64
    zseg, yseg = _segments(info, hp, wp)
    z_dec = MergedChunkedDecoder(z_lays, _starts(B, 1, zseg[0]), dev, err=err)
    y_dec = MergedChunkedDecoder(y_lays, _starts(B, len(yseg), yseg[0]), dev, err=err)
    z_sym = torch.empty((B, info.z_channels, zh, zw), dtype=torch.int32, device=dev)
    z_dec.decode_segments(0, 1, _z_indexes(info.z_channels, zh * zw, B, dev),
                          model.entropy_bottleneck.device_tables(dev), out=z_sym)
    return latent_code(model, z_sym=z_sym, y_chunked=y_dec)


def _per_image(YH, z_sym, y_sym, y_idx, b):
    """Image b's share of latent_code's result (debug=): z / y symbols, y's CDF indexes, y_hat."""
    ns, B = y_sym.shape[0], z_sym.shape[0]
    return {"z": z_sym[b].clone(), "y": y_sym.view(ns, B, -1)[:, b].clone(),
            "idx": y_idx.view(ns, B, -1)[:, b].clone(), "YH": YH.t[b].clone()}


def _models(masknet, net):
    from .models._codec import _check
    dev = next(net.parameters()).device
    if dev.type != "cuda" or next(masknet.parameters()).device != dev:
        raise RuntimeError("rgbac: this module runs on the GPU (HIP) only, both models on one "
                           f"device (got {next(masknet.parameters()).device} and {dev}).")
    _check(masknet)
    _check(net)
    return dev


@torch.no_grad()
def encode_rgba(masknet, net, images, chunk=256, debug=None):
    """images: what anysize.pack_rgba takes (a list of (h, w, 4) uint8 arrays / tensors, any
    sizes) -> list[bytes], one complete file per image.  ``chunk``: symbols per rANS chunk (see
    AutoEncoder.compress).  ``debug``: a list that receives, per image, the encoder's symbols
    and y_hat ({"alpha": {...} or None, "rgb": {"z", "y", "YH"}})."""
    dev = _models(masknet, net)
    chunk = int(chunk)
    if chunk <= 0 or chunk >= 1 << 31:
        raise ValueError("chunk size must be a positive 32-bit number")
    dev, sizes, entries, keep = anysize._sources(images, dev, "encode_rgba")
    flags_dev = anysize._opaque(dev, entries)
    flags = flags_dev.cpu().tolist()        # the one read: which sections, which images to masknet
    info_a, info_r = codec_info(masknet), codec_info(net)
    groups = collections.OrderedDict()
    for k, (h, w) in enumerate(sizes):
        groups.setdefault(anysize.padded_size(h, w), []).append(k)
    files = [None] * len(sizes)
    if debug is not None:
        debug[:] = [None] * len(sizes)
    for members in groups.values():
        coded = _encode_group(masknet, net, dev, [sizes[k] for k in members],
                              [entries[k] for k in members], [flags[k] for k in members],
                              flags_dev[torch.tensor(members, device=dev)].contiguous(), chunk,
                              debug is not None)
        for k, (secs, dbg) in zip(members, coded):
            files[k] = build_rgba_file(*sizes[k], chunk, bool(flags[k]), info_a, info_r, secs)
            if debug is not None:
                debug[k] = dbg
    return files


def _encode_group(masknet, net, dev, sizes, entries, opaque, opaque_dev, chunk, want_debug):
    """One batched coding pass over images that share a canvas (encode_rgba's group body; the
    tiled encoder runs its tiles through it too).  sizes / entries: as anysize._sources returns
    them; opaque: per image, truthy where every alpha byte is 255 (host list), opaque_dev the
    same as a device int32 tensor (the pack's per-image pad modes).  -> per image
    (its four sections in SECTIONS order, the alpha ones b"" when opaque; its debug record or
    None)."""
    from .models._codec import latent_code
    from .models.AutoEncoderMask_Journal import _run_seq
    p = anysize._pack(dev, sizes, entries, None, opaque_dev)
    nonop = [j for j, f in enumerate(opaque) if not f]
    jobs = []
    with rt.fixed_tiles(per_image=True):
        if nonop:
            am = p["alpha"][torch.tensor(nonop, device=dev)]
            ya = _run_seq(masknet.EncoderMask, rt.to_nhwc(am, masknet.compute_dtype))
            lat_a = latent_code(masknet, y=ya)
            jobs += _latent_jobs(masknet, *lat_a[1:])
        _, me = mask_pyramid(p["alpha"], 4)          # the TRUE alpha, as compress takes it
        y = net.Encoder.nhwc(rt.to_nhwc(p["masked"], net.compute_dtype), me[1], me[2])
        lat_r = latent_code(net, y=y)
        jobs += _latent_jobs(net, *lat_r[1:])
    blobs = encode_image_major(jobs, chunk)
    out = []
    for j in range(len(sizes)):
        a = nonop.index(j) if j in nonop else None
        secs = ([b"", b""] if a is None else [blobs[0][a], blobs[1][a]]) + \
            [blobs[-2][j], blobs[-1][j]]
        dbg = None
        if want_debug:
            dbg = {"alpha": None if a is None else _per_image(*lat_a, a),
                   "rgb": _per_image(*lat_r, j)}
        out.append((secs, dbg))
    return out


@torch.no_grad()
def decode_rgba(masknet, net, blobs, debug=None):
    """blobs: files from encode_rgba, any number, any order -> list of (h, w, 4) uint8 GPU
    tensors in the same order.  Every header is parsed and validated on the host before any
    launch (RuntimeError); files that share a canvas and a chunk size decode as one batch; the
    one error word of all rANS launches is read once, after the last synthesis is queued.
    ``debug``: a list that receives, per file, the decoded symbols, y_hat and the reconstructed
    alpha plane ({"alpha": {...} or None, "rgb": {...}, "alpha_plane": (hp, wp) fp32})."""
    dev = _models(masknet, net)
    blobs = list(blobs)
    if not blobs:
        raise ValueError("decode_rgba: no files")
    info_a, info_r = codec_info(masknet), codec_info(net)
    parsed = [parse_rgba_file(b, info_a, info_r) for b in blobs]
    groups = collections.OrderedDict()
    for k, f in enumerate(parsed):
        groups.setdefault(f["canvas"] + (f["chunk"],), []).append(k)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    outs = [None] * len(blobs)
    if debug is not None:
        debug[:] = [None] * len(blobs)
    for (hp, wp, _), members in groups.items():
        fs = [parsed[k] for k in members]
        x_hat, alpha, dbgs = _decode_group(masknet, net, fs, hp, wp, dev, err, debug is not None)
        rgba = anysize.unpack_rgba(x_hat, alpha, [(f["h"], f["w"]) for f in fs])
        for j, k in enumerate(members):
            outs[k] = rgba[j]
            if debug is not None:
                debug[k] = dbgs[j]
    _raise_code("RGBA file decode", int(err.item()))
    return outs


def _decode_group(masknet, net, fs, hp, wp, dev, err, want_debug):
    """One batched decoding pass over parsed files that share the canvas hp x wp and a chunk size
    (decode_rgba's group body; the tiled decoder runs its tiles through it too).  fs: dicts with
    "opaque" and the four SECTIONS layouts.  -> (x_hat (B,3,hp,wp) fp32 clamped to [0, 1], the
    reconstructed alpha (B,1,hp,wp) fp32, ones for an opaque member, the per-member debug
    records or None).  Nothing is read back; rANS errors land in ``err``."""
    from .models._codec import mask_synthesis
    nonop = [j for j, f in enumerate(fs) if not f["opaque"]]
    with rt.fixed_tiles(per_image=True):
        alpha = torch.ones((len(fs), 1, hp, wp), device=dev)
        if nonop:
            lat_a = _decode_latents(masknet, [fs[j]["alpha_z"] for j in nonop],
                                    [fs[j]["alpha_y"] for j in nonop], hp, wp, dev, err)
            xa = mask_synthesis(masknet, lat_a[0])
            ra = recon_alpha(xa)
            alpha.index_copy_(0, torch.tensor(nonop, device=dev), ra)
        lat_r = _decode_latents(net, [f["rgb_z"] for f in fs], [f["rgb_y"] for f in fs],
                                hp, wp, dev, err)
        _, md = mask_pyramid(alpha, 4)
        x_hat = rt.to_nchw(net.Decoder.nhwc(lat_r[0], md[1], md[2])).clamp_(0, 1)
    dbgs = None
    if want_debug:
        dbgs = []
        for j in range(len(fs)):
            a = nonop.index(j) if j in nonop else None
            dbgs.append({"alpha": None if a is None else _per_image(*lat_a, a),
                         "rgb": _per_image(*lat_r, j), "alpha_plane": alpha[j, 0].clone(),
                         "alpha_x_hat": None if a is None else xa[a, 0].clone()})
    return x_hat, alpha, dbgs
