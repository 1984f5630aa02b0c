"""RGBA files with lossless alpha: the RGB codec beside the exact alpha-plane coder.

``encode_rgba_exact`` writes one self-contained ``RGAX`` file per image: the image's alpha plane
as an ``RGAP`` blob (rgbac.alphaexact: bit exact, no second network) and the RGB codec's z and y
sections exactly as an ``RGAF`` file stores them (rgbac.rgbafile).  ``decode_rgba_exact`` takes
any list of such files in any order.  The alpha codec (masknet) is never called.  GPU only.

* The RGB codec runs as rgbafile._encode_group / _decode_group run it: under
  ``rt.fixed_tiles(per_image=True)``, every image on its own 64-aligned canvas, an opaque image
  padded by replication and any other padded transparent.
* The encoder's mask pyramid comes from the true alpha, as there.  The decoder has the true
  alpha too, and derives its pyramid from ``recon_alpha`` of it -- the post-processing the
  ``RGAF`` decoder applies to masknet's output -- so the RGB decode is the ``RGAF`` decode with
  an alpha codec that lost nothing, and both sides agree on the mask by construction.
* An opaque image carries no alpha blob; a fully transparent image is a header only and decodes
  to zeros.

File, little-endian: a 36-byte header ("RGAX", u16 version (1), u16 flags, u32 h, w, chunk K,
CRC32 of the RGB codec's CDF tables, three section byte lengths), then the sections alpha
(an RGAP blob), RGB z, RGB y (chunked containers).  DESIGN.md section 24.
"""
import collections
import struct

import torch

from . import alphaexact, anysize
from . import runtime as rt
from .ans import ChunkedLayout, _raise_code, encode_image_major
from .layers.SupplyMask import mask_pyramid
from .rgba import recon_alpha
from .rgbafile import _decode_latents, _latent_jobs, _segments, codec_info

MAGIC = b"RGAX"
VERSION = 1
FLAG_OPAQUE, FLAG_RGB_BF16, FLAG_TRANSPARENT = 1, 4, 8
_HEADER = struct.Struct("<4sHHIIII3I")
HEADER_BYTES = _HEADER.size          # 36
SECTIONS = ("alpha", "rgb_z", "rgb_y")


def build_rgba_exact(h, w, chunk, kind, rgb, sections):
    """kind: "opaque", "transparent" or "mixed"; rgb: CodecInfo; sections: the three sections'
    bytes in SECTIONS order (alpha empty unless mixed, all empty when transparent)."""
    flags = ({"opaque": FLAG_OPAQUE, "transparent": FLAG_TRANSPARENT, "mixed": 0}[kind]
             | (FLAG_RGB_BF16 if rgb.bf16 else 0))
    sections = [bytes(s) for s in sections]
    if len(sections) != 3:
        raise ValueError("an RGAX file has three sections")
    return _HEADER.pack(MAGIC, VERSION, flags, int(h), int(w), int(chunk), rgb.crc,
                        *[len(s) for s in sections]) + b"".join(sections)


def parse_rgba_exact(blob, rgb):
    """bytes -> {"h", "w", "canvas", "chunk", "opaque", "transparent", "alpha": the parsed RGAP
    blob or None, "rgb_z" / "rgb_y": ChunkedLayout or None}.  Pure host code; raises RuntimeError
    on anything wrong: bad magic, version or flags, a truncated or over-long file, sections the
    flags do not allow or that are missing, an alpha blob that parse_alpha_planes rejects or
    whose size is not the file's, and for the RGB sections everything parse_rgba_file rejects
    (compute dtype, CRC of the CDF tables, chunk size, segment lengths).  rgb: CodecInfo of the
    decoder's model."""
    blob = bytes(blob)
    if len(blob) < HEADER_BYTES:
        raise RuntimeError(f"RGAX file: truncated ({len(blob)} bytes, the header has "
                           f"{HEADER_BYTES})")
    magic, version, flags, h, w, chunk, crc, *lens = _HEADER.unpack_from(blob)
    if magic != MAGIC:
        raise RuntimeError("RGAX file: bad magic (not an RGAX file)")
    if version != VERSION:
        raise RuntimeError(f"RGAX file: unsupported version {version}")
    opaque, transparent = bool(flags & FLAG_OPAQUE), bool(flags & FLAG_TRANSPARENT)
    if flags & ~(FLAG_OPAQUE | FLAG_RGB_BF16 | FLAG_TRANSPARENT) or (opaque and transparent):
        raise RuntimeError(f"RGAX file: unknown flags {flags:#x}")
    if (h < 1 or w < 1 or h > alphaexact.MAX_SIDE or w > alphaexact.MAX_SIDE or chunk < 1
            or chunk >= 1 << 31):
        raise RuntimeError(f"RGAX file: bad size {h}x{w} or chunk size {chunk}")
    total = HEADER_BYTES + sum(lens)
    if total != len(blob):
        kind = "truncated" if len(blob) < total else "over-long"
        raise RuntimeError(f"RGAX file: {kind}: the section lengths say {total} bytes, the file "
                           f"has {len(blob)}")
    if ((opaque or transparent) and lens[0]) or (transparent and (lens[1] or lens[2])):
        raise RuntimeError("RGAX file: a section the flags do not allow")
    if (not (opaque or transparent) and not lens[0]) or (not transparent
                                                         and not (lens[1] and lens[2])):
        raise RuntimeError("RGAX file: a section the flags ask for is empty")
    hp, wp = anysize.padded_size(h, w)
    out = {"h": h, "w": w, "canvas": (hp, wp), "chunk": chunk, "opaque": opaque,
           "transparent": transparent, "alpha": None, "rgb_z": None, "rgb_y": None}
    if transparent:
        return out
    if bool(flags & FLAG_RGB_BF16) != rgb.bf16:
        raise RuntimeError(f"RGAX file: coded with the RGB codec in "
                           f"{'bf16' if flags & FLAG_RGB_BF16 else 'fp32'}, the model given runs "
                           f"in {'bf16' if rgb.bf16 else 'fp32'} (compute dtype)")
    if crc != rgb.crc:
        raise RuntimeError(f"RGAX file: the RGB codec's CDF tables differ from the encoder's "
                           f"(CRC {rgb.crc:#010x}, the file says {crc:#010x}): other weights")
    pos = HEADER_BYTES
    if lens[0]:
        a = alphaexact.parse_alpha_planes(blob[pos:pos + lens[0]])
        if (a["h"], a["w"]) != (h, w):
            raise RuntimeError(f"RGAX file: the alpha plane is {a['h']}x{a['w']}, the image "
                               f"{h}x{w}")
        out["alpha"] = a
    pos += lens[0]
    for name, n, want in zip(SECTIONS[1:], lens[1:], _segments(rgb, hp, wp)):
        lay = ChunkedLayout(blob[pos:pos + n])
        if lay.K != chunk or lay.seg_lengths.tolist() != want:
            raise RuntimeError(f"RGAX file: section {name} has chunk size {lay.K} and segments "
                               f"{lay.seg_lengths.tolist()}; a {h}x{w} image needs {chunk} and "
                               f"{want}")
        out[name] = lay
        pos += n
    return out


def _model(net):
    from .models._codec import _check
    dev = next(net.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("rgbac: this module runs on the GPU (HIP) only; there is no CPU "
                           f"fallback in the product path (the model is on {dev}).")
    _check(net)
    return dev


def _by_canvas(keys):
    groups = collections.OrderedDict()
    for k, key in keys:
        groups.setdefault(key, []).append(k)
    return groups


def _alpha_entries(entries):
    """RGBA descriptor entries -> the same rectangles' alpha bytes, 4 bytes apart."""
    return [(ptr + 3, h, w, stride) for ptr, h, w, stride in entries]


@torch.no_grad()
def encode_rgba_exact(images, rgbnet, chunk=256):
    """images: what anysize.pack_rgba takes (a list of (h, w, 4) uint8 arrays / tensors, any
    sizes) -> list[bytes], one complete file per image.  ``chunk``: symbols per rANS chunk of
    the RGB sections.  One classification read decides each image's kind; the alpha planes of all
    mixed images are coded by one pass of the plane coder, the RGB sections per canvas group."""
    dev = _model(rgbnet)
    chunk = int(chunk)
    if chunk <= 0 or chunk >= 1 << 31:
        raise ValueError("chunk size must be a positive 32-bit number")
    dev, sizes, entries, keep = anysize._sources(images, dev, "encode_rgba_exact")
    if max(max(s) for s in sizes) > alphaexact.MAX_SIDE:
        raise ValueError(f"encode_rgba_exact: an image side is at most {alphaexact.MAX_SIDE}")
    cls_dev = anysize._alpha_class(dev, entries)
    cls = cls_dev.cpu().tolist()           # the one read: 1 opaque, 2 transparent, 0 mixed
    info = codec_info(rgbnet)
    mixed = [k for k, c in enumerate(cls) if c == 0]
    alpha = {}
    if mixed:
        alpha = dict(zip(mixed, alphaexact._encode(
            dev, [sizes[k] for k in mixed], _alpha_entries([entries[k] for k in mixed]), 4)))
    files = [None] * len(sizes)
    groups = _by_canvas((k, anysize.padded_size(*sizes[k])) for k, c in enumerate(cls) if c != 2)
    for members in groups.values():
        opaque_dev = (cls_dev[torch.tensor(members, device=dev)] == 1).to(torch.int32)
        rgb = _encode_rgb_group(rgbnet, dev, [sizes[k] for k in members],
                                [entries[k] for k in members], opaque_dev.contiguous(), chunk)
        for k, (z, y) in zip(members, rgb):
            files[k] = build_rgba_exact(*sizes[k], chunk, "opaque" if cls[k] == 1 else "mixed",
                                        info, [alpha.get(k, b""), z, y])
    for k, c in enumerate(cls):
        if c == 2:
            files[k] = build_rgba_exact(*sizes[k], chunk, "transparent", info, [b""] * 3)
    return files


def _encode_rgb_group(net, dev, sizes, entries, opaque_dev, chunk):
    """The RGB half of rgbafile._encode_group for images that share a canvas: the same pack,
    pad modes, mask pyramid (from the true alpha) and tile rule -> per image (z, y) sections."""
    from .models._codec import latent_code
    p = anysize._pack(dev, sizes, entries, None, opaque_dev)
    with rt.fixed_tiles(per_image=True):
        _, me = mask_pyramid(p["alpha"], 4)
        y = net.Encoder.nhwc(rt.to_nhwc(p["masked"], net.compute_dtype), me[1], me[2])
        lat = latent_code(net, y=y)
        jobs = _latent_jobs(net, *lat[1:])
    z, y = encode_image_major(jobs, chunk)
    return list(zip(z, y))


@torch.no_grad()
def decode_rgba_exact(blobs, rgbnet):
    """blobs: files from encode_rgba_exact, any number, any order -> list of (h, w, 4) uint8 GPU
    tensors in the same order; the alpha bytes are the encoder's input bit for bit.  Every header
    and every alpha blob is parsed and validated on the host before any launch (RuntimeError);
    one plane-decoder launch restores all alpha planes; files that share a canvas and a chunk
    size decode their RGB as one batch; the one error word of all rANS launches is read once."""
    dev = _model(rgbnet)
    blobs = list(blobs)
    if not blobs:
        raise ValueError("decode_rgba_exact: no files")
    info = codec_info(rgbnet)
    parsed = [parse_rgba_exact(b, info) for b in blobs]
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    # the true RGBA bytes the pack reads: alpha 255, overwritten where a blob says otherwise
    srcs = [torch.full((f["h"], f["w"], 4), 255, dtype=torch.uint8, device=dev) for f in parsed]
    entries = [(t.data_ptr(), f["h"], f["w"], t.stride(0)) for t, f in zip(srcs, parsed)]
    mixed = [k for k, f in enumerate(parsed) if f["alpha"] is not None]
    if mixed:
        alphaexact._decode([parsed[k]["alpha"] for k in mixed],
                           _alpha_entries([entries[k] for k in mixed]), 4, dev, err)
    outs = [None] * len(blobs)
    groups = _by_canvas((k, f["canvas"] + (f["chunk"],)) for k, f in enumerate(parsed)
                        if not f["transparent"])
    for (hp, wp, _), members in groups.items():
        fs = [parsed[k] for k in members]
        opaque_dev = torch.tensor([int(f["opaque"]) for f in fs], dtype=torch.int32).to(dev)
        sizes = [(f["h"], f["w"]) for f in fs]
        alpha = anysize._pack(dev, sizes, [entries[k] for k in members], None,
                              opaque_dev)["alpha"]
        x_hat = _decode_rgb_group(rgbnet, fs, alpha, hp, wp, dev, err)
        for k, im in zip(members, anysize.unpack_rgba(x_hat, alpha, sizes)):
            outs[k] = im
    for k, f in enumerate(parsed):
        if f["transparent"]:
            outs[k] = torch.zeros((f["h"], f["w"], 4), dtype=torch.uint8, device=dev)
    _raise_code("RGAX file decode", int(err.item()))
    return outs


def _decode_rgb_group(net, fs, alpha, hp, wp, dev, err):
    """The RGB half of rgbafile._decode_group with the true alpha canvas in masknet's place:
    recon_alpha of it for the members that are not opaque, ones for the others."""
    nonop = [j for j, f in enumerate(fs) if not f["opaque"]]
    with rt.fixed_tiles(per_image=True):
        mask = torch.ones((len(fs), 1, hp, wp), device=dev)
        if nonop:
            idx = torch.tensor(nonop, device=dev)
            mask.index_copy_(0, idx, recon_alpha(alpha[idx]))
        lat = _decode_latents(net, [f["rgb_z"] for f in fs], [f["rgb_y"] for f in fs], hp, wp,
                              dev, err)
        _, md = mask_pyramid(mask, 4)
        return rt.to_nchw(net.Decoder.nhwc(lat[0], md[1], md[2])).clamp_(0, 1)
