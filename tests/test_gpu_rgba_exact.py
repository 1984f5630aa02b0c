"""GPU: the lossless alpha-plane coder (csrc/alpha_exact.hip, rgbac/alphaexact.py) and the RGAX
files built on it (rgbac/rgbaexact.py).  The reference is the input itself.

* round trip, bit exact, for the cross of sizes and contents, coded in one ragged call, alone
  and in reversed order -- equal bytes every way -- and through strided views;
* the stream is the chunked rANS format's: symbols and contexts computed here pixel by pixel
  from the rules, the tables their normalised histograms, every chunk decoded by the host chunk
  decoder of rgbac.ans;
* the payload is no larger than the model's code length plus the flush of every chunk;
* files: exact alpha, the RGB sections of rgbafile._encode_group, any batch and order.
"""
import math
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 7), (16, 16), (17, 33), (70, 129)]
KINDS = ["zeros", "full", "mid", "disc", "ramp", "noise", "last_pixel", "last_block"]
CASES = [(s, k) for s in SIZES for k in KINDS]
# a chunk's state starts at kL = 2^31 and stays below 2^63 (rans_chunk.h): chunk_encode flushes
# it as two 32-bit words, and every other word carries 32 bits the model accounts for
FLUSH_BYTES = 8


def _plane(h, w, kind, seed=0):
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    if kind in ("zeros", "full", "mid"):
        a = torch.full((h, w), {"zeros": 0, "full": 255, "mid": 128}[kind])
    elif kind == "disc":
        a = torch.where((yy - h / 2) ** 2 + (xx - w / 2) ** 2 < (min(h, w) / 3) ** 2, 255, 0)
    elif kind == "ramp":
        a = (xx * 255 // max(w - 1, 1) + yy) % 256
    elif kind == "noise":
        a = torch.randint(0, 256, (h, w), generator=torch.Generator().manual_seed(seed))
    else:
        a = torch.full((h, w), 128)
        if kind == "last_pixel":
            a[-1, -1] = 7
        else:
            a[(h - 1) // 16 * 16, (w - 1) // 16 * 16] = 7
    return a.to(torch.uint8)


def _model(a):
    """Symbols and contexts of a plane, pixel by pixel from the rules of DESIGN.md section 24."""
    a = a.astype(np.int64)
    sym, ctx = np.zeros(a.shape, np.int32), np.zeros(a.shape, np.int32)
    for r in range(a.shape[0]):
        for c in range(a.shape[1]):
            br, bc = r % 16, c % 16
            if br == 0 and bc == 0:
                pred, k = 0, 4
            else:
                L = a[r, c - 1] if bc else a[r - 1, c]
                U = a[r - 1, c] if br else a[r, c - 1]
                D = a[r - 1, c - 1] if br and bc else L
                pred = min(L, U) if D >= max(L, U) else max(L, U) if D <= min(L, U) else L + U - D
                d = max(L, U, D) - min(L, U, D)
                k = 0 if d == 0 else 1 if d <= 8 else 2 if d <= 64 else 3
            sym[r, c], ctx[r, c] = (a[r, c] - pred) & 255, k
    return sym, ctx


def _into_frames(blobs, sizes, device):
    """Decodes into the middle of 0xA5-filled buffers -> (planes, frames)."""
    from rgbac.alphaexact import decode_alpha_planes
    frames = [torch.full((h + 6, w + 10), 0xA5, dtype=torch.uint8, device=device)
              for h, w in sizes]
    outs = [f[3:3 + h, 5:5 + w] for f, (h, w) in zip(frames, sizes)]
    decode_alpha_planes(blobs, out=outs)
    return outs, frames


def _frame_untouched(frame):
    f = frame.clone()
    f[3:-3, 5:-5] = 0xA5
    return bool((f == 0xA5).all())


@pytest.fixture(scope="module")
def coded(device):
    """Every case coded in one ragged call, and again in reversed order; decoded in one call."""
    from rgbac.alphaexact import encode_alpha_planes
    planes = [_plane(h, w, k, i).to(device) for i, ((h, w), k) in enumerate(CASES)]
    blobs = encode_alpha_planes(planes)
    rev = encode_alpha_planes(planes[::-1])[::-1]
    outs, frames = _into_frames(blobs, [s for s, _ in CASES], device)
    return {"planes": planes, "blobs": blobs, "rev": rev, "outs": outs, "frames": frames}


@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{h}x{w}-{k}" for (h, w), k in CASES])
def test_round_trip_exact(coded, device, i):
    from rgbac.alphaexact import encode_alpha_planes, encode_alpha_plane_host
    x = coded["planes"][i]
    alone = encode_alpha_planes([x])[0]
    assert alone == coded["blobs"][i] == coded["rev"][i]
    assert alone == encode_alpha_plane_host(x.cpu().numpy())
    assert torch.equal(coded["outs"][i], x) and _frame_untouched(coded["frames"][i])
    outs, frames = _into_frames([alone], [CASES[i][0]], device)
    assert torch.equal(outs[0], x) and _frame_untouched(frames[0])


def test_strided_views(device):
    """Views into larger noise buffers: the bytes around them must not reach the blob."""
    from rgbac.alphaexact import decode_alpha_planes, encode_alpha_planes
    g = torch.Generator().manual_seed(5)
    big = torch.randint(0, 256, (40, 90), generator=g, dtype=torch.uint8).to(device)
    rgba = torch.randint(0, 256, (50, 60, 4), generator=g, dtype=torch.uint8).to(device)
    views = [[big[3:3 + 17, 5:5 + 33]], [rgba[2:2 + 33, 3:3 + 18], rgba[7:7 + 21, 1:1 + 40, 3]]]
    for call in views:
        dense = [(v if v.dim() == 2 else v[..., 3]).contiguous() for v in call]
        blobs = encode_alpha_planes(call)
        assert blobs == encode_alpha_planes(dense)
        for out, want in zip(decode_alpha_planes(blobs), dense):
            assert torch.equal(out, want)


@pytest.mark.parametrize("kind", ["ramp", "noise"])
def test_stream_is_the_chunked_format(coded, kind):
    from rgbac import ans
    from rgbac.alphaexact import _blocks, host_tables, normalise_counts, parse_alpha_planes
    i = CASES.index(((17, 33), kind))
    f = parse_alpha_planes(coded["blobs"][i])
    sym, ctx = _model(coded["planes"][i].cpu().numpy())
    keep = np.flatnonzero(f["cls"] == 0)
    assert keep.tolist() == [0, 1, 2, 3, 4]     # 2 x 3 blocks; the last is one pixel: constant
    s = np.concatenate([_blocks(sym)[k] for k in keep])
    c = np.concatenate([_blocks(ctx)[k] for k in keep])
    for k in range(5):
        assert (f["freqs"][k] == normalise_counts(np.bincount(s[c == k], minlength=256))).all()
    seg = np.array([_blocks(sym)[k].size for k in keep])
    container = (ans._header(256, seg).tobytes() + f["counts"][keep].astype("<u4").tobytes()
                 + f["payload"].astype("<u4").tobytes())
    assert (ans.decode_chunked_host(container, c, host_tables(f["freqs"])) == s).all()


@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{h}x{w}-{k}" for (h, w), k in CASES])
def test_size_is_the_models(coded, i):
    from rgbac.alphaexact import _blocks, parse_alpha_planes
    f = parse_alpha_planes(coded["blobs"][i])
    x = coded["planes"][i].cpu().numpy()
    if (x == x.flat[0]).all():
        assert f["payload"].size == 0 and not (f["cls"] == 0).any()
        return
    sym, ctx = _model(x)
    bound = 0
    for k in np.flatnonzero(f["cls"] == 0):
        freq = f["freqs"][_blocks(ctx)[k], _blocks(sym)[k]]
        assert (freq > 0).all()
        bound += math.ceil(float(-np.log2(freq / 65536.0).sum()) / 8) + FLUSH_BYTES
    print(f"{CASES[i]}: payload {4 * f['payload'].size} bytes, bound {bound}")
    assert 4 * f["payload"].size <= bound


# ------------------------------------------------------------------ files
FILE_CASES = [((70, 129), "disc"), ((64, 64), "full"), ((100, 77), "ramp")]


@pytest.fixture(scope="module")
def files(device):
    from bench import rgb_net
    from rgbac.rgbaexact import decode_rgba_exact, encode_rgba_exact
    net = rgb_net()
    net.update()
    net = net.to(device)
    images = []
    for i, ((h, w), kind) in enumerate(FILE_CASES):
        im = torch.randint(0, 256, (h, w, 4), generator=torch.Generator().manual_seed(20 + i),
                           dtype=torch.uint8)
        im[..., 3] = _plane(h, w, kind)
        images.append(im.to(device))
    blobs = encode_rgba_exact(images, net)
    return {"net": net, "images": images, "blobs": blobs,
            "all": decode_rgba_exact(blobs, net)}


def test_file_alpha_exact_and_rgb_sections(files, device):
    from rgbac import anysize, rgbafile
    from rgbac.rgbaexact import parse_rgba_exact
    net, images = files["net"], files["images"]
    for im, out in zip(images, files["all"]):
        assert out.shape == im.shape and torch.equal(out[..., 3], im[..., 3])
    parsed = [parse_rgba_exact(b, rgbafile.codec_info(net)) for b in files["blobs"]]
    assert [f["opaque"] for f in parsed] == [False, True, False]
    assert parsed[1]["alpha"] is None and parsed[0]["alpha"] is not None
    # the RGB half of rgbafile._encode_group on the same images (masknet is never reached: every
    # member is declared opaque to the host, the pad modes stay the true ones)
    dev, sizes, entries, keep = anysize._sources(images, device, "test")
    flags = anysize._opaque(dev, entries)
    for k, blob in enumerate(files["blobs"]):
        secs, _ = rgbafile._encode_group(None, net, dev, [sizes[k]], [entries[k]], [1],
                                         flags[k:k + 1].contiguous(), 256, False)[0]
        assert blob.endswith(secs[2] + secs[3])
        assert struct.unpack_from("<2I", blob, 28) == (len(secs[2]), len(secs[3]))


@pytest.mark.parametrize("order", [[0], [1], [2], [2, 1, 0]], ids=str)
def test_file_any_batch_any_order(files, order):
    from rgbac.rgbaexact import decode_rgba_exact
    outs = decode_rgba_exact([files["blobs"][k] for k in order], files["net"])
    for k, out in zip(order, outs):
        assert torch.equal(out, files["all"][k])


def test_file_transparent_and_errors(files, device):
    from rgbac import rgbaexact as rx
    net = files["net"]
    blank = torch.zeros((9, 20, 4), dtype=torch.uint8, device=device)
    blank[..., :3] = 200
    blob = rx.encode_rgba_exact([blank], net)[0]
    assert len(blob) == rx.HEADER_BYTES
    assert not rx.decode_rgba_exact([blob], net)[0].any()
    # a flipped payload word of the alpha blob: reported through the error word
    good = files["blobs"][0]
    alpha_len = struct.unpack_from("<I", good, 24)[0]
    bad = bytearray(good)
    bad[rx.HEADER_BYTES + alpha_len - 3] ^= 0x10
    with pytest.raises(RuntimeError, match="RGAX file decode: error"):
        rx.decode_rgba_exact([bytes(bad)], net)
    # header errors raise on the host, before any launch
    with pytest.raises(RuntimeError, match="truncated"):
        rx.decode_rgba_exact([good[:-4]], net)
    with pytest.raises(RuntimeError, match="bad magic"):
        rx.decode_rgba_exact([b"RGAF" + good[4:]], net)
    with pytest.raises(RuntimeError, match="GPU"):
        rx.alphaexact.encode_alpha_planes([blank.cpu()], device="cpu")
