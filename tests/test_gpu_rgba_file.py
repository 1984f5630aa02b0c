"""GPU: self-contained RGBA files (rgbac/rgbafile.py) and the pieces under them.

* rgbac_rgba_opaque and the per-image-mode pack against torch on the same bytes;
* the alpha codec's compress / decompress: lossless in the latent, x_hat as the forward's;
* a file decodes alone, in any batch and in any order to the same symbols, y_hat, alpha bytes
  and (fp32) RGBA bytes -- on the canvas and batch sizes at which the plain fixed tile rule is
  known to change its split-K (tests/test_rgba_file_host.py);
* mixed canvases / opacity in one call, fidelity against the evaluation forward, size
  accounting, and a corrupt payload reported through the error word.

The nets are the benchmark's (random init, the conv feeding each latent scaled by 20, update()
called): at plain random init every symbol is 0 and a round trip proves nothing.
"""
import struct

import numpy as np
import pytest
import torch

from test_gpu_models import _inputs

pytestmark = pytest.mark.gpu

SIZES4 = [(128, 128), (100, 77), (65, 128), (128, 90)]       # one 128 x 128 canvas
KINDS4 = ["blob", "opaque", "half", "ramp"]
SUBSETS = {"all": [0, 1, 2, 3], "alone": [2], "pair": [3, 0]}


def _rgba(h, w, kind, seed):
    """(h, w, 4) uint8: random RGB, alpha by kind."""
    g = torch.Generator().manual_seed(seed)
    im = torch.randint(0, 256, (h, w, 4), generator=g, dtype=torch.uint8)
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    if kind == "opaque":
        a = torch.full((h, w), 255)
    elif kind == "zero":
        a = torch.zeros((h, w))
    elif kind == "half":
        a = torch.where(xx < w // 2, 0, 255)
    elif kind == "blob":
        r = ((yy - h / 2) ** 2 + (xx - w / 2) ** 2).float().sqrt()
        a = torch.round(torch.clamp((min(h, w) / 3 - r) / 8, 0, 1) * 255)
    else:                                                    # "ramp": every level occurs
        a = (xx * 255 // max(w - 1, 1) + yy) % 256
    im[..., 3] = a.to(torch.uint8)
    return im


@pytest.fixture(scope="module")
def nets(device):
    from bench import mask_net, rgb_net
    masknet, net = mask_net(), rgb_net()
    masknet.update()
    net.update()
    return masknet.to(device), net.to(device)


def _nonzero(sym):
    return (sym != 0).float().mean().item()


def _shared(dtype, nets):
    """Four images on one 128 x 128 canvas, encoded once; decoded all together, image 2
    alone, and images [3, 0]; with the debug records of every pass."""
    from rgbac.rgbafile import decode_rgba, encode_rgba
    masknet, net = nets
    dt = torch.float32 if dtype == "fp32" else torch.bfloat16
    masknet.set_compute_dtype(dt)
    net.set_compute_dtype(dt)
    try:
        images = [_rgba(h, w, k, 10 + i) for i, ((h, w), k) in enumerate(zip(SIZES4, KINDS4))]
        enc = []
        files = encode_rgba(masknet, net, images, debug=enc)
        dec = {}
        for name, sub in SUBSETS.items():
            dbg = []
            out = decode_rgba(masknet, net, [files[i] for i in sub], debug=dbg)
            dec[name] = {i: (out[j], dbg[j]) for j, i in enumerate(sub)}
        torch.cuda.synchronize()
    finally:
        masknet.set_compute_dtype(torch.float32)
        net.set_compute_dtype(torch.float32)
    return {"dtype": dtype, "images": images, "files": files, "enc": enc, "dec": dec}


@pytest.fixture(scope="module")
def shared(nets):
    return _shared("fp32", nets)


@pytest.fixture(scope="module")
def shared_bf16(nets):
    return _shared("bf16", nets)


# ------------------------------------------------------------------ the two new kernels
def test_opaque_flags_and_per_image_pack(device):
    from rgbac import anysize
    images, want = [], []
    for s, (h, w) in enumerate([(1, 1), (5, 7), (64, 64), (70, 129)]):
        for kind in ("opaque", "last254", "zero"):
            im = _rgba(h, w, "zero" if kind == "zero" else "opaque", 40 + s)
            if kind == "last254":
                im[h - 1, w - 1, 3] = 254
            images.append(im)
            want.append(1 if kind == "opaque" else 0)
    # views read in place: rows of a larger buffer (strided), and a start that is not
    # 4-byte aligned (copied to an aligned buffer by the host before the launch)
    big = _rgba(80, 140, "opaque", 50).to(device)
    big[79, 139, 3] = 0                                      # outside both views below
    images.append(big[3:3 + 70, 5:5 + 129])
    want.append(1)
    big2 = big.clone()
    big2[3 + 69, 5 + 128, 3] = 17                            # the view's last pixel
    images.append(big2[3:3 + 70, 5:5 + 129])
    want.append(0)
    flat = torch.zeros(1 + 5 * 7 * 4, dtype=torch.uint8, device=device)
    flat[1:] = _rgba(5, 7, "opaque", 51).reshape(-1).to(device)
    mis = flat[1:].view(5, 7, 4)
    assert mis.data_ptr() % 4 == 1
    images.append(mis)
    want.append(1)
    flags = anysize.opaque_flags(images, device=device)
    torch_flags = [int(bool((torch.as_tensor(im)[..., 3] == 255).all())) for im in images]
    assert flags.dtype == torch.int32 and flags.cpu().tolist() == want == torch_flags
    # the per-image-mode pack: image by image the scalar-mode pack of its own mode
    per = anysize.pack_rgba_modes(images, flags, device=device)
    tr = anysize.pack_rgba(images, "transparent", device=device)
    rp = anysize.pack_rgba(images, "replicate", device=device)
    assert per["sizes"] == tr["sizes"]
    for b, f in enumerate(want):
        ref = rp if f else tr
        for key in ("masked", "alpha", "rgb"):
            assert torch.equal(per[key][b], ref[key][b]), (b, key)
    # modes given by name
    named = anysize.pack_rgba_modes(images, ["replicate" if f else "transparent" for f in want],
                                    device=device)
    assert all(torch.equal(named[k], per[k]) for k in ("masked", "alpha", "rgb"))
    assert not torch.equal(tr["alpha"][0], rp["alpha"][0])   # the two modes do differ here


# ------------------------------------------------------------------ the alpha codec
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_alpha_latent_round_trip_is_lossless(device, nets, dtype):
    from rgbac import runtime as rt
    from rgbac.ans import BufferedRansEncoder, RansDecoder
    from rgbac.models._codec import latent_code
    from rgbac.models.AutoEncoderMask_Journal import _run_seq
    masknet = nets[0].set_compute_dtype(dtype)
    try:
        a = _inputs(3, 64, 128, seed=5)[1][1:].to(device)        # half, blob: B = 2
        with torch.no_grad():
            y = _run_seq(masknet.EncoderMask, rt.to_nhwc(a, dtype))
            YH, zs, ys, yi = latent_code(masknet, y=y)
            assert ys.shape == (5, 2 * 16 * 8 * 16)
            enc = BufferedRansEncoder()
            enc.encode_with_indexes(ys.cpu().reshape(-1), yi.cpu().reshape(-1),
                                    masknet.gaussian_conditional.tables())
            dec = RansDecoder()
            dec.set_stream(enc.flush())
            YH2, _, ys2, yi2 = latent_code(masknet, z_sym=zs, y_decoder=dec)
        torch.cuda.synchronize()
        assert _nonzero(ys) > 0.10, "the alpha latent is (nearly) all zero: the test shows nothing"
        assert torch.equal(ys2, ys) and torch.equal(yi2, yi)
        assert torch.equal(YH2.t, YH.t)
    finally:
        masknet.set_compute_dtype(torch.float32)


@pytest.mark.parametrize("coder", ["host", "device"])
def test_alpha_compress_decompress_fp32(device, nets, coder):
    masknet = nets[0].set_compute_dtype(torch.float32)
    a = _inputs(3, 64, 128, seed=5)[1][1:].to(device)
    out = masknet.compress(a, coder=coder)
    assert out["shape"] == torch.Size((1, 2))
    assert len(out["strings"][0]) == 1 and len(out["strings"][1]) == 2
    rec = masknet.decompress(out["strings"], out["shape"], coder=coder)["x_hat"]
    assert rec.shape == (2, 1, 64, 128) and rec.min() >= 0 and rec.max() <= 1
    with torch.no_grad():
        fwd = masknet(a)
    assert (rec - fwd[0].clamp(0, 1)).abs().max().item() < 1e-3


# ------------------------------------------------------------------ files
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_decodable_alone_and_in_any_batch(request, dtype):
    """Per image: z / y symbols, CDF indexes and y_hat rows of both codecs are bit-equal across
    the three decodes and equal the encoder's.  fp32 also asserts the reconstructed alpha planes
    and the RGBA bytes; bf16 asserts the symbol identity only (what decodability rests on) and
    prints whether the bytes were identical."""
    shared = request.getfixturevalue("shared" if dtype == "fp32" else "shared_bf16")
    enc, dec = shared["enc"], shared["dec"]
    for codec in ("rgb", "alpha"):
        ys = torch.cat([e[codec]["y"].reshape(-1) for e in enc if e[codec] is not None])
        assert _nonzero(ys) > 0.10, f"the {codec} latent is (nearly) all zero"
    assert enc[1]["alpha"] is None and all(enc[i]["alpha"] is not None for i in (0, 2, 3))
    same_bytes = same_alpha = True
    for name, sub in SUBSETS.items():
        for i in sub:
            out, dbg = dec[name][i]
            ref_out, ref = dec["all"][i]
            for codec in ("rgb", "alpha"):
                if enc[i][codec] is None:
                    assert dbg[codec] is None
                    continue
                for key in ("z", "y", "idx", "YH"):
                    assert torch.equal(dbg[codec][key], enc[i][codec][key]), (name, i, codec, key)
            assert out.shape == (*SIZES4[i], 4) and out.dtype == torch.uint8
            same_alpha &= bool(torch.equal(dbg["alpha_plane"], ref["alpha_plane"]) and
                               torch.equal(out[..., 3], ref_out[..., 3]))
            same_bytes &= bool(torch.equal(out, ref_out))
    print(f"rgba-file {dtype}: across batchings the alpha bytes are identical: {same_alpha}, "
          f"the RGBA bytes: {same_bytes}")
    if dtype == "fp32":
        assert same_alpha, "the reconstructed alpha depends on the batch"
        assert same_bytes, "latents and alpha are identical: the RGB synthesis is not"


def test_opaque_member_and_accounting(shared, nets):
    from rgbac import rgbafile as rf
    files, dec = shared["files"], shared["dec"]
    infos = [rf.codec_info(m) for m in nets]
    for i, blob in enumerate(files):
        lens = struct.unpack_from("<4I", blob, 28)
        assert len(blob) == rf.HEADER_BYTES + sum(lens)
        f = rf.parse_rgba_file(blob, *infos)
        assert (f["h"], f["w"]) == SIZES4[i] and f["canvas"] == (128, 128) and f["chunk"] == 256
        assert f["opaque"] == (KINDS4[i] == "opaque")
        if f["opaque"]:
            assert lens[0] == lens[1] == 0 and f["alpha_z"] is None and f["alpha_y"] is None
            assert bool((dec["all"][i][0][..., 3] == 255).all())
        else:
            assert f["alpha_z"].seg_lengths.tolist() == [192 * 4]
            assert f["alpha_y"].seg_lengths.tolist() == [16 * 256] * 5
        assert f["rgb_z"].seg_lengths.tolist() == [192 * 4]
        assert f["rgb_y"].seg_lengths.tolist() == [8 * 256] * 10


def test_fidelity_against_the_forward(shared, nets, device):
    """fp32, the non-opaque images: the decoded RGBA against rgba_forward_any's.  The alpha
    bytes agree except where either side's x_hat * 255 lies within 1e-3 of a rounding tie (the
    forward fuses (mu|sigma) with the Gaussian epilogue, the decoder does not); where the alpha
    agrees RGB is within one level."""
    from rgbac.anysize import pack_rgba, rgba_forward_any
    masknet, net = nets
    idxs = [0, 2, 3]
    images = [shared["images"][i] for i in idxs]
    fwd = rgba_forward_any(masknet, net, images, pad="transparent")
    with torch.no_grad():
        xa_fwd = masknet(pack_rgba(images, "transparent", device=device)["alpha"])[0].clamp(0, 1)
    ties = 0
    for j, i in enumerate(idxs):
        out, dbg = shared["dec"]["all"][i]
        h, w = SIZES4[i]
        got, ref = out.int(), fwd["rgba"][j].int()
        diff = got[..., 3] != ref[..., 3]

        def near_tie(x):
            v = x[:h, :w] * 255
            return ((v - torch.floor(v)) - 0.5).abs() < 1e-3
        allowed = near_tie(xa_fwd[j, 0]) | near_tie(dbg["alpha_x_hat"])
        assert not bool((diff & ~allowed).any()), (i, int((diff & ~allowed).sum()))
        ties += int(diff.sum())
        agree = ~diff
        worst = (got[..., :3] - ref[..., :3]).abs().amax(dim=2)[agree].max().item()
        assert worst <= 1, (i, worst)
    print(f"rgba-file fidelity: {ties} alpha bytes differ from the forward's at rounding ties")


def test_mixed_canvases_and_opacity(device, nets):
    """Six files from two canvases, opaque and not, shuffled: decoded in input order; an
    all-transparent image round-trips."""
    from rgbac import rgbafile as rf
    masknet, net = nets
    spec = [((64, 64), "opaque"), ((128, 64), "half"), ((50, 60), "zero"),
            ((100, 33), "opaque"), ((64, 64), "blob"), ((128, 64), "ramp")]
    images = [_rgba(h, w, k, 70 + i) for i, ((h, w), k) in enumerate(spec)]
    files = rf.encode_rgba(masknet, net, images)
    infos = [rf.codec_info(m) for m in nets]
    order = [4, 1, 0, 5, 3, 2]
    outs = rf.decode_rgba(masknet, net, [files[i] for i in order])
    alone = {i: rf.decode_rgba(masknet, net, [files[i]])[0] for i in (2, 3)}
    for out, i in zip(outs, order):
        (h, w), kind = spec[i]
        assert out.shape == (h, w, 4) and out.device.type == "cuda"
        f = rf.parse_rgba_file(files[i], *infos)
        assert f["opaque"] == (kind == "opaque")
        assert f["canvas"] == (-(-h // 64) * 64, 64)
        if kind == "opaque":
            assert bool((out[..., 3] == 255).all())
        if i in alone:
            assert torch.equal(out, alone[i]), i
    # the all-transparent image came back (no error above): RGB is zeroed where its alpha is 0
    z = outs[order.index(2)]
    assert bool((z[..., :3][z[..., 3] == 0] == 0).all())


def test_corrupt_payload_word_raises(shared, nets):
    """One word of one file's RGB y payload flipped: the chunk decoder reports it through the
    shared error word (RuntimeError), reading nothing out of bounds.  Which flips a rANS
    stream notices is a property of the stream, so the word is chosen with the CPU twin of the
    same decoder core, on slice 0 (whose CDF indexes do not depend on decoded symbols)."""
    from rgbac import ans, rgbafile as rf
    masknet, net = nets
    files, enc = shared["files"], shared["enc"]
    infos = [rf.codec_info(m) for m in nets]
    f = rf.parse_rgba_file(files[2], *infos)
    lay = f["rgb_y"]
    sec = len(files[2]) - struct.unpack_from("<4I", files[2], 28)[3]      # the y section's start
    body = 4 + lay.seg_lengths.size + lay.counts.size                     # words before the payload
    idx = enc[2]["rgb"]["idx"].cpu().numpy().reshape(-1)
    tab = net.gaussian_conditional.tables()
    words = np.frombuffer(files[2][sec:], dtype="<u4")
    found = None
    for k in range(int(lay.counts[:int(lay.first[1])].sum())):          # the words of slice 0
        bad = words.copy()
        bad[body + k] ^= 0xFFFFFFFF
        try:
            ans.decode_chunked_host(bad.tobytes(), idx, tab)
        except RuntimeError:
            found = k
            break
    assert found is not None, "no flipped word of slice 0 is noticed by the decoder core"
    blob = bytearray(files[2])
    off = sec + 4 * (body + found)
    blob[off:off + 4] = bytes(b ^ 0xFF for b in blob[off:off + 4])
    with pytest.raises(RuntimeError, match="RGBA file decode: error"):
        rf.decode_rgba(masknet, net, [files[0], bytes(blob), files[3]])
    # the untouched files still decode
    out = rf.decode_rgba(masknet, net, [files[0]])[0]
    assert torch.equal(out, shared["dec"]["all"][0][0])


def test_files_of_other_weights_are_rejected(shared, nets):
    from rgbac import rgbafile as rf
    masknet, net = nets
    net.set_compute_dtype(torch.bfloat16)
    try:
        with pytest.raises(RuntimeError, match="RGB codec in fp32"):
            rf.decode_rgba(masknet, net, shared["files"][:1])
    finally:
        net.set_compute_dtype(torch.float32)
    blob = bytearray(shared["files"][0])
    blob[24] ^= 1
    with pytest.raises(RuntimeError, match="RGB codec's CDF tables differ"):
        rf.decode_rgba(masknet, net, [bytes(blob)])
