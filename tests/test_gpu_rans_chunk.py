"""GPU: the device-side chunked rANS coder (csrc/rans_dev.hip) and compress / decompress with
coder="device".

* rgbac_rans_chunk_sizes / _encode give counts and a container byte-identical to the host
  twins (which tests/test_rans_chunk.py ties, chunk by chunk, to the single-stream host coder),
  rgbac_rans_chunk_decode gives the symbols back; cases of tests/rans_chunk_cases.py, the
  64*64+1 one included (more than one workgroup, a partial last wave);
* a chunk that ends early is reported through the error word, with a full-shape result;
* model level: the device-coder round trip reproduces the host-coder round trip's x_hat bit for
  bit, its containers hold the host coder's bytes, and the default format is unchanged."""
import numpy as np
import pytest
import torch

import rans_chunk_cases as rc
from oracle import ans_ref as oa
from test_gpu_models import _inputs

pytestmark = pytest.mark.gpu


def _dev(c, device):
    from rgbac import ans
    return (torch.tensor(c.sym, device=device), torch.tensor(c.idx, device=device),
            ans.DeviceCdfTables(c.tables, device))


@pytest.mark.parametrize("name", rc.NAMES)
def test_kernels_match_host_twin(device, name):
    from rgbac import _lib, ans
    c = rc.cases()[name]
    sym, idx, tab = _dev(c, device)
    # the sizes kernel alone
    table = torch.from_numpy(c.layout.table.copy()).to(device)
    nch = table.shape[1]
    counts = torch.full((nch,), -1, dtype=torch.int32, device=device)
    err = torch.zeros(1, dtype=torch.int32, device=device)
    _lib.call("rgbac_rans_chunk_sizes", sym.data_ptr(), idx.data_ptr(), sym.numel(), 0,
              table[0].data_ptr(), table[1].data_ptr(), nch, c.K, *tab.args(),
              counts.data_ptr(), err.data_ptr(), _lib.stream_ptr(device))
    assert counts.cpu().tolist() == c.layout.counts.tolist()
    assert err.item() == 0
    # sizes + scan + encode: the container, byte for byte
    blob = ans.encode_chunked(sym, idx, tab, c.segs, c.K)
    assert blob == c.blob
    # decode
    dec = ans.ChunkedDecoder(c.blob, device)
    out = dec.decode_segments(0, len(c.segs), idx, tab)
    dec.check()
    assert out.dtype == torch.int32 and out.shape == sym.shape
    assert torch.equal(out, sym)


def test_decode_a_range_of_segments(device):
    from rgbac import ans
    c = rc.cases()["two_segments"]
    sym, idx, tab = _dev(c, device)
    dec = ans.ChunkedDecoder(c.blob, device)
    a = c.segs[0]
    out = torch.full((sym.numel(),), 7, dtype=torch.int32, device=device)
    dec.decode_segments(1, 2, idx[a:], tab, out=out[a:])
    assert torch.equal(out[a:], sym[a:]) and (out[:a] == 7).all()
    dec.decode_segments(0, 1, idx[:a], tab, out=out[:a])
    dec.check()
    assert torch.equal(out, sym)
    with pytest.raises(RuntimeError, match="indexes given"):
        dec.decode_segments(0, 2, idx[:-1], tab)


@pytest.mark.parametrize("name", ["two_segments", "gauss_n63"])
def test_short_chunk_sets_the_error_word(device, name):
    """The last chunk's count reduced by one, the payload trimmed to match: in-bounds memory
    only (the host sanitizer program runs the same core on exact-size buffers); the lane reads
    0 past its chunk's end, records error 1 and zero-fills."""
    from rgbac import ans
    c = rc.cases()[name]
    sym, idx, tab = _dev(c, device)
    dec = ans.ChunkedDecoder(rc.short_chunk_blob(c), device)
    out = dec.decode_segments(0, len(c.segs), idx, tab)
    assert out.shape == sym.shape
    with pytest.raises(RuntimeError, match=r"error 1 \(read past the end of a chunk\)"):
        dec.check()
    a = int(c.layout.table[0, -1])
    assert torch.equal(out[:a], sym[:a])              # the other chunks are untouched
    assert out[-1].item() == 0


def test_rejected_before_any_launch(device):
    from rgbac import ans
    c = rc.cases()["two_segments"]
    w = np.frombuffer(c.blob, dtype="<u4").copy()
    w[0] ^= 1
    with pytest.raises(RuntimeError, match="bad magic"):
        ans.ChunkedDecoder(w.tobytes(), device)
    with pytest.raises(RuntimeError, match="counts sum"):
        ans.ChunkedDecoder(c.blob[:-4], device)
    sym, idx, tab = _dev(c, device)
    with pytest.raises(RuntimeError, match="GPU"):
        ans.encode_chunked(sym.cpu(), idx, tab, c.segs, c.K)
    bad = idx.clone()
    bad[5] = 64
    with pytest.raises(RuntimeError, match="error 2"):
        ans.encode_chunked(sym, bad, tab, c.segs, c.K)


# ------------------------------------------------------------------------------ model level
@pytest.fixture(scope="module")
def codec_net():
    from rgbac.models.AutoEncoderRGB_Journal import AutoEncoder
    torch.manual_seed(234)
    net = AutoEncoder().eval()
    net.update()
    return net


def _config(which):
    if which == "fp32":
        x, a = _inputs(2, 64, 128, seed=2)
        return torch.float32, x, a, 256
    x, a = _inputs(3, 128, 128, seed=9)
    return torch.bfloat16, x[2:3], a[2:3], 64


@pytest.mark.parametrize("which", ["fp32", "bf16"])
def test_device_coder_round_trip_equals_host_coder(device, codec_net, which):
    from rgbac import ans
    from rgbac import runtime as rt
    from rgbac.layers.SupplyMask import mask_pyramid
    from rgbac.models._codec import latent_code
    dtype, x, a, chunk = _config(which)
    net = codec_net.to(device).set_compute_dtype(dtype)
    x, a = x.to(device), a.to(device)
    B = x.shape[0]
    host = net.compress(x, a)
    assert "coder" not in host
    rec_host = net.decompress(host["strings"], host["shape"], a)["x_hat"]
    out = net.compress(x, a, coder="device", chunk=chunk)
    assert out["coder"] == "device" and out["shape"] == host["shape"]
    assert len(out["strings"][0]) == 1 and len(out["strings"][1]) == B
    rec = net.decompress(out["strings"], out["shape"], a, coder="device")["x_hat"]
    assert torch.equal(rec, rec_host)

    # the containers against the host coder on the same latent_code symbols
    with torch.no_grad():
        _, me = mask_pyramid(a, 4)
        y = net.Encoder.nhwc(rt.to_nhwc(x.contiguous().float(), dtype), me[1], me[2])
        _, zs, ys, yi = latent_code(net, y=y)
    ys, yi, zs = ys.cpu().numpy(), yi.cpu().numpy(), zs.cpu().numpy()
    ns, n = ys.shape
    gtab = net.gaussian_conditional.tables()
    lay = ans.ChunkedLayout(out["strings"][0][0])
    assert lay.K == chunk and lay.seg_lengths.tolist() == [n] * ns
    enc = ans.RansEncoder()
    fs, fi = ys.reshape(-1), yi.reshape(-1)
    for i, (s, m) in enumerate(lay.table.T):
        assert lay.chunk_bytes(i) == enc.encode_with_indexes(fs[s:s + m], fi[s:s + m], gtab), i
    assert out["strings"][0][0] == ans.encode_chunked_host(fs, fi, gtab, [n] * ns, chunk)
    # the z containers decode to the same z_sym
    ztab = net.entropy_bottleneck.tables()
    C, zh, zw = zs.shape[1:]
    z_idx = np.repeat(np.arange(C, dtype=np.int32), zh * zw)
    for b in range(B):
        zl = ans.ChunkedLayout(out["strings"][1][b])
        assert zl.seg_lengths.tolist() == [C * zh * zw] and zl.K == chunk
        got = ans.decode_chunked_host(out["strings"][1][b], z_idx, ztab)
        assert np.array_equal(got, zs[b].reshape(-1))
    # the default call still writes the single-stream format: the oracle coder's bytes
    o = oa.BufferedRansEncoder()
    tab = net.gaussian_conditional
    o.encode_with_indexes(fs.tolist(), fi.tolist(), tab.quantized_cdf.tolist(),
                          tab.cdf_length.tolist(), tab.offset.tolist())
    assert o.flush() == host["strings"][0][0]
    # a host-format string is not a container
    with pytest.raises(RuntimeError, match="chunked stream"):
        net.decompress(host["strings"], host["shape"], a, coder="device")
    with pytest.raises(ValueError, match="coder"):
        net.compress(x, a, coder="gpu")
    net.set_compute_dtype(torch.float32)
