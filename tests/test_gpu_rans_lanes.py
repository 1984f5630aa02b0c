"""GPU: the lane-interleaved rANS kernels (csrc/rans_lanes.hip) against their host twins, the
coder="lanes" path of both models against coder="device", and version-2 RGAF files against
version 1."""
import numpy as np
import pytest
import torch

import rans_lanes_cases as lc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _case(W, k, stride):
    from rgbac import ans
    n = lc.sizes_of(W)[k]
    sym, idx = lc.symbols(W, n)
    host = ans.CdfTables(*lc.tables(stride))
    return sym, idx, host, ans.DeviceCdfTables(host, DEV), n


# stride 0: the tables are staged in LDS; a stride above the LDS budget forces the global path
@pytest.mark.parametrize("stride", [0, 24577], ids=["lds", "global"])
@pytest.mark.parametrize("W", lc.WIDTHS)
@pytest.mark.parametrize("k", range(6))
def test_kernels_equal_host_twin(W, k, stride):
    from rgbac import ans
    sym, idx, host, dev, n = _case(W, k, stride)
    assert (2 * max(stride, 44) <= ans.LANES_LDS_ENTRIES) == (stride == 0)
    want = ans.encode_lanes_host(sym, idx, host, [n], lanes=W, steps=lc.K)
    dsym, didx = torch.from_numpy(sym).to(DEV), torch.from_numpy(idx).to(DEV)
    assert ans.encode_lanes(dsym, didx, dev, [n], lanes=W, steps=lc.K) == want
    dec = ans.LanesDecoder(want, DEV)
    out = dec.decode_segments(0, 1, didx, dev)
    dec.check()
    assert np.array_equal(out.cpu().numpy(), sym)


@pytest.mark.parametrize("damage", ["flip", "cut"])
def test_corruption_is_reported_and_contained(damage):
    """Three groups; the middle one is damaged in a copy.  check() raises, the other groups'
    symbols stay intact (bounded reads, error word: no fault)."""
    from rgbac import ans
    W, n = 8, 3 * 8 * lc.K
    sym, idx, host, dev, _ = _case(8, 0, 0)
    sym, idx = lc.symbols(W, n, seed=5)
    blob = ans.encode_lanes_host(sym, idx, host, [n], lanes=W, steps=lc.K)
    lay = ans.LanesLayout(blob)
    head = len(blob) - lay.payload.size
    raw = bytearray(blob)
    if damage == "flip":
        raw[head + int(lay.offsets[1]) + 4 * W + 2] ^= 0x55
    else:                                   # the middle group loses its last 4 bytes
        w = np.frombuffer(blob, dtype="<u4").copy()
        w[5 + 1 + 1] -= 4
        end = head + int(lay.offsets[2])
        raw = bytearray(w.tobytes()[:head]) + raw[head:end - 4] + raw[end:]
        raw += b"\0" * (-len(raw) % 4)
    dec = ans.LanesDecoder(bytes(raw), DEV)
    out = dec.decode_segments(0, 1, torch.from_numpy(idx).to(DEV), dev).cpu().numpy()
    with pytest.raises(RuntimeError, match="lanes stream decode: error"):
        dec.check()
    g = W * lc.K
    assert np.array_equal(out[:g], sym[:g]) and np.array_equal(out[2 * g:], sym[2 * g:])


@pytest.fixture(scope="module")
def nets(device):
    from bench import mask_net, rgb_net
    masknet, net = mask_net(), rgb_net()
    masknet.update()
    net.update()
    return masknet.to(device), net.to(device)


@pytest.mark.parametrize("which", ["alpha", "rgb"])
def test_models_lanes_equal_device_coder(device, nets, which):
    """64 x 64, B = 2, fp32: the lanes round trip gives the x_hat of the chunked round trip bit
    for bit (the same y symbols went through both coders), and the z containers of both formats
    decode to the same symbols."""
    from rgbac import ans
    from rgbac.models._codec import _z_indexes
    from test_gpu_models import _inputs
    x, a = (t.to(device) for t in _inputs(2, 64, 64, seed=3)[:2])
    net = nets[which == "rgb"].set_compute_dtype(torch.float32)
    args = (x, a) if which == "rgb" else (a,)
    tail = (a,) if which == "rgb" else ()
    outs = {c: net.compress(*args, coder=c) for c in ("device", "lanes")}
    assert outs["lanes"]["coder"] == "lanes"
    rec = {c: net.decompress(o["strings"], o["shape"], *tail, coder=c)["x_hat"]
           for c, o in outs.items()}
    assert torch.equal(rec["lanes"], rec["device"])
    eb = net.entropy_bottleneck
    z_idx = _z_indexes(eb.channels, 1, device)
    for zl, zd in zip(outs["lanes"]["strings"][1], outs["device"]["strings"][1]):
        sym = [D(s, device).decode_segments(0, 1, z_idx, eb.device_tables(device))
               for D, s in ((ans.LanesDecoder, zl), (ans.ChunkedDecoder, zd))]
        assert torch.equal(*sym)
    with pytest.raises(RuntimeError, match="bad magic"):
        net.decompress(outs["device"]["strings"], outs["device"]["shape"], *tail, coder="lanes")


def test_version2_files(device, nets):
    """Four images on one 128 x 128 canvas, version 2 at W = 16, K = 512 (and, for decoding, at the
    default geometry too): version-2 files of one batch equal those of single calls; they decode alone, shuffled and mixed with version-1 files to the RGBA bytes of the
    version-1 decode; each is smaller than its version-1 file at chunk = 256; the version-1
    parser's rule for flag bit 3 still holds for version-1 headers."""
    from rgbac import ans, rgbafile as rf
    from test_gpu_rgba_file import KINDS4, SIZES4, _rgba
    masknet, net = (m.set_compute_dtype(torch.float32) for m in nets)
    images = [_rgba(h, w, k, 10 + i) for i, ((h, w), k) in enumerate(zip(SIZES4, KINDS4))]
    v1 = rf.encode_rgba(masknet, net, images, chunk=256)
    geo = {"lanes": 16, "steps": 512}
    v2 = rf.encode_rgba(masknet, net, images, coder="lanes", **geo)
    assert v2 == [rf.encode_rgba(masknet, net, [im], coder="lanes", **geo)[0] for im in images]
    dflt = rf.encode_rgba(masknet, net, images, coder="lanes")      # the committed default
    print("default", ans.LANES_DEFAULT, [len(f) for f in dflt])
    w, k = ans.LANES_DEFAULT
    assert all(int.from_bytes(f[16:20], "little") == w | k << 8 for f in dflt)
    for a, b in zip(v1, v2):
        print(f"version 1: {len(a)} B, version 2: {len(b)} B")
        assert len(b) < len(a) and b[4:8] == b"\x02\x00" + bytes([b[6]]) + b"\x00" and b[6] & 8
        assert int.from_bytes(b[16:20], "little") == 16 | 512 << 8
    want = [t.cpu() for t in rf.decode_rgba(masknet, net, v1)]
    for order in ([2], [3, 1, 0, 2]):
        got = rf.decode_rgba(masknet, net, [v2[i] for i in order])
        assert all(torch.equal(g.cpu(), want[i]) for g, i in zip(got, order))
    mixed = rf.decode_rgba(masknet, net, [v2[1], v1[0], dflt[3], v1[2], dflt[0]])
    assert all(torch.equal(g.cpu(), want[i]) for g, i in zip(mixed, [1, 0, 3, 2, 0]))
    info = rf.codec_info(masknet), rf.codec_info(net)
    bad = bytearray(v1[0])
    bad[6] |= 8
    with pytest.raises(RuntimeError, match="unknown flags"):
        rf.parse_rgba_file(bytes(bad), *info)
    bad = bytearray(v2[0])
    bad[16] = 12                                        # W = 12
    with pytest.raises(RuntimeError, match="lanes geometry"):
        rf.parse_rgba_file(bytes(bad), *info)
    with pytest.raises(RuntimeError, match="truncated"):
        rf.parse_rgba_file(v2[0][:-4], *info)


@pytest.mark.parametrize("W", [16, 32])
def test_long_groups_cross_the_stream_window(W):
    """Two groups of 300 steps and a short third: many window flushes (encoder) and refills
    (decoder) per group, byte-unaligned group edges; device bytes against the host twin."""
    from rgbac import ans
    K, n = 300, 2 * W * 300 + 5
    sym, idx = lc.symbols(W, n, seed=9)
    host = ans.CdfTables(*lc.tables())
    dev = ans.DeviceCdfTables(host, DEV)
    want = ans.encode_lanes_host(sym, idx, host, [n], lanes=W, steps=K)
    lay = ans.LanesLayout(want)
    assert lay.counts.size == 3 and (lay.counts[:2] > 16 * W * 4).all() and lay.offsets[1] % 4
    dsym, didx = torch.from_numpy(sym).to(DEV), torch.from_numpy(idx).to(DEV)
    assert ans.encode_lanes(dsym, didx, dev, [n], lanes=W, steps=K) == want
    dec = ans.LanesDecoder(want, DEV)
    out = dec.decode_segments(0, 1, didx, dev)
    dec.check()
    assert np.array_equal(out.cpu().numpy(), sym)
