"""CPU: the chunked rANS stream format through the host twins of the device coder
(rgbac_rans_chunk_encode_host / _decode_host over csrc/rans_chunk.h, the code a GPU lane runs).

* every chunk of a container is byte-identical to the single-stream host coder
  (RansEncoder.encode_with_indexes, csrc/rans.cpp) on that chunk's symbols, and the container
  is exactly header + count table + those bytes;
* containers round-trip, and every chunk also decodes with the host RansDecoder;
* malformed containers are rejected before decoding; a chunk that ends early is reported
  through the error word;
* tests/native/rans_chunk_check.cpp drives the core alone under AddressSanitizer + UBSan."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rans_chunk_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-learning-based-rgba-image-compression-with-masked-window-based-attention_amd")


@pytest.mark.parametrize("name", rc.NAMES)
def test_chunks_equal_single_stream_coder(name):
    c = rc.cases()[name]
    lay = c.layout
    assert lay.K == c.K and lay.seg_lengths.tolist() == c.segs
    per = [-(-n // c.K) for n in c.segs]
    assert lay.counts.size == sum(per) == len(c.ref)
    for i, ref in enumerate(c.ref):
        assert lay.chunk_bytes(i) == ref, (name, i)
    head = 4 * (rc.header_words(c) + len(c.ref))
    assert len(c.blob) == head + sum(len(r) for r in c.ref)
    assert c.blob[head:] == b"".join(c.ref)
    w = np.frombuffer(c.blob, dtype="<u4")
    assert w[:4].tolist() == [0x43524752, 1, c.K, len(c.segs)]
    assert w[4:4 + len(c.segs)].tolist() == c.segs
    # at most 10 records per symbol plus the state
    assert (lay.counts <= 10 * lay.table[1] + 2).all()


def test_cases_cover_the_escape_paths():
    """The Gaussian cases hold symbols below the offset, at and above max_value and +-2^30."""
    c = rc.cases()["gauss_n4097"]
    off = c.tables.offsets[c.idx].astype(np.int64)
    mx = c.tables.sizes[c.idx].astype(np.int64) - 2
    v = c.sym.astype(np.int64) - off
    assert (v < 0).any() and (v == mx).any() and (v > mx).any()
    assert ((v >= 0) & (v < mx)).sum() > c.sym.size // 2
    assert (c.sym == rc.BIG).any() and (c.sym == -rc.BIG).any()
    assert rc.cases()["gauss_n1"].sym[0] == rc.BIG            # eight nibbles in a 1-symbol stream
    assert len(rc.cases()["gauss_n1"].blob) == 4 * (5 + 1) + len(rc.cases()["gauss_n1"].ref[0])


def test_peak_segments_reach_the_no_refill_path():
    """A chunk of exactly two words (the final state, no renormalisation word)."""
    for name in ("peak_wide_k3", "peak_narrow"):
        c = rc.cases()[name]
        assert (c.layout.counts == 2).any(), (name, c.layout.counts)
        assert np.unique(c.sym).size == 1
    wide = rc.cases()["peak_wide_k3"]
    assert (wide.idx == wide.tables.sizes.size - 1).all()


@pytest.mark.parametrize("name", rc.NAMES)
def test_round_trip(name):
    from rgbac import ans
    c = rc.cases()[name]
    out = ans.decode_chunked_host(c.blob, c.idx, c.tables)
    assert out.dtype == np.int32 and np.array_equal(out, c.sym)
    dec = ans.RansDecoder()
    for i, (a, n) in enumerate(c.layout.table.T):
        got = dec.decode_with_indexes(c.layout.chunk_bytes(i), c.idx[a:a + n], c.tables)
        assert got == c.sym[a:a + n].tolist(), (name, i)


def test_rejected_containers():
    from rgbac import ans
    c = rc.cases()["two_segments"]
    w = np.frombuffer(c.blob, dtype="<u4")

    def rejects(words, match):
        with pytest.raises(RuntimeError, match=match):
            ans.decode_chunked_host(np.asarray(words, dtype="<u4").tobytes(), c.idx, c.tables)

    bad = w.copy()
    bad[0] ^= 1
    rejects(bad, "bad magic")
    bad = w.copy()
    bad[1] = 2
    rejects(bad, "version")
    rejects(w[:-1], "counts sum")                      # payload shorter than the counts say
    rejects(w[:-3], "counts sum")
    # a chunk count that disagrees with a segment length: one count dropped / one added
    body = rc.header_words(c)
    rejects(np.delete(w, body), "chunk count disagrees|counts sum")
    bad = w.copy()
    bad[4] += c.K                                      # the first segment claims one more chunk
    rejects(bad, "chunk count disagrees|counts sum")
    bad = w.copy()
    bad[body] = 1                                      # no room for the state words
    rejects(bad, "chunk count disagrees")
    bad = w.copy()
    bad[5] = 0
    rejects(bad, "empty segment")
    with pytest.raises(RuntimeError, match="whole 32-bit words"):
        ans.decode_chunked_host(c.blob[:-1], c.idx, c.tables)
    # a single-stream (compressai-format) string is not a container
    with pytest.raises(RuntimeError, match="bad magic|whole 32-bit words"):
        ans.decode_chunked_host(c.ref[0], c.idx, c.tables)
    with pytest.raises(RuntimeError, match="indexes given"):
        ans.decode_chunked_host(c.blob, c.idx[:-1], c.tables)


@pytest.mark.parametrize("name", ["two_segments", "gauss_n63"])
def test_short_chunk_raises_from_the_error_word(name):
    from rgbac import ans
    c = rc.cases()[name]
    blob = rc.short_chunk_blob(c)
    lay = ans.ChunkedLayout(blob)                      # passes header validation
    assert lay.counts[-1] == c.layout.counts[-1] - 1 and lay.counts[-1] >= 2
    with pytest.raises(RuntimeError, match=r"error 1 \(read past the end of a chunk\)"):
        ans.decode_chunked_host(blob, c.idx, c.tables)


def test_argument_errors():
    from rgbac import _lib, ans
    c = rc.cases()["gauss_n65"]
    with pytest.raises(ValueError, match="at least one symbol"):
        ans.encode_chunked_host(c.sym, c.idx, c.tables, [65, 0], 64)
    with pytest.raises(ValueError, match="chunk size"):
        ans.encode_chunked_host(c.sym, c.idx, c.tables, [65], 0)
    with pytest.raises(ValueError, match="disagree"):
        ans.encode_chunked_host(c.sym, c.idx, c.tables, [64], 64)
    bad_idx = c.idx.copy()
    bad_idx[3] = c.tables.sizes.size
    with pytest.raises(RuntimeError, match="error 2"):
        ans.encode_chunked_host(c.sym, bad_idx, c.tables, [65], 64)
    with pytest.raises(RuntimeError, match="error 2"):
        ans.decode_chunked_host(c.blob, bad_idx, c.tables)
    # the C ABI rejects K <= 0 and null pointers without a launch (device entry points too)
    for fn, nargs in (("rgbac_rans_chunk_sizes", 16), ("rgbac_rans_chunk_encode", 19),
                      ("rgbac_rans_chunk_decode", 19)):
        with pytest.raises(RuntimeError, match=f"{fn} failed \\(-1\\)"):
            _lib.call(fn, *[0] * nargs)
    # CPU tensors passed to the device functions raise, as everywhere else in the package
    import torch
    with pytest.raises(RuntimeError, match="GPU"):
        ans.encode_chunked(torch.from_numpy(c.sym.copy()), torch.from_numpy(c.idx.copy()),
                           c.tables, [65], 64)
    with pytest.raises(RuntimeError, match="GPU"):
        ans.ChunkedDecoder(c.blob, "cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        ans.DeviceCdfTables(c.tables, "cpu")


def _sanitizer_build(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "rans_chunk_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(PKG, "csrc"),
           os.path.join(ROOT, "tests", "native", "rans_chunk_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        low = r.stderr.lower()
        if "asan" in low or "ubsan" in low or "sanitize" in low:
            pytest.skip("the host compiler has no sanitizer runtime: " + r.stderr[-300:])
        pytest.fail("rans_chunk_check.cpp did not compile:\n" + r.stderr[-2000:])
    return exe


def test_core_under_address_and_ub_sanitizer(tmp_path):
    """The coder core alone (rans_chunk.h) in a stand-alone program built with
    -fsanitize=address,undefined: exact-size heap buffers, so any read or write outside a
    chunk's words, symbols or table row aborts the program."""
    exe = _sanitizer_build(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "rans_chunk_check: ok" in r.stdout
