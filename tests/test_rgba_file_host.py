"""CPU: the host half of the RGBA file codec (rgbac/rgbafile.py).

* the file header: build -> parse round trip, and every rejection the parser promises, each
  from a one-byte or one-field corruption;
* the per-image split of one image-major coding pass and the merged decode tables, against the
  chunk coder's host twins (rgbac.ans.*_host);
* the per-image tile rule (rt.fixed_tiles(per_image=True)) does not see the batch size, on
  every conv launch of both models' latent paths -- and the plain rule does, which is why the
  mode exists -- while the plain rule's answers are the ones recorded before the mode existed
  (tests/golden/fixed_rule_legacy.json).
"""
import struct

import numpy as np
import pytest

import rgba_file_cases as cases
from rans_chunk_cases import _gauss_symbols, gauss


@pytest.fixture(scope="module")
def infos():
    from rgbac.rgbafile import CodecInfo
    return (CodecInfo(0x1234ABCD, False, 192, 5, 16), CodecInfo(0x0BADF00D, False, 192, 10, 8))


def _container(seg_lengths, chunk, seed):
    """A valid container of the given segment lengths (symbols from the host coder)."""
    from rgbac.ans import encode_chunked_host
    sym, idx = _gauss_symbols(int(sum(seg_lengths)), seed)
    return encode_chunked_host(sym, idx, gauss().tables, seg_lengths, chunk)


def _file(infos, h, w, chunk=64, opaque=False):
    from rgbac import anysize, rgbafile as rf
    hp, wp = anysize.padded_size(h, w)
    az, ay = rf._segments(infos[0], hp, wp)
    rz, ry = rf._segments(infos[1], hp, wp)
    secs = [b"", b""] if opaque else [_container(az, chunk, 1), _container(ay, chunk, 2)]
    secs += [_container(rz, chunk, 3), _container(ry, chunk, 4)]
    return rf.build_rgba_file(h, w, chunk, opaque, infos[0], infos[1], secs), secs


def test_header_round_trip(infos):
    from rgbac import rgbafile as rf
    assert rf.HEADER_BYTES == 44
    for h, w, opaque in ((70, 129, False), (1, 1, True), (64, 64, False)):
        blob, secs = _file(infos, h, w, opaque=opaque)
        assert len(blob) == rf.HEADER_BYTES + sum(len(s) for s in secs)
        f = rf.parse_rgba_file(blob, *infos)
        hp, wp = -(-h // 64) * 64, -(-w // 64) * 64
        assert (f["h"], f["w"], f["canvas"], f["chunk"], f["opaque"]) == (h, w, (hp, wp), 64, opaque)
        for name, sec in zip(rf.SECTIONS, secs):
            if not sec:
                assert f[name] is None
            else:
                assert f[name].K == 64
        if not opaque:
            m = (hp // 8) * (wp // 8)
            assert f["alpha_z"].seg_lengths.tolist() == [192 * (hp // 64) * (wp // 64)]
            assert f["alpha_y"].seg_lengths.tolist() == [16 * m] * 5
            assert f["rgb_y"].seg_lengths.tolist() == [8 * m] * 10
    # an opaque file is accepted whatever the alpha codec at hand
    blob, _ = _file(infos, 5, 7, opaque=True)
    rf.parse_rgba_file(blob, infos[0]._replace(crc=1, bf16=True), infos[1])


def test_parser_rejections(infos):
    from rgbac import rgbafile as rf
    blob, secs = _file(infos, 70, 129)
    H = rf.HEADER_BYTES

    def rejects(bad, pattern, a=infos[0], r=infos[1]):
        with pytest.raises(RuntimeError, match=pattern):
            rf.parse_rgba_file(bytes(bad), a, r)

    def patched(off, fmt, value):
        b = bytearray(blob)
        struct.pack_into(fmt, b, off, value)
        return b

    flip = bytearray(blob)
    flip[0] ^= 1
    rejects(flip, "bad magic")
    rejects(patched(4, "<H", 2), "unsupported version")
    rejects(patched(6, "<H", 8), "unknown flags")
    rejects(blob[:20], "truncated")                                  # inside the header
    rejects(blob[:-4], "truncated")                                  # inside the last section
    rejects(blob + b"\0\0\0\0", "over-long")
    # one section length off by a word: disagrees with the file length
    (l2,) = struct.unpack_from("<I", blob, 36)
    rejects(patched(36, "<I", l2 + 4), "section lengths say")
    # two lengths traded against each other: the sum fits, a container does not
    (l3,) = struct.unpack_from("<I", blob, 40)
    b = patched(36, "<I", l2 + 4)
    struct.pack_into("<I", b, 40, l3 - 4)
    rejects(b, "chunked stream|segments")
    # the size field of another image: the containers' segments are not the ones it implies
    rejects(patched(8, "<I", 200), "needs")
    rejects(patched(12, "<I", 64), "needs")
    rejects(patched(8, "<I", 0), "bad size")
    # the chunk size field disagrees with the containers'
    rejects(patched(16, "<I", 128), "needs")
    # the opaque flag on a file with alpha sections, and off on one without
    rejects(patched(6, "<H", rf.FLAG_OPAQUE), "empty alpha sections")
    ob, _ = _file(infos, 70, 129, opaque=True)
    b = bytearray(ob)
    struct.pack_into("<H", b, 6, 0)
    rejects(b, "is empty")
    # a segment count changed inside a container (its own header word 3)
    b = bytearray(blob)
    struct.pack_into("<I", b, H + 12, 2)
    rejects(b, "chunked stream|needs")
    # CRC and dtype against the models given
    rejects(patched(20, "<I", 0x1234ABCC), "alpha codec's CDF tables differ")
    rejects(patched(24, "<I", 0), "RGB codec's CDF tables differ")
    rejects(blob, "RGB codec's CDF tables differ", r=infos[1]._replace(crc=5))
    rejects(patched(6, "<H", rf.FLAG_ALPHA_BF16), "alpha codec in bf16")
    rejects(patched(6, "<H", rf.FLAG_RGB_BF16), "RGB codec in bf16")
    rejects(blob, "RGB codec in fp32", r=infos[1]._replace(bf16=True))


def test_split_and_merge_tables_against_host_twins():
    """B = 3 images, 5 segments, symbols in latent_code's (segment, image, m) layout: one
    image-major pass cut per image equals coding each image alone, byte for byte; the merged
    tables of a shuffled subset of the files decode every image's symbols."""
    from rgbac import ans
    from rgbac.rgbafile import _starts
    tab = gauss().tables
    B, nseg, m, K = 3, 5, 333, 64                       # 333 = 5 chunks of 64 + one of 13
    sym, idx = _gauss_symbols(nseg * B * m, 11)         # in-range, escapes and 2^30 outliers
    sym, idx = sym.reshape(nseg, B, m), idx.reshape(nseg, B, m)
    starts = _starts(B, nseg, m)
    assert starts[2, 3] == (3 * B + 2) * m
    table, nch = ans.image_major_table(starts, [m] * nseg, K)
    assert nch == nseg * 6 and table.shape == (2, B * nch)
    assert table[0, nch + 6] == starts[1, 1] and table[1, nch + 5] == 13
    words = ans.encode_table_host(sym, idx, tab, table, K)
    files = ans.split_containers(words, B, [m] * nseg, K)
    for b in range(B):
        alone = ans.encode_chunked_host(sym[:, b].reshape(-1), idx[:, b].reshape(-1), tab,
                                        [m] * nseg, K)
        assert files[b] == alone, b
    # a shuffled subset: files [2, 0] as a group of two
    order = [2, 0]
    lays = [ans.ChunkedLayout(files[b]) for b in order]
    st2 = _starts(len(order), nseg, m)
    payload, meta, counts, first = ans.merged_decode_tables(lays, st2)
    assert payload.size == sum(lay.payload.size for lay in lays)
    assert first.tolist() == [12 * s for s in range(nseg + 1)]
    assert meta.shape == (3, 2 * nch) and counts.shape == (2 * nch,)
    got = ans.decode_merged_host(lays, st2, idx[:, order].reshape(-1), tab)
    assert np.array_equal(got.reshape(nseg, len(order), m), sym[:, order])
    # all three, in another order, and a single file alone
    for order in ([1, 2, 0], [1]):
        lays = [ans.ChunkedLayout(files[b]) for b in order]
        got = ans.decode_merged_host(lays, _starts(len(order), nseg, m),
                                     idx[:, order].reshape(-1), tab)
        assert np.array_equal(got.reshape(nseg, len(order), m), sym[:, order])
    # files whose segments differ cannot form a group
    other = ans.encode_chunked_host(sym[0, 0], idx[0, 0], tab, [m], K)
    with pytest.raises(RuntimeError, match="disagree on their segments"):
        ans.merged_decode_tables([lays[0], ans.ChunkedLayout(other)], _starts(2, nseg, m))


def test_per_image_rule_is_batch_invariant_and_the_plain_rule_is_not():
    from rgbac import runtime as rt
    differs = {}
    n = 0
    for which, dname, H, W in cases.configs():
        per_b = {}
        for B in cases.BATCHES:
            launches = cases.latent_launches(which, B, H, W, cases.DTYPES[dname])
            per_b[B] = [(name, rt.rule_choice(preps, per_image=True),
                         rt.rule_choice(preps, per_image=False)) for name, preps in launches]
        one = per_b[1]
        assert len(one) == (10 + 6 * (6 if which == "rgb" else 5))
        for name, per_image, plain in one:
            assert per_image == plain, (which, dname, H, W, name)     # the plain rule at B = 1
        for B in cases.BATCHES:
            assert [(nm, c) for nm, c, _ in per_b[B]] == [(nm, c) for nm, c, _ in one], \
                (which, dname, H, W, B)
            n += len(one)
        differs[(which, dname, H, W)] = [nm for (nm, _, p1), (_, _, p4) in zip(one, per_b[4])
                                         if p1 != p4]
    assert n > 1000
    # the premise: the plain rule's split-K moves with the batch at 128 x 128 in fp32, B = 1 vs 4
    # (the GPU test decodes a file alone and in a batch of 4 on that canvas)
    assert differs[("rgb", "fp32", 128, 128)], differs
    assert differs[("alpha", "fp32", 128, 128)], differs
    # the issue's worked example: the wide wave's first cc conv (34 K stages, 10 groups)
    assert "slice5.cc.0" in differs[("rgb", "fp32", 128, 128)]


def test_per_image_mode_stays_on_in_nested_contexts():
    from rgbac import runtime as rt
    assert rt._FIXED[0] == 0 and rt._PER_IMAGE[0] == 0
    with rt.fixed_tiles(per_image=True):
        with rt.fixed_tiles():                   # latent_code's own: the mode stays on
            assert rt._FIXED[0] == 2 and rt._PER_IMAGE[0] == 1
        assert rt._PER_IMAGE[0] == 1
    with rt.fixed_tiles():
        assert rt._FIXED[0] == 1 and rt._PER_IMAGE[0] == 0
    assert rt._FIXED[0] == 0 and rt._PER_IMAGE[0] == 0


def test_plain_fixed_rule_is_unchanged():
    from rgbac import runtime as rt
    want = cases.legacy_answers()
    n = 0
    for which, dname, H, W in cases.configs():
        for B in cases.BATCHES:
            got = [[name, *rt.rule_choice(preps)]
                   for name, preps in cases.latent_launches(which, B, H, W, cases.DTYPES[dname])]
            assert got == want[cases.config_key(which, dname, H, W, B)], (which, dname, H, W, B)
            n += len(got)
    assert n > 1000
