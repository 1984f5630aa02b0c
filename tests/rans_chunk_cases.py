"""Shared cases of the chunked rANS coder tests (test_rans_chunk.py on the CPU,
test_gpu_rans_chunk.py on the GPU).  Everything is built once per process and never modified:
the symbols / indexes, the host twin's container and the per-chunk reference bytes of the
single-stream host coder (rgbac.ans.RansEncoder, csrc/rans.cpp)."""
import functools
from types import SimpleNamespace

import numpy as np

K = 64
BIG = 1 << 30                      # raw value of 2^31 - ish: eight bypass nibbles


@functools.lru_cache(maxsize=None)
def gauss():
    """The real GaussianConditional tables (64 scales, 0.11 .. 256) + their scale table."""
    from rgbac.entropy import GaussianConditional
    from rgbac.models.AutoEncoderRGB_Journal import get_scale_table
    gc = GaussianConditional(None)
    gc.update_scale_table(get_scale_table())
    return SimpleNamespace(tables=gc.tables(), scales=gc.scale_table.numpy().astype(np.float64))


@functools.lru_cache(maxsize=None)
def tiny():
    """One synthetic table of length 3: one symbol plus the escape."""
    from rgbac.ans import CdfTables
    return CdfTables([[0, 60000, 65536]], [3], [0])


def _gauss_symbols(n, seed):
    """In-range symbols, and at fixed strides: just below the offset, at max_value, above
    max_value and +-2^30 (eight bypass nibbles); every kind occurs for n >= 1 through the
    per-case phase."""
    g = gauss()
    tab = g.tables
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, tab.sizes.size, n).astype(np.int32)
    sym = np.rint(rng.standard_normal(n) * g.scales[idx]).astype(np.int64)
    pos = np.arange(n) + seed
    off, mx = tab.offsets[idx].astype(np.int64), tab.sizes[idx].astype(np.int64) - 2
    sym = np.where(pos % 11 == 0, off - 1 - (pos % 5), sym)          # below the offset
    sym = np.where(pos % 13 == 0, off + mx, sym)                      # at max_value
    sym = np.where(pos % 17 == 0, off + mx + 1 + (pos % 300), sym)    # above max_value
    sym = np.where(pos % 29 == 0, BIG, sym)
    sym = np.where(pos % 31 == 0, -BIG, sym)
    return sym.astype(np.int32), idx


def _peak(row):
    """(most probable symbol, its CDF index) of table ``row`` of the Gaussian tables."""
    tab = gauss().tables
    size = int(tab.sizes[row])
    freq = np.diff(tab.cdfs[row, :size - 1])          # the last interval is the escape
    return int(np.argmax(freq)) + int(tab.offsets[row])


def _build():
    cases = []

    def add(name, tables, k, segs, sym, idx):
        cases.append(SimpleNamespace(name=name, tables=tables, K=k, segs=list(segs),
                                     sym=np.ascontiguousarray(sym, dtype=np.int32),
                                     idx=np.ascontiguousarray(idx, dtype=np.int32)))

    g = gauss().tables
    # seeds chosen so that position 0 is special for n = 1 too (seed % 29 == 0: +2^30)
    for n, seed in ((1, 29), (63, 1), (64, 2), (65, 3), (64 * 64 + 1, 4)):
        add(f"gauss_n{n}", g, K, [n], *_gauss_symbols(n, seed))
    add("two_segments", g, K, [100, 37], *_gauss_symbols(137, 5))
    rng = np.random.default_rng(6)
    add("tiny_table", tiny(), K, [130], rng.integers(-2, 3, 130), np.zeros(130))
    # only the most probable symbol of the widest-scale table (p ~ 1/640, 9.3 bits each): a
    # chunk stays at its two state words while 2^31 / p^k < 2^47 * freq, i.e. up to 3 symbols,
    # so K is shortened to 3 for this segment (71 chunks, the last one of a single symbol)
    wide = g.sizes.size - 1
    n = 3 * 70 + 1
    add("peak_wide_k3", g, 3, [n], np.full(n, _peak(wide)), np.full(n, wide))
    # the same for the narrowest scale (p ~ 1): whole chunks of 64 symbols fit the state
    add("peak_narrow", g, K, [K * 2 + 5], np.full(K * 2 + 5, _peak(0)), np.zeros(K * 2 + 5))
    return cases


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case, each with .blob (the host twin's container), .layout (parsed) and
    .ref (the single-stream host coder's bytes of every chunk)."""
    from rgbac import ans
    out = {}
    for c in _build():
        c.blob = ans.encode_chunked_host(c.sym, c.idx, c.tables, c.segs, c.K)
        c.layout = ans.ChunkedLayout(c.blob)
        enc = ans.RansEncoder()
        c.ref = []
        for a, n in c.layout.table.T:
            c.ref.append(enc.encode_with_indexes(c.sym[a:a + n], c.idx[a:a + n], c.tables))
        for arr in (c.sym, c.idx):
            arr.setflags(write=False)
        out[c.name] = c
    return out


NAMES = ["gauss_n1", "gauss_n63", "gauss_n64", "gauss_n65", "gauss_n4097", "two_segments",
         "tiny_table", "peak_wide_k3", "peak_narrow"]


def header_words(case):
    return 4 + len(case.segs)


def short_chunk_blob(case):
    """The container with its last chunk's count reduced by one and the payload trimmed to
    match: passes header validation, and the last chunk then reads past its end."""
    w = np.frombuffer(case.blob, dtype="<u4").copy()
    last = header_words(case) + case.layout.counts.size - 1
    w[last] -= 1
    return w[:-1].tobytes()
