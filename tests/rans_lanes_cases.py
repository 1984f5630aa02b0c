"""Shared inputs of test_rans_lanes_host.py and test_gpu_rans_lanes.py: two CDF rows (one of 3
entries, one wide), symbols drawn from them, and one planted escape of every kind (below the
range, above it, magnitude 2^30 = 8 digits) on lane 0, on lane W - 1 and on two adjacent lanes
of one step."""
import numpy as np

K = 4
WIDTHS = (8, 64)
BIG = 1 << 30


def sizes_of(W):
    return (1, W - 1, W, W + 1, W * K, W * K + 1)


def tables(stride=0):
    """(cdfs int32 (2, stride), lengths, offsets): row 0 is {0, 60000, 65536}; row 1 a peaked
    row of 41 symbols plus the escape.  ``stride`` pads the rows (default: the wide row)."""
    f = np.maximum(1, (3000 * np.exp(-0.5 * ((np.arange(42) - 20) / 4.0) ** 2)).astype(np.int64))
    f[20] += 65536 - f.sum()
    wide = np.concatenate([[0], np.cumsum(f)])
    cdfs = np.zeros((2, max(stride, wide.size)), dtype=np.int32)
    cdfs[0, :3] = [0, 60000, 65536]
    cdfs[1, :wide.size] = wide
    return cdfs, np.array([3, wide.size], dtype=np.int32), np.array([0, -20], dtype=np.int32)


def symbols(W, n, seed=0):
    """-> (sym, idx) int32 of n symbols for W lanes."""
    rng = np.random.default_rng(1000 * W + n + seed)
    cdfs, lengths, offsets = tables()
    idx = (rng.random(n) < 0.7).astype(np.int32)
    p = np.diff(cdfs[1, :lengths[1]])[:-1].astype(np.float64)        # in-range symbols of row 1
    sym = np.where(idx == 1, rng.choice(p.size, size=n, p=p / p.sum()) - 20, 0).astype(np.int32)
    lo, hi = lambda i: offsets[i] - 3, lambda i: offsets[i] + lengths[i] + 5
    plant = {0: BIG, W - 1: lo, 2: hi, 3: lo, W + 2: -BIG, W + 3: BIG, W * K: hi}
    for j, v in plant.items():
        if j < n:
            sym[j] = v(idx[j]) if callable(v) else v
    return sym, idx
