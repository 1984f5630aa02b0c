"""Tile geometry and the seam-blend rule of tiled RGBA files.  Host only:
pure Python and numpy, no GPU, no models.

An image is cut into a grid of fixed-size tiles that overlap their neighbours by ``overlap``
pixels.  Per axis of length n, with stride S = tile - overlap: k = max(1, ceil((n - overlap) / S))
tiles, tile i at origin o_i = i S with extent e_i = min(tile, n - o_i); tiles are numbered
row-major.  ``blend_tiles_host`` is the numpy twin of rgbac_rgba_blend_tiles (csrc/anysize.hip):
the same fp32 operations in the same order, so it is both the reference of the byte-exact test
and the statement of the rule.
"""
import collections

import numpy as np

TILE, OVERLAP = 256, 32       # defaults: a choice, not a measurement (section 23)

Axis = collections.namedtuple("Axis", "k origins extents")
Grid = collections.namedtuple("Grid", "h w tile overlap ky kx y x")


def _check(tile, overlap):
    tile, overlap = int(tile), int(overlap)
    if tile < 64 or tile % 64:
        raise ValueError(f"tiling: the tile size must be a positive multiple of 64, got {tile}")
    if not 0 <= overlap <= tile // 2:
        raise ValueError(f"tiling: the overlap must lie in [0, tile // 2], got {overlap} for "
                         f"tile {tile}")
    return tile, overlap


def tile_axis(n, tile, overlap):
    """One axis: Axis(k, origins, extents)."""
    tile, overlap = _check(tile, overlap)
    n = int(n)
    if n < 1:
        raise ValueError(f"tiling: an axis must have at least 1 pixel, got {n}")
    S = tile - overlap
    k = max(1, -(-(n - overlap) // S))
    origins = [i * S for i in range(k)]
    return Axis(k, origins, [min(tile, n - o) for o in origins])


def tile_grid(h, w, tile=TILE, overlap=OVERLAP):
    """-> Grid(h, w, tile, overlap, ky, kx, y: Axis, x: Axis); tile t = iy * kx + ix."""
    tile, overlap = _check(tile, overlap)
    y, x = tile_axis(h, tile, overlap), tile_axis(w, tile, overlap)
    return Grid(int(h), int(w), tile, overlap, y.k, x.k, y, x)


def tile_rect(grid, t):
    """(oy, ox, ey, ex) of tile t."""
    iy, ix = divmod(int(t), grid.kx)
    return grid.y.origins[iy], grid.x.origins[ix], grid.y.extents[iy], grid.x.extents[ix]


def check_region(grid, region):
    """None (the whole image) or (y0, x0, h, w) inside it -> (y0, x0, h, w); ValueError."""
    if region is None:
        return 0, 0, grid.h, grid.w
    y0, x0, hr, wr = (int(v) for v in region)
    if y0 < 0 or x0 < 0 or hr < 1 or wr < 1 or y0 + hr > grid.h or x0 + wr > grid.w:
        raise ValueError(f"tiling: the region {(y0, x0, hr, wr)} is not inside the "
                         f"{grid.h}x{grid.w} image")
    return y0, x0, hr, wr


def _axis_hits(axis, lo, n):
    return [i for i, (o, e) in enumerate(zip(axis.origins, axis.extents)) if o < lo + n and o + e > lo]


def region_tiles(grid, region=None):
    """The tiles that intersect the region, ascending (row-major)."""
    y0, x0, hr, wr = check_region(grid, region)
    xs = _axis_hits(grid.x, x0, wr)
    return [iy * grid.kx + ix for iy in _axis_hits(grid.y, y0, hr) for ix in xs]


def axis_weights(axis, i, overlap, lo, hi):
    """fp32 weights of tile i at the pixels lo .. hi-1 (all inside the tile): in the overlap with
    tile i - 1, r = (float(p - o_i) + 0.5f) / float(overlap); in the overlap with tile i + 1,
    1.0f - r of that tile; exactly 1.0f elsewhere.  Each operation rounded in fp32."""
    p = np.arange(lo, hi, dtype=np.int64)
    w = np.ones(p.shape, dtype=np.float32)
    if overlap == 0:
        return w
    ov = np.float32(overlap)
    d = p - axis.origins[i]
    if i >= 1:
        m = d < overlap
        w[m] = (d[m].astype(np.float32) + np.float32(0.5)) / ov
    if i + 1 < axis.k:
        dn = p - axis.origins[i + 1]
        m = dn >= 0
        w[m] = np.float32(1.0) - (dn[m].astype(np.float32) + np.float32(0.5)) / ov
    return w


def quant_u8(v):
    """(uint8) clamp(v * 255 + 0.5, 0, 255), multiply and add each rounded in fp32."""
    v = np.asarray(v, dtype=np.float32)
    q = v * np.float32(255.0) + np.float32(0.5)
    q = np.where(np.isnan(q), np.float32(0.0), q)       # fminf(fmaxf(NaN, 0), 255) = 0
    return np.clip(q, np.float32(0.0), np.float32(255.0)).astype(np.uint8)


def blend_tiles_host(grid, tiles, region=None):
    """tiles: {t: (x_hat, alpha)} with x_hat a (3, hp, wp) fp32 array and alpha an (hp, wp) fp32
    array or None (1.0 everywhere); a tile that is absent or None is transparent / not decoded
    (alpha 0, no colour).  -> (hr, wr, 4) uint8 of ``region`` (None: the whole image).

    Per pixel, over its covering tiles in row-major order, w_t = wy * wx:
      A = sum w_t a_t;  W+ = sum of w_t over a_t > 0;  C_c = (sum over a_t > 0 of w_t x_t,c) / W+
    (0 when no tile has a_t > 0), the sums starting from 0.0f and every operation rounded in
    fp32; then quant_u8 of A and C_c, and RGB = 0 where the alpha byte is 0.  Only the
    ey x ex rectangle of a tile's planes is read."""
    y0, x0, hr, wr = check_region(grid, region)
    A = np.zeros((hr, wr), dtype=np.float32)
    Wp = np.zeros((hr, wr), dtype=np.float32)
    C = np.zeros((3, hr, wr), dtype=np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in region_tiles(grid, region):
            if tiles.get(t) is None:
                continue
            x_hat, alpha = tiles[t]
            oy, ox, ey, ex = tile_rect(grid, t)
            iy, ix = divmod(t, grid.kx)
            ya, yb = max(y0, oy), min(y0 + hr, oy + ey)
            xa, xb = max(x0, ox), min(x0 + wr, ox + ex)
            w = (axis_weights(grid.y, iy, grid.overlap, ya, yb)[:, None] *
                 axis_weights(grid.x, ix, grid.overlap, xa, xb)[None, :])
            src = (slice(ya - oy, yb - oy), slice(xa - ox, xb - ox))
            dst = (slice(ya - y0, yb - y0), slice(xa - x0, xb - x0))
            a = (np.ones(w.shape, dtype=np.float32) if alpha is None
                 else np.asarray(alpha, dtype=np.float32)[src])
            A[dst] = A[dst] + w * a
            pos = a > 0
            Wp[dst] = np.where(pos, Wp[dst] + w, Wp[dst])
            for c in range(3):
                x = np.asarray(x_hat[c], dtype=np.float32)[src]
                C[c][dst] = np.where(pos, C[c][dst] + w * x, C[c][dst])
        out = np.zeros((hr, wr, 4), dtype=np.uint8)
        out[..., 3] = quant_u8(A)
        keep = (out[..., 3] > 0) & (Wp > 0)
        for c in range(3):
            out[..., c] = np.where(keep, quant_u8(C[c] / np.where(Wp > 0, Wp, np.float32(1.0))), 0)
    return out
