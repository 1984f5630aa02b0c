"""Tiled RGBA files against plain RGBA files: wall-clock and bytes of rgbac.rgbatile's
encode_rgba_tiled / decode_rgba_tiled next to rgbac.rgbafile's encode_rgba / decode_rgba
(unchanged code: the baseline), DESIGN.md section 23.

  python tools/rgba_tiled_bench.py [--out profiles/rgba_tiled_bench.json] [--reps 7] [--warmup 2]
                                   [--dtype bf16|fp32] [--tile 256]

Two workloads, both already on the device:
  * "mixed8": 8 images with 8 different canvases (500 x 375, 640 x 480, 300 x 300, 1024 x 768,
    375 x 500, 800 x 600, 256 x 400, 720 x 540), every other one with a soft-edged alpha, the
    rest opaque -- what the plain codec runs as eight B = 1 passes;
  * "large1": one 2048 x 2048 image whose left half is fully transparent.
Per workload the variants (plain files, tiled at overlap 0, tiled at overlap 32) alternate inside
each repetition so that drift hits them alike, after ``--warmup`` rounds of every variant; each
call is timed with the host clock around the call plus a device synchronise, and the median and
range of the repetitions are reported.  For large1 a 256 x 256 region decode is timed against
the full decode, and the bare blend launch of the full decode is timed with device events
against the bytes it moves (computed from the geometry: per output pixel 4 bytes written, and
16 bytes read per covering tile, 12 for an opaque one).

The nets are the benchmark's (random init, latent gain 20, update() called): the byte counts say
what the containers and the per-tile decisions cost or save, and nothing about rate.  One JSON
line per workload is printed and all of them are written to ``--out``.  GPU only."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-learning-based-rgba-image-compression-with-masked-window-based-attention_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

MIXED = [(500, 375), (640, 480), (300, 300), (1024, 768), (375, 500), (800, 600), (256, 400),
         (720, 540)]
LARGE = (2048, 2048)
REGION = (1024, 1280, 256, 256)


def image(h, w, kind, seed, dev):
    """Smooth colour fields plus noise (latents with structure).  kind: "soft" (a soft-edged
    disc of alpha), "opaque", or "half" (left half transparent, a soft-edged right half)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    base = torch.stack([(xx * (seed + 1) + yy * 2) % 256, (yy * (seed + 2)) % 256, (xx + yy) % 256], -1)
    rgb = (base.float() + torch.randn((h, w, 3), generator=g) * 12).clamp(0, 255)
    a = torch.full((h, w), 255.0)
    if kind == "soft":
        r = ((yy - h / 2) ** 2 + (xx - w / 2) ** 2).float().sqrt()
        a = torch.round(torch.clamp((min(h, w) / 2.2 - r) / 10, 0, 1) * 255)
    elif kind == "half":
        a = torch.round(torch.clamp((xx - w / 2).float() / 10, 0, 1) * 255)
    return torch.cat([rgb, a[..., None]], -1).to(torch.uint8).to(dev)


def stats(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3),
            "max": round(max(xs), 3)}


def blend_traffic(grid, rect, planes):
    """Bytes one blend launch moves for one output, from the geometry."""
    from rgbac import tiling
    y0, x0, hr, wr = rect
    n = 4 * hr * wr
    for t in tiling.region_tiles(grid, rect):
        if planes.get(t) is None:
            continue
        oy, ox, ey, ex = tiling.tile_rect(grid, t)
        area = ((min(y0 + hr, oy + ey) - max(y0, oy)) * (min(x0 + wr, ox + ex) - max(x0, ox)))
        n += area * (12 if planes[t][1] is None else 16)
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgba_tiled_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16")
    ap.add_argument("--blend-iters", type=int, default=50)
    args = ap.parse_args()
    import torch
    from bench import mask_net, rgb_net
    from rgbac import _lib, rgbatile, tiling
    from rgbac.rgbafile import decode_rgba, encode_rgba
    if not torch.cuda.is_available():
        raise SystemExit("rgba_tiled_bench: no GPU visible (there is no CPU path)")
    dev = torch.device("cuda:0")
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    masknet, net = mask_net(), rgb_net()
    masknet.update()
    net.update()
    masknet, net = masknet.to(dev).set_compute_dtype(dt), net.to(dev).set_compute_dtype(dt)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    def tiled(overlap):
        return (lambda ims: rgbatile.encode_rgba_tiled(masknet, net, ims, tile=args.tile,
                                                       overlap=overlap, chunk=args.chunk),
                lambda fs: rgbatile.decode_rgba_tiled(masknet, net, fs))
    variants = {"files": (lambda ims: encode_rgba(masknet, net, ims, chunk=args.chunk),
                          lambda fs: decode_rgba(masknet, net, fs)),
                "tiled_overlap0": tiled(0), "tiled_overlap32": tiled(32)}
    workloads = {
        "mixed8": [image(h, w, "soft" if i % 2 == 0 else "opaque", i, dev)
                   for i, (h, w) in enumerate(MIXED)],
        "large1": [image(*LARGE, "half", 9, dev)],
    }
    base = {"dtype": args.dtype, "chunk": args.chunk, "tile": args.tile, "reps": args.reps,
            "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
            "nets": "random init, latent gain 20: the bytes say nothing about rate"}
    results = []
    for wname, ims in workloads.items():
        files = {}
        for name, (enc, dec) in variants.items():
            for _ in range(args.warmup):
                files[name] = enc(ims)
                dec(files[name])
        te = {n: [] for n in variants}
        td = {n: [] for n in variants}
        for _ in range(args.reps):
            for name, (enc, dec) in variants.items():
                fs, ms = timed(lambda: enc(ims))
                te[name].append(ms)
                _, ms = timed(lambda: dec(fs))
                td[name].append(ms)
        res = dict(base, what=f"rgba tiled files against rgba files: {wname}",
                   sizes=[list(im.shape[:2]) for im in ims],
                   encode_ms={n: stats(te[n]) for n in variants},
                   decode_ms={n: stats(td[n]) for n in variants},
                   total_bytes={n: sum(map(len, files[n])) for n in variants})
        for name in ("tiled_overlap0", "tiled_overlap32"):
            infos = [rgbatile.tiled_info(b) for b in files[name]]
            kinds = [k for i in infos for k in i["kinds"]]
            res[name] = {"tiles": len(kinds), **{k: kinds.count(k) for k in rgbatile.KINDS},
                         "header_and_table_bytes": sum(i["header_bytes"] for i in infos)}
        if wname == "large1":
            blob = files["tiled_overlap32"][0]
            full_ms, reg_ms = [], []
            for i in range(args.warmup + args.reps):
                _, a = timed(lambda: rgbatile.decode_rgba_tiled(masknet, net, [blob]))
                _, b = timed(lambda: rgbatile.decode_rgba_tiled(masknet, net, [blob],
                                                                regions=[REGION]))
                if i >= args.warmup:
                    full_ms.append(a)
                    reg_ms.append(b)
            dbg = []
            full = rgbatile.decode_rgba_tiled(masknet, net, [blob], debug=dbg)[0]
            part = rgbatile.decode_rgba_tiled(masknet, net, [blob], regions=[REGION])[0]
            y0, x0, hr, wr = REGION
            res["region_decode"] = {
                "region": list(REGION), "region_ms": stats(reg_ms), "full_ms": stats(full_ms),
                "tiles_decoded": len(tiling.region_tiles(dbg[0]["grid"], REGION)),
                "tiles_in_full": len(dbg[0]["tiles"]),
                "region_equals_crop": bool(torch.equal(part, full[y0:y0 + hr, x0:x0 + wr]))}
            # the bare blend launch of the full decode: tables uploaded once, device events
            grid, planes = dbg[0]["grid"], dbg[0]["planes"]
            rect = tiling.check_region(grid, None)
            outs, call = rgbatile._blend_tables(dev, [grid], [rect], [planes])
            st = _lib.stream_ptr(dev)
            for _ in range(5):
                _lib.call("rgbac_rgba_blend_tiles", *call[:5], st)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.blend_iters):
                _lib.call("rgbac_rgba_blend_tiles", *call[:5], st)
            e1.record()
            torch.cuda.synchronize()
            us = 1e3 * e0.elapsed_time(e1) / args.blend_iters
            nbytes = blend_traffic(grid, rect, planes)
            res["blend_launch"] = {"what": "rgbac_rgba_blend_tiles, one 2048 x 2048 output",
                                   "iters": args.blend_iters, "us": round(us, 1), "bytes": nbytes,
                                   "gb_per_s": round(nbytes / us / 1e3, 1),
                                   "same_bytes_as_decode": bool(torch.equal(outs[0], full))}
        print(json.dumps(res), flush=True)
        results.append(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(results, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
