"""Lossless RGBA files: time and size of rgbac.rgbalossless (RGAL) against the four planes
through the alpha-plane coder and against zlib.

  python tools/rgba_lossless_bench.py [--out profiles/rgba_lossless_bench.json] [--reps 7]
                                      [--warmup 3] [--no-headline]

The workload is section 21 / 24's: 8 images of 500 x 375 already on the device.  Four carry an
alpha (soft-edged, hard-edged) over smooth and textured colour, four are opaque.  Reported:
  * encode_rgba_lossless / decode_rgba_lossless for the batch: host clock around the call plus a
    device synchronise, median (min to max) of ``--reps`` runs after ``--warmup``;
  * the same job the way it was done before: R, G, B, A as 32 unrelated planes through
    encode_alpha_planes / decode_alpha_planes (read in place at pixel stride 4, decoded into
    the four byte lanes of packed outputs), timed the same way, alternating with RGAL inside
    each repetition;
  * bytes per image of both, of zlib.compress(raw RGBA, 9) and of zlib on the RGBA with the
    colour of hidden pixels zeroed (what RGAL stores);
  * unless --no-headline: ``bench.py --gpus 1 --steps 20 --warmup 5`` in a fresh process.
GPU only."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-learning-based-rgba-image-compression-with-masked-window-based-attention_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

N, H, W = 8, 500, 375


def images(dev):
    """i < 4: alpha (even soft, odd hard) over smooth (i < 2) or textured colour; i >= 4: opaque,
    smooth and textured alternating.  Smooth: three unrelated ramps.  Textured: the ramps plus
    noise of +-12 -- in images 2 and 5 mostly luminance (one value for the three channels, +-2 of
    their own), as in photographs; in 3 and 7 independent per channel, the case in which
    subtracting green can only add noise."""
    import torch
    g = torch.Generator().manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    out = []
    for i in range(N):
        smooth = torch.stack([(xx + 2 * yy + 9 * i) // 3, (2 * xx + yy) // 4 + 30,
                              255 - (xx + yy) // 4], dim=-1) % 256
        own = torch.randint(-12, 13, (H, W, 3), generator=g)
        luma = torch.randint(-12, 13, (H, W, 1), generator=g) + own // 6
        rgb = smooth if i in (0, 1, 4, 6) else (smooth + (luma if i in (2, 5) else own)).clamp(0, 255)
        a = torch.full((H, W), 255.0)
        if i < 4:
            r = ((yy - H / 2 - 3 * i) ** 2 + (xx - W / 2 + 2 * i) ** 2).float().sqrt()
            edge = 10.0 if i % 2 == 0 else 1e-3
            a = torch.round(torch.clamp((min(H, W) / 2.2 - r) / edge, 0, 1) * 255)
        out.append(torch.cat([rgb, a[..., None]], dim=-1).to(torch.uint8).to(dev))
    return out


def stats(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3),
            "max": round(max(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgba_lossless_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-headline", action="store_true")
    args = ap.parse_args()
    import torch
    from rgbac import alphaexact as ax
    from rgbac import rgbalossless as rl
    if not torch.cuda.is_available():
        raise SystemExit("rgba_lossless_bench: no GPU visible (there is no CPU path)")
    dev = torch.device("cuda:0")
    ims = images(dev)
    planes = [im[..., c] for im in ims for c in range(4)]

    def planes_decode(blobs):
        outs = [torch.empty((H, W, 4), dtype=torch.uint8, device=dev) for _ in ims]
        ax.decode_alpha_planes(blobs, out=[o[..., c] for o in outs for c in range(4)])
        return outs

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    variants = {"rgal": (lambda: rl.encode_rgba_lossless(ims), rl.decode_rgba_lossless),
                "four_planes": (lambda: ax.encode_alpha_planes(planes), planes_decode)}
    coded, decoded = {}, {}
    for name, (enc, dec) in variants.items():
        for _ in range(args.warmup):
            coded[name] = enc()
            decoded[name] = dec(coded[name])
    want = [im.clone() for im in ims]
    for im in want:
        im[..., :3][im[..., 3] == 0] = 0
    if not all(torch.equal(a, b) for a, b in zip(decoded["rgal"], want)):
        raise SystemExit("rgba_lossless_bench: the RGAL round trip is not exact")
    if not all(torch.equal(a, b) for a, b in zip(decoded["four_planes"], ims)):
        raise SystemExit("rgba_lossless_bench: the plane round trip is not exact")
    te = {n: [] for n in variants}
    td = {n: [] for n in variants}
    for _ in range(args.reps):
        for name, (enc, dec) in variants.items():
            c, ms = timed(enc)
            te[name].append(ms)
            td[name].append(timed(lambda: dec(c))[1])
    four = coded["four_planes"]
    res = {"what": "lossless RGBA files against four planes through the alpha coder and zlib",
           "images": N, "size": [H, W], "reps": args.reps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0),
           "encode_ms": {n: stats(te[n]) for n in variants},
           "decode_ms": {n: stats(td[n]) for n in variants},
           "rgal_bytes": [len(b) for b in coded["rgal"]],
           "rgal_alpha_bytes": [int.from_bytes(b[16:20], "little") for b in coded["rgal"]],
           "four_planes_bytes": [sum(len(b) for b in four[4 * i:4 * i + 4]) for i in range(N)],
           "zlib9_bytes": [len(zlib.compress(im.cpu().numpy().tobytes(), 9)) for im in ims],
           "zlib9_hidden_zeroed_bytes": [len(zlib.compress(im.cpu().numpy().tobytes(), 9))
                                         for im in want],
           "raw_bytes_per_image": H * W * 4}
    print(json.dumps(res), flush=True)
    if not args.no_headline:
        del coded, decoded
        torch.cuda.empty_cache()
        run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                              "--steps", "20", "--warmup", "5"], capture_output=True, text=True,
                             cwd=ROOT)
        lines = [ln for ln in run.stdout.splitlines() if ln.startswith("{")]
        res["headline"] = json.loads(lines[-1]) if lines else {"error": run.stderr[-500:]}
        print(json.dumps(res["headline"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
