"""Composite-bounded near-lossless RGBA files: size and time of rgbac.rgbanear with
bound="composite" against bound="pixel" and the exact files (RGAL), delta in {1, 2, 4} (DESIGN.md
section 29).

  python tools/rgba_blend_bench.py [--out profiles/rgba_blend_bench.json] [--reps 7] [--warmup 3]
                                   [--no-headline] [--calls-only] [--flat] [--kernels TRACE.csv]

The workload is section 28's eight 500 x 375 images, each under a SOFT alpha plane: a disc with a
feathered edge 60 pixels wide, and inside it a translucent band of alpha 96 (section 28's own
planes are hard-edged or opaque and would show nothing).  Reported:
  * encode / decode call times of every variant: host clock around the call plus a device
    synchronise, median (min to max) of ``--reps`` runs after ``--warmup``, the variants
    alternating inside each repetition;
  * bytes per image of every variant;
  * unless --no-headline: ``bench.py --gpus 1 --steps 20 --warmup 5`` in a fresh process.
--flat times something else: the pixel-bound (version 1) files decoded by csrc/color_near.hip, as
a list of their own, against the same files decoded by csrc/color_blend.hip with a flat table, as
a list that also holds one 1 x 1 version 2 file; its call times go under "flat_decode_ms".
--calls-only runs just the warm-up and the repetitions, for a ``rocprofv3 --kernel-trace`` run of
its own; --kernels reads that run's kernel trace CSV and adds the median duration of every colour
kernel (us) to the JSON of an earlier run, under "flat_kernel_us" with --flat.  GPU only."""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys

from rgba_lossless_bench import ROOT, H, W, N, images, stats
from rgba_near_bench import DELTAS


def kernel_medians(path):
    """rocprofv3's kernel trace CSV -> {kernel name: [launches, median, min, max us]} of the
    blend_* and near_* kernels (over all of DELTAS together)."""
    times = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0]
            name = name.replace("void ", "")
            if name.startswith(("blend_", "near_")):
                times.setdefault(name, []).append(
                    (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: [len(v), round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)]
            for k, v in sorted(times.items())}


def soft_images(dev):
    import torch
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    out = []
    for i, im in enumerate(images(dev)):
        r = ((yy - H / 2 - 3 * i) ** 2 + (xx - W / 2 + 2 * i) ** 2).float().sqrt()
        a = torch.clamp((min(H, W) / 2.1 - r) / 60.0, 0, 1) * 255
        a[H // 2 - 40:H // 2 + 40] = a[H // 2 - 40:H // 2 + 40].clamp(max=96)
        im = im.clone()
        im[..., 3] = torch.round(a).to(torch.uint8).to(dev)
        out.append(im)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgba_blend_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-headline", action="store_true")
    ap.add_argument("--calls-only", action="store_true")
    ap.add_argument("--flat", action="store_true")
    ap.add_argument("--kernels")
    args = ap.parse_args()

    def merge(update):
        res = {}
        if os.path.exists(args.out):
            with open(args.out) as fh:
                res = json.load(fh)
        res.update(update)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
        return res

    if args.kernels:
        res = merge({"flat_kernel_us" if args.flat else "kernel_us": kernel_medians(args.kernels)})
        print(json.dumps(res["flat_kernel_us" if args.flat else "kernel_us"]))
        return 0
    import time
    import torch
    from rgbac import rgbalossless as rl
    from rgbac import rgbanear as rn
    if not torch.cuda.is_available():
        raise SystemExit("rgba_blend_bench: no GPU visible (there is no CPU path)")
    dev = torch.device("cuda:0")
    ims = soft_images(dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    if args.flat:
        one = rn.encode_rgba_near([ims[0][:1, :1]], 1, bound="composite")
        variants = {}
        for d in DELTAS:
            variants[f"near_{d}"] = (lambda d=d: rn.encode_rgba_near(ims, d), rn.decode_rgba_near)
            variants[f"flat_{d}"] = (lambda d=d: rn.encode_rgba_near(ims, d) + one,
                                     lambda c: rn.decode_rgba_near(c)[:N])
    else:
        variants = {"rgal": (lambda: rl.encode_rgba_lossless(ims), rl.decode_rgba_lossless)}
        for d in DELTAS:
            for b in rn.BOUNDS:
                variants[f"{b}_{d}"] = (lambda d=d, b=b: rn.encode_rgba_near(ims, d, bound=b),
                                        rn.decode_rgba_near)
    coded, decoded = {}, {}
    for _ in range(args.warmup):
        for name, (enc, dec) in variants.items():
            coded[name] = enc()
            decoded[name] = dec(coded[name])
    for d in DELTAS:
        if args.flat:
            ok = all(torch.equal(x, y) for x, y in zip(decoded[f"near_{d}"], decoded[f"flat_{d}"]))
        else:
            ok = all(torch.equal(x[..., 3], y[..., 3]) and not y[..., :3][x[..., 3] == 0].any()
                     and int((x[..., 3:].int() * (x[..., :3].int() - y[..., :3].int()).abs()).max())
                     <= 255 * d for x, y in zip(ims, decoded[f"composite_{d}"]))
        if not ok:
            raise SystemExit(f"rgba_blend_bench: delta {d} does not decode to what it must")
    te = {n: [] for n in variants}
    td = {n: [] for n in variants}
    for _ in range(args.reps):
        for name, (enc, dec) in variants.items():
            c, ms = timed(enc)
            te[name].append(ms)
            td[name].append(timed(lambda: dec(c))[1])
    if args.calls_only:
        return 0
    if args.flat:
        print(json.dumps(merge({"flat_decode_ms": {n: stats(td[n]) for n in variants}})))
        return 0
    res = {"what": "composite-bounded near-lossless RGBA files against the pixel bound and RGAL",
           "images": N, "size": [H, W], "reps": args.reps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0),
           "encode_ms": {n: stats(te[n]) for n in variants},
           "decode_ms": {n: stats(td[n]) for n in variants},
           "bytes": {n: [len(b) for b in coded[n]] for n in variants},
           "alpha_bytes": [int.from_bytes(b[16:20], "little") for b in coded["rgal"]],
           "chunks": {n: [int((rn.parse_rgba_near(b)["counts"] > 0).sum()) for b in coded[n]]
                      for n in variants if n != "rgal"}}
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
    merge(res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
