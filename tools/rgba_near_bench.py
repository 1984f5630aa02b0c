"""Near-lossless RGBA files: size and time of rgbac.rgbanear (RGAN) for delta in {1, 2, 4} against
the exact files of rgbac.rgbalossless (RGAL).

  python tools/rgba_near_bench.py [--out profiles/rgba_near_bench.json] [--reps 7] [--warmup 3]
                                  [--no-headline] [--calls-only] [--kernels TRACE.csv]

The workload is section 26's (tools/rgba_lossless_bench.py): 8 images of 500 x 375 on the device.
Reported:
  * encode / decode call times of every variant: host clock around the call plus a device
    synchronise, median (min to max) of ``--reps`` runs after ``--warmup``, the variants
    alternating inside each repetition;
  * bytes per image of every variant, and how many colour chunks each RGAN file has left;
  * unless --no-headline: ``bench.py --gpus 1 --steps 20 --warmup 5`` in a fresh process.
--calls-only runs just the warm-up and the repetitions, for a ``rocprofv3 --kernel-trace`` run of
its own; --kernels reads that run's kernel trace CSV and adds the median duration of every
colour / alpha kernel (us) to the JSON of an earlier run.  GPU only."""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys

from rgba_lossless_bench import ROOT, H, W, N, images, stats

DELTAS = (1, 2, 4)


def kernel_medians(path):
    """rocprofv3's kernel trace CSV -> {kernel name: [launches, median, min, max us]} of the coders'
    kernels (the RGAN kernels over all of DELTAS together)."""
    times = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0]
            name = name.replace("void ", "")
            if any(k in name for k in ("near_", "color_", "alpha_")):
                times.setdefault(name, []).append(
                    (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: [len(v), round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)]
            for k, v in sorted(times.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgba_near_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-headline", action="store_true")
    ap.add_argument("--calls-only", action="store_true")
    ap.add_argument("--kernels")
    args = ap.parse_args()
    if args.kernels:
        with open(args.out) as fh:
            res = json.load(fh)
        res["kernel_us"] = kernel_medians(args.kernels)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
        print(json.dumps(res["kernel_us"]))
        return 0
    import time
    import torch
    from rgbac import rgbalossless as rl
    from rgbac import rgbanear as rn
    if not torch.cuda.is_available():
        raise SystemExit("rgba_near_bench: no GPU visible (there is no CPU path)")
    dev = torch.device("cuda:0")
    ims = images(dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    variants = {"rgal": (lambda: rl.encode_rgba_lossless(ims), rl.decode_rgba_lossless)}
    for d in DELTAS:
        variants[f"rgan_{d}"] = (lambda d=d: rn.encode_rgba_near(ims, d), rn.decode_rgba_near)
    coded, decoded = {}, {}
    for _ in range(args.warmup):
        for name, (enc, dec) in variants.items():
            coded[name] = enc()
            decoded[name] = dec(coded[name])
    for d in DELTAS:
        for x, y in zip(ims, decoded[f"rgan_{d}"]):
            vis = x[..., 3] != 0
            if not torch.equal(x[..., 3], y[..., 3]) or y[..., :3][~vis].any() \
                    or int((x[..., :3].int() - y[..., :3].int()).abs()[vis].max()) > d:
                raise SystemExit(f"rgba_near_bench: delta {d} does not keep its guarantee")
    te = {n: [] for n in variants}
    td = {n: [] for n in variants}
    for _ in range(args.reps):
        for name, (enc, dec) in variants.items():
            c, ms = timed(enc)
            te[name].append(ms)
            td[name].append(timed(lambda: dec(c))[1])
    if args.calls_only:
        return 0
    res = {"what": "near-lossless RGBA files against the exact files",
           "images": N, "size": [H, W], "reps": args.reps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0),
           "encode_ms": {n: stats(te[n]) for n in variants},
           "decode_ms": {n: stats(td[n]) for n in variants},
           "bytes": {n: [len(b) for b in coded[n]] for n in variants},
           "alpha_bytes": [int.from_bytes(b[16:20], "little") for b in coded["rgal"]],
           "chunks": {n: [int((rn.parse_rgba_near(b)["counts"] > 0).sum()) for b in coded[n]]
                      for n in variants if n != "rgal"},
           "chunks_rgal": [int((rl.parse_rgba_lossless(b)["counts"] > 0).sum())
                           for b in coded["rgal"]]}
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
