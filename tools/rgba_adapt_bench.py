"""Lossless RGBA files: the per-block colour transform (transform="adaptive", DESIGN.md section
30) against subtract-green everywhere (section 26), in size and time.

  python tools/rgba_adapt_bench.py [--out profiles/rgba_adapt_bench.json] [--reps 7] [--warmup 3]
                                   [--no-headline] [--kernel-trace DIR]

The workload and the protocol are tools/rgba_lossless_bench.py's: its 8 images of 500 x 375 on
the device, host clock around the call plus a device synchronise, median (min to max) of
``--reps`` runs after ``--warmup``, green and adaptive alternating inside each repetition.
Reported per image: bytes as green, as adaptive and as four planes through the alpha coder, and
how many blocks chose the plain channel in the red and in the blue slot.  Kernel times do not
come from this process: run it once more under ``rocprofv3 --kernel-trace -f csv -d DIR --
python tools/rgba_adapt_bench.py --no-headline --out /dev/null`` and then with ``--kernel-trace
DIR``, which adds the median duration of every colour kernel found in that trace to the result.
Unless --no-headline: ``bench.py --gpus 1 --steps 20 --warmup 5`` in a fresh process.  GPU only."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

from rgba_lossless_bench import PKG, ROOT, H, N, W, images, stats  # noqa: F401 (PKG: sys.path)


def kernel_medians(trace_dir):
    """rocprofv3's kernel trace CSVs under ``trace_dir`` -> {kernel: {"median_us", "calls"}} for
    the kernels of color_exact.hip and color_adapt.hip."""
    spans = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row["Kernel_Name"]
                for tag in ("color_", "adapt_"):
                    if tag in name and "_kernel" in name:
                        short = name[name.index(tag):name.index("_kernel")]
                        if short.endswith("_code"):
                            short += "<encode>" if "Lb1" in name or "<true>" in name else "<sizes>"
                        us = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
                        spans.setdefault(short, []).append(us)
                        break
    return {k: {"median_us": round(statistics.median(v), 1), "calls": len(v)}
            for k, v in sorted(spans.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgba_adapt_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-headline", action="store_true")
    ap.add_argument("--kernel-trace", default=None, metavar="DIR")
    args = ap.parse_args()
    import torch
    from rgbac import alphaexact as ax
    from rgbac import rgbalossless as rl
    if not torch.cuda.is_available():
        raise SystemExit("rgba_adapt_bench: no GPU visible (there is no CPU path)")
    dev = torch.device("cuda:0")
    ims = images(dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    coded = {}
    want = [im.clone() for im in ims]
    for im in want:
        im[..., :3][im[..., 3] == 0] = 0
    for t in rl.TRANSFORMS:
        for _ in range(args.warmup):
            coded[t] = rl.encode_rgba_lossless(ims, transform=t)
            out = rl.decode_rgba_lossless(coded[t])
        if not all(torch.equal(a, b) for a, b in zip(out, want)):
            raise SystemExit(f"rgba_adapt_bench: the {t} round trip is not exact")
    te = {t: [] for t in rl.TRANSFORMS}
    td = {t: [] for t in rl.TRANSFORMS}
    for _ in range(args.reps):
        for t in rl.TRANSFORMS:
            c, ms = timed(lambda: rl.encode_rgba_lossless(ims, transform=t))
            te[t].append(ms)
            td[t].append(timed(lambda: rl.decode_rgba_lossless(c))[1])
    four = ax.encode_alpha_planes([im[..., c] for im in ims for c in range(4)])
    cls = [rl.parse_rgba_lossless(b)["cls"] for b in coded["adaptive"]]
    res = {"what": "lossless RGBA files: colour transform per block against subtract-green",
           "images": N, "size": [H, W], "reps": args.reps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0),
           "encode_ms": {t: stats(te[t]) for t in rl.TRANSFORMS},
           "decode_ms": {t: stats(td[t]) for t in rl.TRANSFORMS},
           "green_bytes": [len(b) for b in coded["green"]],
           "adaptive_bytes": [len(b) for b in coded["adaptive"]],
           "alpha_bytes": [int.from_bytes(b[16:20], "little") for b in coded["adaptive"]],
           "four_planes_bytes": [sum(len(b) for b in four[4 * i:4 * i + 4]) for i in range(N)],
           "blocks": [int(c.size) for c in cls],
           "visible_blocks": [int((c != 1).sum()) for c in cls],
           "plain_red_blocks": [int((c & rl.PLAIN_R != 0).sum()) for c in cls],
           "plain_blue_blocks": [int((c & rl.PLAIN_B != 0).sum()) for c in cls]}
    if args.kernel_trace:
        res["kernel_us"] = {"source": "rocprofv3 --kernel-trace in a run of its own",
                            "kernels": kernel_medians(args.kernel_trace)}
    print(json.dumps(res), flush=True)
    if not args.no_headline:
        del coded
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
