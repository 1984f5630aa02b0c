"""Lossless RGBA files: palette mode (transform="palette") against the
colour coders of sections 26 and 30, in size and time.

  python tools/rgba_palette_bench.py [--out profiles/rgba_palette_bench.json] [--reps 7]
                                     [--warmup 3] [--no-headline] [--kernel-trace DIR]

Ten images of 500 x 375 on the device.  Eight have 4 / 16 / 64 / 256 colours drawn from a seeded
palette, as flat regions (a smooth field quantised to that many levels) and as an ordered 4 x 4
dither between neighbouring levels; the 16- and 256-colour ones have a transparent surround
(a hard-edged disc).  Two are images 4 and 3 of tools/rgba_lossless_bench.py (opaque ramps;
textured colour under a hard alpha): they have far more than 256 colours and show what the
fall-back costs.  Reported per image: bytes as palette (version 3), neighbour (version 4,
index_model="neighbour"), adaptive and green files, the palette
size, and zlib 9 of the index plane; per call: encode and decode of all ten as "palette", as
"neighbour" and as "adaptive", host clock plus a device synchronise, median (min to max) of ``--reps`` runs after
``--warmup``, the two alternating inside each repetition.  Kernel times do not come from this
process: run it once under ``rocprofv3 --kernel-trace -f csv -d DIR -- python
tools/rgba_palette_bench.py --no-headline --out /dev/null`` and then with ``--kernel-trace DIR``,
which adds the median duration of the palette kernels, of the plane coder's and of the index
coder's.  Unless
--no-headline: ``bench.py --gpus 1 --steps 20 --warmup 5`` in a fresh process.  GPU only."""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import time
import zlib

from rgba_lossless_bench import PKG, ROOT, H, W, images, stats  # noqa: F401 (PKG: sys.path)

COLOURS = (4, 16, 64, 256)


def palette_images(dev):
    """-> (names, images): colours x (flat, dither), then the two fall-back images."""
    import numpy as np
    import torch
    g = np.random.default_rng(7)
    yy, xx = np.mgrid[:H, :W]
    field = np.sin(xx / 61.0) + np.cos(yy / 47.0) + 0.004 * xx + 0.002 * yy
    field = (field - field.min()) / (np.ptp(field) + 1e-9)
    bayer = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]]) / 16.0
    disc = np.sqrt((yy - H / 2) ** 2 + (xx - W / 2) ** 2) < min(H, W) / 2.2
    names, out = [], []
    for n in COLOURS:
        pal = g.integers(0, 256, (n, 3))
        for kind in ("flat", "dither"):
            level = field * (n - 1) + (bayer[yy % 4, xx % 4] if kind == "dither" else 0.5)
            im = np.full((H, W, 4), 255, dtype=np.uint8)
            im[..., :3] = pal[np.clip(level.astype(np.int64), 0, n - 1)]
            if n in (16, 256):
                im[~disc, 3] = 0
            names.append(f"{n}-{kind}{'-cutout' if n in (16, 256) else ''}")
            out.append(torch.from_numpy(im).to(dev))
    base = images(dev)
    return names + ["ramps-opaque", "texture-cutout"], out + [base[4], base[3]]


def kernel_medians(trace_dir):
    """rocprofv3's kernel trace CSVs under ``trace_dir`` -> {kernel: {"median_us", "calls"}} for
    the kernels of color_palette.hip, alpha_exact.hip and index_exact.hip."""
    spans = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                found = re.search(r"::((?:palette|alpha|index)_\w+?)_kernel(<\w+>)?\(", row["Kernel_Name"])
                if found:
                    short = found.group(1) + {"<true>": "<encode>", "<false>": "<sizes>",
                                              None: ""}[found.group(2)]
                    us = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
                    spans.setdefault(short, []).append(us)
    return {k: {"median_us": round(statistics.median(v), 1), "calls": len(v)}
            for k, v in sorted(spans.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgba_palette_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-headline", action="store_true")
    ap.add_argument("--kernel-trace", default=None, metavar="DIR")
    args = ap.parse_args()
    import torch
    from rgbac import rgbalossless as rl
    if not torch.cuda.is_available():
        raise SystemExit("rgba_palette_bench: no GPU visible (there is no CPU path)")
    dev = torch.device("cuda:0")
    names, ims = palette_images(dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    modes = ("adaptive", "palette", "neighbour")

    def encode(t):
        if t == "neighbour":
            return rl.encode_rgba_lossless(ims, transform="palette", index_model="neighbour")
        return rl.encode_rgba_lossless(ims, transform=t)

    coded = {"green": rl.encode_rgba_lossless(ims)}
    want = [im.clone() for im in ims]
    for im in want:
        im[im[..., 3] == 0] = 0
    for t in modes:
        for _ in range(args.warmup):
            coded[t] = encode(t)
            out = rl.decode_rgba_lossless(coded[t])
        if not all(torch.equal(a, b) for a, b in zip(out, want)):
            raise SystemExit(f"rgba_palette_bench: the {t} round trip is not exact")
    te, td = {t: [] for t in modes}, {t: [] for t in modes}
    for _ in range(args.reps):
        for t in modes:
            c, ms = timed(lambda: encode(t))
            te[t].append(ms)
            td[t].append(timed(lambda: rl.decode_rgba_lossless(c))[1])
    parsed = [rl.parse_rgba_lossless(b) for b in coded["palette"]]
    index = []
    for f, im in zip(parsed, want):
        if f["transform"] != "palette":
            index.append(None)
            continue
        px = im.cpu().numpy().view("<u4")[..., 0]
        order = f["palette"].argsort()
        plane = order[f["palette"][order].searchsorted(px)].astype("u1")
        index.append(len(zlib.compress(plane.tobytes(), 9)))
    res = {"what": "lossless RGBA files: palette mode against the per-block colour coders",
           "images": names, "size": [H, W], "reps": args.reps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0),
           "encode_ms": {t: stats(te[t]) for t in modes},
           "decode_ms": {t: stats(td[t]) for t in modes},
           "versions": [int(b[4]) for b in coded["palette"]],
           "palette_colours": [int(f["palette"].size) if "palette" in f else None for f in parsed],
           "palette_bytes": [len(b) for b in coded["palette"]],
           "neighbour_versions": [int(b[4]) for b in coded["neighbour"]],
           "neighbour_bytes": [len(b) for b in coded["neighbour"]],
           "adaptive_bytes": [len(b) for b in coded["adaptive"]],
           "green_bytes": [len(b) for b in coded["green"]],
           "zlib9_index_plane_bytes": index,
           "raw_bytes_per_image": H * W * 4}
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
