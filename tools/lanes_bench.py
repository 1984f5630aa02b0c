"""Lanes coder against the chunked coder at chunk=256: wall-clock and bytes over the sweep
W in {8, 16, 32, 64} x K in {256, 512, 1024, 2048}.

  python tools/lanes_bench.py [--out profiles/lanes_bench.json] [--reps 7] [--warmup 3]
                              [--no-headline]

Workloads: section 18a's two configurations (AutoEncoder.compress / decompress, B=8 at 256x256
and B=1 at 1024x1024, bf16, latent gain 20) and section 21's eight 500 x 375 files
(encode_rgba / decode_rgba, bf16, four images with a soft-edged alpha and four opaque;
tools/rgba_file_bench.py's images).  In every workload the chunked coder at chunk=256 and the
16 lanes variants alternate inside each repetition; every call is timed with the host clock
around the call plus a device synchronise; ``--warmup`` calls of every variant run first, and
there every variant's decoded output is compared with chunk-256's (must be equal).  Reported:
median (min to max) per variant and call, the bytes written, and the variant section 25's rule
picks: the fewest file bytes on the section 21 workload among the variants whose decode_rgba
AND encode_rgba medians do not exceed chunk-256's of the same run; if none qualifies, the
fastest (smallest encode + decode median) and its shortfall.  Unless --no-headline,
``bench.py --gpus 1 --steps 20 --warmup 5`` runs last in a fresh process.  GPU only."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-learning-based-rgba-image-compression-with-masked-window-based-attention_amd")
for p in (ROOT, PKG, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

WIDTHS = (8, 16, 32, 64)
STEPS = (256, 512, 1024, 2048)
CONFIGS = [(8, 256), (1, 1024)]
GAIN = 20.0
VARIANTS = [("chunk256", {"coder": "device", "chunk": 256})] + \
    [(f"lanes_w{w}_k{k}", {"coder": "lanes", "lanes": w, "steps": k}) for w in WIDTHS for k in STEPS]


def stats(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3),
            "max": round(max(xs), 3)}


def sweep(enc, dec, same, size, reps, warmup):
    """enc(kw) -> coded, dec(coded, kw) -> output; -> one row per variant."""
    import torch

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    coded, ref = {}, None
    for name, kw in VARIANTS:
        for _ in range(warmup):
            coded[name] = enc(kw)
            out = dec(coded[name], kw)
        torch.cuda.synchronize()
        if ref is None:
            ref = out
        elif not same(out, ref):
            raise SystemExit(f"lanes_bench: {name} decodes to something else than chunk256")
    te = {n: [] for n, _ in VARIANTS}
    td = {n: [] for n, _ in VARIANTS}
    for _ in range(reps):
        for name, kw in VARIANTS:
            c, ms = timed(lambda: enc(kw))
            te[name].append(ms)
            td[name].append(timed(lambda: dec(c, kw))[1])
    return [{"variant": name, "lanes": kw.get("lanes"), "steps": kw.get("steps"),
             "encode_ms": stats(te[name]), "decode_ms": stats(td[name]),
             "bytes": size(coded[name])} for name, kw in VARIANTS]


def choose(rows):
    """Section 25's rule on the file workload's rows -> (variant row, qualified?)."""
    base = rows[0]
    ok = [r for r in rows[1:] if r["encode_ms"]["median"] <= base["encode_ms"]["median"]
          and r["decode_ms"]["median"] <= base["decode_ms"]["median"]]
    if ok:
        return min(ok, key=lambda r: r["bytes"]), True
    return min(rows[1:], key=lambda r: r["encode_ms"]["median"] + r["decode_ms"]["median"]), False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lanes_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-headline", action="store_true")
    args = ap.parse_args()
    import torch
    from bench import mask_net, rgb_net, synth_inputs
    from rgba_file_bench import images
    from rgbac.rgbafile import decode_rgba, encode_rgba
    if not torch.cuda.is_available():
        raise SystemExit("lanes_bench: no GPU visible (there is no CPU path)")
    dev = torch.device("cuda:0")
    net = rgb_net(GAIN).to(dev).set_compute_dtype(torch.bfloat16)
    net.update()
    res = {"what": "lanes coder sweep against the chunked coder at chunk=256", "dtype": "bf16",
           "latent_gain": GAIN, "reps": args.reps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "workloads": []}
    for B, S in CONFIGS:
        x, a = (t.to(dev) for t in synth_inputs(B, S, S, seed=0))
        rows = sweep(lambda kw: net.compress(x, a, **kw),
                     lambda o, kw: net.decompress(o["strings"], o["shape"], a,
                                                  coder=kw["coder"])["x_hat"],
                     torch.equal,
                     lambda o: sum(map(len, o["strings"][0] + o["strings"][1])),
                     args.reps, args.warmup)
        res["workloads"].append({"workload": f"compress/decompress B={B} {S}x{S}", "rows": rows})
        print(json.dumps(res["workloads"][-1]), flush=True)
    masknet = mask_net()
    masknet.update()
    masknet = masknet.to(dev).set_compute_dtype(torch.bfloat16)
    ims = images(dev, False)
    rows = sweep(lambda kw: encode_rgba(masknet, net, ims, **kw),
                 lambda fs, kw: decode_rgba(masknet, net, fs),
                 lambda a, b: all(torch.equal(u, v) for u, v in zip(a, b)),
                 lambda fs: sum(map(len, fs)), args.reps, args.warmup)
    pick, qualified = choose(rows)
    res["workloads"].append({"workload": "encode_rgba/decode_rgba, 8 files of 500x375",
                             "rows": rows})
    res["chosen"] = {"variant": pick["variant"], "lanes": pick["lanes"], "steps": pick["steps"],
                     "qualified": qualified,
                     "encode_vs_chunk256": round(pick["encode_ms"]["median"]
                                                 / rows[0]["encode_ms"]["median"], 3),
                     "decode_vs_chunk256": round(pick["decode_ms"]["median"]
                                                 / rows[0]["decode_ms"]["median"], 3),
                     "bytes_vs_chunk256": [pick["bytes"], rows[0]["bytes"]]}
    print(json.dumps(res["workloads"][-1]), flush=True)
    print(json.dumps(res["chosen"]), flush=True)
    if not args.no_headline:
        del masknet, net
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
