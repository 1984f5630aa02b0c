"""Lossless alpha planes: time and size of rgbac.alphaexact against the learned alpha codec and
zlib.

  python tools/alpha_exact_bench.py [--out profiles/alpha_exact_bench.json] [--reps 7]
                                    [--warmup 3] [--no-headline]

The workload is section 21's: 8 images of 500 x 375 already on the device, four with a
soft-edged alpha, four with a hard-edged binary disc.  Reported:
  * encode_alpha_planes / decode_alpha_planes for the batch: host clock around the call plus a
    device synchronise, median (min to max) of ``--reps`` runs after ``--warmup``; the bare
    decode launch (tables already uploaded) with device events;
  * the same planes through the learned alpha codec's compress / decompress (bench.mask_net,
    device coder, fp32, the 512 x 384 canvas), timed the same way, alternating with the plane
    coder inside each repetition;
  * bytes per plane against zlib.compress(plane, 9) and against the learned codec's streams;
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


def planes(dev):
    import torch
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    out = []
    for i in range(N):
        r = ((yy - H / 2 - 3 * i) ** 2 + (xx - W / 2 + 2 * i) ** 2).float().sqrt()
        edge = 10.0 if i % 2 == 0 else 1e-3                 # soft edge / binary disc
        a = torch.round(torch.clamp((min(H, W) / 2.2 - r) / edge, 0, 1) * 255)
        out.append(a.to(torch.uint8).to(dev))
    return out


def stats(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3),
            "max": round(max(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alpha_exact_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-headline", action="store_true")
    args = ap.parse_args()
    import torch
    from bench import mask_net
    from rgbac import alphaexact as ax
    from rgbac import anysize
    if not torch.cuda.is_available():
        raise SystemExit("alpha_exact_bench: no GPU visible (there is no CPU path)")
    dev = torch.device("cuda:0")
    masknet = mask_net()
    masknet.update()
    masknet = masknet.to(dev)
    ps = planes(dev)
    rgba = [torch.zeros((H, W, 4), dtype=torch.uint8, device=dev) for _ in ps]
    for im, a in zip(rgba, ps):
        im[..., 3] = a
    canvas = anysize.pack_rgba(rgba, "transparent", device=dev)["alpha"]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    variants = {
        "plane_coder": (lambda: ax.encode_alpha_planes(ps), ax.decode_alpha_planes),
        "learned_codec": (lambda: masknet.compress(canvas, coder="device"),
                          lambda o: masknet.decompress(o["strings"], o["shape"], coder="device")),
    }
    coded = {}
    for name, (enc, dec) in variants.items():
        for _ in range(args.warmup):
            coded[name] = enc()
            out = dec(coded[name])
    if not all(torch.equal(a, b) for a, b in zip(ax.decode_alpha_planes(coded["plane_coder"]), ps)):
        raise SystemExit("alpha_exact_bench: the round trip is not exact")
    te = {n: [] for n in variants}
    td = {n: [] for n in variants}
    for _ in range(args.reps):
        for name, (enc, dec) in variants.items():
            c, ms = timed(enc)
            te[name].append(ms)
            td[name].append(timed(lambda: dec(c))[1])
    # the bare decode launch: everything uploaded, device events around the launch alone
    blobs = coded["plane_coder"]
    outs = [torch.empty((H, W), dtype=torch.uint8, device=dev) for _ in ps]
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    job = ax._decode_job([ax.parse_alpha_planes(b) for b in blobs],
                         [(t.data_ptr(), H, W, t.stride(0)) for t in outs], 1, dev, err)
    launch_ms = []
    for i in range(args.warmup + args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        job()
        e1.record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            launch_ms.append(e0.elapsed_time(e1))
    assert int(err.item()) == 0 and all(torch.equal(a, b) for a, b in zip(outs, ps))
    host = [p.cpu().numpy() for p in ps]
    learned = coded["learned_codec"]["strings"]
    res = {"what": "lossless alpha planes against the learned alpha codec and zlib", "planes": N,
           "size": [H, W], "reps": args.reps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0),
           "encode_ms": {n: stats(te[n]) for n in variants},
           "decode_ms": {n: stats(td[n]) for n in variants},
           "decode_launch_ms": stats(launch_ms),
           "blob_bytes": [len(b) for b in blobs],
           "zlib9_bytes": [len(zlib.compress(p.tobytes(), 9)) for p in host],
           "learned_codec_bytes_batch": sum(len(s) for part in learned for s in part),
           "raw_bytes_per_plane": H * W}
    print(json.dumps(res), flush=True)
    if not args.no_headline:
        del masknet, canvas
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
