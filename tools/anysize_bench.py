"""Cost of the any-size pack / unpack launches (rgbac.anysize, csrc/anysize.hip) next to the same
results composed from torch ops, one image at a time.

  python tools/anysize_bench.py [--batch 8 --height 500 --width 375 --iters 2000]

The sources are uint8 (h, w, 4) GPU tensors (the decoded images already uploaded), so both sides
time device work plus their own launch overhead: `pack_rgba` is one descriptor upload and one
launch, the torch composition is per image permute / float / div / F.pad / where and a stack;
`unpack_rgba` is one upload and one launch, the torch composition per image slice / mul / add /
clamp / to(uint8) / cat / permute.  Outputs are compared with torch.equal before anything is
timed.  Also prints the bytes each launch must move and, from a timing of the bare launch
(descriptors uploaded once), the bandwidth that implies.  One JSON line per measurement.  GPU
only."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-learning-based-rgba-image-compression-with-masked-window-based-attention_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)


def _events(run, iters):
    """us per call of run(): device events around ``iters`` calls after warm calls."""
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters


def torch_pack(imgs, hp, wp, pad):
    mode = "constant" if pad == "transparent" else "replicate"
    al, rgb, msk = [], [], []
    # a tensor divisor: torch's GPU division by a Python scalar multiplies by the reciprocal,
    # which is not the IEEE quotient ToTensor computes on the CPU (and the kernel on the GPU)
    d255 = torch.full((), 255.0, device=imgs[0].device)
    for im in imgs:
        h, w = im.shape[:2]
        f = im.permute(2, 0, 1).float().div(d255)
        fp = F.pad(f[None], (0, wp - w, 0, hp - h), mode=mode)[0]
        a, c = fp[3:4], fp[:3]
        al.append(a)
        rgb.append(c)
        msk.append(torch.where(a > 0, c, a))
    return torch.stack(msk), torch.stack(al), torch.stack(rgb)


def torch_unpack(x_hat, alpha, sizes):
    outs = []
    for b, (h, w) in enumerate(sizes):
        q = torch.cat([x_hat[b, :, :h, :w], alpha[b, :, :h, :w]])
        q = q.mul(255).add(0.5).clamp(0, 255).to(torch.uint8)
        q[:3] = q[:3] * (q[3:] != 0)
        outs.append(q.permute(1, 2, 0).contiguous())
    return outs


def main(args):
    from rgbac import _lib
    from rgbac import anysize as az
    dev = torch.device("cuda:0")
    B, h, w = args.batch, args.height, args.width
    g = torch.Generator().manual_seed(0)
    imgs = [torch.randint(0, 256, (h, w, 4), generator=g, dtype=torch.uint8).to(dev)
            for _ in range(B)]
    sizes = [(h, w)] * B
    hp, wp = az.canvas(sizes)
    base = {"batch": B, "size": [h, w], "canvas": [hp, wp], "iters": args.iters}
    for pad in ("transparent", "replicate"):
        p = az.pack_rgba(imgs, pad=pad, device=dev)
        t = torch_pack(imgs, hp, wp, pad)
        same = all(torch.equal(u, v) for u, v in zip((p["masked"], p["alpha"], p["rgb"]), t))
        us_hip = _events(lambda: az.pack_rgba(imgs, pad=pad, device=dev), args.iters)
        us_torch = _events(lambda: torch_pack(imgs, hp, wp, pad), args.iters)
        print(json.dumps(dict(base, what="pack", pad=pad, equal=same, hip_us=round(us_hip, 1),
                              torch_us=round(us_torch, 1))), flush=True)
    p = az.pack_rgba(imgs, pad="transparent", device=dev)
    x_hat, alpha = p["rgb"], p["alpha"]
    got, want = az.unpack_rgba(x_hat, alpha, sizes), torch_unpack(x_hat, alpha, sizes)
    same = all(torch.equal(u, v) for u, v in zip(got, want))
    us_hip = _events(lambda: az.unpack_rgba(x_hat, alpha, sizes), args.iters)
    us_torch = _events(lambda: torch_unpack(x_hat, alpha, sizes), args.iters)
    print(json.dumps(dict(base, what="unpack", equal=same, hip_us=round(us_hip, 1),
                          torch_us=round(us_torch, 1))), flush=True)

    # the bare launches: descriptors uploaded once, outputs allocated once
    st = _lib.stream_ptr(dev)
    d_in = az._upload_descs([(im.data_ptr(), h, w, 4 * w) for im in imgs], dev)
    outs = [torch.empty((B, c, hp, wp), device=dev) for c in (1, 3, 3)]
    us = _events(lambda: _lib.call("rgbac_rgba_pack", B, d_in.data_ptr(), hp, wp, 0,
                                   *[o.data_ptr() for o in outs], st), args.iters)
    nbytes = B * (4 * h * w + 28 * hp * wp)
    print(json.dumps(dict(base, what="rgbac_rgba_pack launch", us=round(us, 1), bytes=nbytes,
                          gb_per_s=round(nbytes / us / 1e3, 1))), flush=True)
    flat = torch.empty(B * h * w * 4, dtype=torch.uint8, device=dev)
    d_out = az._upload_descs([(flat.data_ptr() + k * h * w * 4, h, w, 4 * w) for k in range(B)], dev)
    us = _events(lambda: _lib.call("rgbac_rgba_unpack", B, d_out.data_ptr(), hp, wp,
                                   x_hat.data_ptr(), alpha.data_ptr(), 1, st), args.iters)
    nbytes = B * 20 * h * w
    print(json.dumps(dict(base, what="rgbac_rgba_unpack launch", us=round(us, 1), bytes=nbytes,
                          gb_per_s=round(nbytes / us / 1e3, 1))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=500)
    ap.add_argument("--width", type=int, default=375)
    ap.add_argument("--iters", type=int, default=2000)
    a_ = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("anysize_bench: no GPU visible (there is no CPU path)")
    main(a_)
