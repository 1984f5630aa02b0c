"""Cost of the MS-SSIM training distortion (trainRGB.py:183) on the HIP path.

  python tools/msssim_loss_bench.py step [--batch 16 --size 256 --dtype bf16 --iters 20]
      the trainRGB.py step (bench.py's config 3: forward, backward, clamp + Adam) with the
      distortion mse | msssim | masked, each eager and replayed from a HIP graph; device
      events over --iters warm iterations -> ms per step.
  python tools/msssim_loss_bench.py loss [--batch 16 --size 256 --iters 20] [--masked]
      only loss = 1 - ms_ssim(x, x_hat); loss.backward() on fp32 planes: events around the
      forward and around the backward, plus the bytes the backward launches must move (from
      shapes).  Run it under ``rocprofv3 --kernel-trace --stats`` for per-kernel times, or
      under ``rocprofv3 --pmc ...`` (a run of its own) for counters.

Prints one JSON line per measurement.  GPU only."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-learning-based-rgba-image-compression-with-masked-window-based-attention_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)


def _events(run, iters):
    """ms per call of run(), device events around ``iters`` calls after a warm call."""
    run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def _distortion(kind, x, a, out):
    from rgbac.metrics import masked_ms_ssim_torch as mm
    from rgbac.metrics import ms_ssim_torch as pm
    if kind == "mse":
        return out[1]
    if kind == "msssim":
        return 1 - pm.ms_ssim(x, out[0], data_range=1.0)
    return 1 - mm.ms_ssim(x, out[0], a, data_range=1.0)


def main_step(args):
    from bench import capture_train, synth_inputs
    from rgbac import runtime as rt
    from rgbac.layers.SupplyMask import mask_pyramid
    from rgbac.models.AutoEncoderRGB_Journal import AutoEncoder
    from rgbac.optim import AdamClamp
    from rgbac.parallel import DataParallelTrainer
    dev = torch.device("cuda:0")
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    B, S = args.batch, args.size
    x, a = synth_inputs(B, S, S, seed=0)
    x, a = x.to(dev), a.to(dev)
    _, me = mask_pyramid(a, 4)
    xin = (x * (a > 0)).detach()
    tune = os.path.join(ROOT, "profiles", f"tune_train_{args.dtype}_b{B}_{S}.json")
    if os.path.exists(tune):          # bench.py's committed tile choices: no autotuning here
        rt.load_tune_cache(tune)
    for kind in ("mse", "msssim", "masked"):
        for graph in (False, True):
            torch.manual_seed(234)
            net = AutoEncoder().train().to(dev).set_compute_dtype(dt)
            opt = AdamClamp(net.parameters(), lr=1e-4, clip=5.0)
            trainer = DataParallelTrainer(net, opt)

            def step():
                out = net(x, a, a, *me)
                loss = 4096.0 * _distortion(kind, xin, a, out) + out[2]
                trainer.step(loss)
                return loss.detach()

            for _ in range(3):
                step()
            torch.cuda.synchronize()
            run, g, gout = capture_train(step, opt, dev, not graph)
            ms = _events(run, args.iters)
            loss = run()
            print(json.dumps({"what": "train step", "loss": kind, "hip_graph": graph,
                              "batch": B, "size": S, "dtype": args.dtype, "iters": args.iters,
                              "ms_per_step": round(ms, 3), "loss_value": float(loss)}),
                  flush=True)
            del run, g, gout, trainer, opt, net


def backward_bytes(B, C, S, levels, masked, win=11):
    """Bytes each level-backward launch must move (fp32): read X, Y, (mask,) the coarser
    gradient; write dY."""
    rows = []
    h = w = S
    for i in range(levels):
        n = B * C * h * w
        hc, wc = (h + 2 * (h % 2) - 2) // 2 + 1, (w + 2 * (w % 2) - 2) // 2 + 1
        coarse = B * C * hc * wc if i + 1 < levels else 0
        rows.append({"level": i, "h": h, "w": w,
                     "bytes": 4 * (3 * n + coarse + (B * h * w if masked else 0))})
        h, w = hc, wc
    return rows


def main_loss(args):
    from bench import synth_inputs
    from rgbac.metrics import masked_ms_ssim_torch as mm
    from rgbac.metrics import ms_ssim_torch as pm
    dev = torch.device("cuda:0")
    B, S = args.batch, args.size
    x, a = synth_inputs(B, S, S, seed=0)
    x, a = x.to(dev), a.to(dev)
    g = torch.Generator().manual_seed(1)
    y = torch.clamp(x.cpu() + 0.05 * torch.randn(x.shape, generator=g), 0, 1).to(dev)
    y.requires_grad_()
    state = {}

    def fwd():
        v = mm.ms_ssim(x, y, a, data_range=1.0) if args.masked else \
            pm.ms_ssim(x, y, data_range=1.0)
        state["loss"] = 1 - v

    def bwd():
        y.grad = None
        state["loss"].backward(retain_graph=True)

    t_f = _events(fwd, args.iters)
    t_b = _events(bwd, args.iters)
    rows = backward_bytes(B, x.shape[1], S, 5, args.masked)
    print(json.dumps({"what": "loss only", "masked": args.masked, "batch": B, "size": S,
                      "iters": args.iters, "forward_ms": round(t_f, 4),
                      "backward_ms": round(t_b, 4), "loss_value": float(state["loss"]),
                      "backward_level_bytes": rows,
                      "backward_bytes": sum(r["bytes"] for r in rows)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["step", "loss"])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--masked", action="store_true")
    a_ = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("msssim_loss_bench: no GPU visible (there is no CPU path)")
    (main_step if a_.mode == "step" else main_loss)(a_)
