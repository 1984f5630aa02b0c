"""Cost of the ragged MS-SSIM (rgbac.metrics.ms_ssim_any, csrc/msssim_any.hip: 11 launches for
the whole batch) next to the only correct way before it: a loop of the uniform `ms_ssim` over
every image's crop (per image 15 launches plus the two crop copies).

  python tools/eval_any_bench.py [--batch 8 --height 500 --width 375 --iters 200 --reps 7]

DESIGN.md section 20's workload: 8 images of 500 x 375 on the 512 x 384 canvas, replicated
outside each rectangle.  The two forms are first compared (max |difference| per image), then
timed with device events around ``iters`` calls after warm-up calls, ``reps`` times each in
alternation (batch, loop, batch, loop, ...), so that clock drift hits both alike.  Prints one JSON
line per repetition and one with the median and range of each form.  The masked pair
(`masked_ms_ssim_any` against a loop of the masked `ms_ssim`) follows in the same way.  GPU only."""
import argparse
import json
import os
import statistics
import sys

import torch

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


def _ab(name, base, batch_fn, loop_fn, args):
    got, want = batch_fn(), loop_fn()
    diff = (got - want).abs().max().item()
    tb, tl = [], []
    for r in range(args.reps):
        tb.append(_events(batch_fn, args.iters))
        tl.append(_events(loop_fn, args.iters))
        print(json.dumps(dict(base, what=name, rep=r, batch_us=round(tb[-1], 1),
                              loop_us=round(tl[-1], 1))), flush=True)
    print(json.dumps(dict(base, what=name + " summary", max_abs_diff=diff,
                          bit_identical=bool(torch.equal(got, want)),
                          batch_us_median=round(statistics.median(tb), 1),
                          batch_us_range=[round(min(tb), 1), round(max(tb), 1)],
                          loop_us_median=round(statistics.median(tl), 1),
                          loop_us_range=[round(min(tl), 1), round(max(tl), 1)],
                          loop_over_batch=round(statistics.median(tl) / statistics.median(tb), 2))),
          flush=True)


def main(args):
    from rgbac import anysize as az
    from rgbac.metrics import masked_ms_ssim_any, ms_ssim_any
    from rgbac.metrics import masked_ms_ssim_torch as mm
    from rgbac.metrics.ms_ssim_torch import ms_ssim
    dev = torch.device("cuda:0")
    B, h, w = args.batch, args.height, args.width
    g = torch.Generator().manual_seed(0)
    x = torch.rand((B, 3, h, w), generator=g)
    x = torch.nn.functional.avg_pool2d(x, 3, 1, 1)
    y = (x + 0.05 * torch.randn((B, 3, h, w), generator=g)).clamp(0, 1)
    m = (torch.rand((B, 1, h, w), generator=g) > 0.3).float()
    X, Y, M = (az.pad_planes(t.to(dev), "replicate") for t in (x, y, m))
    sizes = [(h, w)] * B
    base = {"batch": B, "size": [h, w], "canvas": list(X.shape[2:]), "iters": args.iters}

    def loop():
        return torch.cat([ms_ssim(X[b:b + 1, :, :h, :w].contiguous(),
                                  Y[b:b + 1, :, :h, :w].contiguous(), data_range=1.0,
                                  size_average=False) for b in range(B)])

    def loop_masked():
        return torch.cat([mm.ms_ssim(X[b:b + 1, :, :h, :w].contiguous(),
                                     Y[b:b + 1, :, :h, :w].contiguous(),
                                     M[b:b + 1, :, :h, :w].contiguous(), data_range=1.0,
                                     size_average=False) for b in range(B)])

    _ab("ms_ssim", base, lambda: ms_ssim_any(X, Y, sizes), loop, args)
    _ab("masked_ms_ssim", base, lambda: masked_ms_ssim_any(X, Y, M, sizes), loop_masked, args)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=500)
    ap.add_argument("--width", type=int, default=375)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    a_ = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_any_bench: no GPU visible (there is no CPU path)")
    main(a_)
