"""Gradients of the HIP SSIM / MS-SSIM metrics (rgbac.metrics.ms_ssim_torch and
masked_ms_ssim_torch, backward in csrc/msssim_bwd.hip) against torch.autograd through the CPU
oracle restatement (oracle/ref_metrics.py).

Tolerance, self-calibrating: the oracle gradient is computed in fp64 (g64, with the fp32 window
widened to double) and in fp32 (g32).  With e_ref = max|g32 - g64| and e_gpu = max|g_gpu - g64|
the test requires e_gpu <= 8 * e_ref: the GPU path differs from the fp32 oracle only in fp32
summation order and in the e11 - m1^2 cancellation, so it lands within a small multiple of the
oracle's own rounding.  g64 is asserted finite and non-zero first; no element is excluded.
Inputs use noise 0.05 - 0.2, which keeps every level's cs positive in the oracle."""
import functools

import pytest
import torch

from oracle import ref_metrics as rm

pytestmark = pytest.mark.gpu


def _pair(B, C, H, W, seed, noise=0.05):
    g = torch.Generator().manual_seed(seed)
    X = torch.round(torch.rand((B, C, H, W), generator=g) * 255) / 255
    X = torch.nn.functional.avg_pool2d(X, 3, 1, 1)          # some spatial structure
    Y = torch.clamp(X + noise * torch.randn((B, C, H, W), generator=g), 0, 1)
    return X, Y


def _alpha(B, Cm, H, W, seed):
    """An alpha-like mask: an off-centre disc of full opacity, a soft rim, a few holes."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32),
                            torch.arange(W, dtype=torch.float32), indexing="ij")
    m = torch.empty((B, Cm, H, W))
    for b in range(B):
        cy, cx = H * (0.4 + 0.2 * b / max(B, 1)), W * 0.55
        r = torch.sqrt((yy - cy) ** 2 + (xx - cx) ** 2) / (0.45 * min(H, W))
        m[b] = torch.clamp(1.5 - r, 0, 1)
    holes = torch.rand((B, Cm, H, W), generator=g) < 0.02
    m[holes] = 0
    return m


def _upstream(B):
    """A non-uniform per-image upstream gradient."""
    return torch.linspace(0.5, 1.5, B) if B > 1 else torch.tensor([0.7])


def _oracle_grads(monkeypatch, fn, X, Y, up):
    """(g32, g64), each (dX, dY), of fn(X, Y) by torch.autograd on the CPU; fp64 with the
    oracle's fp32 window widened to double (the oracle itself is not edited)."""
    out = []
    orig = rm.fspecial_gauss_1d
    for dt in (torch.float32, torch.float64):
        with monkeypatch.context() as mp:
            if dt == torch.float64:
                mp.setattr(rm, "fspecial_gauss_1d", lambda size, sigma: orig(size, sigma).double())
            x = X.detach().clone().to(dt).requires_grad_()
            y = Y.detach().clone().to(dt).requires_grad_()
            v = fn(x, y, dt)
            v.backward(None if up is None else up.to(dt))
        out.append((x.grad, y.grad))
    return out


def _gpu_grads(fn, X, Y, up, device):
    x = X.detach().to(device).requires_grad_()
    y = Y.detach().to(device).requires_grad_()
    v = fn(x, y)
    assert v.grad_fn is not None
    v.backward(None if up is None else up.to(device))
    return x.grad.cpu(), y.grad.cpu()


def _compare(name, got, g32, g64):
    for which, g, r32, r64 in zip("XY", got, g32, g64):
        assert torch.isfinite(r64).all() and r64.abs().max().item() > 0, (name, which)
        assert torch.isfinite(g).all(), (name, which)
        e_ref = (r32.double() - r64).abs().max().item()
        e_gpu = (g.double() - r64).abs().max().item()
        print(f"{name} d{which}: e_gpu/e_ref = {e_gpu / e_ref:.3f}  (e_gpu {e_gpu:.3e}, e_ref "
              f"{e_ref:.3e}, e_ref/max|g64| {e_ref / r64.abs().max().item():.2e})")
        assert e_gpu <= 8 * e_ref, (name, which, e_gpu, e_ref)


# shape, noise, keyword arguments (weights as the oracle takes them: a tensor or None)
MS_CASES = [((1, 1, 161, 177), 0.05, {}),
            ((2, 3, 40, 49), 0.1, dict(weights=[0.3, 0.7])),
            ((1, 2, 33, 39), 0.2, dict(win_size=7, weights=[0.2, 0.3, 0.5]))]


def _ref_kw(kw, as_tensor):
    kw = dict(kw)
    if as_tensor and "weights" in kw:
        kw["weights"] = torch.tensor(kw["weights"], dtype=torch.float32)
    return kw


@pytest.mark.parametrize("size_average", [True, False])
@pytest.mark.parametrize("case", range(len(MS_CASES)))
def test_ms_ssim_grad(device, monkeypatch, case, size_average):
    from rgbac.metrics.ms_ssim_torch import ms_ssim
    shape, noise, kw = MS_CASES[case]
    X, Y = _pair(*shape, seed=sum(shape), noise=noise)
    up = None if size_average else _upstream(shape[0])
    rkw = _ref_kw(kw, True)
    g32, g64 = _oracle_grads(
        monkeypatch, lambda x, y, dt: rm.ms_ssim(x, y, data_range=1.0,
                                                 size_average=size_average, **rkw), X, Y, up)
    got = _gpu_grads(lambda x, y: ms_ssim(x, y, data_range=1.0, size_average=size_average, **kw),
                     X, Y, up, device)
    _compare(f"ms_ssim {shape} size_average={size_average}", got, g32, g64)


@pytest.mark.parametrize("win_size", [7, 11, 15])
def test_ssim_grad(device, monkeypatch, win_size):
    from rgbac.metrics.ms_ssim_torch import ssim
    shape = (2, 3, 64, 80)
    X, Y = _pair(*shape, seed=win_size, noise=0.1)
    up = _upstream(2)
    g32, g64 = _oracle_grads(
        monkeypatch, lambda x, y, dt: rm.ssim(x, y, win_size=win_size, data_range=1.0,
                                              size_average=False), X, Y, up)
    got = _gpu_grads(lambda x, y: ssim(x, y, win_size=win_size, data_range=1.0,
                                       size_average=False), X, Y, up, device)
    _compare(f"ssim win {win_size}", got, g32, g64)


MASK_CH = [1, 3, 1]          # mask channels per MS_CASES entry: 1, C, 1


@pytest.mark.parametrize("size_average", [True, False])
@pytest.mark.parametrize("case", range(len(MS_CASES)))
def test_masked_ms_ssim_grad(device, monkeypatch, case, size_average):
    from rgbac.metrics.masked_ms_ssim_torch import ms_ssim
    shape, noise, kw = MS_CASES[case]
    cm = MASK_CH[case]
    X, Y = _pair(*shape, seed=sum(shape) + 1, noise=noise)
    M = _alpha(shape[0], cm, shape[2], shape[3], seed=shape[2])
    up = None if size_average else _upstream(shape[0])
    g32, g64 = _oracle_grads(
        monkeypatch, lambda x, y, dt: rm.masked_ms_ssim(x, y, M.to(dt), data_range=1.0,
                                                        size_average=size_average, **kw),
        X, Y, up)
    Md = M.to(device)
    got = _gpu_grads(lambda x, y: ms_ssim(x, y, Md, data_range=1.0, size_average=size_average,
                                          **kw), X, Y, up, device)
    _compare(f"masked ms_ssim {shape} cm={cm} size_average={size_average}", got, g32, g64)
    off = (M <= 0).expand(shape)
    assert off.any()
    for g in got:
        assert (g[off] == 0.0).all()


def test_masked_ms_ssim_all_transparent(device):
    from rgbac.metrics.masked_ms_ssim_torch import ms_ssim
    X, Y = _pair(2, 3, 40, 49, seed=5, noise=0.1)
    x = X.to(device).requires_grad_()
    y = Y.to(device).requires_grad_()
    v = ms_ssim(x, y, torch.zeros((2, 1, 40, 49), device=device), data_range=1.0,
                weights=[0.3, 0.7])
    assert v.item() == 0.0
    v.backward()
    for g in (x.grad, y.grad):
        assert torch.isfinite(g).all() and (g == 0.0).all()


@pytest.mark.parametrize("nonnegative_ssim", [False, True])
def test_masked_ssim_grad(device, monkeypatch, nonnegative_ssim):
    from rgbac.metrics.masked_ms_ssim_torch import ssim
    shape = (2, 3, 64, 80)
    X, Y = _pair(*shape, seed=17, noise=0.1)
    M = _alpha(2, 1, 64, 80, seed=4)
    up = _upstream(2)
    g32, g64 = _oracle_grads(
        monkeypatch, lambda x, y, dt: rm.masked_ssim(x, y, M.to(dt), data_range=1.0,
                                                     size_average=False,
                                                     nonnegative_ssim=nonnegative_ssim),
        X, Y, up)
    Md = M.to(device)
    got = _gpu_grads(lambda x, y: ssim(x, y, Md, data_range=1.0, size_average=False,
                                       nonnegative_ssim=nonnegative_ssim), X, Y, up, device)
    _compare(f"masked ssim nonnegative={nonnegative_ssim}", got, g32, g64)


def _loss_fns(device):
    """name -> f(X, Y) for the four differentiable entry points, at fixed small arguments."""
    from rgbac.metrics import masked_ms_ssim_torch as mm
    from rgbac.metrics import ms_ssim_torch as pm
    M = _alpha(2, 1, 40, 49, seed=8).to(device)
    kw = dict(data_range=1.0, weights=[0.3, 0.7])
    return {
        "ms_ssim": lambda x, y: pm.ms_ssim(x, y, **kw),
        "ssim": lambda x, y: pm.ssim(x, y, data_range=1.0),
        "masked ms_ssim": lambda x, y: mm.ms_ssim(x, y, M, **kw),
        "masked ssim": lambda x, y: mm.ssim(x, y, M, data_range=1.0),
    }


def test_value_identical_with_and_without_grad(device):
    """With Y.requires_grad_() the value is bit-identical to the no-grad call's."""
    X, Y = _pair(2, 3, 40, 49, seed=21, noise=0.1)
    Xd, Yd = X.to(device), Y.to(device)
    for name, f in _loss_fns(device).items():
        plain = f(Xd, Yd)
        assert plain.grad_fn is None, name
        with_grad = f(Xd, Yd.clone().requires_grad_())
        assert with_grad.grad_fn is not None, name
        assert torch.equal(plain, with_grad.detach()), name
        with torch.no_grad():
            assert torch.equal(plain, f(Xd, Yd.clone().requires_grad_())), name
    from rgbac.metrics.ms_ssim_torch import ssim
    s, cs = ssim(Xd, Yd.clone().requires_grad_(), data_range=1.0, full=True)
    s0, cs0 = ssim(Xd, Yd, data_range=1.0, full=True)
    assert s.grad_fn is not None and cs.grad_fn is not None
    assert torch.equal(s.detach(), s0) and torch.equal(cs.detach(), cs0)


def test_backward_is_bit_reproducible(device):
    X, Y = _pair(2, 3, 40, 49, seed=22, noise=0.1)
    for name, f in _loss_fns(device).items():
        grads = []
        for _ in range(2):
            x = X.to(device).requires_grad_()
            y = Y.to(device).requires_grad_()
            f(x, y).backward()
            grads.append((x.grad, y.grad))
        assert torch.equal(grads[0][0], grads[1][0]), name
        assert torch.equal(grads[0][1], grads[1][1]), name
        assert grads[0][1].abs().max().item() > 0, name


@pytest.mark.parametrize("masked", [False, True])
def test_loss_and_backward_capture_in_a_graph(device, masked):
    """loss = 1 - ms_ssim(X, Y); loss.backward() captured in a HIP graph; new contents copied
    into Y and replayed give bitwise the eager gradient of the new contents."""
    fns = _loss_fns(device)
    f = fns["masked ms_ssim" if masked else "ms_ssim"]
    X, Y = _pair(2, 3, 40, 49, seed=23, noise=0.1)
    _, Y2 = _pair(2, 3, 40, 49, seed=23, noise=0.2)
    Xd = X.to(device)
    Yd = Y.to(device).requires_grad_()
    Y2d = Y2.to(device)

    def step():
        loss = 1 - f(Xd, Yd)
        loss.backward()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            Yd.grad = None
            step()
    torch.cuda.current_stream().wait_stream(side)
    Yd.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    with torch.no_grad():
        Yd.copy_(Y2d)
    graph.replay()
    torch.cuda.synchronize()
    got = Yd.grad.clone()
    Ye = Y2d.clone().requires_grad_()
    (1 - f(Xd, Ye)).backward()
    assert Ye.grad.abs().max().item() > 0
    assert torch.equal(got, Ye.grad)


# ---- the whole training step with the MS-SSIM distortion (trainRGB.py:183), as
# tests/test_gpu_train.py::test_rgb_train_step_grads does for the MSE one: B=2, 64x64, fp32,
# the same noise and half-transparent alpha, the same nrel metric and 1e-4 bar.  64x64 with two
# levels is the smallest frame the model accepts whose second level (32x32) holds the window.

def nrel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@functools.lru_cache(maxsize=None)
def _train_setup():
    """Inputs and the oracle forward (CPU, once for both loss variants)."""
    from oracle import ref_model as ref
    from rgbac.models.AutoEncoderRGB_Journal import AutoEncoder
    torch.manual_seed(234)
    net = AutoEncoder().train()
    g = torch.Generator().manual_seed(61)
    B, H, W = 2, 64, 64
    x = (torch.randint(0, 256, (B, 3, H, W), generator=g).float() / 255)
    a = torch.ones((B, 1, H, W))
    a[1, :, :, : W // 2] = 0
    me = ref.supply_mask(a)
    nz = torch.rand((B, 192, 1, 1), generator=g) - 0.5
    ny = torch.rand((B, 80, 8, 8), generator=g) - 0.5
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point())
          for k, v in net.state_dict().items()}
    xin = x * (a > 0)
    out = ref.rgb_forward(sd, xin, a, a, *me[:4], training=True, noise_z=nz, noise_y=ny)
    return dict(net=net, sd=sd, xin=xin, a=a, me=me, nz=nz, ny=ny, out=out)


@pytest.mark.parametrize("masked", [False, True])
def test_rgb_train_step_grads_ms_ssim_loss(device, masked):
    """rd_loss = 4096 * (1 - ms_ssim(x, x_hat)) + bpp backward: every parameter gradient of the
    HIP path against the oracle's autograd (oracle model -> ref_metrics on the CPU)."""
    from rgbac.metrics import masked_ms_ssim_torch as mm
    from rgbac.metrics import ms_ssim_torch as pm
    from rgbac.models.AutoEncoderRGB_Journal import AutoEncoder
    s = _train_setup()
    sd, out, xin, a = s["sd"], s["out"], s["xin"], s["a"]
    for v in sd.values():
        v.grad = None
    w = torch.tensor([0.3, 0.7])
    if masked:
        val = rm.masked_ms_ssim(xin, out[0], a, data_range=1.0, weights=[0.3, 0.7])
    else:
        val = rm.ms_ssim(xin, out[0], data_range=1.0, weights=w)
    (4096 * (1 - val) + out[2]).backward(retain_graph=True)
    netg = AutoEncoder().to(device).train()
    netg.load_state_dict(s["net"].state_dict())
    xg, ag_ = xin.to(device), a.to(device)
    meg = [t.to(device) for t in s["me"]]
    o = netg(xg, ag_, ag_, *meg[:4], noise_z=s["nz"].permute(0, 2, 3, 1).to(device),
             noise_y=s["ny"].permute(0, 2, 3, 1).to(device))
    if masked:
        got = mm.ms_ssim(xg, o[0], ag_, data_range=1.0, weights=[0.3, 0.7])
    else:
        got = pm.ms_ssim(xg, o[0], data_range=1.0, weights=[0.3, 0.7])
    print("ms_ssim value: gpu", got.item(), "oracle", val.item())
    assert torch.isfinite(val).all()
    (4096 * (1 - got) + o[2]).backward()
    bad, errs = [], []
    for n, p in netg.named_parameters():
        r = sd[n].grad
        if r is None or r.abs().max() == 0:
            continue
        e = nrel(p.grad, r)
        errs.append((e, n))
        if not e <= 1e-4:
            bad.append((n, e))
    errs.sort()
    assert errs
    print("rgb codec grads, ms-ssim loss, masked =", masked, ": median rel",
          errs[len(errs) // 2], "max", errs[-3:])
    assert not bad, bad[:10]
