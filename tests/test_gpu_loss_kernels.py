"""Element-wise reference tests of the entropy, loss and activation-backward kernels:
GaussFn (rgbac_gaussian_slice / rgbac_gaussian_bwd), EBFn (rgbac_eb_forward / rgbac_eb_bwd),
MSEFn (rgbac_finalize / rgbac_mse_bwd), rgbac_act_bwd (generic, flat bf16 and the fast GELU
derivative) and the helpers rgbac_pixel_shuffle, rgbac_colsum, rgbac_sum_partials.

Every kernel here loads, computes in fp32 and stores one element at a time, so on the same
(bf16-representable, in bf16 mode) inputs an fp64 reference predicts each output element to
fp32 rounding plus, in bf16, one output rounding.  The reference is oracle/ref_model.py run in
fp64 (g64) and in fp32 (g32), or the closed-form derivative for rgbac_act_bwd.  With

    E(a) = max_i |a_i - g64_i| / (|g64_i| + 1e-3 * max|g64|)      (no element excluded)

the tests require E(gpu) <= 8 * E(g32) for fp32 results and E(gpu) <= 8 * E(g32) + 2^-8 for
results stored as bf16 (half an ulp is 2^-9 relative, with a factor of 2); results a bf16-mode
kernel stores as fp32 (likelihoods, bits, parameter gradients) keep the fp32 bar.  Where
E(g32) is exactly 0 (copies, selects) that means equality in fp32 and 2^-8 in bf16.  g64 is
asserted finite and non-zero first; a reference gradient that is identically zero (dmu in
dequantize mode, the median gradient in noise mode) demands exact zeros.  Parameter gradients
of the entropy bottleneck are compared norm-wise, ||g - g64|| / ||g64||, under the same 8x rule.

Input conditions, asserted on the CPU against the reference alone: no y - mu (z - median) within
1e-3 of a half-integer and no ReLU / LeakyReLU input within 1e-3 of 0 (such elements are
nudged, not masked); the fp32 and fp64 oracles take the same likelihood-clamp decision on every
element and no fp64 likelihood lies within 1 % of the 1e-9 bound; between 2 % and 30 % of the
Gaussian elements are clamped (scale under the bound, or likelihood at its bound).

Worst measured figures per kernel and dtype (MI355X).  fp32 column, and every result stored
as fp32: E(gpu) / E(g32), bar 8.  bf16 column, results stored as bf16: E(gpu) / bound, bar 1 (the
2^-8 term dominates there; one correct rounding of a value just above a power of two costs
2^-8 relative, so figures close to 1 are honest rounding).  "=": E(g32) is 0 and the result is
bit-equal to the reference.

    tensor                                   fp32     bf16
    gaussian hat                             1.00 (bit-equal to g32)   0.98
    gaussian lik (stored fp32)               1.07     1.02 (E/E32)
    gaussian dy / dmu / dsigma, noise        2.77 / 0.94 / 1.00        0.92 / 0.97 / 0.95
    gaussian dy / dsigma, dequantize         = / 2.72                  = / 0.95
    gaussian long forward  hat / lik         1.00 / 1.02
    gaussian long backward dy / dmu / dsigma 1.04 / 0.90 / 0.98
    eb z_hat                                 =        0.27
    eb dz, noise (dequantize: =)             1.06     0.98
    eb raw parameter gradients (norm-wise)   1.52     1.24 (stored fp32)
    eb quantiles gradient (norm-wise)        1.38     1.53 (stored fp32)
    mse dx_hat                               1.00     0.99
    act_bwd none, relu, masksel, dr1 copies  =        =
    act_bwd gelu dz                          0.62     0.93 (fast derivative, flat and generic)
    act_bwd lrelu / tanh_half / gate dz      1.00 / 1.00 / 1.00        0.79 / 0.85 / 0.88
    act_bwd gate dr1                         1.00     0.99
    act_bwd gdn dz / dr1                     1.12 / 1.23               0.93 / 0.98
    act_bwd igdn dz / dr1                    0.97 / 1.02               0.96 / 0.98

No bar was raised above 8x.  The bf16 GELU allowance (1.5e-7 * |g|) is far below the bf16 output
rounding, so that case bounds the fast derivative at the bf16 level only; it was not needed.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import ref_model as ref

pytestmark = pytest.mark.gpu

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
DTYPES = [F32, BF16]
BF16_EPS = 2.0 ** -8
NAN = float("nan")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rt():
    from rgbac import runtime as rt
    return rt


def _rnd(t, dtype):
    """The value the kernel sees: rounded to bf16 in bf16 mode (kept as fp32 on the CPU)."""
    return t.to(BF16).float() if dtype == BF16 else t


# --------------------------------------------------------------------------
# the comparison
# --------------------------------------------------------------------------
def _E(a, g64):
    den = g64.abs() + 1e-3 * g64.abs().max()
    return ((a.double() - g64).abs() / den).max().item()


def _check(name, g, g32, g64, lowp, factor=8.0, extra=None):
    """E(g) <= factor * E(g32) (+ 2^-8 when the result was stored as bf16), asserted per
    element; ``extra``: an absolute per-element allowance added to the bound."""
    g, g32, g64 = (t.detach().double().cpu() for t in (g, g32, g64))
    assert g.shape == g64.shape == g32.shape, (name, g.shape, g64.shape)
    assert torch.isfinite(g64).all() and g64.abs().max().item() > 0, name
    assert torch.isfinite(g).all(), name
    den = g64.abs() + 1e-3 * g64.abs().max()
    e_ref = _E(g32, g64)
    err = (g - g64).abs()
    e_gpu = (err / den).max().item()
    bound = factor * e_ref + (BF16_EPS if lowp else 0.0)
    ratio = e_gpu / e_ref if e_ref > 0 else (0.0 if e_gpu == 0 else float("inf"))
    print(f"{name}: E(gpu)/E(g32) = {ratio:.3f}  (E(gpu) {e_gpu:.3e}, E(g32) {e_ref:.3e}, "
          f"bound {bound:.3e}, E(gpu)/bound {e_gpu / bound if bound > 0 else 0.0:.3f})")
    allow = bound * den if extra is None else bound * den + extra.double().cpu()
    bad = err > allow
    assert not bad.any(), (name, int(bad.sum()), e_gpu, e_ref, bound)
    return ratio


def _check_zero(name, g):
    """The reference is identically zero: so is the result (or it is absent)."""
    assert g is None or not g.detach().cpu().any(), name


def _check_norm(name, g, g32, g64, factor=8.0):
    g, g32, g64 = (t.detach().double().cpu() for t in (g, g32, g64))
    assert torch.isfinite(g64).all() and g64.norm().item() > 0, name
    assert torch.isfinite(g).all(), name
    n_ref = ((g32 - g64).norm() / g64.norm()).item()
    n_gpu = ((g - g64).norm() / g64.norm()).item()
    ratio = n_gpu / n_ref if n_ref > 0 else (0.0 if n_gpu == 0 else float("inf"))
    print(f"{name}: norm-wise gpu/g32 = {ratio:.3f}  (gpu {n_gpu:.3e}, g32 {n_ref:.3e})")
    assert n_gpu <= factor * n_ref, (name, n_gpu, n_ref)
    return ratio


def _untie(t, base, dtype, step=0.25):
    """Nudge (in place) the elements of t whose t - base lies within 1e-3 of a half-integer;
    the step is a multiple of the bf16 spacing below 64.  Returns how many were nudged."""
    nudged = 0
    for _ in range(4):
        d = t.double() - base.double()
        bad = ((d - torch.floor(d)) - 0.5).abs() < 1e-3
        if not bad.any():
            break
        nudged += int(bad.sum())
        t[bad] = _rnd(t[bad] + step, dtype)
    d = t.double() - base.double()
    assert not (((d - torch.floor(d)) - 0.5).abs() < 1e-3).any()
    assert t.abs().max().item() < 64
    return nudged


# --------------------------------------------------------------------------
# 1. Gaussian conditional
# --------------------------------------------------------------------------
LIK_BOUND = 1e-9
SCALE_BOUND = torch.tensor([0.11], dtype=F32).item()        # gc_forward's fp32 bound
SCALE_LO, SCALE_HI = 0.10986328125, 0.1103515625            # its two bf16 neighbours


def _raw_lik64(x, mu, sc):
    """The unclamped fp64 likelihood of the quantised value x (the oracle's own pieces)."""
    v = (x.double() - mu.double()).abs()
    s = torch.clamp(sc.double(), min=SCALE_BOUND)
    return ref._std_cumulative((0.5 - v) / s) - ref._std_cumulative((-0.5 - v) / s)


def _quantised(y, mu, noise):
    if noise is not None:
        return y + noise
    return torch.round(y.double() - mu.double()) + mu.double()


def _gauss_inputs(shape, dtype, noisy, seed, plants):
    """y, mu, scale, noise, upstream a -- element-wise tensors of ``shape`` (fp32 on the CPU,
    bf16-representable in bf16 mode; the noise stays fp32, as the kernel reads it)."""
    g = _gen(seed)
    y = torch.randn(shape, generator=g) * 1.5
    mu = torch.randn(shape, generator=g) * 0.5
    sc = 0.06 + 1.5 * torch.rand(shape, generator=g) ** 2         # ~18 % under the bound
    noise = (torch.rand(shape, generator=g) - 0.5) if noisy else None
    a = torch.randn(shape, generator=g)
    idx = {}
    if plants:
        n = y.numel()
        fy, fm, fs = y.view(-1), mu.view(-1), sc.view(-1)
        k = torch.arange(40)
        idx = {"edge": 11 + 641 * k, "low": 7 + 641 * k, "tail": 3 + 641 * k, "eq": 13 + 641 * k}
        assert all(int(v.max()) < n for v in idx.values())
        assert len(torch.cat(list(idx.values())).unique()) == 160
        fs[idx["edge"][:20]] = SCALE_LO
        fs[idx["edge"][20:]] = SCALE_HI
        fs[idx["low"][:20]] = 0.02
        fs[idx["low"][20:]] = 0.05
        sgn = torch.where(k % 2 == 0, 1.0, -1.0)
        far = 1.0 + (8.0 + 0.5 * (k % 8)) * torch.clamp(fs[idx["tail"]], min=0.11)
        far[::5] = 24.0
        fy[idx["tail"]] = fm[idx["tail"]] + sgn * far
    y, mu, sc, a = (_rnd(t, dtype) for t in (y, mu, sc, a))
    if plants:
        y.view(-1)[idx["eq"]] = mu.view(-1)[idx["eq"]]            # y == mu exactly
    for _ in range(4):
        _untie(y, mu, dtype)
        # a likelihood within 1 % of its bound moves one step further into the tail
        near = (_raw_lik64(_quantised(y, mu, noise), mu, sc) / LIK_BOUND - 1).abs() < 1e-2
        if not near.any():
            break
        y[near] = _rnd(y[near] + torch.where(y[near] >= mu[near], 1.0, -1.0), dtype)
    return y, mu, sc, noise, a, idx


def _gauss_oracle(y, mu, sc, noise, a, dt, cs=(0.01, -0.01)):
    """The oracle on one dtype: hat, lik, bits, the clamp decision and, per sign of the
    bits gradient c, (dy, dmu, dsigma) of bits * c + (hat * a).sum()."""
    yl, ml, sl = (t.detach().clone().to(dt).requires_grad_() for t in (y, mu, sc))
    nz = None if noise is None else noise.to(dt)
    _, lik = ref.gc_forward(yl, sl, ml, noise is not None, nz)
    hat = ref.ste_round(yl - ml) + ml
    bits = ref._bits(lik)
    out = dict(hat=hat.detach(), lik=lik.detach(), bits=bits.item(),
               clamped=lik.detach() <= torch.tensor(LIK_BOUND, dtype=dt), grads={})
    for c in cs:
        for t in (yl, ml, sl):
            t.grad = None
        (bits * c + (hat * a.to(dt)).sum()).backward(retain_graph=True)
        out["grads"][c] = (yl.grad.clone(), ml.grad.clone(), sl.grad.clone())
    return out


def _gauss_conditions(y, mu, sc, noise, o32, o64, idx):
    raw = _raw_lik64(_quantised(y, mu, noise), mu, sc)
    assert torch.equal(o32["clamped"], o64["clamped"]), \
        int((o32["clamped"] != o64["clamped"]).sum())
    assert torch.equal(o64["clamped"], raw <= LIK_BOUND)
    assert not ((raw / LIK_BOUND - 1).abs() < 1e-2).any()
    b64 = -torch.log(o64["lik"] + 1e-10) / 0.6931471805599453
    assert (b64 > 1e-7).all() and (b64 < 49).all()        # the bits clamp(0, 50) is never live
    share = ((sc < SCALE_BOUND) | o64["clamped"]).double().mean().item()
    n_lik = int(o64["clamped"].sum())
    print(f"gaussian inputs: {share:.1%} clamped ({n_lik} at the likelihood bound)")
    assert 0.02 <= share <= 0.30, share
    if idx:
        assert n_lik >= 40
        assert (raw.view(-1)[idx["tail"]] < 1e-10).all()
        assert (sc.view(-1)[idx["edge"][:20]] == SCALE_LO).all()
        assert (sc.view(-1)[idx["edge"][20:]] == SCALE_HI).all()
        assert SCALE_LO < SCALE_BOUND < SCALE_HI
        assert (sc.view(-1)[idx["low"]] < 0.06).all()
        assert (y.view(-1)[idx["eq"]] == mu.view(-1)[idx["eq"]]).all()


GAUSS_SHAPE = (3, 8, 37, 29)          # 25 752 elements: 100 blocks and a ragged one
GAUSS_M, GAUSS_COFF = 24, 8


@functools.lru_cache(maxsize=None)
def _gauss_case(lowp, noisy):
    dtype = BF16 if lowp else F32
    y, mu, sc, noise, a, idx = _gauss_inputs(GAUSS_SHAPE, dtype, noisy, 300 + 2 * lowp + noisy,
                                             True)
    o32 = _gauss_oracle(y, mu, sc, noise, a, F32)
    o64 = _gauss_oracle(y, mu, sc, noise, a, F64)
    _gauss_conditions(y, mu, sc, noise, o32, o64, idx)
    B, cs, H, W = GAUSS_SHAPE
    y24 = _rnd(torch.randn((B, GAUSS_M, H, W), generator=_gen(5)), dtype)
    y24[:, GAUSS_COFF:GAUSS_COFF + cs] = y
    return dict(y24=y24, mu=mu, sc=sc, noise=noise, a=a, o32=o32, o64=o64)


def _nhwc_f32(x, device):
    return None if x is None else x.permute(0, 2, 3, 1).contiguous().to(device)


def _gslice(dtype, y_t, coff, cs, mu_t, sc_t, nz):
    """rgbac_gaussian_slice called directly on NHWC tensors, hat and lik pre-filled with NaN
    -> (hat fp32, lik as (B, H, W, cs), the fp64 partial sums of the bits)."""
    from rgbac import _lib
    dev = y_t.device
    npix = y_t.shape[0] * y_t.shape[1] * y_t.shape[2]
    hat = torch.full_like(mu_t, NAN)
    lik = torch.full(tuple(mu_t.shape[:3]) + (cs,), NAN, dtype=F32, device=dev)
    part = torch.full((_lib.load().rgbac_reduce_blocks(npix * cs),), NAN, dtype=F64, device=dev)
    _lib.call("rgbac_gaussian_slice", _lib.dtype_code(dtype), npix, cs,
              y_t.data_ptr() + coff * y_t.element_size(), y_t.shape[3], mu_t.data_ptr(),
              mu_t.shape[3], sc_t.data_ptr(), sc_t.shape[3], _lib.ptr(nz), hat.data_ptr(),
              hat.shape[3], lik.data_ptr(), part.data_ptr(), _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return hat.float().cpu(), lik.cpu(), part.cpu()


def _gbwd(dtype, y_t, coff, cs, mu_t, sc_t, nz, c, dh_t):
    """rgbac_gaussian_bwd called directly, every output pre-filled with NaN."""
    from rgbac import _lib
    dev = y_t.device
    npix = y_t.shape[0] * y_t.shape[1] * y_t.shape[2]
    dy, dmu, dsc = (torch.full_like(t, NAN) for t in (y_t, mu_t, sc_t))
    gb = torch.tensor([c], dtype=F32, device=dev)
    _lib.call("rgbac_gaussian_bwd", _lib.dtype_code(dtype), npix, cs,
              y_t.data_ptr() + coff * y_t.element_size(), y_t.shape[3], mu_t.data_ptr(),
              mu_t.shape[3], sc_t.data_ptr(), sc_t.shape[3], _lib.ptr(nz), gb.data_ptr(),
              dh_t.data_ptr(), dh_t.shape[3], dy.data_ptr() + coff * dy.element_size(),
              dy.shape[3], dmu.data_ptr(), dmu.shape[3], dsc.data_ptr(), dsc.shape[3],
              _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return dy.float().cpu(), dmu.float().cpu(), dsc.float().cpu()


@pytest.mark.parametrize("noisy", [True, False], ids=["noise", "dequantize"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_gaussian_conditional(device, dtype, noisy):
    """GaussFn on an 8-channel slice at channel 8 of a 24-channel y: hat, the likelihood map,
    bits and (dy, dmu, dsigma) for both signs of the bits gradient (the likelihood LowerBound
    passes it for one and blocks it for the other), element by element against the fp64
    oracle; the other 16 channels of dy stay untouched."""
    from rgbac import autograd as ag
    rt = _rt()
    lowp = dtype == BF16
    s = _gauss_case(lowp, noisy)
    o32, o64 = s["o32"], s["o64"]
    B, cs, H, W = GAUSS_SHAPE
    co = GAUSS_COFF
    tag = f"gauss {'bf16' if lowp else 'f32'} {'noise' if noisy else 'dequantize'}"
    nz = _nhwc_f32(s["noise"], device)
    ga = rt.to_nhwc(s["a"].to(device), dtype)
    fy = rt.to_nhwc(s["y24"].to(device), dtype)
    fmu, fsc = rt.to_nhwc(s["mu"].to(device), dtype), rt.to_nhwc(s["sc"].to(device), dtype)
    assert (fy.ldc, fmu.ldc, fsc.ldc) == (GAUSS_M, cs, cs)

    # forward, entry point called directly with the likelihood map requested
    hat, lik, part = _gslice(dtype, fy.t, co, cs, fmu.t, fsc.t, nz)
    hat, lik = hat.permute(0, 3, 1, 2), lik.permute(0, 3, 1, 2)
    _check(f"{tag} hat", hat, o32["hat"], o64["hat"], lowp)
    if not lowp:
        assert torch.equal(hat, o32["hat"])
    _check(f"{tag} lik", lik, o32["lik"], o64["lik"], False)
    assert torch.equal(lik <= torch.tensor(LIK_BOUND, dtype=F32), o64["clamped"])
    assert abs(part.sum().item() - o64["bits"]) <= 1e-6 * o64["bits"]

    for c in (0.01, -0.01):
        for t in (fy.t, fmu.t, fsc.t):
            t.grad = None
            t.requires_grad_(True)
        h, bits = ag.gauss_t(fy, co, fmu, fsc, nz)
        assert torch.equal(h.t.detach().float().cpu().permute(0, 3, 1, 2), hat)
        assert abs(bits.item() - o64["bits"]) <= 1e-6 * o64["bits"]
        torch.autograd.backward([h.t, bits], [ga.t, torch.tensor(c, device=device)])
        dy = rt.to_nchw(rt.Feat(fy.t.grad, GAUSS_M)).cpu()
        dmu = rt.to_nchw(rt.Feat(fmu.t.grad, cs)).cpu()
        dsc = rt.to_nchw(rt.Feat(fsc.t.grad, cs)).cpu()
        r32, r64 = o32["grads"][c], o64["grads"][c]
        _check(f"{tag} c={c:+} dy", dy[:, co:co + cs], r32[0], r64[0], lowp)
        assert not dy[:, :co].any() and not dy[:, co + cs:].any()
        if noisy:
            _check(f"{tag} c={c:+} dmu", dmu, r32[1], r64[1], lowp)
        else:
            assert not r64[1].any()          # x - mu does not depend on mu
            _check_zero(f"{tag} dmu", dmu)
        _check(f"{tag} c={c:+} dsigma", dsc, r32[2], r64[2], lowp)
        # the backward entry point itself writes its slice and nothing else
        with torch.no_grad():
            ny, nmu, nsc = _gbwd(dtype, fy.t, co, cs, fmu.t, fsc.t, nz, c, ga.t)
        other = torch.ones(GAUSS_M, dtype=torch.bool)
        other[co:co + cs] = False
        assert torch.isnan(ny[..., other]).all()
        assert torch.equal(ny[..., co:co + cs].permute(0, 3, 1, 2), dy[:, co:co + cs])
        assert torch.equal(nmu.permute(0, 3, 1, 2), dmu)
        assert torch.equal(nsc.permute(0, 3, 1, 2), dsc)


def _halves(t, h0):
    return [None, None] if t is None else [t[:, :h0].contiguous(), t[:, h0:].contiguous()]


def test_gaussian_slice_grid_stride(device):
    """gaussian_slice_kernel past its 1024-block cap ((1, 8, 257, 128): 263 168 elements, the
    last 1024 on a second trip of the grid-stride loop): bit-equal to the two halves run
    without the loop, and element-wise against fp64."""
    H, W, cs = 257, 128, 8
    assert H * W * cs > 1024 * 256 and (H // 2 + 1) * W * cs <= 1024 * 256
    y, mu, sc, noise, a, _ = _gauss_inputs((1, H, W, cs), F32, True, 41, False)
    o32 = _gauss_oracle(y, mu, sc, noise, a, F32, cs=())
    o64 = _gauss_oracle(y, mu, sc, noise, a, F64, cs=())
    _gauss_conditions(y, mu, sc, noise, o32, o64, {})
    yd, md, sd, nd = (t.to(device) for t in (y, mu, sc, noise))
    hat, lik, part = _gslice(F32, yd, 0, cs, md, sd, nd)
    assert part.numel() == 1024
    parts = [_gslice(F32, *ts) for ts in zip(_halves(yd, H // 2), (0, 0), (cs, cs),
                                             _halves(md, H // 2), _halves(sd, H // 2),
                                             _halves(nd, H // 2))]
    assert torch.equal(hat, torch.cat([p[0] for p in parts], 1))
    assert torch.equal(lik, torch.cat([p[1] for p in parts], 1))
    split_bits = sum(p[2].sum().item() for p in parts)
    assert abs(part.sum().item() - split_bits) <= 1e-12 * split_bits
    assert torch.equal(hat, o32["hat"])
    _check("gauss long fwd hat", hat, o32["hat"], o64["hat"], False)
    _check("gauss long fwd lik", lik, o32["lik"], o64["lik"], False)
    assert abs(part.sum().item() - o64["bits"]) <= 1e-6 * o64["bits"]


def test_gaussian_bwd_grid_stride(device):
    """gaussian_bwd_kernel past its 8192-block cap ((1, 8, 513, 512): 2 101 248 elements, the
    last 4096 on a second trip): bit-equal to the two halves run without the loop, and
    element-wise against fp64."""
    H, W, cs = 513, 512, 8
    assert H * W * cs > 8192 * 256 and (H // 2 + 1) * W * cs <= 8192 * 256
    y, mu, sc, noise, a, _ = _gauss_inputs((1, H, W, cs), F32, True, 43, False)
    c = 0.01
    o32 = _gauss_oracle(y, mu, sc, noise, a, F32, cs=(c,))
    o64 = _gauss_oracle(y, mu, sc, noise, a, F64, cs=(c,))
    _gauss_conditions(y, mu, sc, noise, o32, o64, {})
    yd, md, sd, nd, ad = (t.to(device) for t in (y, mu, sc, noise, a))
    got = _gbwd(F32, yd, 0, cs, md, sd, nd, c, ad)
    parts = [_gbwd(F32, ts[0], 0, cs, ts[1], ts[2], ts[3], c, ts[4])
             for ts in zip(*(_halves(t, H // 2) for t in (yd, md, sd, nd, ad)))]
    for k, name in enumerate(("dy", "dmu", "dsigma")):
        assert torch.equal(got[k], torch.cat([p[k] for p in parts], 1)), name
        _check(f"gauss long bwd {name}", got[k], o32["grads"][c][k], o64["grads"][c][k], False)


# --------------------------------------------------------------------------
# 2. Entropy bottleneck
# --------------------------------------------------------------------------
EB_C = 16
EB_SHAPES = [(3, EB_C, 19, 23), (1, EB_C, 1, 3)]      # npix 1311: six trips, ragged; npix 3


@functools.lru_cache(maxsize=None)
def _eb_module():
    """EntropyBottleneck(16) with the parameter perturbation of
    test_gpu_train.test_entropy_bottleneck_grads, and medians off zero (multiples of 1/8, so
    bf16 holds z - median exactly where it holds z)."""
    from rgbac.entropy import EntropyBottleneck
    g = _gen(41)
    with torch.random.fork_rng(devices=[]):       # the biases draw from the global generator
        torch.manual_seed(41)
        eb = EntropyBottleneck(EB_C)
    with torch.no_grad():
        for n, p in eb.named_parameters():
            if n.startswith("_factor"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)
            elif n.startswith("_matrix"):
                p.add_(torch.randn(p.shape, generator=g) * 0.3)
        eb.quantiles[:, 0, 1] = torch.randint(-8, 9, (EB_C,), generator=g).float() / 8
    return eb


def _eb_oracle(eb, z, noise, a, dt, cs=(0.01, -0.01)):
    sd = {"eb." + k: v.detach().clone().to(dt).requires_grad_(v.is_floating_point())
          for k, v in eb.state_dict().items()}
    zl = z.detach().clone().to(dt).requires_grad_()
    nz = None if noise is None else noise.to(dt)
    _, lik = ref.eb_forward(zl, sd, "eb", noise is not None, nz)
    med = ref.eb_medians(sd, "eb").reshape(1, EB_C, 1, 1)
    zh = ref.ste_round(zl - med) + med
    bits = ref._bits(lik)
    out = dict(zh=zh.detach(), lik=lik.detach(), bits=bits.item(),
               clamped=lik.detach() <= torch.tensor(LIK_BOUND, dtype=dt), grads={})
    for c in cs:
        zl.grad = None
        for v in sd.values():
            v.grad = None
        (bits * c + (zh * a.to(dt)).sum()).backward(retain_graph=True)
        out["grads"][c] = (zl.grad.clone(),
                           {k[3:]: (None if v.grad is None else v.grad.clone())
                            for k, v in sd.items() if v.requires_grad})
    return out


EB_TAILS = (-480.0, 480.0, -352.0, 416.0)


@functools.lru_cache(maxsize=None)
def _eb_case(lowp, noisy, which):
    dtype = BF16 if lowp else F32
    shape = EB_SHAPES[which]
    eb = _eb_module()
    g = _gen(500 + 4 * which + 2 * lowp + noisy)
    z = torch.randn(shape, generator=g) * 3
    noise = (torch.rand(shape, generator=g) - 0.5) if noisy else None
    a = _rnd(torch.randn(shape, generator=g), dtype)
    tails = torch.zeros(shape, dtype=torch.bool)
    if which == 0:                                  # a few far-tail elements
        fz, ft = z.view(-1), tails.view(-1)
        pos = 17 + 1999 * torch.arange(len(EB_TAILS))
        fz[pos] = torch.tensor(EB_TAILS)
        ft[pos] = True
    z = _rnd(z, dtype)
    med = eb.quantiles.detach()[:, 0, 1].reshape(1, EB_C, 1, 1).expand(shape)
    near = ~tails
    zn = z[near]
    _untie(zn, med[near], dtype)
    z[near] = zn
    d = z.double() - med.double()
    assert not (((d - torch.floor(d)) - 0.5).abs() < 1e-3).any()
    o32 = _eb_oracle(eb, z, noise, a, F32)
    o64 = _eb_oracle(eb, z, noise, a, F64)
    # the clamp decision: the same in both oracles, on the planted tails in particular
    assert torch.equal(o32["clamped"], o64["clamped"])
    assert o64["clamped"][tails].all() and int(o64["clamped"].sum()) == int(tails.sum())
    b64 = -torch.log(o64["lik"] + 1e-10) / 0.6931471805599453
    assert (b64 > 1e-7).all() and (b64 < 49).all()
    return dict(eb=eb, z=z, noise=noise, a=a, o32=o32, o64=o64)


@pytest.mark.parametrize("which", [0, 1], ids=["3x16x19x23", "1x16x1x3"])
@pytest.mark.parametrize("noisy", [True, False], ids=["noise", "dequantize"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_entropy_bottleneck(device, dtype, noisy, which):
    """EBFn with npix = 1311 (six trips of the per-channel pixel loop, the last ragged, all
    four waves live in the parameter-gradient reduction) and npix = 3 (most threads idle):
    z_hat, bits, dz element-wise and every raw parameter gradient norm-wise against the fp64
    oracle; in dequantize mode that includes the median (quantiles) gradient."""
    from rgbac import autograd as ag
    from rgbac.entropy import EntropyBottleneck
    from rgbac.train_forward import eb_params_t
    rt = _rt()
    lowp = dtype == BF16
    s = _eb_case(lowp, noisy, which)
    o32, o64 = s["o32"], s["o64"]
    tag = (f"eb {'bf16' if lowp else 'f32'} {'noise' if noisy else 'dequantize'} "
           f"{tuple(EB_SHAPES[which])}")
    ebg = EntropyBottleneck(EB_C).to(device)
    ebg.load_state_dict(s["eb"].state_dict())
    nz = _nhwc_f32(s["noise"], device)
    ga = rt.to_nhwc(s["a"].to(device), dtype)
    for c in (0.01, -0.01):
        fz = rt.to_nhwc(s["z"].to(device), dtype)
        assert fz.ldc == EB_C
        fz.t.requires_grad_(True)
        for p in ebg.parameters():
            p.grad = None
        zh_t, bits = ag.EBFn.apply(fz.t, EB_C, eb_params_t(ebg), nz)
        zh = rt.to_nchw(rt.Feat(zh_t.detach(), EB_C)).cpu()
        _check(f"{tag} z_hat", zh, o32["zh"], o64["zh"], lowp)
        assert abs(bits.item() - o64["bits"]) <= 1e-6 * o64["bits"]
        torch.autograd.backward([zh_t, bits], [ga.t, torch.tensor(c, device=device)])
        r32, r64 = o32["grads"][c], o64["grads"][c]
        _check(f"{tag} c={c:+} dz", rt.to_nchw(rt.Feat(fz.t.grad, EB_C)).cpu(), r32[0], r64[0],
               lowp)
        seen = 0
        for n, p in ebg.named_parameters():
            want = r64[1][n]
            if n == "quantiles" and noisy:
                assert want is None or not want.any()
                _check_zero(f"{tag} {n}", p.grad)
                continue
            assert want is not None, n
            _check_norm(f"{tag} c={c:+} {n}", p.grad, r32[1][n], want)
            seen += 1
        assert seen == (14 if noisy else 15)
        if not noisy:
            q = ebg.quantiles.grad.cpu()
            assert q[:, 0, 1].abs().max().item() > 0 and not q[:, 0, 0].any() and \
                not q[:, 0, 2].any()


# --------------------------------------------------------------------------
# 3. MSE
# --------------------------------------------------------------------------
MSE_CASES = [(3, 33, 29), (1, 130, 127)]       # HW 957; HW 16 510 > 64 * 256: a second trip


@functools.lru_cache(maxsize=None)
def _mse_case(lowp, which):
    dtype = BF16 if lowp else F32
    B, H, W = MSE_CASES[which]
    g = _gen(700 + 2 * which + lowp)
    x = torch.round(torch.rand((B, 3, H, W), generator=g) * 255) / 255
    xh = _rnd(x + 0.1 * torch.randn((B, 3, H, W), generator=g), dtype)
    mask = (torch.rand((B, 1, H, W), generator=g) > 0.3).float()
    if B > 1:
        mask[1] = 0.0                                                  # cnt = 0
        mask[2] = torch.rand((1, H, W), generator=g) * (mask[2] > 0)   # fractional alpha
        assert ((mask[2] > 0) & (mask[2] < 1)).sum() > 100 and (mask[2] == 0).any()
    else:
        mask[0, 0, :, ::7] = 0.25
    refs = {}
    for mode in (0, 1):
        for dt in (F32, F64):
            h = xh.detach().clone().to(dt).requires_grad_()
            if mode == 0:
                v = ref.reconstruct_error(x.to(dt), h, mask.to(dt))
            else:
                v = F.mse_loss(h, x.to(dt))
            (v * 4096.0).backward()
            refs[(mode, dt)] = (v.item(), h.grad)
    return dict(x=x, xh=xh, mask=mask, refs=refs)


@pytest.mark.parametrize("ld", [4, 8])
@pytest.mark.parametrize("which", [0, 1], ids=["3x33x29", "1x130x127"])
@pytest.mark.parametrize("mode", [0, 1], ids=["masked", "plain"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_mse(device, dtype, mode, which, ld):
    """MSEFn value and dx_hat (cx = 3 in rows of 4 and 8) against reconstruct_error / plain
    MSE in fp64: an image with an all-zero mask (cnt = 0 -> max(cnt, 1)), one with fractional
    alpha (the rule is mask > 0), and more than 16 384 pixels (second trip of the backward's
    pixel loop); the pad channels of the gradient come back as zeros from a NaN-filled
    buffer.  The value is a fp64 sum of fp32 squares rounded once per image: 1e-6 relative."""
    from rgbac import _lib
    from rgbac import autograd as ag
    rt = _rt()
    lowp = dtype == BF16
    s = _mse_case(lowp, which)
    B, H, W = MSE_CASES[which]
    tag = f"mse {'bf16' if lowp else 'f32'} mode {mode} {MSE_CASES[which]} ld {ld}"
    x, mask = s["x"].to(device), s["mask"].to(device)
    xh = rt.to_nhwc(s["xh"].to(device), dtype, ldc=ld)
    xh.t[..., 3:] = NAN                                  # the pad channels are never read
    v32, g32 = s["refs"][(mode, F32)]
    v64, g64 = s["refs"][(mode, F64)]
    xh.t.requires_grad_(True)
    v = ag.MSEFn.apply(xh.t, 3, x, mask, mode)
    assert v64 > 0 and abs(v.item() - v64) <= 1e-6 * v64, (v.item(), v64)
    (v * 4096.0).backward()
    dx = xh.t.grad
    assert dx.shape[3] == ld and not dx[..., 3:].any()
    got = rt.to_nchw(rt.Feat(dx, 3)).cpu()
    _check(f"{tag} dx_hat", got, g32, g64, lowp)
    if mode == 0 and B > 1:
        assert not g64[1].any() and not got[1].any()
    # the entry points directly, the gradient buffer pre-filled with NaN
    scratch = torch.empty(_lib.finalize_scratch_doubles(B, H, W), dtype=F64, device=device)
    zero = torch.zeros(1, dtype=F64, device=device)
    out = torch.empty(4, dtype=F32, device=device)
    xt = xh.t.detach()
    _lib.call("rgbac_finalize", _lib.dtype_code(dtype), mode, B, 3, H, W, x.data_ptr(),
              xt.data_ptr(), ld, mask.data_ptr(), zero.data_ptr(), 1, zero.data_ptr(), 1,
              scratch.data_ptr(), out.data_ptr(), _lib.stream_ptr(device))
    dn = torch.full_like(xt, NAN)
    gm = torch.tensor([4096.0], dtype=F32, device=device)
    _lib.call("rgbac_mse_bwd", _lib.dtype_code(dtype), mode, B, 3, H, W, x.data_ptr(),
              xt.data_ptr(), ld, mask.data_ptr(), scratch.data_ptr(), gm.data_ptr(),
              dn.data_ptr(), ld, _lib.stream_ptr(device))
    torch.cuda.synchronize()
    assert out[0].item() == v.item()
    assert torch.equal(dn, dx)                           # pads included: zeros, not NaN


# --------------------------------------------------------------------------
# 4. act_bwd
# --------------------------------------------------------------------------
ACT_LAYOUTS = [(24, 24), (13, 16), (3, 8)]
ACT_NPIX = 63                                           # 7 x 9 pixels
LRELU_SLOPE = torch.tensor([0.2], dtype=F32).item()     # the slope as the C float carries it
ACTS = ["none", "gelu", "relu", "lrelu", "tanh_half", "gate", "gdn", "igdn", "masksel"]


def _act_ref(act, g, v, a, on, dt):
    """Closed-form (dz, dr1) of y = act(v [, r1]) on dtype dt; dr1 None where r1 does not
    enter the activation."""
    g, v, a = g.to(dt), v.to(dt), a.to(dt)
    if act == "none":
        return g.clone(), None
    if act == "gelu":
        cdf = 0.5 * torch.erfc(-v * (0.5 ** 0.5))
        pdf = torch.exp(-0.5 * v * v) * 0.3989422804014327
        return g * (cdf + v * pdf), None
    if act == "relu":
        return torch.where(v > 0, g, torch.zeros_like(g)), None
    if act == "lrelu":
        return torch.where(v > 0, g, g * LRELU_SLOPE), None
    if act == "tanh_half":
        t = torch.tanh(v)
        return g * 0.5 * (1 - t * t), g.clone()
    if act == "gate":
        s = torch.sigmoid(v)
        return g * a * (s * (1 - s)), g * s
    if act == "gdn":
        return g * a * -0.5 / (torch.sqrt(v) * v), g / torch.sqrt(v)
    if act == "igdn":
        return g * a * 0.5 / torch.sqrt(v), g * torch.sqrt(v)
    if act == "masksel":
        return torch.where(on[:, None], g, torch.zeros_like(g)), g.clone()
    raise ValueError(act)


@pytest.mark.parametrize("C,ld", ACT_LAYOUTS, ids=["24of24", "13of16", "3of8"])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_act_bwd(device, dtype, act, C, ld):
    """rgbac_act_bwd called directly: dz and dr1 of every activation with a backward against
    the closed-form derivative in fp64.  (24, 24) in bf16 takes the flat kernel (except
    masksel, whose sel map forces the generic one); (13, 16) and (3, 8) take the generic
    kernel's padded-tail branch.  Outputs are pre-filled with NaN: channels [C, ld) come back
    as zeros; the inputs' pad channels hold NaN and are never read.  bf16 GELU uses the fast
    derivative (A&S 7.1.26, |erf error| <= 1.5e-7 by the comment in common.h, so 0.75e-7 on
    the CDF): twice that, 1.5e-7 * |g|, is added to the bound per element."""
    from rgbac import _lib
    lowp = dtype == BF16
    g_ = _gen(900 + 16 * ACTS.index(act) + C)
    n = ACT_NPIX
    gy = _rnd(torch.randn((n, C), generator=g_), dtype)
    if act in ("gdn", "igdn"):
        v = _rnd(0.1 + 3 * torch.rand((n, C), generator=g_), dtype)
        assert (v > 0).all()
    else:
        v = _rnd(12 * torch.rand((n, C), generator=g_) - 6, dtype)       # tails covered
    if act in ("relu", "lrelu"):
        near = v.abs() < 1e-3
        v[near] = _rnd(v[near] + 0.25, dtype)
        assert not (v.abs() < 1e-3).any()
    a = _rnd(torch.randn((n, C), generator=g_), dtype)
    on = torch.rand(n, generator=g_) > 0.4
    assert on.any() and not on.all()
    z32, r32 = _act_ref(act, gy, v, a, on, F32)
    z64, r64 = _act_ref(act, gy, v, a, on, F64)

    def dev(t):                                   # (n, C) -> (n, ld) with NaN pad channels
        p = torch.full((n, ld), NAN)
        p[:, :C] = t
        return p.to(dtype).to(device)

    dy_d, z_d, a_d = dev(gy), dev(v), dev(a)
    uses_r1 = act in ("gate", "gdn", "igdn")
    want_r1 = r64 is not None
    sel = on.to(torch.uint8).to(device) if act == "masksel" else None
    dz = torch.full((n, ld), NAN, dtype=dtype, device=device)
    dr1 = torch.full((n, ld), NAN, dtype=dtype, device=device) if want_r1 else None
    need_z = act not in ("none", "masksel")
    _lib.call("rgbac_act_bwd", _lib.dtype_code(dtype), _lib.ACT[act],
              LRELU_SLOPE if act == "lrelu" else 0.0, n, C, dy_d.data_ptr(), ld,
              z_d.data_ptr() if need_z else None, ld if need_z else 0,
              a_d.data_ptr() if uses_r1 else None, ld if uses_r1 else 0, _lib.ptr(sel),
              dz.data_ptr(), ld, _lib.ptr(dr1), ld if want_r1 else 0, _lib.stream_ptr(device))
    torch.cuda.synchronize()
    tag = f"act_bwd {'bf16' if lowp else 'f32'} {act} ({C}, {ld})"
    extra = 1.5e-7 * gy.abs() if (lowp and act == "gelu") else None
    dz, dr1 = dz.float().cpu(), (None if dr1 is None else dr1.float().cpu())
    assert not dz[:, C:].any(), "pad channels of dz must be zero"
    _check(f"{tag} dz", dz[:, :C], z32, z64, lowp, extra=extra)
    if want_r1:
        assert not dr1[:, C:].any(), "pad channels of dr1 must be zero"
        _check(f"{tag} dr1", dr1[:, :C], r32, r64, lowp)


# --------------------------------------------------------------------------
# 5. helpers
# --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_pixel_shuffle(device, dtype):
    """rgbac_pixel_shuffle both ways with padded rows == F.pixel_shuffle / F.pixel_unshuffle
    on the NCHW view, bit for bit; pad channels are not written; the round trip is the
    identity."""
    from rgbac import _lib
    B, H, W, C = 2, 5, 7, 6
    ldi, ldo = 4 * C + 8, C + 2
    x = torch.randn((B, 4 * C, H, W), generator=_gen(11)).to(dtype)
    lo = torch.full((B, H, W, ldi), NAN, dtype=dtype)
    lo[..., :4 * C] = x.permute(0, 2, 3, 1)
    lo = lo.to(device)
    hi = torch.full((B, 2 * H, 2 * W, ldo), NAN, dtype=dtype, device=device)
    _lib.call("rgbac_pixel_shuffle", _lib.dtype_code(dtype), 0, B, H, W, C, lo.data_ptr(), ldi,
              hi.data_ptr(), ldo, _lib.stream_ptr(device))
    torch.cuda.synchronize()
    assert torch.equal(hi[..., :C].permute(0, 3, 1, 2).cpu(), F.pixel_shuffle(x, 2))
    assert torch.isnan(hi[..., C:]).all()
    back = torch.full((B, H, W, ldi), NAN, dtype=dtype, device=device)
    _lib.call("rgbac_pixel_shuffle", _lib.dtype_code(dtype), 1, B, H, W, C, hi.data_ptr(), ldo,
              back.data_ptr(), ldi, _lib.stream_ptr(device))
    torch.cuda.synchronize()
    assert torch.equal(back[..., :4 * C].permute(0, 3, 1, 2).cpu(),
                       F.pixel_unshuffle(F.pixel_shuffle(x, 2), 2))
    assert torch.equal(back[..., :4 * C].cpu(), lo[..., :4 * C].cpu())
    assert torch.isnan(back[..., 4 * C:]).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_colsum(device, dtype):
    """ag.colsum and rgbac_colsum (13 channels in rows of 16, 1000 pixels; 7 chunks; more
    chunks than pixels, whose empty chunks write zero partials into a NaN-filled buffer)
    against the fp64 column sum: fp32 sequential sums, within npix * 2^-24 * sum|x|."""
    from rgbac import _lib
    from rgbac import autograd as ag
    rt = _rt()
    C, ld = 13, 16
    x = torch.randn((2, 20, 25, ld), generator=_gen(13)).to(dtype)
    x[..., C:] = NAN                                       # pad channels are never read
    xd = x.to(device)
    flat = x[..., :C].double().reshape(-1, C)
    npix = flat.shape[0]
    assert npix == 1000
    want, tol = flat.sum(0), npix * 2.0 ** -24 * flat.abs().sum(0)
    got = ag.colsum(rt.Feat(xd, C), C).cpu().double()
    assert torch.isfinite(got).all() and ((got - want).abs() <= tol).all()

    def direct(n, nsplit):
        part = torch.full((nsplit, C), NAN, dtype=F32, device=device)
        _lib.call("rgbac_colsum", _lib.dtype_code(dtype), n, C, xd.data_ptr(), ld, nsplit,
                  part.data_ptr(), _lib.stream_ptr(device))
        torch.cuda.synchronize()
        return part.cpu()

    p7 = direct(npix, 7)
    assert torch.isfinite(p7).all() and ((p7.double().sum(0) - want).abs() <= tol).all()
    chunk = -(-npix // 7)
    for k in range(7):                                     # each chunk is its own pixels' sum
        ck = flat[k * chunk:(k + 1) * chunk]
        assert ((p7[k].double() - ck.sum(0)).abs() <= npix * 2.0 ** -24 * ck.abs().sum(0)).all()
    p8 = direct(5, 8)                                      # chunks 5..7 hold no pixel
    assert torch.isfinite(p8).all() and not p8[5:].any()
    assert torch.equal(p8[:5], flat[:5].float())


def test_sum_partials(device):
    """rgbac_sum_partials, 3 rows of 1000 fp64 partials (four trips of the 256-thread loop,
    the last ragged): the fp64 row sums rounded to fp32, exactly.  The partials are multiples
    of 2^-12 below 2^18, so every fp64 summation order gives the same sum."""
    from rgbac import _lib
    part = torch.randint(-2 ** 30, 2 ** 30, (3, 1000), generator=_gen(17)).double() / 4096
    out = torch.full((3,), NAN, dtype=F32, device=device)
    pd = part.to(device)
    _lib.call("rgbac_sum_partials", 3, 1000, pd.data_ptr(), out.data_ptr(),
              _lib.stream_ptr(device))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), part.sum(1).float())
