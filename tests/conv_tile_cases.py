"""The shared case table of the conv tile tests (tests/test_conv_tile_coverage.py on the CPU,
tests/test_gpu_conv_tiles.py on the GPU): which convs, on which shapes and with which
epilogues, every tile of csrc/conv.hip and csrc/pw3.hip is run on, the CPU operands of a case
(rounded to the case dtype before either side sees them), its Prepared records, the
(tile, ksplit) pairs the library accepts for it, and its reference in fp64 / fp32.

No GPU use at import.  ``build_preps`` works on the CPU as well: the records then hold CPU
pointers, which rgbac_conv2d_grouped_describe never dereferences.

A case is geometry (every accepted tile and split runs it), epilogue (one tile per kernel kind
runs it, plus one split-K and one phase-split launch for the reduce kernel's own epilogue) or
GAUSS (every accepted tile).  ``kinds`` narrows a case to some kernel kinds: the inner-choice
sweeps of plan_conv and the many-tiles cases would otherwise run on every streaming tile too."""
import dataclasses
import functools
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
DTYPES = {"f32": F32, "bf16": BF16}
SENTINEL = 1000.0               # pre-fill of every output buffer (finite, exact in bf16)
LIK_BOUND = 1e-9
SCALE_BOUND = torch.tensor([0.11], dtype=F32).item()

F32_KINDS = ("stream", "deep", "pers", "wres", "direct")


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    mode: str                   # "conv" | "convt" (5x5 / s2) | "subpel"
    k: int
    stride: int
    cins: tuple                 # real channels of each source (padded to 8 in memory)
    couts: tuple                # output channels per grouped conv (one entry: a plain launch)
    B: int
    H: int
    W: int
    dtype: str                  # "f32" | "bf16"
    act: str = "gelu"
    act_param: float = 0.0
    bias: bool = True
    res0: bool = True
    res1: bool = False
    res2: bool = False
    sel: bool = False
    zout: bool = False
    out_coff: int = 0
    out_extra: int = 0          # output ldc = round_up(cout, 8) + out_extra
    square: bool = False
    seed: int = 0
    scope: str = "geometry"     # "geometry" | "epilogue" | "gauss"
    kinds: tuple = ()           # () = every kind

    @property
    def tdtype(self):
        return DTYPES[self.dtype]

    @property
    def id(self):
        return f"{self.name}-{self.dtype}"


def round_up(x, m):
    return (x + m - 1) // m * m


def rnd(t, dtype):
    """The value the kernel sees (kept as fp32 on the CPU)."""
    return t.to(BF16).float() if dtype == BF16 else t.float()


# --------------------------------------------------------------------------
# the table
# --------------------------------------------------------------------------
def _both(**kw):
    return [Case(dtype=d, **kw) for d in ("f32", "bf16")]


def _geometry_cases():
    c = []
    conv = dict(mode="conv", stride=1, B=2, H=12, W=20)
    # linear-M kinds: M = 480 (a ragged last M tile, rows wrapping inside a tile)
    c += _both(name="g-k3-96to40", k=3, cins=(96,), couts=(40,), seed=1, **conv)
    c += _both(name="g-k1-96to72", k=1, cins=(96,), couts=(72,), seed=2, **conv)
    c += _both(name="g-k3-16to24", k=3, cins=(16,), couts=(24,), seed=3, **conv)
    c += _both(name="g-k3-3src-to72", k=3, cins=(80, 32, 8), couts=(72,), seed=4, **conv)
    c += _both(name="g-k1-3src-to13", k=1, cins=(80, 32, 8), couts=(13,), seed=5, **conv)
    c += _both(name="g-k5s2-3src-to136", mode="conv", k=5, stride=2, cins=(32, 16, 8),
               couts=(136,), B=2, H=12, W=20, seed=6)
    c += _both(name="g-convt-64to24", mode="convt", k=5, stride=2, cins=(64,), couts=(24,),
               B=2, H=12, W=20, seed=7)
    # M < one tile
    c += _both(name="g-tiny-k1-64to13", mode="conv", k=1, stride=1, cins=(64,), couts=(13,),
               B=1, H=4, W=4, seed=8)
    c += _both(name="g-tiny-k3-40to40", mode="conv", k=3, stride=1, cins=(40,), couts=(40,),
               B=1, H=4, W=4, seed=9)
    # cout = bn + 3 for bn 16 .. 192, cin (40, 13) no multiple of the k-step
    for i, co in enumerate((19, 35, 51, 67, 99, 131, 195)):
        c += _both(name=f"g-k1-40to{co}", k=1, cins=(40,), couts=(co,), seed=10 + i, **conv)
    c += _both(name="g-k3-13to35", k=3, cins=(13,), couts=(35,), seed=18, **conv)
    # more output tiles than the persistent / weight-resident / direct grids have workgroups
    c += _both(name="g-many-k1-96to72", mode="conv", k=1, stride=1, cins=(96,), couts=(72,),
               B=4, H=96, W=128, seed=19, kinds=("pers", "wres", "direct"))
    c += _both(name="g-many-k3-16to24", mode="conv", k=3, stride=1, cins=(16,), couts=(24,),
               B=3, H=100, W=90, seed=20, kinds=("pers", "wres", "direct"))
    # plan_conv's inner choices: smallk NT x NKS (and grid y = 2), pw NKS, wstream waves
    for co in (24, 48, 72, 136):
        for ci in (64, 128, 192, 256):
            c.append(Case(name=f"g-pw-{ci}to{co}", dtype="bf16", k=1, cins=(ci,), couts=(co,),
                          seed=100 + co + ci, kinds=("smallk", "pw"), **conv))
    # smallk NKS 1 / 2 / 5, and the pw kernel neither pw2_ok (cout % 8) nor pw3_ok admits, NKS 6
    for ci, co in ((16, 24), (32, 3), (80, 40), (192, 100)):
        c.append(Case(name=f"g-pw-{ci}to{co}", dtype="bf16", k=1, cins=(ci,), couts=(co,),
                      seed=90 + ci, kinds=("smallk", "pw"), **conv))
    for ci in (64, 128):
        c.append(Case(name=f"g-ws-k3-{ci}to24", dtype="bf16", k=3, cins=(ci,), couts=(24,),
                      seed=30 + ci, kinds=("wstream",), **conv))
    c.append(Case(name="g-ws-k1-96to32", dtype="bf16", k=1, cins=(96,), couts=(32,), seed=33,
                  kinds=("wstream",), **conv))
    # patch kinds (bf16): 2 x 32 x 32, every halo side an image border and a tile boundary
    p = dict(mode="conv", k=3, stride=1, B=2, H=32, W=32, dtype="bf16")
    for i, (ci, co) in enumerate((((40,), 88), ((192,), 12), ((88,), 64), ((80, 32, 8), 88),
                                  ((224,), 64), ((128,), 8), ((64,), 24))):
        c.append(Case(name=f"p-k3-{sum(ci)}to{co}", cins=ci, couts=(co,), seed=40 + i, **p))
    # cout past 128: the 192- and 256-channel tiles read whole BN-row weight tiles (cpt 3 / 4 / 7)
    for i, ci in enumerate(((96,), (80, 32, 8), (224,))):
        c.append(Case(name=f"p-k3-{sum(ci)}to136", cins=ci, couts=(136,), seed=47 + i, **p))
    # the folded activation backward has its own conv_patch_kernel instantiations
    c.append(Case(name="p-k3-dgelu-96to88", cins=(96,), couts=(88,), seed=56, act="dgelu",
                  bias=False, kinds=("patch",), **p))
    c.append(Case(name="p-convt-dlrelu-64to136", mode="convt", k=5, stride=2, cins=(64,),
                  couts=(136,), B=2, H=16, W=32, dtype="bf16", seed=57, act="dlrelu",
                  act_param=0.2, bias=False, kinds=("patch",)))
    h = dict(p, H=16, W=16)
    for i, (ci, co) in enumerate(((256, 64), (288, 64), (320, 88))):
        c.append(Case(name=f"p-hyper-{ci}to{co}", cins=(ci,), couts=(co,), seed=50 + i, **h))
    t = dict(mode="convt", k=5, stride=2, B=2, H=16, W=32, dtype="bf16")
    c.append(Case(name="p-convt-192to192", cins=(192,), couts=(192,), seed=60, **t))
    c.append(Case(name="p-convt-80to192", cins=(80,), couts=(192,), seed=61, **t))
    c.append(Case(name="p-convt-192to3", cins=(192,), couts=(3,), seed=62, res0=False, **t))
    s = dict(mode="subpel", k=3, stride=1, B=2, dtype="bf16", res0=False)
    c.append(Case(name="p-subpel-192to192", cins=(192,), couts=(192,), H=16, W=32, seed=63, **s))
    c.append(Case(name="p-subpel-288to80", cins=(288,), couts=(80,), H=16, W=16, seed=64, **s))
    c.append(Case(name="p-subpel-192to12", cins=(192,), couts=(12,), H=16, W=32, seed=65, **s))
    s2 = dict(mode="conv", k=5, stride=2, B=2, H=32, W=64, dtype="bf16")
    c.append(Case(name="p-k5s2-192to192", cins=(192,), couts=(192,), seed=66, **s2))
    c.append(Case(name="p-k5s2-3src-to192", cins=(80, 32, 8), couts=(192,), seed=67, **s2))
    for i, co in enumerate((32, 24)):
        c.append(Case(name=f"p-spatial-32to{co}", cins=(32,), couts=(co,), seed=70 + i, **p))
    return c


# name -> the fields that differ from "gelu + res0 + bias"
EPILOGUES = {
    "nobias": dict(act="none", bias=False, res0=False),
    "bias": dict(act="none", res0=False),
    "relu": dict(act="relu", res0=False),
    "lrelu": dict(act="lrelu", act_param=0.2, res0=False),
    "gelu-res0": dict(),
    "res0-res2": dict(act="none", res2=True),
    "tanh-res1": dict(act="tanh_half", res0=False, res1=True),
    "gate-res1-res2": dict(act="gate", res0=False, res1=True, res2=True),
    "masksel": dict(act="masksel", res0=False, res1=True, sel=True),
    "zout": dict(zout=True),
    "coff8": dict(out_coff=8, out_extra=24),
    "sqbwd": dict(act="sqbwd", bias=False, res1=True),
    "dgelu": dict(act="dgelu", bias=False),
    "dlrelu": dict(act="dlrelu", act_param=0.2, bias=False),
    "grouped": dict(),
}


def _epilogue_cases():
    """Each kernel kind's smallest geometry case under every epilogue it takes: a 1x1 conv for
    the pointwise kinds (and wres / direct / the streaming kinds), a 3x3 conv of 96 channels
    for the patch kinds (and wstream / npatch at cout 24), 32 channels for the spatial tile."""
    c = []
    shapes = [("pt", dict(mode="conv", k=1, stride=1, cins=(96,), B=2, H=12, W=20), (72, 40),
               ("f32", "bf16")),
              ("k3", dict(mode="conv", k=3, stride=1, cins=(96,), B=2, H=16, W=32), (88, 40),
               ("f32", "bf16")),
              ("narrow", dict(mode="conv", k=3, stride=1, cins=(64,), B=2, H=16, W=32), (24, 8),
               ("bf16",)),
              ("sp", dict(mode="conv", k=3, stride=1, cins=(32,), B=2, H=16, W=32), (24, 32),
               ("bf16",))]
    seed = 200
    for tag, geo, couts, dts in shapes:
        kinds = {"narrow": ("wstream", "npatch"), "sp": ("spatial",)}.get(tag, ())
        for name, epi in EPILOGUES.items():
            for d in dts:
                seed += 1
                c.append(Case(name=f"e-{tag}-{name}", dtype=d, seed=seed, scope="epilogue",
                              couts=couts if name == "grouped" else couts[:1], kinds=kinds,
                              **geo, **epi))
    # gdn / igdn: 1x1 on the squared input, res1 = x; 192 channels (pw3), 80 (pw2) and 72
    for act in ("gdn", "igdn"):
        for ch in (192, 80, 72):
            for d in ("f32", "bf16"):
                seed += 1
                c.append(Case(name=f"e-{act}-{ch}", dtype=d, mode="conv", k=1, stride=1,
                              cins=(ch,), couts=(ch,), B=2, H=12, W=20, act=act, res0=False,
                              res1=True, square=True, seed=seed, scope="epilogue"))
        c.append(Case(name=f"e-{act}-192-zout", dtype="bf16", mode="conv", k=1, stride=1,
                      cins=(192,), couts=(192,), B=2, H=12, W=20, act=act, res0=False, res1=True,
                      square=True, zout=True, seed=seed + 50, scope="epilogue"))
    # the gate on conv_pw3_kernel: pw3_ok takes it from 8192 16-pixel tiles on
    c.append(Case(name="e-gate-pw3", dtype="bf16", mode="conv", k=1, stride=1, cins=(192,),
                  couts=(192,), B=8, H=128, W=128, act="gate", res0=False, res1=True, res2=True,
                  seed=299, scope="epilogue", kinds=("pw",)))
    # convT, 5x5/s2 and subpel under the epilogues their modes take
    t = dict(mode="convt", k=5, stride=2, cins=(64,), couts=(24,), B=2, H=16, W=32,
             scope="epilogue")
    for name in ("nobias", "res0-res2", "zout", "coff8", "dgelu", "lrelu"):
        for d in ("f32", "bf16"):
            seed += 1
            c.append(Case(name=f"e-convt-{name}", dtype=d, seed=seed, **t, **EPILOGUES[name]))
    s2 = dict(mode="conv", k=5, stride=2, cins=(40,), couts=(72,), B=2, H=32, W=64, dtype="bf16",
              scope="epilogue")
    for name in ("nobias", "res0-res2", "zout", "coff8", "tanh-res1"):
        seed += 1
        c.append(Case(name=f"e-k5s2-{name}", seed=seed, **s2, **EPILOGUES[name]))
    s = dict(mode="subpel", k=3, stride=1, cins=(96,), couts=(24,), B=2, H=16, W=32,
             scope="epilogue", res0=False)
    for name, epi in (("none", dict(act="none")), ("nobias", dict(act="none", bias=False)),
                      ("gelu", dict()), ("zout", dict(zout=True)),
                      ("coff8", dict(out_coff=8, out_extra=24))):
        for d in ("f32", "bf16"):
            seed += 1
            c.append(Case(name=f"e-subpel-{name}", dtype=d, seed=seed, **s, **epi))
    return c


def _gauss_cases():
    """(mu | sigma) of 8 and 16 channels from two 3x3 convs of 64 channels each (K = 1152: the
    8-wave wstream kernel) and, at 8 channels, two 1x1 convs of 32 (4 waves)."""
    c = []
    for cs, k, ci, seed in ((8, 3, 64, 301), (16, 3, 64, 302), (8, 1, 32, 303)):
        for d in ("f32", "bf16"):
            c.append(Case(name=f"gauss-{cs}-k{k}", dtype=d, mode="conv", k=k, stride=1,
                          cins=(ci, ci), couts=(2 * cs,), B=2, H=16, W=32, act="gauss",
                          res0=False, res1=True, seed=seed, scope="gauss"))
    return c


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = _geometry_cases() + _epilogue_cases() + _gauss_cases()
    assert len({c.id for c in cases}) == len(cases)
    return tuple(cases)


def cases(scope):
    return [c for c in all_cases() if c.scope == scope]


# --------------------------------------------------------------------------
# operands (CPU, rounded to the case dtype)
# --------------------------------------------------------------------------
def out_hw(case):
    if case.mode == "conv":
        pad = case.k // 2
        return ((case.H + 2 * pad - case.k) // case.stride + 1,
                (case.W + 2 * pad - case.k) // case.stride + 1)
    return 2 * case.H, 2 * case.W


def _untie(y, mu64, dtype):
    """Nudge (in place, by 0.25) the y whose y - mu lies within 1e-2 of a rounding tie."""
    for _ in range(6):
        d = y.double() - mu64
        bad = ((d - torch.floor(d)) - 0.5).abs() < 1e-2
        if not bad.any():
            break
        y[bad] = rnd(y[bad] + 0.25, dtype)
    return y


def build_operands(case):
    """Per grouped conv a dict of CPU fp32 tensors, every value representable in the case
    dtype: xs (NCHW, one per source), w (the nn module's weight layout), b, r0 / r1 / r2
    (NCHW on the output grid) and sel (uint8 per output pixel), as the case asks."""
    dt = case.tdtype
    g = torch.Generator().manual_seed(1000 + case.seed)
    Ho, Wo = out_hw(case)
    cin = sum(case.cins)
    if case.act == "gauss":
        return [_gauss_operands(case, g)]
    ops = []
    xs = [rnd(torch.randn((case.B, c, case.H, case.W), generator=g), dt) for c in case.cins]
    for cout in case.couts:
        o = {"xs": xs}
        bound = 1.0 / math.sqrt(cin * case.k * case.k)
        if case.mode == "convt":
            shape = (cin, cout, 5, 5)
            bound *= 2.0                          # a quarter of the 25 taps reach an output
        elif case.mode == "subpel":
            shape = (4 * cout, cin, 3, 3)
        else:
            shape = (cout, cin, case.k, case.k)
        if case.square:                           # GDN: gamma >= 0, beta > 0
            w = 0.1 * torch.rand(shape, generator=g)
            b = 0.5 + torch.rand(shape[0], generator=g)
        else:
            w = (2 * torch.rand(shape, generator=g) - 1) * bound
            b = (2 * torch.rand(shape[0] if case.mode != "convt" else cout, generator=g) - 1) * 0.5
        o["w"], o["b"] = rnd(w, dt), rnd(b, dt)
        for name in ("r0", "r1", "r2"):
            if getattr(case, "res" + name[1]):
                o[name] = rnd(torch.randn((case.B, cout, Ho, Wo), generator=g), dt)
        if case.square:
            o["r1"] = xs[0]                       # x / sqrt(norm): the conv's own source
        if case.act in ("dgelu", "dlrelu"):
            z = o["r0"]
            z[z == 0] = 0.5
            assert not (z == 0).any()
        if case.sel:
            o["sel"] = (torch.rand((case.B, Ho, Wo), generator=g) > 0.5).to(torch.uint8)
            first = o["sel"].reshape(-1)[:16]
            assert first.any() and not first.all()     # both values within one 16-pixel tile
        ops.append(o)
    return ops


def _gauss_operands(case, g):
    dt, cs, ci, k = case.tdtype, case.couts[0] // 2, case.cins[0], case.k
    shape = (case.B, ci, case.H, case.W)
    bound = 1.0 / math.sqrt(ci * k * k)
    o = {"xs": [rnd(torch.randn(shape, generator=g), dt) for _ in range(2)]}
    o["wm"] = rnd((2 * torch.rand((cs, ci, k, k), generator=g) - 1) * bound, dt)
    o["wsg"] = rnd((2 * torch.rand((cs, ci, k, k), generator=g) - 1) * bound, dt)
    o["bm"] = rnd(torch.rand(cs, generator=g) - 0.5, dt)
    o["bsg"] = rnd(0.3 + 0.5 * torch.rand(cs, generator=g), dt)   # ~ a quarter under the bound
    y = rnd(3.0 * torch.randn((case.B, cs, case.H, case.W), generator=g), dt)
    mu64, sg64 = _musigma(o, k, F64)
    for _ in range(6):
        _untie(y, mu64, dt)
        hat = torch.round(y.double() - mu64) + mu64
        near = (_raw_lik(hat, mu64, sg64) / LIK_BOUND - 1).abs() < 1e-2
        if not near.any():
            break
        y[near] = rnd(y[near] + 1.0, dt)
    o["y"] = y
    return o


def _musigma(o, k, D):
    mu = F.conv2d(o["xs"][0].to(D), o["wm"].to(D), o["bm"].to(D), padding=k // 2)
    sg = F.conv2d(o["xs"][1].to(D), o["wsg"].to(D), o["bsg"].to(D), padding=k // 2)
    return mu, sg


def _std_cum(t):
    return 0.5 * torch.erfc(float(-(2 ** -0.5)) * t)


def _raw_lik(hat, mu, sg):
    v = (hat - mu).abs()
    s = torch.clamp(sg, min=SCALE_BOUND)
    return _std_cum((0.5 - v) / s) - _std_cum((-0.5 - v) / s)


def check_gauss_conditions(case, o):
    """Asserted on the CPU against the reference alone: no y - mu within 1e-2 of a rounding
    tie, the fp32 and fp64 references take the same likelihood-clamp decision everywhere, and
    no fp64 likelihood lies within 1 % of the bound."""
    mu64, sg64 = _musigma(o, case.k, F64)
    mu32, sg32 = _musigma(o, case.k, F32)
    d = o["y"].double() - mu64
    assert not (((d - torch.floor(d)) - 0.5).abs() < 1e-2).any()
    assert o["y"].abs().max().item() < 64
    l64 = _raw_lik(torch.round(o["y"].double() - mu64) + mu64, mu64, sg64)
    l32 = _raw_lik(torch.round(o["y"] - mu32) + mu32, mu32, sg32)
    assert not ((l64 / LIK_BOUND - 1).abs() < 1e-2).any()
    assert torch.equal(l64 < LIK_BOUND, l32 < LIK_BOUND)
    assert torch.equal(torch.round(o["y"].double() - mu64), torch.round(o["y"] - mu32).double())


# --------------------------------------------------------------------------
# the reference: torch CPU conv plus the epilogue written out, in fp64 or fp32
# --------------------------------------------------------------------------
def _gelu(v):
    return v * 0.5 * torch.erfc(-v * (0.5 ** 0.5))


def _gelu_grad(z):
    cdf = 0.5 * torch.erfc(-z * (0.5 ** 0.5))
    pdf = torch.exp(-0.5 * z * z) * (1.0 / math.sqrt(2.0 * math.pi))
    return cdf + z * pdf


def reference(case, ops, D):
    """Per grouped conv {"out": NCHW, "z": the pre-activation side output or None}; GAUSS:
    {"out": y_hat, "lik", "bits": the summed bits}.  Computed in dtype ``D`` throughout."""
    return [_reference_one(case, o, D) for o in ops]


def _reference_one(case, o, D):
    if case.act == "gauss":
        mu, sg = _musigma(o, case.k, D)
        y = o["y"].to(D)
        hat = torch.round(y - mu) + mu
        lik = torch.clamp(_raw_lik(hat, mu, sg), min=LIK_BOUND)
        bits = torch.clamp(-1.0 * torch.log(lik + 1e-10) / math.log(2.0), 0, 50)
        return {"out": hat, "lik": lik, "bits": bits.double().sum().reshape(1), "z": None}
    x = torch.cat(o["xs"], 1).to(D)
    if case.square:
        x = x * x
    w = o["w"].to(D)
    b = o["b"].to(D) if case.bias else None
    if case.mode == "convt":
        v = F.conv_transpose2d(x, w, b, stride=2, padding=2, output_padding=1)
    elif case.mode == "subpel":
        v = F.pixel_shuffle(F.conv2d(x, w, b, padding=1), 2)
    else:
        v = F.conv2d(x, w, b, stride=case.stride, padding=case.k // 2)
    r0, r1, r2 = (o[n].to(D) if n in o else None for n in ("r0", "r1", "r2"))
    act = case.act
    if act == "dgelu":
        v = v * _gelu_grad(r0)
    elif act == "dlrelu":
        v = torch.where(r0 > 0, v, v * case.act_param)
    elif act == "sqbwd":
        v = r0 + 2.0 * r1 * v
    elif r0 is not None:
        v = v + r0
    z = v if case.zout else None
    if act == "gelu":
        v = _gelu(v)
    elif act == "relu":
        v = torch.clamp(v, min=0)
    elif act == "lrelu":
        v = torch.where(v > 0, v, v * case.act_param)
    elif act == "tanh_half":
        v = r1 + 0.5 * torch.tanh(v)
    elif act == "gate":
        v = r1 * torch.sigmoid(v)
    elif act == "gdn":
        v = r1 / torch.sqrt(v)
    elif act == "igdn":
        v = r1 * torch.sqrt(v)
    elif act == "masksel":
        v = torch.where(o["sel"][:, None].bool(), r1 + v, r1)
    if r2 is not None:
        v = v + r2
    return {"out": v, "z": z}


# --------------------------------------------------------------------------
# Prepared records (device "cpu": for the describe entry point only)
# --------------------------------------------------------------------------
def feat(rt, t, dtype, device, ldc=None, fill=0.0):
    """NCHW fp32 CPU tensor -> rt.Feat on ``device`` (pad channels ``fill``)."""
    B, C, H, W = t.shape
    buf = torch.full((B, H, W, ldc or round_up(C, 8)), fill, dtype=dtype)
    buf[..., :C] = t.permute(0, 2, 3, 1).to(dtype)
    return rt.Feat(buf.to(device), C)


def _module(case, o):
    from rgbac.layers._blocks import subpel_conv3x3
    cin, cout = sum(case.cins), o["w"].shape[1 if case.mode == "convt" else 0]
    if case.mode == "convt":
        m = nn.ConvTranspose2d(cin, cout, 5, stride=2, padding=2, output_padding=1)
        conv = m
    elif case.mode == "subpel":
        m = subpel_conv3x3(cin, cout // 4, 2)
        conv = m[0]
    else:
        m = nn.Conv2d(cin, cout, case.k, stride=case.stride, padding=case.k // 2)
        conv = m
    with torch.no_grad():
        conv.weight.copy_(o["w"])
        conv.bias.copy_(o["b"])
    return m


def build_preps(rt, case, ops, device):
    """(preps, bufs): the Prepared record of every grouped conv through prep_conv /
    prep_subpel / rt.prepare, and per conv the buffers the checks read: "srcs", "out", "zout"
    (Feats; the outputs pre-filled with SENTINEL) and for GAUSS "lik" / "partial"."""
    from rgbac.layers.TransformRGB import prep_conv
    dt = case.tdtype
    Ho, Wo = out_hw(case)
    preps, bufs = [], []
    for o in ops:
        fs = [feat(rt, x, dt, device) for x in o["xs"]]
        srcs = [f.src() for f in fs]
        cstore = case.couts[len(preps)] // (2 if case.act == "gauss" else 1)
        ldc = round_up(cstore, 8) + case.out_extra
        out = rt.Feat(torch.full((case.B, Ho, Wo, ldc), SENTINEL, dtype=dt, device=device), cstore)
        bf = {"srcs": fs, "out": out, "zout": None}
        if case.act == "gauss":
            from rgbac.models._latent import _musigma_pack
            k, cs, ci = case.k, cstore, case.cins[0]
            mconv, sconv = (nn.Conv2d(ci, cs, k, padding=k // 2) for _ in range(2))
            with torch.no_grad():
                mconv.weight.copy_(o["wm"]), mconv.bias.copy_(o["bm"])
                sconv.weight.copy_(o["wsg"]), sconv.bias.copy_(o["bsg"])
            pk = _musigma_pack(mconv.to(device), sconv.to(device), dt, fs[0].ldc)
            bf["y"] = feat(rt, o["y"], dt, device)
            bf["lik"] = torch.full((case.B, Ho, Wo, cs), SENTINEL, dtype=F32, device=device)
            bf["partial"] = torch.zeros(-(-case.B * Ho * Wo // 16), dtype=F64, device=device)
            pr = rt.prepare(pk, srcs, out=out, act="gauss", res1=(bf["y"], 0), aux1=bf["lik"],
                            partial=bf["partial"])
        else:
            kw = dict(out=out, out_coff=case.out_coff, act=case.act, act_param=case.act_param,
                      bias=case.bias, square=case.square)
            for name in ("r0", "r1", "r2"):
                if name in o:
                    kw["res" + name[1]] = fs[0] if case.square and name == "r1" else \
                        feat(rt, o[name], dt, device)
            if case.sel:
                kw["sel"] = o["sel"].reshape(-1).contiguous().to(device)
            if case.zout:
                kw["zout"] = bf["zout"] = rt.Feat(torch.full_like(out.t, SENTINEL), cstore)
            m = _module(case, o).to(device)
            bf["keep"] = (m, kw)
            if case.mode != "subpel":
                pr = prep_conv(m, srcs, **kw)
            else:                       # prep_subpel's two steps, with the output given
                pk = rt.packed(m[0], dt, rt.segs_of(*srcs), rt.SUBPEL2)
                pr = rt.prepare(pk, srcs, **kw)
        preps.append(pr)
        bufs.append(bf)
    return preps, bufs


def kind_of(rt, tile):
    return rt._TABLE[tile][2]


def pairs(rt, case, preps):
    """The (tile, ksplit) pairs to run: exactly those the library accepts, over every tile and
    ksplit 1 and 3, plus the phase split (4) on the conv_patch_kernel tiles where it applies.
    Epilogue cases keep the first tile of each kind at ksplit 1, one split-K and one
    phase-split launch."""
    out = []
    for t in range(len(rt.TILES)):
        if case.kinds and kind_of(rt, t) not in case.kinds:
            continue
        for ks in (1, 3):
            if rt._choice_valid(t, preps, ks):
                out.append((t, ks))
        if t in rt.PATCH_SIG and rt._patch_split_ok(preps) and rt._choice_valid(t, preps, 4):
            out.append((t, 4))
    if case.scope == "epilogue":
        seen, keep = set(), []
        for t, ks in out:
            key = (kind_of(rt, t), ks) if ks == 1 else ks
            if key not in seen:
                seen.add(key)
                keep.append((t, ks))
        out = keep
    return out
