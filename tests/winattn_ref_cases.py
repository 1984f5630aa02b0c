"""Cases, operand builders, references and per-element allowances of the forward window
attention kernels (csrc/winattn.hip, csrc/winblock.hip).  CPU only, independent of rgbac.

Two operations are written out plainly in torch, in any dtype (fp64 / fp32):

  core_ref   the attention core on a given qkv tensor: cyclic shift, window partition,
             softmax(q k^T scale + B_rel + M_shift + M_explicit) v per window and head, window
             drop (windows whose alpha sums to zero give 0), scatter back; plus the per-pixel
             keep flags (``sel``);
  block_ref  the whole block: x + proj(core(qkv(x))) on active windows, x elsewhere.

Next to the fp64 reference the same walk computes a first-order allowance for the bf16 chains
(DESIGN section 27): every rounding to bf16 contributes half a bf16 ulp of the value rounded,
carried through a product by the product of absolute values and through the softmax by
dP_j <= P_j (|ds_j| + sum_k P_k |ds_k|); and a "twin", the same chain in fp64 with torch's
bf16 rounding at exactly those points, which tests/test_winattn_ref_host.py holds inside the
allowance before any kernel is involved.

Rounding points.  bf16 MFMA core (winattn_mfma_kernel<bf16_t>): q * scale when staged, P when
written to LDS, the store (k and v are the bf16 inputs themselves).  Fused blocks
(winblock_v2_kernel, winblock_kernel + winproj_kernel, winblock4_kernel): q (scale * log2 e
folded in), k, v, P and O are each packed to bf16 for the next product, the proj accumulates
in fp32, one store rounds x + y.
"""
import dataclasses
import math

import torch

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
SENTINEL = 1000.0               # pre-fill of every output buffer (finite, exact in bf16)
SEL_SENTINEL = 0xAB
TINY_ALPHA = 2.0 ** -20
LOG2E = 1.4426950408889634
BF16_EPS = 2.0 ** -8            # one store rounding, worst case relative


def f32_scale(d):
    """The scale the layer passes to the kernels: head_dim ** -0.5 rounded to fp32."""
    return float(torch.tensor(d ** -0.5, dtype=F32))


def round_to(t, dtype):
    """Round to the case dtype and return fp64 (what both sides see)."""
    return t.to(dtype).double()


def half_ulp(v):
    """Half a bf16 ulp of every element of ``v`` (0 where v == 0): bf16 keeps 8 significant
    bits, so for |v| in [2^e, 2^(e+1)) one ulp is 2^(e-7)."""
    v = v.double().abs()
    _, e = torch.frexp(v)                                # |v| = m 2^e, m in [0.5, 1)
    h = torch.ldexp(torch.ones_like(v), e - 9)
    return torch.where(v > 0, h, torch.zeros_like(v))


def rbf(v):
    """torch's bf16 rounding (nearest even) of an fp64 tensor, back in fp64."""
    return v.to(F32).to(BF16).double()


# --------------------------------------------------------------------------------------
# index permutations
# --------------------------------------------------------------------------------------
def partition(t, ws):
    """(B, H, W, X) -> (B * nW, ws * ws, X), windows in (b, wy, wx) order."""
    B, H, W, X = t.shape
    t = t.reshape(B, H // ws, ws, W // ws, ws, X).permute(0, 1, 3, 2, 4, 5)
    return t.reshape(-1, ws * ws, X)


def reverse(win, ws, B, H, W):
    """Inverse of partition."""
    t = win.reshape(B, H // ws, W // ws, ws, ws, -1).permute(0, 1, 3, 2, 4, 5)
    return t.reshape(B, H, W, -1)


def roll(t, s):
    return t if s == 0 else torch.roll(t, shifts=(s, s), dims=(1, 2))


def shift_mask(B, H, W, ws, shift, dtype):
    """Additive (B * nW, N, N) mask of the shifted frame: rows and columns are cut into the
    bands [0, L - ws), [L - ws, L - shift), [L - shift, L); tokens of different (row band,
    column band) regions get -100."""
    def band(L):
        i = torch.arange(L)
        return (i >= L - ws).long() + (i >= L - shift).long()
    rid = 3 * band(H)[:, None] + band(W)[None, :]
    rw = partition(rid[None, :, :, None].expand(B, H, W, 1), ws)[..., 0]
    cut = rw[:, :, None] != rw[:, None, :]
    return torch.where(cut, torch.tensor(-100.0, dtype=dtype), torch.tensor(0.0, dtype=dtype))


def relpos_index(ws):
    """(N, N) index into the (2 ws - 1)^2 relative-position table: query i, key j."""
    t = torch.arange(ws * ws)
    y, x = t // ws, t % ws
    return (y[:, None] - y[None, :] + ws - 1) * (2 * ws - 1) + (x[:, None] - x[None, :] + ws - 1)


def dense_bias(table, ws):
    """(table rows, heads) -> [heads][N][N]."""
    N = ws * ws
    return table[relpos_index(ws).reshape(-1)].reshape(N, N, -1).permute(2, 0, 1).contiguous()


def keep_flags(alpha, B, H, W, ws, shift):
    """Per window of the shifted frame: its alpha sums to non-zero (alpha None: all kept)."""
    if alpha is None:
        return torch.ones(B * (H // ws) * (W // ws), dtype=torch.bool)
    a = roll(alpha.reshape(B, H, W, 1).double(), -shift)
    return partition(a, ws).sum(dim=(1, 2)) != 0


def per_pixel(flags, B, H, W, ws, shift):
    """Window flags -> (B, H, W) in the original frame."""
    N = ws * ws
    f = flags.reshape(-1, 1, 1).expand(-1, N, 1)
    return roll(reverse(f, ws, B, H, W), shift)[..., 0]


# --------------------------------------------------------------------------------------
# the attention chain on partitioned windows
# --------------------------------------------------------------------------------------
@dataclasses.dataclass
class Chain:
    out: torch.Tensor            # the result in the walk's dtype
    allow: torch.Tensor = None   # fp64 first-order allowance of the bf16 chain (no noise term)
    twin: torch.Tensor = None    # fp64 chain with bf16 rounding at the stated points
    probs: torch.Tensor = None   # softmax probabilities (G, heads, N, N)


def _softmax_carry(P, ds):
    return P * (ds + (P * ds).sum(-1, keepdim=True))


def attend(q, k, v, add, scale, chain=None):
    """q, k, v: (G, heads, N, d); add: (G, heads, N, N) additive terms.  Returns o (G, heads, N,
    d) and, for chain = "core" / "block" (fp64 only), the allowance of o before its own
    rounding and the twin's o before its own rounding."""
    s = (q * scale) @ k.transpose(-2, -1) + add
    P = torch.softmax(s, dim=-1)
    o = P @ v
    if chain is None:
        return o, None, None, P
    if chain == "core":                                  # q * scale | P | (store, by the caller)
        qr = rbf(q * scale)
        kr, vr = k, v
        dq, dk, dv = half_ulp(q * scale), torch.zeros_like(k), torch.zeros_like(v)
        st = qr @ kr.transpose(-2, -1) + add
    else:                                                # q * scale * log2 e | k | v | P | O
        q2 = q * (scale * LOG2E)
        qr, kr, vr = rbf(q2), rbf(k), rbf(v)
        dq, dk, dv = half_ulp(q2) / LOG2E, half_ulp(k), half_ulp(v)
        st = (qr @ kr.transpose(-2, -1)) / LOG2E + add
    ds = dq @ k.abs().transpose(-2, -1) + (q * scale).abs() @ dk.transpose(-2, -1)
    dP = _softmax_carry(P, ds) + half_ulp(P)
    do = dP @ v.abs() + P @ dv
    ot = rbf(torch.softmax(st, dim=-1)) @ vr
    return o, do, ot, P


def _split_heads(win, C, heads):
    G, N, _ = win.shape
    d = C // heads
    t = win.reshape(G, N, 3, heads, d).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def _merge_heads(o):
    G, h, N, d = o.shape
    return o.transpose(1, 2).reshape(G, N, h * d)


def _additive(dense, B, H, W, ws, shift, amask, G, dtype):
    add = dense.to(dtype)[None]
    if shift > 0:
        add = add + shift_mask(B, H, W, ws, shift, dtype)[:, None]
    if amask is not None:
        add = add + amask.to(dtype)[torch.arange(G) % amask.shape[0]][:, None]
    return add


def core_ref(qkv, alpha, dense, amask, C, ws, heads, shift, scale, dtype, chain=None):
    """The attention core.  qkv: (B, H, W, >= 3C), only the first 3C channels are read; alpha:
    (B, H, W) >= 0 or None (unmasked); dense: [heads][N][N]; amask: (nW, N, N) or None.
    Returns (Chain over (B, H, W, C), sel (B, H, W) bool)."""
    B, H, W, _ = qkv.shape
    win = partition(roll(qkv[..., :3 * C].to(dtype), -shift), ws)
    G = win.shape[0]
    q, k, v = _split_heads(win, C, heads)
    keep = keep_flags(alpha, B, H, W, ws, shift)
    add = _additive(dense, B, H, W, ws, shift, amask, G, dtype)
    o, do, ot, P = attend(q, k, v, add, scale, chain)
    km = keep.reshape(-1, 1, 1).to(dtype)

    def back(t):
        return roll(reverse(_merge_heads(t) * km, ws, B, H, W), shift)
    res = Chain(back(o), probs=P[keep])
    if chain is not None:
        res.allow = back(do + half_ulp(o))               # + the store
        res.twin = back(rbf(ot))
    return res, per_pixel(keep, B, H, W, ws, shift)


def block_ref(x, alpha, ops, C, ws, heads, shift, scale, dtype, masked=True, chain=None):
    """The whole block on x (B, H, W, C): x + proj(core(qkv(x))) on active windows, x
    elsewhere.  ops: wq (3C, C), bq (3C), wp (C, C), bp (C), table ((2 ws - 1)^2, heads).
    Returns (Chain, keep per pixel, y = out - x of the reference)."""
    B, H, W, _ = x.shape
    x = x[..., :C].to(dtype)
    wq, bq, wp, bp = (ops[n].to(dtype) for n in ("wq", "bq", "wp", "bp"))
    dense = dense_bias(ops["table"].to(dtype), ws)
    xw = partition(roll(x, -shift), ws)
    G = xw.shape[0]
    q, k, v = _split_heads(xw @ wq.t() + bq, C, heads)
    keep = keep_flags(alpha if masked else None, B, H, W, ws, shift)
    add = _additive(dense, B, H, W, ws, shift, None, G, dtype)
    o, do, ot, P = attend(q, k, v, add, scale, "block" if chain else None)
    km = keep.reshape(-1, 1, 1).to(dtype)
    y = (_merge_heads(o) @ wp.t() + bp) * km
    out = xw + y

    def back(t):
        return roll(reverse(t, ws, B, H, W), shift)
    res = Chain(back(out), probs=P[keep])
    if chain:
        dy = (_merge_heads(do + half_ulp(o)) @ wp.abs().t()) * km
        res.allow = back(dy + half_ulp(out) * km)        # transparent windows: exactly x
        yt = (_merge_heads(rbf(ot)) @ wp.t() + bp) * km
        res.twin = back(torch.where(km.bool(), rbf(xw + yt), xw))
    return res, per_pixel(keep, B, H, W, ws, shift), back(y)


# --------------------------------------------------------------------------------------
# the bar
# --------------------------------------------------------------------------------------
class Bar:
    """References and per-element allowance of one launch.

    E(a) = max_i |a_i - g64_i| / (|g64_i| + 1e-3 max|g64|), den_i its denominator.
      kind "f32":  |err_i| <= 8 E(g32) den_i, and max|err| <= 2e-5 max|g64|
      kind "st":   |err_i| <= (8 E(g32) + 2^-8) den_i      (bf16 store of an fp32 chain)
      kind "prop": |err_i| <= allow_i + 8 E(g32) den_i     (bf16 chain, propagated allowance)
    Elements of transparent windows are compared exactly by the caller (allow_i = 0 there,
    the references agree bit for bit)."""

    def __init__(self, kind, g64, g32, allow=None):
        g64, g32 = g64.double(), g32.double()
        assert torch.isfinite(g64).all() and g64.abs().max().item() > 0
        self.kind, self.g64 = kind, g64
        self.gmax = g64.abs().max().item()
        self.den = g64.abs() + 1e-3 * self.gmax
        self.e_ref = ((g32 - g64).abs() / self.den).max().item()
        noise = 8.0 * self.e_ref * self.den
        if kind == "f32":
            self.allow = noise
        elif kind == "st":
            self.allow = noise + BF16_EPS * self.den
        else:
            assert allow is not None and allow.shape == g64.shape
            self.allow = noise + allow.double()

    def to(self, device):
        self.g64, self.den, self.allow = (t.to(device) for t in (self.g64, self.den, self.allow))
        return self

    def figures(self, got):
        """(E(got), E at the allowance where the worst ratio sits, worst |err| / allow, number of
        elements over the bar)."""
        err = (got.double() - self.g64).abs()
        ratio = err / self.allow
        ratio = torch.where(err == 0, torch.zeros_like(ratio), ratio)
        i = ratio.argmax()
        nbad = int((err > self.allow).sum().item())
        if not torch.isfinite(got).all().item():
            nbad = max(nbad, 1)
        if self.kind == "f32" and err.max().item() > 2e-5 * self.gmax:
            nbad = max(nbad, 1)
        return ((err / self.den).max().item(), (self.allow / self.den).reshape(-1)[i].item(),
                ratio.max().item(), nbad)


def ratio_line(tag, bar, got):
    """Prints "RATIO tag E(gpu) allowance ratio ok|BAD"; returns None or what is wrong."""
    e, a, r, nbad = bar.figures(got)
    print(f"RATIO {tag} {e:.3e} {a:.3e} {r:.3f} {'BAD' if nbad else 'ok'}  "
          f"(E(g32) {bar.e_ref:.3e}, bar {bar.kind})")
    if nbad:
        return f"{tag}: {nbad} elements over the bar, E {e:.3e}, worst err/allow {r:.3f}"
    return None


# --------------------------------------------------------------------------------------
# alpha patterns (built in the shifted window frame, rolled back to the image frame)
# --------------------------------------------------------------------------------------
def make_alpha(kind, B, H, W, ws, shift, gen):
    """None (unmasked) or (B, H, W) fp32 >= 0.
      active       every pixel in (0.25, 1.25)
      transparent  all zero
      pixel        all zero but one pixel of 2^-20, the last token of the last window
      mixed        about a third of the windows transparent (ws 4: windows 1, and every third
                   after it, so the first 64-token group has one transparent window among
                   three active ones), one of the active ones alive by its last token alone
      quarter      the first max(1, nwin // 4) windows transparent plus one more kept alive by
                   a single pixel of 2^-20"""
    if kind == "unmasked":
        return None
    nwin = B * (H // ws) * (W // ws)
    N = ws * ws
    a = torch.rand((nwin, N), generator=gen) + 0.25
    if kind == "transparent":
        a.zero_()
    elif kind == "pixel":
        a.zero_()
        a[nwin - 1, N - 1] = TINY_ALPHA
    elif kind == "mixed":
        a[1::3] = 0
        a[nwin - 1] = 0
        a[nwin - 1, N - 1] = TINY_ALPHA
    elif kind == "quarter":
        nz = max(1, nwin // 4)
        a[:min(nz + 1, nwin)] = 0
        a[min(nz, nwin - 1), N // 2] = TINY_ALPHA
    else:
        assert kind == "active", kind
    return roll(reverse(a.reshape(nwin, N, 1), ws, B, H, W), shift)[..., 0].float().contiguous()


def make_amask(nw, N, gen):
    """Explicit additive mask (nW, N, N): 0 / -100 at random with the diagonal kept 0 (no row is
    cut whole), and one -inf entry off the diagonal."""
    m = torch.where(torch.rand((nw, N, N), generator=gen) < 0.3, -100.0, 0.0)
    m[:, torch.arange(N), torch.arange(N)] = 0.0
    m[nw - 1, 1, 2] = float("-inf")
    return m.float().contiguous()


# --------------------------------------------------------------------------------------
# Part A: the core alone
# --------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class CoreConfig:
    id: str
    ws: int
    C: int
    heads: int
    kernel: str                  # "mfma" | "generic": what rgbac_winattn_core_ex must take

    @property
    def d(self):
        return self.C // self.heads


CORE_CONFIGS = [
    CoreConfig("mfma-ws8-dh24", 8, 192, 8, "mfma"),
    CoreConfig("mfma-ws4-dh10", 4, 80, 8, "mfma"),
    CoreConfig("generic-ws8-dh12", 8, 96, 8, "generic"),
    CoreConfig("generic-ws4-dh8", 4, 64, 8, "generic"),
    CoreConfig("generic-ws4-dh24", 4, 192, 8, "generic"),    # dh 24 at ws 4 is no MFMA shape
    CoreConfig("mfma-ws8-dh24-1head", 8, 24, 1, "mfma"),     # one head group
]


@dataclasses.dataclass(frozen=True)
class CoreLaunch:
    B: int
    H: int
    W: int
    shift: int
    alpha: str
    amask_nw: int = 0            # 0: no explicit mask
    strided: bool = True         # ldq = 3C + 8, ldo = C + 8
    hpbs: tuple = (1,)

    def tag(self):
        return (f"B{self.B}x{self.H}x{self.W}-s{self.shift}-{self.alpha}"
                f"{'-am%d' % self.amask_nw if self.amask_nw else ''}{'' if self.strided else '-tight'}")


def core_launches(cfg):
    """Every branch of winattn.hip at the smallest frames that reach it.  ws 8: 1, 3, 6 and 9
    windows (9 = one padded group of 8 plus one); ws 4: 1 window, 3 (B 1 of 4 x 12) and 5
    (B 5 of 4 x 4) windows, which leave the last 64-token group short, B 3 of 4 x 4 (one group
    spans three images) and 6 / 12 windows.  Shifts 0, ws / 2, 1, ws - 1 on one window (every
    region wraps) and on non-square frames."""
    ws = cfg.ws
    L = CoreLaunch
    hp = (1, 8, 3) if cfg.kernel == "mfma" else (1,)
    s = (0, ws // 2, 1, ws - 1)
    out = []
    for sh in s:                                         # one window: H = W = ws
        out.append(L(1, ws, ws, sh, "unmasked" if sh in (0, 1) else "active", strided=sh != 1))
    out += [L(1, ws, ws, 0, "transparent"), L(1, ws, ws, ws - 1, "pixel", hpbs=hp)]
    for i, sh in enumerate(s):                           # 1 x 3 windows
        out.append(L(1, ws, 3 * ws, sh, ("mixed", "active", "unmasked", "mixed")[i],
                     hpbs=hp if i == 0 else (1,)))
    for i, sh in enumerate(s):                           # 2 x 3 and 3 x 2 windows
        out.append(L(1, 2 * ws, 3 * ws, sh, ("active", "mixed", "mixed", "unmasked")[i],
                     hpbs=hp if i == 3 else (1,), strided=i != 2))
    out += [L(1, 3 * ws, 2 * ws, 1, "mixed"), L(1, 3 * ws, 2 * ws, ws - 1, "mixed")]
    out += [L(3, ws, 3 * ws, 0, "mixed", hpbs=hp), L(3, ws, 3 * ws, ws - 1, "unmasked"),
            L(3, ws, 3 * ws, 1, "transparent")]
    if ws == 4:
        out += [L(5, 4, 4, 0, "mixed"), L(5, 4, 4, 2, "pixel"), L(3, 4, 4, 3, "mixed"),
                L(3, 4, 4, 0, "active"), L(2, 8, 12, 1, "mixed", hpbs=hp)]
    # explicit mask: nW below the window count (gw % nW wraps), with and without the others
    out += [L(3, ws, 3 * ws, 0, "unmasked", amask_nw=2), L(1, 2 * ws, 3 * ws, 1, "mixed", amask_nw=4),
            L(1, ws, ws, 0, "unmasked", amask_nw=1, strided=False)]
    return out


def core_operands(cfg, ln, dtype, seed):
    """qkv (B, H, W, ldq) with NaN pad channels, alpha, dense bias, amask, rounded to ``dtype``
    where the kernel takes them in it (qkv); the others are fp32 operands."""
    g = torch.Generator().manual_seed(seed)
    C = cfg.C
    ldq = 3 * C + (8 if ln.strided else 0)
    qkv = torch.full((ln.B, ln.H, ln.W, ldq), float("nan"), dtype=F64)
    qkv[..., :3 * C] = round_to(torch.randn((ln.B, ln.H, ln.W, 3 * C), generator=g) * 1.25, dtype)
    N = cfg.ws ** 2
    dense = (torch.randn((cfg.heads, N, N), generator=g) * 0.5).float()
    alpha = make_alpha(ln.alpha, ln.B, ln.H, ln.W, cfg.ws, ln.shift, g)
    amask = make_amask(ln.amask_nw, N, g) if ln.amask_nw else None
    return {"qkv": qkv, "dense": dense, "alpha": alpha, "amask": amask,
            "ldo": C + (8 if ln.strided else 0)}


def core_bar(cfg, ln, ops, dtype):
    """(Bar, sel, Chain in fp64) of one core launch."""
    scale = f32_scale(cfg.d)
    prop = dtype == BF16 and cfg.kernel == "mfma"
    args = (ops["alpha"], ops["dense"], ops["amask"], cfg.C, cfg.ws, cfg.heads, ln.shift, scale)
    r64, sel = core_ref(ops["qkv"], *args, F64, chain="core" if prop else None)
    r32, sel32 = core_ref(ops["qkv"], *args, F32)
    assert torch.equal(sel, sel32)
    if not sel.any():
        return None, sel, r64
    kind = "f32" if dtype == F32 else ("prop" if prop else "st")
    return Bar(kind, r64.out, r32.out, r64.allow), sel, r64


# --------------------------------------------------------------------------------------
# Part B: the fused blocks
# --------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class BlockCase:
    form: str                    # "v2" | "pair" (RGBAC_WINBLOCK_FORM 2 / 3) | "ws4"
    B: int
    H: int
    W: int

    @property
    def ws(self):
        return 4 if self.form == "ws4" else 8

    @property
    def C(self):
        return 80 if self.form == "ws4" else 192

    @property
    def id(self):
        return f"{self.form}-B{self.B}x{self.H}x{self.W}"


BLOCK_CASES = ([BlockCase(f, *s) for f in ("v2", "pair") for s in ((1, 8, 8), (1, 8, 24), (2, 16, 24))] +
               [BlockCase("ws4", *s) for s in ((1, 4, 4), (3, 4, 12), (2, 8, 12))])


def block_launches(case):
    """(shift, alpha kind): every mask at shift 0; on the non-square frames the four shifts
    unmasked and with a quarter of the windows transparent plus one alive by one pixel.
    "quarter" leaves the head-pair form a compacted window list shorter than the frame,
    "transparent" an empty one."""
    ws = case.ws
    out = [(0, k) for k in ("unmasked", "active", "transparent", "quarter")]
    if case.H != case.W:
        for sh in (ws // 2, 1, ws - 1):
            out += [(sh, "unmasked"), (sh, "quarter")]
        out += [(ws - 1, "transparent"), (1, "pixel")]
    else:
        out += [(ws - 1, "pixel")]
    return out


def block_alphas(case, seed=9):
    """[(shift, kind, alpha)] of a case's launches: the same on the host and on the GPU."""
    g = torch.Generator().manual_seed(seed)
    return [(sh, k, make_alpha(k, case.B, case.H, case.W, case.ws, sh, g))
            for sh, k in block_launches(case)]


def block_operands(case, seed=27):
    """Operands that do not hide the attention term: x of std 0.5, q and k of std about 1.3
    (scores of std about 1.7: neither flat nor one-hot), v and the proj large enough that
    rms(y) >= 2 rms(x); non-zero qkv and proj biases, a relative-position table of std 0.5.
    x and the weights are rounded to bf16 (the kernels take them in bf16), the biases and the
    table are fp32 operands.

    The proj weights are a signed permutation of gain 3 plus dense noise of std 0.01, not a
    dense Gaussian: the allowance carries the error of O through the proj by sum_c |Wp_mc|
    dO_c, which for 192 dense terms of random sign is 14 times what their sum can be expected
    to reach, and the bar would be larger than y itself (measured: rms 2.7 against rms(y)
    1.6).  With one dominant input per output the sum is as tight as its largest term, while
    every k-step of the proj still decides 32 (ws 4: 16) outputs."""
    g = torch.Generator().manual_seed(seed + case.C + 7 * case.B + case.H + 3 * case.W)
    C, ws = case.C, case.ws
    rn = lambda *s: torch.randn(s, generator=g)
    x = round_to(rn(case.B, case.H, case.W, C) * 0.5, BF16)
    gain = 1.0 / (0.5 * math.sqrt(C))                    # unit-variance projections of x
    wq = rn(3 * C, C) * gain
    wq[:2 * C] *= 1.3
    wq[2 * C:] *= 2.0
    wp = rn(C, C) * 0.01
    sign = torch.where(torch.rand(C, generator=g) < 0.5, -3.0, 3.0)
    wp[torch.arange(C), torch.randperm(C, generator=g)] += sign
    ops = {"wq": round_to(wq, BF16), "bq": (rn(3 * C) * 0.3).float().double(),
           "wp": round_to(wp, BF16), "bp": (rn(C) * 0.3).float().double(),
           "table": (rn((2 * ws - 1) ** 2, 8) * 0.5).float().double()}
    return x, ops


def block_bar(case, x, ops, shift, alpha):
    """(Bar or None when every window is transparent, keep per pixel, Chain, y) of one launch."""
    scale = f32_scale(case.C // 8)
    args = (x, alpha, ops, case.C, case.ws, 8, shift, scale)
    r64, keep, y = block_ref(*args, F64, masked=alpha is not None, chain=True)
    r32, keep32, _ = block_ref(*args, F32, masked=alpha is not None)
    assert torch.equal(keep, keep32)
    if not keep.any():
        return None, keep, r64, y
    return Bar("prop", r64.out, r32.out, r64.allow), keep, r64, y
