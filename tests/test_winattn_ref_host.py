"""CPU checks of tests/winattn_ref_cases.py, before any kernel is involved: the references
agree with oracle/ref_model.py in fp64, the bf16 twins stay inside the propagated allowance
on every element of every case, and the block operands do not hide the attention term."""
import pytest
import torch

import winattn_ref_cases as wrc
from oracle import ref_model as ref

F32, F64, BF16 = wrc.F32, wrc.F64, wrc.BF16


def _sd(ops, ws):
    return {"m.attn.qkv.weight": ops["wq"], "m.attn.qkv.bias": ops["bq"],
            "m.attn.proj.weight": ops["wp"], "m.attn.proj.bias": ops["bp"],
            "m.attn.relative_position_bias_table": ops["table"],
            "m.attn.relative_position_index": ref.relative_position_index(ws)}


def _rand_ops(C, ws, heads, g):
    rn = lambda *s: torch.randn(s, generator=g, dtype=F64)
    return {"wq": rn(3 * C, C) * C ** -0.5, "bq": rn(3 * C) * 0.3, "wp": rn(C, C) * C ** -0.5,
            "bp": rn(C) * 0.3, "table": rn((2 * ws - 1) ** 2, heads) * 0.5}


def _oracle_block(x, alpha, ops, ws, shift, heads):
    B, H, W, _ = x.shape
    a = None if alpha is None else alpha.double().reshape(B, 1, H, W)
    out = ref.win_based_attention(x.permute(0, 3, 1, 2), a, _sd(ops, ws), "m", ws, shift,
                                  heads=heads, masked=alpha is not None)
    return out.permute(0, 2, 3, 1)


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


def test_half_ulp_bounds_bf16_rounding():
    g = torch.Generator().manual_seed(1)
    v = torch.randn(100000, generator=g, dtype=F64) * torch.logspace(-6, 6, 100000, dtype=F64)
    v = torch.cat([v, torch.tensor([1.0, 1.00390625, 0.0, -2.0], dtype=F64)])
    err = (wrc.rbf(v) - v).abs()
    # (rbf rounds through fp32 as the kernels do: half an fp32 ulp more on a tie)
    assert (err <= wrc.half_ulp(v) + v.abs() * 2.0 ** -24).all()
    assert wrc.half_ulp(torch.tensor([1.0, 1.99, 0.0])).tolist() == [2.0 ** -8, 2.0 ** -8, 0.0]
    assert (err / wrc.half_ulp(v).clamp_min(1e-300)).max().item() > 0.99      # and it is attained


@pytest.mark.parametrize("cfg", wrc.CORE_CONFIGS, ids=[c.id for c in wrc.CORE_CONFIGS])
def test_reference_matches_oracle_core_shapes(cfg):
    """The references on the frames, shifts and masks of Part A (the oracle runs whole blocks:
    random qkv / proj weights around the core), 1e-12 relative in fp64."""
    g = torch.Generator().manual_seed(5)
    ops = _rand_ops(cfg.C, cfg.ws, cfg.heads, g)
    seen = set()
    for ln in wrc.core_launches(cfg):
        key = (ln.B, ln.H, ln.W, ln.shift, ln.alpha)
        if ln.amask_nw or key in seen:
            continue
        seen.add(key)
        x = torch.randn((ln.B, ln.H, ln.W, cfg.C), generator=g, dtype=F64)
        alpha = wrc.make_alpha(ln.alpha, ln.B, ln.H, ln.W, cfg.ws, ln.shift, g)
        r, keep, _ = wrc.block_ref(x, alpha, ops, cfg.C, cfg.ws, cfg.heads, ln.shift,
                                   cfg.d ** -0.5, F64, masked=alpha is not None)
        want = _oracle_block(x, alpha, ops, cfg.ws, ln.shift, cfg.heads)
        assert _rel(r.out, want) <= 1e-12, (ln.tag(), _rel(r.out, want))
        # the core alone on the same qkv, then the proj by hand: the two references agree
        qkv = x @ ops["wq"].t() + ops["bq"]
        c, sel = wrc.core_ref(qkv, alpha, wrc.dense_bias(ops["table"], cfg.ws), None, cfg.C,
                              cfg.ws, cfg.heads, ln.shift, cfg.d ** -0.5, F64)
        assert torch.equal(sel, keep)
        y = (c.out @ ops["wp"].t() + ops["bp"]) * sel[..., None]
        assert _rel(x + y, want) <= 1e-12, ln.tag()
    assert len(seen) >= 15


@pytest.mark.parametrize("cfg", wrc.CORE_CONFIGS[:4], ids=[c.id for c in wrc.CORE_CONFIGS[:4]])
def test_reference_matches_oracle_explicit_mask(cfg):
    """The explicit mask, in the one form the oracle has it: WindowAttention.forward on
    windows (every window a one-window image, shift 0, no window drop)."""
    g = torch.Generator().manual_seed(6)
    ops = _rand_ops(cfg.C, cfg.ws, cfg.heads, g)
    N = cfg.ws ** 2
    xw = torch.randn((6, N, cfg.C), generator=g, dtype=F64)
    amask = wrc.make_amask(3, N, g)
    want = ref.window_attention(xw, _sd(ops, cfg.ws), "m.attn", cfg.ws, cfg.heads, amask.double())
    qkv = (xw @ ops["wq"].t() + ops["bq"]).reshape(6, cfg.ws, cfg.ws, 3 * cfg.C)
    c, _ = wrc.core_ref(qkv, None, wrc.dense_bias(ops["table"], cfg.ws), amask, cfg.C, cfg.ws,
                        cfg.heads, 0, cfg.d ** -0.5, F64)
    got = c.out.reshape(6, N, cfg.C) @ ops["wp"].t() + ops["bp"]
    assert _rel(got, want) <= 1e-12


@pytest.mark.parametrize("case", wrc.BLOCK_CASES, ids=[c.id for c in wrc.BLOCK_CASES])
def test_block_reference_operands_and_twin(case):
    """Part B, every launch: the reference agrees with the oracle; on active windows
    rms(y) >= 2 rms(x); the softmax is neither flat nor one-hot (the median over query rows of
    exp(entropy), the effective number of keys, lies in [2, N / 2]: N is flat, 1 is one-hot);
    the twin stays inside the allowance."""
    x, ops = wrc.block_operands(case)
    N = case.ws ** 2
    worst = 0.0
    for shift, kind, alpha in wrc.block_alphas(case):
        want = _oracle_block(x, alpha, ops, case.ws, shift, 8)
        r, _, _ = wrc.block_ref(x, alpha, ops, case.C, case.ws, 8, shift, (case.C // 8) ** -0.5,
                                F64, masked=alpha is not None)
        assert _rel(r.out, want) <= 1e-12, (shift, kind)
        bar, keep, r64, y = wrc.block_bar(case, x, ops, shift, alpha)
        if bar is None:
            assert kind == "transparent" and torch.equal(r64.out, x)
            continue
        rx = x[keep].pow(2).mean().sqrt().item()
        ry = y[keep].pow(2).mean().sqrt().item()
        P = r64.probs
        neff = torch.exp(-(P * torch.log(P.clamp_min(1e-300))).sum(-1)).median().item()
        _, _, ratio, nbad = bar.figures(r64.twin)
        prop = ((r64.twin - r64.out).abs() / r64.allow.clamp_min(1e-300))[keep].max().item()
        print(f"BLOCK {case.id} s{shift} {kind}: rms(y)/rms(x) {ry / rx:.2f}, n_eff {neff:.1f} "
              f"of {N}, twin/allowance {ratio:.3f} (against the propagated part alone {prop:.3f})")
        assert ry >= 2.0 * rx, (shift, kind, ry, rx)
        assert 2.0 <= neff <= N / 2, (shift, kind, neff)
        assert nbad == 0 and not torch.equal(r64.twin, r64.out), (shift, kind, ratio)
        assert torch.equal(r64.twin[~keep], x[~keep])
        worst = max(worst, ratio)
    print(f"TWIN {case.id} worst twin/allowance {worst:.3f}")


@pytest.mark.parametrize("cfg", [c for c in wrc.CORE_CONFIGS if c.kernel == "mfma"],
                         ids=[c.id for c in wrc.CORE_CONFIGS if c.kernel == "mfma"])
def test_core_twin_inside_allowance(cfg):
    """Part A, the bf16 MFMA core: the twin (q * scale, P and the store rounded to bf16) stays
    inside the allowance on every element of every launch; the softmax of the operands is
    neither flat nor one-hot."""
    worst = 0.0
    N = cfg.ws ** 2
    for i, ln in enumerate(wrc.core_launches(cfg)):
        ops = wrc.core_operands(cfg, ln, BF16, 100 + i)
        bar, sel, r64 = wrc.core_bar(cfg, ln, ops, BF16)
        if bar is None:
            continue
        _, _, ratio, nbad = bar.figures(r64.twin)
        assert nbad == 0 and not torch.equal(r64.twin, r64.out), (ln.tag(), ratio)
        worst = max(worst, ratio)
        if ln.shift == 0 and not ln.amask_nw:
            P = r64.probs
            neff = torch.exp(-(P * torch.log(P.clamp_min(1e-300))).sum(-1)).median().item()
            assert 2.0 <= neff <= N / 2, (ln.tag(), neff)
    print(f"TWIN {cfg.id} worst twin/allowance {worst:.3f}")


def test_case_lists_cover_the_issue():
    """Every kernel selection, shift, window count, mask and stride the tests are meant to
    reach is in the lists."""
    for cfg in wrc.CORE_CONFIGS:
        mf = (cfg.ws == 8 and cfg.d == 24) or (cfg.ws == 4 and cfg.d == 10)
        assert (cfg.kernel == "mfma") == mf, cfg.id
        lns = wrc.core_launches(cfg)
        ws = cfg.ws
        one = [l for l in lns if l.H == ws and l.W == ws and l.B == 1]
        nsq = [l for l in lns if l.H != l.W]
        for group in (one, nsq):
            assert {l.shift for l in group} >= {0, ws // 2, 1, ws - 1}, cfg.id
        assert {l.alpha for l in lns} >= {"unmasked", "active", "transparent", "pixel", "mixed"}
        assert {l.strided for l in lns} == {True, False}
        assert any(l.amask_nw and l.amask_nw < l.B * (l.H // ws) * (l.W // ws) for l in lns)
        counts = {l.B * (l.H // ws) * (l.W // ws) for l in lns}
        assert counts >= ({1, 3, 9} if ws == 8 else {1, 3, 5})
        if ws == 4:
            assert any((l.B, l.H, l.W) == (3, 4, 4) for l in lns)
        if cfg.kernel == "mfma":
            assert {h for l in lns for h in l.hpbs} == {1, 8, 3}
    assert {c.form for c in wrc.BLOCK_CASES} == {"v2", "pair", "ws4"}
    for case in wrc.BLOCK_CASES:
        ls = wrc.block_launches(case)
        assert {k for _, k in ls} >= {"unmasked", "active", "transparent", "quarter"}
        if case.H != case.W:
            assert {s for s, _ in ls} >= {0, case.ws // 2, 1, case.ws - 1}
