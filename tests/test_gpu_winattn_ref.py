"""Element-wise fp64 reference tests of the forward window attention kernels: the attention
core (csrc/winattn.hip: winattn_core_kernel and winattn_mfma_kernel, fp32 and bf16, called
through rgbac_winattn_core_ex on a given qkv tensor) and the fused blocks (csrc/winblock.hip:
winblock_v2_kernel, the winflag / winblock / winproj head-pair form, winblock4_kernel, through
WindowAttention.run_block).  Cases, references and allowances are in
tests/winattn_ref_cases.py; DESIGN section 27 has the derivation and the measured figures.

Every output element is compared with the fp64 reference of the same operation on the same
operands (rounded to the case dtype before either side saw them).  With
E(a) = max_i |a_i - g64_i| / (|g64_i| + 1e-3 max|g64|):

  fp32, both core kernels   E(gpu) <= 8 E(g32) and the max-norm 2e-5
  bf16, generic core        E(gpu) <= 8 E(g32) + 2^-8   (fp32 chain, one store rounding)
  bf16 MFMA core, blocks    |err_i| <= allow_i + 8 E(g32) den_i, allow_i the first-order
                            propagation of half a bf16 ulp per rounding point; no factor

Every launch also checks: ``sel`` equals the reference's keep flags exactly; outputs of
transparent windows are exactly 0 (core) or x bit for bit (block); the output was pre-filled
with a sentinel and its pad channels [C, ld) still hold it; the sources are unchanged (the pad
channels of qkv hold NaN, so a read past 3C shows).  Each launch prints "RATIO tag E(gpu)
allowance ratio ok|BAD"; a case runs all its launches and then fails with the list of bad ones."""
import os

import pytest
import torch

import winattn_ref_cases as wrc

pytestmark = pytest.mark.gpu

F32, BF16 = wrc.F32, wrc.BF16


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _pads_hold(out, C):
    return out.shape[-1] == C or bool((out[..., C:] == wrc.SENTINEL).all().item())


# ---------------------------------------------------------------------------------------
# Part A: the core alone
# ---------------------------------------------------------------------------------------
_CORE = [(c, dt) for c in wrc.CORE_CONFIGS for dt in (F32, BF16)]


@pytest.mark.parametrize("cfg,dt", _CORE,
                         ids=[f"{c.id}-{'f32' if dt == F32 else 'bf16'}" for c, dt in _CORE])
def test_winattn_core_vs_fp64(device, cfg, dt):
    from rgbac import _lib
    C, ws, heads = cfg.C, cfg.ws, cfg.heads
    scale = wrc.f32_scale(cfg.d)
    fails = []
    for i, ln in enumerate(wrc.core_launches(cfg)):
        ops = wrc.core_operands(cfg, ln, dt, 100 + i)
        bar, sel, _ = wrc.core_bar(cfg, ln, ops, dt)
        if bar is not None:
            bar.to(device)
        seld = sel.to(device)
        q = ops["qkv"].to(dt).to(device)
        dense = ops["dense"].to(device)
        alpha = None if ops["alpha"] is None else ops["alpha"].to(device)
        amask = None if ops["amask"] is None else ops["amask"].to(device)
        keepsrc = [(t, t.clone()) for t in (q, dense, alpha, amask) if t is not None]
        ldq, ldo = q.shape[-1], ops["ldo"]
        for hpb in ln.hpbs:
            tag = f"{cfg.id} {'f32' if dt == F32 else 'bf16'} {ln.tag()} hpb{hpb}"
            out = torch.full((ln.B, ln.H, ln.W, ldo), wrc.SENTINEL, dtype=dt, device=device)
            selb = None
            if alpha is not None:
                selb = torch.full((ln.B, ln.H, ln.W), wrc.SEL_SENTINEL, dtype=torch.uint8,
                                  device=device)
            _lib.call("rgbac_winattn_core_ex", _lib.dtype_code(dt), ln.B, ln.H, ln.W, C, heads, ws,
                      ln.shift, 0 if alpha is None else 1, scale, q.data_ptr(), ldq,
                      _lib.ptr(alpha), dense.data_ptr(), out.data_ptr(), ldo, _lib.ptr(selb),
                      _lib.ptr(amask), ln.amask_nw, hpb, _lib.stream_ptr(device))
            torch.cuda.synchronize()
            if not _pads_hold(out, C):
                fails.append(f"{tag}: a pad channel of the output was written")
            for t, t0 in keepsrc:
                if not torch.equal(_bits(t), _bits(t0)):
                    fails.append(f"{tag}: a source was written")
            if selb is not None and not torch.equal(selb, seld.to(torch.uint8)):
                fails.append(f"{tag}: sel differs from the reference's keep flags")
            got = out[..., :C].float()
            if not bool((got[~seld] == 0).all().item()):
                fails.append(f"{tag}: a transparent window's output is not exactly 0")
            if bar is not None:
                fails.append(wrc.ratio_line(tag, bar, got))
    fails = [f for f in fails if f]
    assert not fails, (len(fails), fails[:12])


# ---------------------------------------------------------------------------------------
# Part B: the fused blocks
# ---------------------------------------------------------------------------------------
def _module(case, ops, device):
    from rgbac.layers.masked_win_attention import WinBasedAttention
    m = WinBasedAttention(case.C, 8, case.ws, 0).to(device).eval()
    with torch.no_grad():
        m.attn.qkv.weight.copy_(ops["wq"].float())
        m.attn.qkv.bias.copy_(ops["bq"].float())
        m.attn.proj.weight.copy_(ops["wp"].float())
        m.attn.proj.bias.copy_(ops["bp"].float())
        m.attn.relative_position_bias_table.copy_(ops["table"].float())
    return m


@pytest.mark.parametrize("case", wrc.BLOCK_CASES, ids=[c.id for c in wrc.BLOCK_CASES])
def test_winattn_block_vs_fp64(device, case, monkeypatch):
    from rgbac import runtime as rt
    C = case.C
    x, ops = wrc.block_operands(case)
    m = _module(case, ops, device)
    f = rt.Feat(torch.zeros((case.B, case.H, case.W, C + 8), dtype=BF16, device=device), C)
    f.t[..., :C] = x.to(BF16).to(device)
    x0 = f.t.clone()
    xd = f.t[..., :C]

    def wide(B, H, W, Cn, dtype, dev, zero=None):      # run_block's output: sentinel, ld = C + 8
        return rt.Feat(torch.full((B, H, W, Cn + 8), wrc.SENTINEL, dtype=dtype, device=dev), Cn)
    monkeypatch.setattr(rt, "new_feat", wide)
    if case.form != "ws4":
        monkeypatch.setenv("RGBAC_WINBLOCK_FORM", "3" if case.form == "pair" else "2")
    fails = []
    for shift, kind, alpha in wrc.block_alphas(case):
        tag = f"{case.id} s{shift} {kind}"
        bar, keep, _, _ = wrc.block_bar(case, x, ops, shift, alpha)
        if bar is not None:
            bar.to(device)
        keepd = keep.to(device)
        ad = None if alpha is None else alpha.reshape(case.B, 1, case.H, case.W).to(device)
        a0 = None if ad is None else ad.clone()
        with torch.no_grad():
            assert m.attn.block_fused_ok(f, True, None)
            outs = [m.attn.run_block(f, ad, shift, ad is not None).t
                    for _ in range(1 if case.form == "ws4" else 2)]
        torch.cuda.synchronize()
        out = outs[0]
        assert out.shape[-1] == C + 8
        if len(outs) == 2 and not torch.equal(_bits(outs[0]), _bits(outs[1])):
            fails.append(f"{tag}: the second launch on the same workspace differs from the first")
        if not _pads_hold(out, C):
            fails.append(f"{tag}: a pad channel of the output was written")
        if not torch.equal(_bits(f.t), _bits(x0)) or (ad is not None and not torch.equal(ad, a0)):
            fails.append(f"{tag}: a source was written")
        got = out[..., :C]
        if not torch.equal(_bits(got[~keepd].contiguous()), _bits(xd[~keepd].contiguous())):
            fails.append(f"{tag}: a transparent window's pixels differ from x")
        if bar is not None:
            fails.append(wrc.ratio_line(tag, bar, got.float()))
    fails = [f for f in fails if f]
    assert not fails, (len(fails), fails[:12])
