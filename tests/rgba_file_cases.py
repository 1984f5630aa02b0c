"""Shared by the RGBA file tests: the conv launches of latent_code (rgbac/models/_codec.py) as
Prepared records on CPU tensors -- nothing is launched, the tile rule and the library's describe
entry point only look at shapes -- and the fixed-rule answers of the commit before the
per-image mode existed (tests/golden/fixed_rule_legacy.json, written by
tests/golden/make_fixed_rule.py)."""
import functools
import json
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LEGACY_JSON = os.path.join(HERE, "golden", "fixed_rule_legacy.json")
BATCHES = (1, 3, 4, 8)
CANVASES = ((64, 64), (128, 128))
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
MODELS = ("alpha", "rgb")


@functools.lru_cache(maxsize=None)
def model(which):
    torch.manual_seed(7)
    if which == "alpha":
        from rgbac.models.AutoEncoderMask_Journal import AutoEncoder
    else:
        from rgbac.models.AutoEncoderRGB_Journal import AutoEncoder
    return AutoEncoder().eval()


def latent_launches(which, B, H, W, dtype):
    """[(name, [Prepared, ...]), ...]: every grouped conv launch of latent_code for a B x H x W
    input, encode and decode sides, in its order: hyper-analysis, hyper-synthesis, then per
    slice wave cc_* (two layers), mu|sigma, lrp_* (three layers)."""
    import torch.nn as nn
    from rgbac import runtime as rt
    from rgbac.layers.TransformRGB import prep_conv, prep_subpel
    from rgbac.models._latent import _musigma_pack
    m = model(which)
    dev = torch.device("cpu")
    ns, msup, M = m.num_slices, m.max_support_slices, m.h_a[0].in_channels
    cs = M // ns
    h, w = H // 8, W // 8
    out = []

    def add(name, preps):
        out.append((name, preps))
        return [pr.out for pr in preps]

    t = rt.new_feat(B, h, w, M, dtype, dev)
    for idx in (0, 2, 4, 6, 8):
        t, = add(f"h_a.{idx}", [prep_conv(m.h_a[idx], [t.src()], act="gelu" if idx != 8 else "none")])
    z_hat = rt.new_feat(B, t.H, t.W, t.C, dtype, dev)
    hs, ts = (m.h_scale_s, m.h_mean_s), [z_hat, z_hat]
    for idx in (0, 2, 4, 6, 8):
        act = "gelu" if idx != 8 else "none"
        ts = add(f"h_s.{idx}", [prep_subpel(hh[idx], [tt.src()], act=act)
                                if isinstance(hh[idx], nn.Sequential)
                                else prep_conv(hh[idx], [tt.src()], act=act) for hh, tt in zip(hs, ts)])
    scales, means = ts
    YH = rt.new_feat(B, h, w, M, dtype, dev)
    waves = [[i] for i in range(min(msup, ns))]
    if ns > msup:
        waves.append(list(range(msup, ns)))
    for wave in waves:
        sup = [cs * min(i, msup) for i in wave]
        k, tag = len(wave), f"slice{wave[0]}"
        t1 = add(f"{tag}.cc.0",
                 [prep_conv(m.cc_mean_transforms[i][0], [means.src(), YH.src(0, s)], act="gelu")
                  for i, s in zip(wave, sup)] +
                 [prep_conv(m.cc_scale_transforms[i][0], [scales.src(), YH.src(0, s)], act="gelu")
                  for i, s in zip(wave, sup)])
        t2 = add(f"{tag}.cc.2",
                 [prep_conv(m.cc_mean_transforms[i][2], [t1[j].src()], act="gelu")
                  for j, i in enumerate(wave)] +
                 [prep_conv(m.cc_scale_transforms[i][2], [t1[k + j].src()], act="gelu")
                  for j, i in enumerate(wave)])
        add(f"{tag}.musigma",
            [rt.prepare(_musigma_pack(m.cc_mean_transforms[i][4], m.cc_scale_transforms[i][4],
                                      dtype, t2[j].ldc), [t2[j].src(), t2[k + j].src()],
                        out=rt.new_feat(B, h, w, 2 * cs, dtype, dev)) for j, i in enumerate(wave)])
        pres = [rt.new_feat(B, h, w, cs, dtype, dev) for _ in wave]
        l1 = add(f"{tag}.lrp.0",
                 [prep_conv(m.lrp_transforms[i][0], [means.src(), YH.src(0, s), pres[j].src()],
                            act="gelu") for j, (i, s) in enumerate(zip(wave, sup))])
        l2 = add(f"{tag}.lrp.2", [prep_conv(m.lrp_transforms[i][2], [l1[j].src()], act="gelu")
                                  for j, i in enumerate(wave)])
        add(f"{tag}.lrp.4", [prep_conv(m.lrp_transforms[i][4], [l2[j].src()], out=YH,
                                       out_coff=i * cs, act="tanh_half", res1=pres[j])
                             for j, i in enumerate(wave)])
    return out


def configs():
    for which in MODELS:
        for dname in DTYPES:
            for H, W in CANVASES:
                yield which, dname, H, W


def config_key(which, dname, H, W, B):
    return f"{which}/{dname}/{H}x{W}/B{B}"


def legacy_answers():
    with open(LEGACY_JSON) as fh:
        return json.load(fh)
