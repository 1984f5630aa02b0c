"""Generate tests/golden/conv_dispatch.json: the conv dispatch answers (candidate lists, tile
validity, kernel names, cached-choice fallbacks) of rgbac.runtime on fabricated convs.

Corpus: every key of the committed profiles/tune_*.json, rebuilt as Prepared-like records
with fake 16-byte-aligned pointers (nothing is launched or dereferenced: no GPU needed),
crossed with the variants of VARIANTS that the key's shape admits.

    python tests/golden/make_conv_dispatch.py [out.json]

The committed fixture was recorded at the commit named in its "recorded_at" field, before
the Python mirrors of the launcher's rules were removed; tests/test_conv_dispatch.py holds
every later commit to those answers.  A tile counts as valid there when the Python rule of
that commit offered it AND the library's argument checks accepted it (the rule alone let a
few launches through that the library then refused with an error)."""
import glob
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PKG = os.path.join(ROOT, "deep-learning-based-rgba-image-compression-with-masked-window-based-attention_amd")
sys.path[:0] = [ROOT, PKG]

NTILES = 59
# name -> (needs, settings); the cross product is thinned: the epilogue variants run with a
# fragment-major copy, one source and ksplit 1 only
VARIANTS = {
    "frag": "pack has a fragment-major copy (1) or not (0)",
    "nsrc": "1, 2, 3 sources: splits of cin_pad in multiples of 8",
    "ks": "ksplit 1, and 4 where _patch_split_ok holds",
    "gdn/igdn": "1x1 stride-1 keys: square_input, res1 == src",
    "gate": "1x1 stride-1 keys: res1 + res2",
    "tanh": "1x1 stride-1 keys: tanh-half with res1",
    "zout": "1x1 stride-1 keys: a pre-activation store",
    "dact": "/dact keys: dgelu with res0, no bias (always)",
    "gauss": "GAUSS keys: res1 and a partial buffer (always)",
}


def round_up(x, m):
    return (x + m - 1) // m * m


def parse_key(key):
    f = key.split("/")
    B, H, W = (int(v) for v in f[4].split("x"))
    return dict(dtype=int(f[0]), mode=int(f[1]), ksize=int(f[2]), stride=int(f[3]), B=B, H=H, W=W,
                cin_pad=int(f[5]), cout=int(f[6]), gauss=f[7] == "True", dact="dact" in f[8:-1],
                n=int(f[-1][1:]))


def fabricate(rt, key, frag=True, nsrc=1, epi=None):
    """The grouped convs of a tune-cache key as Prepared-like records, or None if the shape
    does not admit the variant."""
    from rgbac import _lib
    k = parse_key(key)
    if k["cin_pad"] < 8 * nsrc:
        return None
    one = k["mode"] == rt.CONV and k["ksize"] == 1 and k["stride"] == 1
    if epi and (not one or k["gauss"] or k["dact"]):
        return None
    H, W, ks, st = k["H"], k["W"], k["ksize"], k["stride"]
    if k["mode"] == rt.CONV:
        Ho, Wo = (H + 2 * (ks // 2) - ks) // st + 1, (W + 2 * (ks // 2) - ks) // st + 1
        cstore = k["cout"]
    else:
        Ho, Wo = 2 * H, 2 * W
        cstore = k["cout"] if k["mode"] == rt.CONVT_S2 else k["cout"] // 4
    act = "gauss" if k["gauss"] else "dgelu" if k["dact"] else \
        {"gdn": "gdn", "igdn": "igdn", "gate": "gate", "tanh": "tanh_half"}.get(epi, "none")
    if act == "gauss":
        cstore = k["cout"] // 2
    taps = 9 if k["mode"] == rt.CONVT_S2 else ks * ks
    es = 32 if k["dtype"] == 0 else 64
    chunks = k["cin_pad"] // 8
    split = [8 * (chunks // nsrc + (1 if j < chunks % nsrc else 0)) for j in range(nsrc)]
    preps = []
    for i in range(k["n"]):
        base = 0x10000000 * (i + 1)
        a = _lib.ConvArgs()
        a.dtype, a.mode, a.batch, a.in_h, a.in_w = k["dtype"], k["mode"], k["B"], H, W
        a.ksize, a.stride, a.nsrc = ks, st, nsrc
        for j, ch in enumerate(split):
            a.src[j].ptr, a.src[j].ldc, a.src[j].channels = base + 0x100000 * j, ch, ch
        a.cin_pad, a.k_pad = k["cin_pad"], round_up(taps * k["cin_pad"], 64)
        a.weight, a.bias = base + 0x400000, (None if k["dact"] else base + 0x500000)
        a.cout, a.cout_pad = k["cout"], round_up(k["cout"], 128)
        a.out_h, a.out_w, a.out, a.out_ldc = Ho, Wo, base + 0x600000, round_up(cstore, 8)
        a.act = rt.ACT[act]
        if epi in ("gdn", "igdn"):
            a.square_input, a.res1, a.res1_ldc = 1, a.src[0].ptr, a.src[0].ldc
        elif epi in ("gate", "tanh") or k["gauss"]:
            a.res1, a.res1_ldc = base + 0x700000, a.out_ldc
        if epi == "gate":
            a.res2, a.res2_ldc = base + 0x800000, a.out_ldc
        if epi == "zout":
            a.zout, a.zout_ldc = base + 0x900000, a.out_ldc
        if k["dact"]:
            a.res0, a.res0_ldc = base + 0xa00000, a.out_ldc
        if k["gauss"]:
            a.partial = base + 0xb00000
        pk = types.SimpleNamespace(mode=k["mode"], ksize=ks, stride=st, cin_pad=k["cin_pad"],
                                   cout=k["cout"], cout_pad=a.cout_pad, k_pad=a.k_pad,
                                   frag=object() if frag else None)
        preps.append(types.SimpleNamespace(
            a=a, pk=pk, key=key.rsplit("/", 1)[0], partial=None,
            mgrid=k["B"] * (H * W if k["mode"] != rt.CONV else Ho * Wo),
            nphase=4 if k["mode"] == rt.CONVT_S2 else 1,
            nst=-(-taps * k["cin_pad"] // es), nks=-(-taps * k["cin_pad"] // (es // 2))))
    return preps


def cases(rt, key):
    """(variant name, preps, ksplit) of every variant the key's shape admits."""
    for frag in (1, 0):
        for nsrc in (1, 2, 3):
            preps = fabricate(rt, key, bool(frag), nsrc)
            if preps is None:
                continue
            yield f"frag{frag}/nsrc{nsrc}/ks1", preps, 1
            if rt._patch_split_ok(preps):
                yield f"frag{frag}/nsrc{nsrc}/ks4", preps, 4
    for epi in ("gdn", "igdn", "gate", "tanh", "zout"):
        preps = fabricate(rt, key, True, 1, epi)
        if preps is not None:
            yield epi, preps, 1


def answers(rt, preps, ks, cached):
    """One case's record: candidates, per-tile validity at ``ks`` (a string of 0/1), the
    kernel name of every valid tile, and what launch() makes of each cached choice."""
    valid = [rt._choice_valid(t, preps, ks) for t in range(NTILES)]
    return {"cands": [list(c) for c in rt.candidates(preps)],
            "valid": "".join("01"[v] for v in valid),
            "names": [rt.kernel_name(t, preps) for t in range(NTILES) if valid[t]],
            "fallback": [[list(c), list(rt.resolve_choice(tuple(c), preps))] for c in cached]}


def corpus():
    """{key: sorted distinct cached choices} over the committed tune caches."""
    out = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "tune_*.json"))):
        with open(path) as fh:
            for key, choice in json.load(fh).items():
                out.setdefault(key, set()).add(tuple(choice))
    return {k: sorted(v) for k, v in sorted(out.items())}


def generate(rt):
    """{"names": [...], "records": [...], "cases": {key: {variant: record index}}}: kernel
    names and whole records are stored once and referred to by index."""
    names, records, index, out = [], [], {}, {}
    for key, cached in corpus().items():
        for var, preps, ks in cases(rt, key):
            r = answers(rt, preps, ks, cached)
            for nm in r["names"]:
                if nm not in names:
                    names.append(nm)
            r["names"] = [names.index(nm) for nm in r["names"]]
            blob = json.dumps(r, sort_keys=True)
            if blob not in index:
                index[blob] = len(records)
                records.append(r)
            out.setdefault(key, {})[var] = index[blob]
    return {"names": names, "records": records, "cases": out}


def expand(fix, rec):
    """A stored record with its kernel names written out (the form ``answers`` returns)."""
    return dict(rec, names=[fix["names"][i] for i in rec["names"]])


def main(out_path, recorded_at):
    from rgbac import runtime as rt
    fix = {"recorded_at": recorded_at, "variants": VARIANTS, "tiles": NTILES}
    fix.update(generate(rt))
    with open(out_path, "w") as fh:
        json.dump(fix, fh, separators=(",", ":"))
        fh.write("\n")
    n = sum(len(v) for v in fix["cases"].values())
    print(f"{out_path}: {len(fix['cases'])} keys, {n} cases, {len(fix['records'])} records, "
          f"{os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    import subprocess
    head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True,
                          text=True).stdout.strip()
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "conv_dispatch.json"), head)
