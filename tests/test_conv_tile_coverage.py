"""CPU: what the conv tile case table (tests/conv_tile_cases.py) reaches, asked of the
library's describe entry point as tests/test_conv_dispatch.py does (records with CPU pointers:
nothing is launched or dereferenced, no GPU needed).  tests/test_gpu_conv_tiles.py launches
exactly these (case, tile, ksplit) triples on the GPU."""
import json
import os

import pytest

import conv_tile_cases as ctc

HERE = os.path.dirname(os.path.abspath(__file__))

# Kernel names of the model's own launches (the fixture's) the table may leave out: only a name
# the library refuses at every shape of at most 32 x 32 pixels, with the refusing rule's text.
EXEMPT = {}

# Distinct kernel names the table reaches (the fixture has 138, the library 180 instantiations):
# a case deleted later shows here.
NAMES_REACHED = 156


@pytest.fixture(scope="module")
def reached():
    """{kernel name: [(case id, scope, dtype, tile, ksplit), ...]} over the whole table."""
    from rgbac import runtime as rt
    out = {}
    for case in ctc.all_cases():
        preps, _ = ctc.build_preps(rt, case, ctc.build_operands(case), "cpu")
        todo = ctc.pairs(rt, case, preps)
        assert todo, f"{case.id}: no tile takes this case"
        for tile, ks in todo:
            rc, name = rt._describe(tile, ks, preps)
            assert rc == 0 and name, (case.id, tile, ks)
            out.setdefault(name, []).append((case.id, case.scope, case.dtype, tile, ks))
    return out


def test_every_tile_has_a_geometry_case(reached):
    from rgbac import runtime as rt
    got = {(dtype, tile) for hits in reached.values() for _, scope, dtype, tile, _ in hits
           if scope == "geometry"}
    for tile in range(len(rt.TILES)):
        assert ("bf16", tile) in got, f"tile {tile}: no bf16 geometry case"
        if ctc.kind_of(rt, tile) in ctc.F32_KINDS:
            assert ("f32", tile) in got, f"tile {tile}: no fp32 geometry case"
        else:
            assert ("f32", tile) not in got, f"tile {tile} takes fp32: add it to F32_KINDS"


def test_every_kernel_of_the_model_is_reached(reached):
    with open(os.path.join(HERE, "golden", "conv_dispatch.json")) as fh:
        names = json.load(fh)["names"]
    assert len(names) == 138
    missing = sorted(set(names) - set(reached) - set(EXEMPT))
    assert not missing, missing
    assert not set(EXEMPT) & set(reached), "an exempt kernel is reached: drop the exemption"
    assert EXEMPT == {}


def test_reached_kernel_count_is_pinned(reached):
    assert len(reached) == NAMES_REACHED, sorted(reached)


def test_every_epilogue_reaches_every_kind_that_takes_it(reached):
    """An epilogue case runs on one tile of every kernel kind the library accepts it on; the
    kinds that take the plain gelu + res0 + bias case of a shape take most of the list, so a
    shape whose epilogue cases lost a whole kind shows here."""
    from rgbac import runtime as rt
    kinds = {}
    for hits in reached.values():
        for cid, scope, _, tile, ks in hits:
            if scope == "epilogue" and ks == 1:
                kinds.setdefault(cid, set()).add(ctc.kind_of(rt, tile))
    for d in ("f32", "bf16"):
        base = kinds[f"e-pt-gelu-res0-{d}"]
        assert base >= ({"stream", "deep", "pers", "wres", "direct"} if d == "f32" else
                        {"stream", "deep", "pers", "wres", "direct", "smallk", "pw"})
        for name in ("nobias", "bias", "relu", "lrelu", "res0-res2", "zout", "coff8", "sqbwd",
                     "dgelu", "dlrelu", "masksel", "tanh-res1", "gate-res1-res2", "grouped"):
            assert kinds[f"e-pt-{name}-{d}"] == base, (name, d)
    assert kinds["e-k3-gelu-res0-bf16"] >= {"stream", "deep", "pers", "patch", "fpatch",
                                            "fpatch_ks"}
    assert kinds["e-narrow-gelu-res0-bf16"] == {"wstream", "npatch"}
    assert kinds["e-sp-gelu-res0-bf16"] == {"spatial"}
