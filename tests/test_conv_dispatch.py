"""CPU: the conv dispatch answers (candidate lists, tile validity, kernel names, what launch()
makes of a cached choice) are those recorded in tests/golden/conv_dispatch.json, for every
key of the committed tune caches crossed with the variants of its header (fabricated convs
with fake pointers: the library's describe entry point launches and dereferences nothing).
The fixture was recorded before the launcher's rules had a single home in csrc/conv.hip; see
tests/golden/make_conv_dispatch.py."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location(
        "make_conv_dispatch", os.path.join(HERE, "golden", "make_conv_dispatch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(HERE, "golden", "conv_dispatch.json")) as fh:
        return json.load(fh)


def test_corpus_is_every_tune_cache_key(gen, fixture):
    from rgbac import runtime as rt
    assert fixture["tiles"] == len(rt.TILES) == gen.NTILES
    assert fixture["variants"] == gen.VARIANTS
    corpus = gen.corpus()
    assert len(corpus) >= 200
    assert set(fixture["cases"]) == set(corpus)
    for key in corpus:
        assert set(fixture["cases"][key]) == {v for v, _, _ in gen.cases(rt, key)}, key


def test_dispatch_answers_are_the_recorded_ones(gen, fixture):
    from rgbac import runtime as rt
    corpus = gen.corpus()
    n = 0
    for key, cached in corpus.items():
        for var, preps, ks in gen.cases(rt, key):
            want = gen.expand(fixture, fixture["records"][fixture["cases"][key][var]])
            got = gen.answers(rt, preps, ks, cached)
            assert got == want, (key, var, {k: (got[k], want[k]) for k in got if got[k] != want[k]})
            n += 1
    assert n == sum(len(v) for v in fixture["cases"].values()) and n > 1000


def test_describe_refusal_matches_the_launch(gen):
    """A refusal of the describe entry point carries the launch's status and error text (the
    launch validates before its first HIP call, so it can be asked here too), and the checks
    on buffers that exist only once a choice is set are exempt."""
    import ctypes
    from rgbac import _lib
    from rgbac import runtime as rt
    lib = _lib.load()
    preps = gen.fabricate(rt, "1/0/3/1/8x32x32/192/192/False/g1", True, 2)
    arr = (_lib.ConvArgs * 1)()
    arr[0] = preps[0].a
    for tile, ks in ((rt.TILE_PW, 1), (rt.TILE_SMALLK, 1), (7, 1), (rt.TILE_NPATCH, 1), (36, 2)):
        arr[0].tile, arr[0].ksplit = tile, ks
        rc = lib.rgbac_conv2d_grouped_describe(ctypes.addressof(arr), 1, None, 0)
        msg = lib.rgbac_last_error()
        assert rc == -1 and msg
        assert lib.rgbac_conv2d_grouped(ctypes.addressof(arr), 1, None) == rc
        assert lib.rgbac_last_error() == msg
    # split-K without a workspace: the launch refuses, describe names the kernel
    arr[0].tile, arr[0].ksplit = 1, 2
    name = ctypes.create_string_buffer(96)
    assert lib.rgbac_conv2d_grouped_describe(ctypes.addressof(arr), 1, name, 96) == 0
    assert name.value == b"conv_kernel<bf16_t, 128, 64, 4, 1, 3, 1>"
    assert lib.rgbac_conv2d_grouped(ctypes.addressof(arr), 1, None) == -1
    assert b"workspace" in lib.rgbac_last_error()
