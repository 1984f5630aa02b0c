"""CPU: the MS-SSIM backward entry points (csrc/msssim_bwd.hip) reject bad arguments with a
RuntimeError before any launch -- zero batch, an even or > 15 window, an image smaller than the
window, mask channels not in {1, C}, null pointers.  No kernel runs here; the pointers that are
not null are dummies that a launch would never be allowed to see."""
import pytest

P = 0x1000      # a non-null dummy pointer: every call below must fail before it is used


def _plain(batch=1, channels=3, h=32, w=32, ws=11, x=P, y=P, win=P, dx=None, dy=P):
    from rgbac import _lib
    _lib.call("rgbac_ssim_level_bwd", batch, channels, h, w, ws, x, y, win, 1e-4, 9e-4, P, P,
              None, None, dx, dy, None)


def _masked(batch=1, channels=3, cm=1, h=32, w=32, ws=11, x=P, y=P, mask=P, win=P, part=P,
            dx=None, dy=P):
    from rgbac import _lib
    _lib.call("rgbac_masked_ssim_level_bwd", batch, channels, cm, h, w, ws, x, y, mask, win,
              1e-4, 9e-4, part, P, P, 1, None, None, dx, dy, None)


@pytest.mark.parametrize("fn", [_plain, _masked])
def test_level_bwd_rejects_bad_arguments(fn):
    name = "rgbac_ssim_level_bwd" if fn is _plain else "rgbac_masked_ssim_level_bwd"
    with pytest.raises(RuntimeError, match=name + r" failed.*shape"):
        fn(batch=0)
    with pytest.raises(RuntimeError, match="shape"):
        fn(channels=0)
    for ws in (10, 17, 0):
        with pytest.raises(RuntimeError, match="window size"):
            fn(ws=ws)
    with pytest.raises(RuntimeError, match="smaller than the window"):
        fn(h=10)
    with pytest.raises(RuntimeError, match="smaller than the window"):
        fn(w=8, ws=9)
    for null in ("x", "y", "win", "dy"):          # dy=None with dx=None: no output at all
        with pytest.raises(RuntimeError, match="null pointer"):
            fn(**{null: None})


def test_masked_level_bwd_rejects_mask_channels_and_null_mask():
    for cm in (0, 2, 4):
        with pytest.raises(RuntimeError, match="mask channels"):
            _masked(cm=cm)
    with pytest.raises(RuntimeError, match="null pointer"):
        _masked(mask=None)
    with pytest.raises(RuntimeError, match="null pointer"):
        _masked(part=None)


def test_combine_bwd_rejects_bad_arguments():
    from rgbac import _lib

    def plain(levels=2, batch=1, mcs=P, s=P, w=P, g=P, u=P):
        _lib.call("rgbac_msssim_combine_bwd", levels, batch, mcs, s, w, g, 1, u, None)

    def masked(levels=2, batch=1, channels=3, mcs=P, s=P, w=P, g=P, u=P):
        _lib.call("rgbac_masked_msssim_combine_bwd", levels, batch, channels, mcs, s, w, g, 1, u,
                  None)

    for fn, name in ((plain, "rgbac_msssim_combine_bwd"),
                     (masked, "rgbac_masked_msssim_combine_bwd")):
        with pytest.raises(RuntimeError, match=name + r" failed.*arguments"):
            fn(batch=0)
        with pytest.raises(RuntimeError, match="arguments"):
            fn(levels=0)
        for null in ("mcs", "s", "w", "g", "u"):
            with pytest.raises(RuntimeError, match="null pointer"):
                fn(**{null: None})
    with pytest.raises(RuntimeError, match="arguments"):
        masked(channels=0)
