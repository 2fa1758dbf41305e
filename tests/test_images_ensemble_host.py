"""Host side of the self-ensemble of predict_images / test_metrics and of the spread maps (no GPU): the numpy restatements of
tests/_ensemble_ref.py against their own properties, the keyword checks, and the argument checks of pssr_dihedral_batch_u8 / _f32,
pssr_ensemble_reduce_u8 and pssr_spread_stack_u8."""
import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch

import _blend_ref as B
import _ensemble_ref as R

ROOT = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------------------------------------ the oracle against its definitions
@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_reduce_of_the_members_of_an_image_is_the_image(E):
    a = np.random.default_rng(E).integers(0, 256, size=(3, 2, 7, 7)).astype(np.float32)       # nothing to clip
    members = R.members_ref(a, E)
    assert members.shape == (3 * E, 2, 7, 7) and members.dtype == np.float32
    np.testing.assert_array_equal(members[::E], a)
    if E == 8:
        assert len({m.tobytes() for m in members[:8]}) == 8
    mean, spread = R.reduce_ref(members, E)
    assert mean.dtype == spread.dtype == np.uint8
    np.testing.assert_array_equal(mean, a.astype(np.uint8))
    assert not spread.any()


@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_reduce_mean_is_the_stitch_of_a_one_tile_sheet(E):
    rng = np.random.default_rng(10 + E)
    y = rng.uniform(-40, 300, size=(2 * E, 2, 9, 9)).astype(np.float32)
    y.reshape(-1)[::11] = np.nan
    mean, spread = R.reduce_ref(y, E)
    q = np.clip(np.nan_to_num(y, nan=0.0), 0, 255).astype(np.uint8)
    turned = np.stack([B.U_d(q[g], g % E) for g in range(len(q))])
    for i in range(2):
        want = B.blend_ref(turned[i * E:(i + 1) * E], 1, 1, 1, 0, 0, 9, 9, "average", E)[0]
        np.testing.assert_array_equal(mean[i], want)
        np.testing.assert_array_equal(spread[i], turned[i * E:(i + 1) * E].max(0) - turned[i * E:(i + 1) * E].min(0))
    if E > 1:
        assert spread.any()
    else:
        assert not spread.any()


def test_clip_restated():
    y = np.array([np.nan, -0.0, -3.0, 0.999, 1.0, 254.999, 255.0, 255.5, 1e9, -1e9], dtype=np.float32)
    np.testing.assert_array_equal(R.clip_u8(y), [0, 0, 0, 0, 1, 254, 255, 255, 255, 0])


# n_slices, c, n_rows, n_cols, S, O, M
@pytest.mark.parametrize("case", [(2, 2, 3, 4, 12, 4, 3), (1, 1, 5, 5, 8, 6, 1), (1, 1, 1, 3, 12, 4, 1), (2, 1, 3, 4, 12, 4, 0)])
@pytest.mark.parametrize("E", [1, 8])
def test_spread_is_zero_exactly_where_nothing_covers(case, E):
    n_slices, c, n_rows, n_cols, S, O, M = case
    H, W = n_rows * (S - O) + O, n_cols * (S - O) + O
    n = n_slices * n_rows * n_cols * E
    # every tile a different constant: two tiles, or two members, over a pixel always differ, so the spread vanishes only where the
    # denominator of the blend does ... or where exactly one prediction covers the pixel
    preds = np.broadcast_to((np.arange(n, dtype=np.uint8) * 3 + 1).reshape(n, 1, 1, 1), (n, c, S, S))
    got = R.spread_stack_ref(preds, n_slices, n_rows, n_cols, O, M, H, W, E)
    assert got.shape == (n_slices, c, H, W) and got.dtype == np.uint8
    den = np.einsum("ry,qx->yx", B.axis_weights(S, O, M, n_rows, "linear"), B.axis_weights(S, O, M, n_cols, "linear"))
    cover = np.einsum("ry,qx->yx", B.axis_weights(S, O, M, n_rows, "average"), B.axis_weights(S, O, M, n_cols, "average")) * E
    np.testing.assert_array_equal(den == 0, cover == 0)
    ones = np.full((n, c, S, S), 255, dtype=np.uint8)
    blank = B.blend_ref(ones, n_slices, n_rows, n_cols, O, M, H, W, "linear", E)               # 255 where den > 0, 0 where den == 0
    np.testing.assert_array_equal(blank[0, 0] == 0, den == 0)
    for k in range(n_slices):
        for ch in range(c):
            np.testing.assert_array_equal(got[k, ch] == 0, cover <= 1)
            assert not got[k, ch][den == 0].any()
    if M == 3:
        assert (den == 0).any()
    np.testing.assert_array_equal(R.spread_stack_ref(preds, n_slices, n_rows, n_cols, O, M, H - 3, W - 5, E), got[..., :H - 3, :W - 5])


def test_spread_of_one_member_without_overlap_is_zero():
    preds = np.random.default_rng(4).integers(0, 256, size=(2 * 2 * 3, 2, 12, 12), dtype=np.uint8)
    got = R.spread_stack_ref(preds, 2, 2, 3, 0, 0, 24, 36, 1)
    assert got.shape == (2, 2, 24, 36) and not got.any()
    eight = np.random.default_rng(5).integers(0, 256, size=(2 * 3 * 8, 1, 12, 12), dtype=np.uint8)
    got = R.spread_stack_ref(eight, 1, 2, 3, 0, 0, 24, 36, 8)
    np.testing.assert_array_equal(got[0, 0, :12, 12:24], eight[8:16, 0].max(0).astype(np.int64) - eight[8:16, 0].min(0))


# ------------------------------------------------------------------------------------------------ keyword checks
class _Never(torch.nn.Module):
    def forward(self, x):                              # pragma: no cover
        raise AssertionError("the keyword checks come before the model runs")

    def to(self, *a, **k):                             # pragma: no cover
        raise AssertionError("the keyword checks come before the model moves")


class _NoData:
    def __getattr__(self, name):                       # pragma: no cover
        raise AssertionError(f"the keyword checks come before the dataset is touched ({name})")


@pytest.mark.parametrize("kw,error,word", [(dict(ensemble=3), ValueError, "ensemble"), (dict(ensemble=0), ValueError, "ensemble"),
                                           (dict(ensemble=16), ValueError, "ensemble"), (dict(ensemble=None), ValueError, "ensemble"),
                                           (dict(spread=True), ValueError, "spread"), (dict(ensemble=1, spread=True), ValueError, "spread"),
                                           (dict(ensemble=4, device="cpu"), RuntimeError, "no CPU fallback"),
                                           (dict(ensemble=8, spread=True, device="cpu"), RuntimeError, "no CPU fallback")])
def test_predict_images_checks_its_keywords_first(kw, error, word):
    from pssr2_amd.predict import predict_images
    kw = {"device": "cuda", **kw}
    with pytest.raises(error, match=word):
        predict_images(_Never(), _NoData(), out_dir=None, **kw)


@pytest.mark.parametrize("kw,error,word", [(dict(ensemble=3), ValueError, "ensemble"), (dict(ensemble=-8), ValueError, "ensemble"),
                                           (dict(ensemble=2, device="cpu"), RuntimeError, "no CPU fallback")])
def test_test_metrics_checks_its_keyword_first(kw, error, word):
    from pssr2_amd.predict import test_metrics
    kw = {"device": "cuda", **kw}
    with pytest.raises(error, match=word):
        test_metrics(_Never(), _NoData(), **kw)


def test_new_arguments_are_keyword_only():
    import inspect
    from pssr2_amd import predict as P
    for fn, names in ((P.predict_images, ("ensemble", "spread")), (P.test_metrics, ("ensemble",)), (P.predict_sheet, ("spread",))):
        params = inspect.signature(fn).parameters
        for name in names:
            assert params[name].kind is inspect.Parameter.KEYWORD_ONLY
            assert params[name].default == (1 if name == "ensemble" else False)
    with pytest.raises(ValueError, match="ensemble"):
        P.predict_sheet(_Never(), np.zeros((1, 40, 40), dtype=np.uint8), tile_res=16, overlap=4, device="cuda", ensemble=3, spread=True)


def test_ensemble_helper_refuses_what_cannot_be_turned():
    from pssr2_amd.predict import _ensemble_pred
    with pytest.raises(ValueError, match="square"):
        _ensemble_pred(_Never(), torch.zeros(2, 1, 8, 12), 4, 2)
    with pytest.raises(ValueError, match="square"):
        _ensemble_pred(_Never(), torch.zeros(1, 8, 8), 4, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _ensemble_pred(_Never(), torch.zeros(2, 1, 8, 8), 4, 2)


# ------------------------------------------------------------------------------------------------ argument checks of the entry points
def _lib():
    path = ROOT / "pssr2_amd" / "libpssr_mi355.so"
    if not path.exists():
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(str(path))
    lib.pssr_last_error.restype = ctypes.c_char_p
    return lib


def test_ensemble_entry_points_validate_without_gpu():
    """Every check happens before the launch: an error code and a message, no crash, no device needed."""
    lib = _lib()
    assert lib.pssr_abi_version() == 5
    i, p = ctypes.c_int, ctypes.c_void_p
    turn_u8, turn_f32, reduce, spread = (lib.pssr_dihedral_batch_u8, lib.pssr_dihedral_batch_f32, lib.pssr_ensemble_reduce_u8,
                                         lib.pssr_spread_stack_u8)
    turn_u8.argtypes = turn_f32.argtypes = [p, p] + [i] * 4 + [p]
    reduce.argtypes = [p, p, p] + [i] * 4 + [p]
    spread.argtypes = [p, p] + [i] * 10 + [p]
    fake = 0x1000          # never dereferenced: every call below fails its checks

    def err(status, word):
        return status == -1 and word in lib.pssr_last_error()

    # in, out, n, m, size, ensemble
    for turn in (turn_u8, turn_f32):
        assert err(turn(None, fake, 3, 2, 33, 8, None), b"null")
        assert err(turn(fake, None, 3, 2, 33, 8, None), b"null")
        for bad in (0, 3, 5, 16, -1):
            assert err(turn(fake, fake, 3, 2, 33, bad, None), b"ensemble")
        for bad in ((0, 2, 33), (3, 0, 33), (3, 2, 0), (-1, 2, 33), (3, 2, -4)):
            assert err(turn(fake, fake, *bad, 8, None), b"positive")
        assert err(turn(fake, fake, 1 << 29, 1, 4, 8, None), b"32-bit")
        assert err(turn(fake, fake, 1, 1, (1 << 31) - 8, 8, None), b"32-bit")
    assert b"dihedral_batch_f32" in lib.pssr_last_error()

    # in, mean, spread (may be null), n, c, size, ensemble
    assert err(reduce(None, fake, fake, 3, 2, 33, 8, None), b"null")
    assert err(reduce(fake, None, fake, 3, 2, 33, 8, None), b"null")
    assert err(reduce(None, None, None, 3, 2, 33, 8, None), b"null")
    for bad in (0, 3, 6, 16):
        assert err(reduce(fake, fake, None, 3, 2, 33, bad, None), b"ensemble")
    for bad in ((0, 2, 33), (3, 0, 33), (3, 2, 0), (3, -2, 33)):
        assert err(reduce(fake, fake, fake, *bad, 8, None), b"positive")
    assert err(reduce(fake, fake, fake, 1 << 30, 1, 4, 2, None), b"32-bit")
    assert err(reduce(fake, fake, fake, 1, 1, 1 << 30, 2, None), b"32-bit")

    # tiles, out, n_slices, c, n_rows, n_cols, size, overlap, margin, out_h, out_w, ensemble; the stitched sheet is 80 by 104
    assert err(spread(None, fake, 3, 2, 3, 4, 32, 8, 3, 80, 104, 8, None), b"null")
    assert err(spread(fake, None, 3, 2, 3, 4, 32, 8, 3, 80, 104, 8, None), b"null")
    for bad in (0, 3, 7, 16):
        assert err(spread(fake, fake, 3, 2, 3, 4, 32, 8, 3, 80, 104, bad, None), b"ensemble")
    assert err(spread(fake, fake, 3, 2, 3, 4, 32, 8, 3, 81, 104, 8, None), b"crop")
    assert err(spread(fake, fake, 3, 2, 3, 4, 32, 8, 3, 80, 0, 8, None), b"crop")
    assert err(spread(fake, fake, 3, 2, 3, 4, 32, 8, 9, 80, 104, 8, None), b"margin")
    assert err(spread(fake, fake, 3, 2, 3, 4, 32, 32, 3, 80, 104, 8, None), b"margin")
    assert err(spread(fake, fake, 0, 2, 3, 4, 32, 8, 3, 80, 104, 8, None), b"bad args")
    assert err(spread(fake, fake, 3, 2, 3, 4, 0, 0, 0, 80, 104, 8, None), b"bad args")
    assert err(spread(fake, fake, 3, 2, 1 << 16, 1 << 16, 32, 8, 3, 80, 104, 8, None), b"32-bit")
    assert b"spread_stack" in lib.pssr_last_error()
