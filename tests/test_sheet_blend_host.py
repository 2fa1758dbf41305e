"""Host side of predict_sheet's ``blend`` / ``ensemble`` (no GPU): the keyword checks, the argument checks of pssr_dihedral_tiles_u8 /
pssr_clip_u8_dihedral / pssr_blend_stack_u8, and the numpy restatements of tests/_blend_ref.py against their own definitions."""
import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch

import _blend_ref as R

ROOT = Path(__file__).resolve().parent.parent


class _Never(torch.nn.Module):
    def forward(self, x):                              # pragma: no cover
        raise AssertionError("the keyword checks come before the model runs")


@pytest.mark.parametrize("kw,word", [(dict(blend="cubic"), "blend"), (dict(ensemble=3), "ensemble"), (dict(ensemble=0), "ensemble"),
                                     (dict(ensemble=16), "ensemble"), (dict(blend=None), "blend")])
def test_predict_sheet_refuses_unknown_blend_and_ensemble_before_any_device_work(kw, word):
    from pssr2_amd.predict import predict_sheet
    with pytest.raises(ValueError, match=word):
        predict_sheet(_Never(), np.zeros((1, 40, 40), dtype=np.uint8), tile_res=16, overlap=4, device="cuda", **kw)


def test_reassemble_sheets_refuses_unknown_blend(tmp_path):
    from pssr2_amd.util import reassemble_sheets
    with pytest.raises(ValueError, match="blend"):
        reassemble_sheets({}, str(tmp_path), 4, blend="cubic")


def _lib():
    path = ROOT / "pssr2_amd" / "libpssr_mi355.so"
    if not path.exists():
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(str(path))
    lib.pssr_last_error.restype = ctypes.c_char_p
    return lib


def test_blend_entry_points_validate_without_gpu():
    """Every check happens before the launch: an error code and a message, no crash, no device needed."""
    lib = _lib()
    assert lib.pssr_abi_version() == 5
    i, p = ctypes.c_int, ctypes.c_void_p
    cut, clip, blend = lib.pssr_dihedral_tiles_u8, lib.pssr_clip_u8_dihedral, lib.pssr_blend_stack_u8
    cut.argtypes = [p, p] + [i] * 12 + [p]
    clip.argtypes = [p, p] + [i] * 5 + [p]
    blend.argtypes = [p, p] + [i] * 11 + [p]
    fake = 0x1000          # never dereferenced: every call below fails its checks

    def err(status, word):
        return status == -1 and word in lib.pssr_last_error()

    # stack, tiles, frames, h, w, m, frame_step, size, stride, tiles_y, tiles_x, ensemble, item0, nitem: 5 slices of 12 tiles, 480 items
    assert err(cut(None, fake, 7, 45, 38, 3, 1, 16, 12, 4, 3, 8, 0, 480, None), b"null")
    assert err(cut(fake, None, 7, 45, 38, 3, 1, 16, 12, 4, 3, 8, 0, 480, None), b"null")
    for bad in (0, 3, 5, 16, -1):
        assert err(cut(fake, fake, 7, 45, 38, 3, 1, 16, 12, 4, 3, bad, 0, 1, None), b"ensemble")
    assert err(cut(fake, fake, 7, 45, 38, 3, 1, 16, 12, 4, 3, 8, 0, 481, None), b"leaves the stack")     # item 480 is slice 5: frames 5..7
    assert err(cut(fake, fake, 7, 45, 38, 3, 1, 16, 12, 4, 3, 8, 480, 1, None), b"leaves the stack")
    assert err(cut(fake, fake, 7, 45, 38, 3, 1, 16, 12, 4, 3, 8, -1, 5, None), b"item0")
    assert err(cut(fake, fake, 7, 45, 38, 3, 1, 16, 12, 4, 3, 8, 0, 0, None), b"item0")
    assert err(cut(fake, fake, 2, 1, 38, 2, 1, 16, 12, 1, 3, 8, 0, 1, None), b"length 1")
    assert err(cut(fake, fake, 2, 45, 1, 2, 1, 16, 12, 4, 1, 8, 0, 1, None), b"length 1")
    assert err(cut(fake, fake, 7, 45, 38, 3, 1, 0, 12, 4, 3, 8, 0, 1, None), b"positive")
    assert err(cut(fake, fake, 7, 45, 38, 3, 1, 16, 12, 1 << 16, 1 << 16, 8, 0, 1, None), b"32-bit")
    assert err(cut(fake, fake, 7, 45, 38, 3, 1, 16, 12, 4, 3, 8, (1 << 31) - 8, 8, None), b"32-bit")

    # in, out, nitem, c, size, ensemble, item0
    assert err(clip(None, fake, 13, 2, 16, 8, 5, None), b"null")
    assert err(clip(fake, None, 13, 2, 16, 8, 5, None), b"null")
    for bad in (0, 3, 6, 16):
        assert err(clip(fake, fake, 13, 2, 16, bad, 5, None), b"ensemble")
    for bad in ((0, 2, 16, 8, 5), (13, 0, 16, 8, 5), (13, 2, 0, 8, 5), (13, 2, 16, 8, -1)):
        assert err(clip(fake, fake, *bad, None), b"positive")

    # tiles, out, n_slices, c, n_rows, n_cols, size, overlap, margin, out_h, out_w, blend, ensemble; the stitched sheet is 80 by 104
    assert err(blend(None, fake, 3, 2, 3, 4, 32, 8, 3, 80, 104, 1, 8, None), b"null")
    assert err(blend(fake, None, 3, 2, 3, 4, 32, 8, 3, 80, 104, 1, 8, None), b"null")
    for bad in (-1, 2):
        assert err(blend(fake, fake, 3, 2, 3, 4, 32, 8, 3, 80, 104, bad, 8, None), b"blend must")
    for bad in (0, 3, 7, 16):
        assert err(blend(fake, fake, 3, 2, 3, 4, 32, 8, 3, 80, 104, 1, bad, None), b"ensemble")
    assert err(blend(fake, fake, 3, 2, 3, 4, 32, 8, 3, 81, 104, 1, 8, None), b"crop")
    assert err(blend(fake, fake, 3, 2, 3, 4, 32, 8, 3, 80, 0, 1, 8, None), b"crop")
    assert err(blend(fake, fake, 3, 2, 3, 4, 32, 8, 9, 80, 104, 1, 8, None), b"margin")
    assert err(blend(fake, fake, 3, 2, 3, 4, 32, 32, 3, 80, 104, 1, 8, None), b"margin")
    assert err(blend(fake, fake, 0, 2, 3, 4, 32, 8, 3, 80, 104, 1, 8, None), b"bad args")


# ------------------------------------------------------------------------------------------------ the oracle against its definitions
def test_members_invert_and_are_distinct():
    a = np.arange(2 * 5 * 5).reshape(2, 5, 5) ** 2 % 37                   # no symmetry under any rotation or flip
    members = [R.T_d(a, d) for d in range(8)]
    for d in range(8):
        np.testing.assert_array_equal(R.U_d(members[d], d), a)
        np.testing.assert_array_equal(R.T_d(R.U_d(a, d), d), a)
        assert members[d].shape == a.shape
    assert len({m.tobytes() for m in members}) == 8
    np.testing.assert_array_equal(members[0], a)
    np.testing.assert_array_equal(members[1][0], np.rot90(a[0]))
    np.testing.assert_array_equal(members[4][1], a[1][:, ::-1])


@pytest.mark.parametrize("S,O,M,n", [(12, 4, 0, 4), (12, 4, 1, 4), (16, 8, 2, 3)])
def test_linear_weights_sum_to_T_with_two_tiles_per_axis(S, O, M, n):
    w = R.axis_weights(S, O, M, n, "linear")
    T = max(O - 2 * M, 0) + 1
    np.testing.assert_array_equal(w.sum(0), np.full(w.shape[1], T))
    assert w.max() == T and ((w > 0).sum(0) <= 2).all()


@pytest.mark.parametrize("S,O,M,n,uncovered,most", [(12, 4, 3, 3, 4, 1), (8, 6, 0, 5, 0, 4)])
def test_linear_support_is_the_averages(S, O, M, n, uncovered, most):
    lin, avg = R.axis_weights(S, O, M, n, "linear"), R.axis_weights(S, O, M, n, "average")
    np.testing.assert_array_equal(lin > 0, avg > 0)
    assert set(np.unique(avg)) <= {0, 1}
    assert (avg.sum(0) == 0).sum() == uncovered and avg.sum(0).max() == most
    if (S, O, M) == (8, 6, 0):
        assert (lin.sum(0).min(), lin.sum(0).max()) == (7, 10)            # uneven sums: the division by the actual sum covers that


@pytest.mark.parametrize("margin", [0, 3])
def test_average_of_one_member_is_patch_images(margin):
    from pssr2_amd.util import _patch_images
    n_slices, c, n_rows, n_cols, S, O = 2, 2, 3, 4, 12, 4
    tiles = np.random.default_rng(11).integers(0, 256, size=(n_slices * n_rows * n_cols, c, S, S), dtype=np.uint8)
    per = n_rows * n_cols
    want = np.stack([np.stack([np.asarray(_patch_images(tiles[k * per:(k + 1) * per, ch], n_cols, n_rows, O, margin), dtype=np.uint8)
                               for ch in range(c)]) for k in range(n_slices)])
    H, W = n_rows * (S - O) + O, n_cols * (S - O) + O
    got = R.blend_ref(tiles, n_slices, n_rows, n_cols, O, margin, H, W, "average", 1)
    assert got.shape == (n_slices, c, H, W) and got.dtype == np.uint8
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(R.blend_ref(tiles, n_slices, n_rows, n_cols, O, margin, H - 5, W - 7, "average", 1), want[..., :H - 5, :W - 7])


def test_dihedral_tiles_ref_of_one_member_is_the_padded_windows():
    stack = np.random.default_rng(12).integers(0, 256, size=(3, 21, 18), dtype=np.uint8)
    ty, tx = R.grid(21, 8, 6), R.grid(18, 8, 6)
    one = R.dihedral_tiles_ref(stack, 2, 1, 8, 6, ty, tx, 2, 1)
    assert one.shape == (2 * ty * tx, 2, 8, 8) and one.dtype == np.float32
    np.testing.assert_array_equal(one[0], stack[0:2, :8, :8])
    np.testing.assert_array_equal(one[ty * tx + 1], stack[1:3, :8, 6:14])
    np.testing.assert_array_equal(one[ty * tx - 1][0, :, -1], np.pad(stack[0], ((0, 5), (0, 2)), mode="reflect")[18:26, 19])
    eight = R.dihedral_tiles_ref(stack, 2, 1, 8, 6, ty, tx, 2, 8)
    np.testing.assert_array_equal(eight[::8], one)
    np.testing.assert_array_equal(eight[8 * 3 + 5], R.T_d(one[3], 5))
