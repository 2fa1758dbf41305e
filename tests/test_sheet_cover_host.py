"""Host side of predict_sheet's ``cover`` / ``n_frames`` / ``slide`` (no GPU): the tile grid, the frame-slice plan, the reflection's
source index against ``np.pad(mode="reflect")``, and the argument checks of pssr_stack_tiles_u8 / pssr_patch_stack_u8."""
import ctypes
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("tile,stride,h,rows", [(32, 24, 100, 4), (32, 24, 90, 4), (32, 24, 104, 4), (32, 24, 5, 1),
                                                (16, 12, 45, 4), (16, 12, 38, 3), (16, 12, 32, 3)])
def test_sheet_grid_cover(tile, stride, h, rows):
    """The smallest grid with (H_p - tile) % stride == 0 and H_p >= max(h, tile), on either axis."""
    from pssr2_amd.predict import _sheet_grid
    assert _sheet_grid(h, 64, tile, stride, True) == (rows, _sheet_grid(64, 64, tile, stride, True)[0])
    assert _sheet_grid(64, h, tile, stride, True)[1] == rows
    h_p = (rows - 1) * stride + tile
    assert h_p >= max(h, tile) and h_p - stride < max(h, tile)


def test_sheet_grid_whole_windows_and_errors():
    from pssr2_amd.predict import _sheet_grid
    assert _sheet_grid(100, 90, 32, 24, False) == (3, 3)
    assert _sheet_grid(104, 80, 32, 24, False) == _sheet_grid(104, 80, 32, 24, True) == (4, 3)
    for h, w in ((31, 90), (90, 31)):
        with pytest.raises(ValueError, match="smaller than one tile"):
            _sheet_grid(h, w, 32, 24, False)
    for h, w in ((1, 90), (90, 1)):
        with pytest.raises(ValueError, match="length 1"):
            _sheet_grid(h, w, 32, 24, True)


def test_slice_plan():
    from pssr2_amd.predict import _slice_plan
    assert _slice_plan(7, 3, True) == (3, 1, 5)
    assert _slice_plan(7, 3, False) == (3, 3, 2)
    assert _slice_plan(7, [3, 1], True) == (3, 1, 5)
    assert _slice_plan(7, [1, 3], False) == (3, 3, 2)
    assert _slice_plan(3, 3, True) == (3, 1, 1) and _slice_plan(3, 3, False) == (3, 3, 1)
    for slide in (True, False):
        with pytest.raises(ValueError, match="2 frames.*3 frames"):
            _slice_plan(2, 3, slide)
        assert _slice_plan(7, -1, slide) == (7, 7, 1)
        assert _slice_plan(1, None, slide) == (1, 1, 1)


def _fold(i, n):
    p = 2 * (n - 1)
    j = i % p
    return j if j < n else p - j


@pytest.mark.parametrize("n", [2, 3, 5, 9])
def test_fold_formula_is_numpys_reflect(n):
    """The source index csrc/tiles.hip uses (include/pssr_mi355.h) picks the pixels np.pad(mode="reflect") appends, folds repeated."""
    ramp = np.arange(n)
    for pad in range(0, 34):
        np.testing.assert_array_equal([_fold(i, n) for i in range(n + pad)], np.pad(ramp, (0, pad), mode="reflect"))


def _lib():
    import torch  # noqa: F401  (one HIP runtime per process: torch's)
    path = ROOT / "pssr2_amd" / "libpssr_mi355.so"
    if not path.exists():
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(str(path))
    lib.pssr_last_error.restype = ctypes.c_char_p
    return lib


def test_stack_entry_points_validate_without_gpu():
    """Every check happens before the launch: an error code and a message, no crash, no device needed."""
    lib = _lib()
    assert lib.pssr_abi_version() == 5
    i, p = ctypes.c_int, ctypes.c_void_p
    cut, patch = lib.pssr_stack_tiles_u8, lib.pssr_patch_stack_u8
    cut.argtypes = [p, p] + [i] * 11 + [p]
    patch.argtypes = [p, p] + [i] * 9 + [p]
    fake = 0x1000          # never dereferenced: every call below fails its checks

    def err(status, word):
        return status == -1 and word in lib.pssr_last_error()

    # stack, tiles, frames, h, w, m, frame_step, size, stride, tiles_y, tiles_x, tile0, ntile
    assert err(cut(None, fake, 7, 45, 38, 3, 1, 16, 12, 4, 3, 0, 60, None), b"null")
    assert err(cut(fake, None, 7, 45, 38, 3, 1, 16, 12, 4, 3, 0, 60, None), b"null")
    assert err(cut(fake, fake, 7, 45, 38, 3, 1, 16, 12, 4, 3, 0, 61, None), b"leaves the stack")       # tile 60 is slice 5: frames 5..7
    assert err(cut(fake, fake, 7, 45, 38, 3, 3, 16, 12, 4, 3, 24, 1, None), b"leaves the stack")       # slice 2 of step 3: frames 6..8
    assert err(cut(fake, fake, 7, 45, 38, 8, 1, 16, 12, 4, 3, 0, 1, None), b"leaves the stack")
    assert err(cut(fake, fake, 2, 1, 38, 2, 1, 16, 12, 1, 3, 0, 1, None), b"length 1")
    assert err(cut(fake, fake, 2, 45, 1, 2, 1, 16, 12, 4, 1, 0, 1, None), b"length 1")
    assert err(cut(fake, fake, 7, 45, 38, 3, 1, 16, 12, 4, 3, -1, 5, None), b"tile0")
    for bad in ((0, 45, 38, 3, 1, 16, 12, 4, 3, 0, 1), (7, 0, 38, 3, 1, 16, 12, 4, 3, 0, 1), (7, 45, 38, 0, 1, 16, 12, 4, 3, 0, 1),
                (7, 45, 38, 3, 0, 16, 12, 4, 3, 0, 1), (7, 45, 38, 3, 1, 0, 12, 4, 3, 0, 1), (7, 45, 38, 3, 1, 16, 0, 4, 3, 0, 1),
                (7, 45, 38, 3, 1, 16, 12, 0, 3, 0, 1), (7, 45, 38, 3, 1, 16, 12, 4, 3, 0, 0)):
        assert err(cut(fake, fake, *bad, None), b"positive")
    assert err(cut(fake, fake, 7, 45, 38, 3, 1, 16, 12, 1 << 16, 1 << 16, 0, 1, None), b"32-bit")
    assert err(cut(fake, fake, 7, 45, 38, 3, 1, 16, 1 << 20, 1 << 12, 3, 0, 1, None), b"32-bit")

    # tiles, out, n_slices, c, n_rows, n_cols, size, overlap, margin, out_h, out_w; the stitched sheet is 3*24+8 = 80 by 4*24+8 = 104
    assert err(patch(None, fake, 3, 2, 3, 4, 32, 8, 3, 80, 104, None), b"null")
    assert err(patch(fake, None, 3, 2, 3, 4, 32, 8, 3, 80, 104, None), b"null")
    assert err(patch(fake, fake, 3, 2, 3, 4, 32, 8, 3, 81, 104, None), b"crop")
    assert err(patch(fake, fake, 3, 2, 3, 4, 32, 8, 3, 80, 105, None), b"crop")
    assert err(patch(fake, fake, 3, 2, 3, 4, 32, 8, 3, 0, 104, None), b"crop")
    assert err(patch(fake, fake, 3, 2, 3, 4, 32, 8, 9, 80, 104, None), b"margin")
    assert err(patch(fake, fake, 3, 2, 3, 4, 32, 32, 3, 80, 104, None), b"margin")
    assert err(patch(fake, fake, 0, 2, 3, 4, 32, 8, 3, 80, 104, None), b"bad args")
