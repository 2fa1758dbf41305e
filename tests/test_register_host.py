"""Registration of real pairs without a GPU: the numpy restatement of tests/_register_ref.py against PIL.Image.resize and against its own
properties, planted shifts, the tie rule, the argument checks of the Python entry points (raised before any device work), and the
argument checks of the three C entry points."""
import ctypes
import inspect
from pathlib import Path

import numpy as np
import pytest
import torch

import _consistency_ref as C
import _register_ref as R

ROOT = Path(__file__).resolve().parent.parent
SCALES = (1, 2, 3, 4, 8, 16)


def _radii(s):
    return sorted({0, 1, 3, s + 1})


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("s", SCALES)
def test_every_reduced_window_is_pillow(s):
    """D_t equals PIL.Image.resize of H[s(m-1)+ty : s(h-m+1)+ty, s(m-1)+tx : s(w-m+1)+tx] to (w'+2, h'+2) with the outer ring dropped, for
    every shift: true by construction of m, and it pins the interior-tap claim."""
    from PIL import Image
    rng = np.random.default_rng(10 + s)
    for radius in _radii(s):
        m = R.margin(s, radius)
        for hc, wc in ((1, 1), (3, 5), (9, 13)):
            h, w = hc + 2 * m, wc + 2 * m
            hr = rng.integers(0, 256, size=(s * h, s * w), dtype=np.uint8)
            windows = R.reduced_windows(hr, h, w, radius)
            assert list(windows) == R.shifts(radius) and len(windows) == (2 * radius + 1) ** 2
            for (ty, tx), d in windows.items():
                cut = hr[s * (m - 1) + ty:s * (h - m + 1) + ty, s * (m - 1) + tx:s * (w - m + 1) + tx]
                want = np.asarray(Image.fromarray(np.ascontiguousarray(cut)).resize((wc + 2, hc + 2), Image.BILINEAR))[1:-1, 1:-1]
                np.testing.assert_array_equal(d, want, err_msg=f"s={s} R={radius} t={(ty, tx)} {hc}x{wc}")


@pytest.mark.parametrize("s", SCALES)
def test_interior_taps_of_any_interior_index(s):
    ks = R.interior_taps(s)
    for n in (3, 4, 7, 40):
        for i, (xmin, k) in enumerate(C.taps(n, n * s)):
            if i * s - s // 2 >= 0 and i * s - s // 2 + 2 * s <= n * s:
                assert xmin == i * s - s // 2 and k == ks
    if s == 1:
        assert ks == [1 << R.PRECISION_BITS, 0]


@pytest.mark.parametrize("s", SCALES)
def test_zero_shift_is_the_plain_reduction(s):
    rng = np.random.default_rng(20 + s)
    for radius in (0, 3):
        m = R.margin(s, radius)
        h, w = 5 + 2 * m, 7 + 2 * m
        hr = rng.integers(0, 256, size=(2, s * h, s * w), dtype=np.uint8)
        np.testing.assert_array_equal(R.reduced_windows(hr, h, w, radius)[(0, 0)], C.reduce_ref(hr, h, w)[:, m:h - m, m:w - m])


def test_scale_one_is_a_plain_crop():
    rng = np.random.default_rng(3)
    radius, m = 3, 4
    hr = rng.integers(0, 256, size=(13, 15), dtype=np.uint8)
    for (ty, tx), d in R.reduced_windows(hr, 13, 15, radius).items():
        np.testing.assert_array_equal(d, hr[m + ty:13 - m + ty, m + tx:15 - m + tx])


def test_sums_layout():
    rng = np.random.default_rng(4)
    hr, lr = rng.integers(0, 256, size=(2, 18, 22), dtype=np.uint8), rng.integers(0, 256, size=(2, 9, 11), dtype=np.uint8)
    rows = R.sums_ref(hr, lr, 1)
    assert len(rows) == 2 and all(len(r) == 3 * 9 + 2 for r in rows)
    lc = lr[1, 2:-2, 2:-2].astype(np.int64)
    d = R.reduced_windows(hr, 9, 11, 1)[(1, -1)][1].astype(np.int64)
    t = (1 + 1) * 3 + (-1 + 1)
    assert rows[1][3 * t:3 * t + 3] == [d.sum(), (d * d).sum(), (d * lc).sum()] and rows[1][-2:] == [lc.sum(), (lc * lc).sum()]


# ------------------------------------------------------------------------------------------------ the choice
def test_every_planted_shift_is_found_with_score_one():
    from pssr2_amd.util import _register_choose
    rng = np.random.default_rng(5)
    s, radius, h, w = 2, 2, 11, 12
    m = R.margin(s, radius)
    n = (h - 2 * m) * (w - 2 * m)
    for t0 in R.shifts(radius):
        hr, lr = R.planted_pair(rng, 1, 1, 1, h, w, s, radius, [t0])
        rows = R.sums_ref(hr[0], lr[0], radius)
        assert R.choose_ref(n, rows, radius) == (t0, 1.0)
        assert _register_choose(n, rows, radius) == (t0, 1.0)
        hr_out, lr_out = R.crop_ref(hr[0], lr[0], t0, radius)
        # the aligned pair shows one field of view: away from the border taps the plain reduction of hr_out is lr_out
        np.testing.assert_array_equal(C.reduce_ref(hr_out, h - 2 * m, w - 2 * m)[:, 1:-1, 1:-1], lr_out[:, 1:-1, 1:-1])


def test_package_choice_is_the_restated_choice():
    """util._register_choose (cross-multiplied Python ints) against the restatement (fractions), on real sums of pooled planes and on
    synthetic rows with exact ties."""
    from pssr2_amd.util import _register_choose
    rng = np.random.default_rng(6)
    for radius in (0, 1, 3):
        for planes in (1, 3):
            hr = rng.integers(0, 256, size=(planes, 3 * 14, 3 * 15), dtype=np.uint8)
            lr = C.reduce_ref(np.roll(hr, (1, -1), axis=(-2, -1)), 14, 15)
            rows = R.sums_ref(hr, lr, radius)
            n = planes * (14 - 2 * R.margin(3, radius)) * (15 - 2 * R.margin(3, radius))
            assert _register_choose(n, rows, radius) == R.choose_ref(n, rows, radius)
    # the same triple at every shift: a nine-way tie, (0, 0) has the smallest ty^2 + tx^2
    row = [10, 60, 70] * 9 + [12, 80]
    assert _register_choose(2, [row], 1) == R.choose_ref(2, [row], 1) and _register_choose(2, [row], 1)[0] == (0, 0)
    # a tie between (-1, 0), (0, -1), (0, 1), (1, 0) only: the smaller ty, then the smaller tx
    row = [10, 50, 60] * 9 + [12, 80]
    for t in (1, 3, 5, 7):
        row[3 * t:3 * t + 3] = [10, 60, 70]
    assert _register_choose(2, [row], 1)[0] == R.choose_ref(2, [row], 1)[0] == (-1, 0)
    row[3:6] = [10, 50, 60]
    assert _register_choose(2, [row], 1)[0] == R.choose_ref(2, [row], 1)[0] == (0, -1)


def test_constant_pairs_choose_the_zero_shift():
    from pssr2_amd.util import _register_choose
    for hr_v, lr_v in ((7, 7), (0, 255), (255, 255)):
        hr, lr = np.full((1, 24, 24), hr_v, dtype=np.uint8), np.full((1, 12, 12), lr_v, dtype=np.uint8)
        rows = R.sums_ref(hr, lr, 2)
        assert _register_choose(64, rows, 2) == R.choose_ref(64, rows, 2) == ((0, 0), 0.0)
    # a constant LR side and a random HR side: denl == 0, every score is 0
    rng = np.random.default_rng(7)
    rows = R.sums_ref(rng.integers(0, 256, size=(1, 24, 24), dtype=np.uint8), np.full((1, 12, 12), 9, dtype=np.uint8), 2)
    assert _register_choose(64, rows, 2) == R.choose_ref(64, rows, 2) == ((0, 0), 0.0)


def test_zero_variance_at_some_shifts_only():
    """An HR plane that is flat where most shifts look and textured at its right edge: den == 0 for those shifts (score 0), > 0 for the
    rest, and a positive correlation must win over the zeros, a negative one must lose to them."""
    from pssr2_amd.util import _register_choose
    rng = np.random.default_rng(8)
    s, radius, h, w = 1, 2, 9, 9
    m = R.margin(s, radius)                                   # 3: windows are 3 x 3, columns 3 + tx .. 5 + tx
    hr = np.full((1, h, w), 100, dtype=np.uint8)
    hr[0, :, 7] = rng.integers(0, 256, size=h, dtype=np.uint8)
    windows = R.reduced_windows(hr, h, w, radius)
    lr = rng.integers(0, 256, size=(1, h, w), dtype=np.uint8)
    lr[0, m:h - m, m:w - m] = windows[(1, 2)][0]
    rows = R.sums_ref(hr, lr, radius)
    dens = {t: 9 * rows[0][3 * i + 1] - rows[0][3 * i] ** 2 for i, t in enumerate(R.shifts(radius))}
    assert all((dens[t] == 0) == (t[1] < 2) for t in dens) and any(v == 0 for v in dens.values())
    assert _register_choose(9, rows, radius) == R.choose_ref(9, rows, radius) == ((1, 2), 1.0)
    lr[0, m:h - m, m:w - m] = 255 - windows[(1, 2)][0]        # anticorrelated with every textured shift it matches: zeros win
    rows = R.sums_ref(hr, lr, radius)
    got = _register_choose(9, rows, radius)
    assert got == R.choose_ref(9, rows, radius) and got[0] != (1, 2)


# ------------------------------------------------------------------------------------------------ argument checks in Python
HR, LR = np.zeros((2, 1, 24, 32), dtype=np.uint8), np.zeros((2, 3, 12, 16), dtype=np.uint8)


@pytest.mark.parametrize("hr,lr,kw,error,word", [
    (HR, LR, dict(radius=33), ValueError, "radius"),
    (HR, LR, dict(radius=-1), ValueError, "radius"),
    (HR, LR, dict(radius=2.0), ValueError, "radius"),
    (HR, LR, dict(radius=True), ValueError, "radius"),
    (HR.astype(np.float32), LR, {}, TypeError, "uint8"),
    (HR, LR.astype(np.int16), {}, TypeError, "uint8"),
    (torch.zeros(2, 1, 24, 32, dtype=torch.uint8), torch.zeros(2, 3, 12, 16, dtype=torch.uint8), {}, RuntimeError, "no CPU fallback"),
    (np.zeros((2, 4, 24, 32), dtype=np.uint8), LR, {}, ValueError, "4 frames"),                     # C > c
    (HR[:1], LR, {}, ValueError, "same number of images"),
    (np.zeros((2, 1, 24, 33), dtype=np.uint8), LR, {}, ValueError, "integer multiple"),             # non-integer ratio
    (np.zeros((2, 1, 24, 48), dtype=np.uint8), LR, {}, ValueError, "integer multiple"),             # anisotropic: 2 and 3
    (np.zeros((2, 1, 6, 8), dtype=np.uint8), LR, {}, ValueError, "integer multiple"),               # smaller than the LR side
    (np.zeros((2, 1, 12 * 17, 16 * 17), dtype=np.uint8), LR, {}, ValueError, "integer multiple"),   # s = 17
    (HR[0], LR, {}, ValueError, "3-D"),
    (HR[0, 0], LR[0, 0], {}, ValueError, "3-D"),
    (HR, LR, dict(radius=10), ValueError, "margin"),                                                # m = 6: h' = 0
    (HR, LR, dict(radius=9), ValueError, "margin"),                                                 # m = 6 still
    (np.zeros((1, 1, 0, 8), dtype=np.uint8), np.zeros((1, 1, 0, 4), dtype=np.uint8), {}, ValueError, "integer multiple"),
])
def test_register_pairs_checks_its_arguments_before_the_device(hr, lr, kw, error, word):
    from pssr2_amd.util import register_pairs
    with pytest.raises(error, match=word):
        register_pairs(hr, lr, **kw)


def test_without_a_device_the_reason_is_given(monkeypatch):
    from pssr2_amd.data import DevicePairedTileDataset, PairedArrayDataset
    from pssr2_amd.util import register_pairs
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="HIP"):
        register_pairs(HR, LR, radius=2)
    for cls in (PairedArrayDataset, DevicePairedTileDataset):
        with pytest.raises(RuntimeError, match="HIP"):
            cls(HR, LR, hr_res=16, lr_scale=2, register=2)


def test_dataset_keyword_is_checked_before_anything_is_read(tmp_path):
    from pssr2_amd.data import DevicePairedTileDataset, PairedArrayDataset, PairedImageDataset

    class Unread:
        def __getattr__(self, name):                           # pragma: no cover
            raise AssertionError(f"the keyword check comes before the stacks are touched ({name})")

    for bad in (-1, 33, 1.5, "3", True):
        for cls in (PairedArrayDataset, DevicePairedTileDataset):
            with pytest.raises(ValueError, match="register"):
                cls(Unread(), Unread(), register=bad)
        with pytest.raises(ValueError, match="register"):
            PairedImageDataset(str(tmp_path / "no_hr"), str(tmp_path / "no_lr"), register=bad)


def test_ops_refuse_host_tensors_and_wrong_arguments():
    from pssr2_amd import ops
    hr, lr = torch.zeros(1, 24, 24, dtype=torch.uint8), torch.zeros(1, 12, 12, dtype=torch.uint8)
    with pytest.raises(ValueError, match="uint8 device tensors"):
        ops.register_shifts_u8(hr, lr, 2)
    with pytest.raises(ValueError, match="uint8 device tensor"):
        ops.crop_shift_u8(hr, [(0, 0)], 4, 4)
    assert ops.register_margin(4, 8) == 3 and ops.register_margin(4, 9) == 4 and ops.register_margin(1, 0) == 1 and ops.register_margin(16, 1) == 2
    assert ops.MAX_REGISTER_RADIUS == 32


def test_new_arguments_are_keyword_only_and_off_by_default():
    from pssr2_amd import data as D
    from pssr2_amd import util as U
    for cls in (D.PairedArrayDataset, D.PairedImageDataset, D.DevicePairedTileDataset):
        p = inspect.signature(cls.__init__).parameters["register"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    params = inspect.signature(U.register_pairs).parameters
    assert [params[k].default for k in ("radius", "to_numpy")] == [8, True]
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("radius", "to_numpy"))
    assert U.Registration._fields == ("hr", "lr", "shift", "score", "margin")
    rng = np.random.default_rng(9)
    hr, lr = rng.integers(0, 256, size=(3, 1, 8, 8), dtype=np.uint8), rng.integers(0, 256, size=(3, 1, 4, 4), dtype=np.uint8)
    ds = D.PairedArrayDataset(hr, lr, hr_res=8, lr_scale=2)
    assert ds.hr_images is hr and ds.lr_images is lr and ds.shifts is None and ds.scores is None


# ------------------------------------------------------------------------------------------------ argument checks of the entry points
def _lib():
    path = ROOT / "pssr2_amd" / "libpssr_mi355.so"
    if not path.exists():
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(str(path))
    lib.pssr_last_error.restype = ctypes.c_char_p
    return lib


def test_register_entry_points_validate_without_gpu():
    """Every check happens before the launch: an error code and a message, no crash, no device needed."""
    lib = _lib()
    assert lib.pssr_abi_version() == 5
    i, i64, p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    shifts, crop, ws = lib.pssr_register_shifts_u8, lib.pssr_crop_shift_u8, lib.pssr_register_shifts_workspace_bytes
    shifts.argtypes = [p] * 3 + [i] * 5 + [p, p]
    crop.argtypes = [p] * 3 + [i] * 5 + [p]
    ws.restype, ws.argtypes = i64, [i] * 5
    fake = 0x1000          # never dereferenced: every call below fails its checks

    def err(status, word):
        return status == -1 and word in lib.pssr_last_error()

    # hr, lr, sums, planes, h, w, s, radius, workspace
    for hole in range(3):
        ptrs = [None if k == hole else fake for k in range(3)]
        assert err(shifts(*ptrs, 2, 16, 16, 4, 2, fake, None), b"null")
    assert err(shifts(fake, fake, fake, 2, 16, 16, 4, 2, None, None), b"null")
    for bad in (0, 17, -1, 32):
        assert err(shifts(fake, fake, fake, 2, 16, 16, bad, 2, fake, None), b"scale")
        assert ws(2, 16, 16, bad, 2) == 0
    for bad in (-1, 33, 100):
        assert err(shifts(fake, fake, fake, 2, 64, 64, 4, bad, fake, None), b"radius")
        assert ws(2, 64, 64, 4, bad) == 0
    for bad in ((0, 16, 16), (2, 0, 16), (2, 16, 0), (-1, 16, 16), (2, -16, 16)):
        assert err(shifts(fake, fake, fake, *bad, 4, 2, fake, None), b"positive")
        assert ws(*bad, 4, 2) == 0
    # h' < 1 or w' < 1: radius 8 at scale 4 has m = 3
    for hw in ((6, 16), (16, 6), (2, 2)):
        assert err(shifts(fake, fake, fake, 1, *hw, 4, 8, fake, None), b"margin")
        assert ws(1, *hw, 4, 8) == 0
    assert ws(1, 7, 7, 4, 8) > 0
    assert err(shifts(fake, fake, fake, 1, 16385, 16384, 1, 0, fake, None), b"2^28")            # one row over 2^28 pixels
    assert err(shifts(fake, fake, fake, 1, 1 << 27, 2, 16, 0, fake, None), b"2^30")             # an axis of hr of 2^31
    assert ws(1, 16385, 16384, 1, 0) == 0
    assert ws(3, 64, 64, 4, 8) >= 3 * (3 * 289 + 2) * 8                                         # a row of sums per plane at least

    # in, out, origins, planes, H, W, ho, wo
    for hole in range(3):
        ptrs = [None if k == hole else fake for k in range(3)]
        assert err(crop(*ptrs, 2, 16, 16, 8, 8, None), b"null")
    for bad in ((0, 16, 16, 8, 8), (2, 0, 16, 8, 8), (2, 16, 16, 0, 8), (2, 16, 16, 8, -1), (-2, 16, 16, 8, 8)):
        assert err(crop(fake, fake, fake, *bad, None), b"positive")
    for bad in ((2, 16, 16, 17, 8), (2, 16, 16, 8, 17)):
        assert err(crop(fake, fake, fake, *bad, None), b"does not fit")
