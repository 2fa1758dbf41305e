"""The noise measurement without a GPU: the restated level table of tests/_levels_ref.py against a plain double loop, util._noise_fit
against the Fraction restatement on planted and hand-built tables, the recovery of planted noise models within measured bounds,
Noise.crappifier, the argument checks of the Python entry points (raised before any device work) and those of the C entry point."""
import ctypes
import inspect
import math
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

import _levels_ref as R

ROOT = Path(__file__).resolve().parent.parent
FITTED = R.FIELDS[:10]

# The worst absolute error of every field against the planted model (poisson = i, gaussian = s, gain = beta = g, saltpepper = 100 amount,
# slope = i^2, intercept = s^2, alpha = 1) over the seeds 0 .. 19 of plant() on scene(8, 64, 64, 1), pool "all", min_count = 32,
# guard = 4.  Obtained by running the Fraction restatement (R.fit_ref of R.table_ref) over those 20 seeds on the CPU and rounding the
# largest error up to four decimals; the product is held to twice each.  The 1/12 of rounding is part of the intercept's error.
# gaussian at (1, 0, 0, 0) is the root of the intercept of a steep line and wanders by 2 grey levels: there the intercept is held against
# its own spread instead (gaussian is not in that row).
WORST = {
    (0, 0, 5, 0): dict(poisson=0.1054, gaussian=0.1657, gain=0.0367, saltpepper=0.0, slope=0.0122, intercept=1.6849, alpha=0.0015, beta=0.1844),
    (1, 0, 0, 0): dict(poisson=0.0197, gain=0.0846, saltpepper=0.0, slope=0.0390, intercept=4.1914, alpha=0.0024, beta=0.2362),
    (0.5, 3, 4, 0): dict(poisson=0.0180, gaussian=0.3276, gain=0.0675, saltpepper=0.0, slope=0.0178, intercept=2.5135, alpha=0.0016, beta=0.1479),
    (1, -2, 6, 0.01): dict(poisson=0.0376, gaussian=0.7036, gain=0.1452, saltpepper=0.1975, slope=0.0739, intercept=8.9387, alpha=0.0029,
                           beta=0.2331),
    (0.7, 0, 2, 0.02): dict(poisson=0.0213, gaussian=0.8224, gain=0.0691, saltpepper=0.3044, slope=0.0302, intercept=2.6132, alpha=0.0016,
                            beta=0.1391),
}
SEEDS = range(20)


def planted_model(i, g, s, amount):
    return dict(poisson=i, gaussian=s, gain=g, saltpepper=100 * amount, slope=i * i, intercept=s * s, alpha=1.0, beta=g)


@pytest.fixture(scope="module")
def scene():
    d = R.scene(8, 64, 64, 1)
    d.setflags(write=False)
    return d


def _same_fit(table, min_count=32, guard=4.0):
    """util._noise_fit of the table against the restatement: the floats to 1e-12, the rest equal.  -> the restatement's dict."""
    from pssr2_amd.util import _noise_fit
    got = _noise_fit(np.asarray(table).tolist(), min_count, guard)
    want = R.fit_ref(table, min_count, guard)
    assert len(got) == len(FITTED)
    for name, value in zip(FITTED, got):
        if name in ("levels", "found"):
            assert value == want[name] and type(value) is type(want[name]), name
        else:
            assert type(value) is float and abs(value - want[name]) <= 1e-12, (name, value, want[name])
    return want


# ------------------------------------------------------------------------------------------------ the table
def test_the_restated_table_is_the_double_loop():
    rng = np.random.default_rng(0)
    d = rng.integers(0, 4, size=(2, 3, 7), dtype=np.uint8) * 85            # the levels 0, 85, 170, 255
    l = rng.choice(np.array([0, 1, 17, 254, 255], dtype=np.uint8), size=(2, 3, 7))
    want = [[[0] * 5 for _ in range(256)] for _ in range(2)]
    for p in range(2):
        for y in range(3):
            for x in range(7):
                row, v = want[p][int(d[p, y, x])], int(l[p, y, x])
                row[0] += 1
                row[1] += v
                row[2] += v * v
                row[3] += v == 0
                row[4] += v == 255
    got = R.table_ref(d, l)
    assert got.dtype == np.int64 and got.shape == (2, 256, 5) and got.tolist() == want
    assert got[..., 0].sum() == 42 and got[:, [0, 85, 170, 255]].sum() == got.sum()
    assert R.table_ref(d.reshape(2, 21), l.reshape(2, 21)).tolist() == want


# ------------------------------------------------------------------------------------------------ the fit
def _two_valued(table, v, k, a, b, zeros=0, full=0):
    """Level v of the table: k pixels, half at a and half at b, then ``zeros`` pixels at 0 and ``full`` at 255."""
    table[v] = [k + zeros + full, k // 2 * (a + b) + 255 * full, k // 2 * (a * a + b * b) + 255 * 255 * full, zeros, full]


def test_fit_on_planted_tables(scene):
    for planting in R.PLANTINGS:
        for seed in (0, 7):
            table = R.table_ref(scene, R.plant(scene, *planting, seed)).sum(axis=0)
            assert _same_fit(table)["found"]
            _same_fit(table, min_count=2, guard=1.5)
            _same_fit(table, min_count=500, guard=8.0)


def test_fit_with_one_used_level():
    table = np.zeros((256, 5), dtype=np.int64)
    _two_valued(table, 100, 40, 99, 103)
    fit = _same_fit(table)
    var = 4 * 40 / 39
    assert (fit["levels"], fit["found"], fit["slope"], fit["alpha"]) == (1, True, 0.0, 1.0)
    assert fit["gain"] == fit["beta"] == 1.0 and math.isclose(fit["intercept"], var) and math.isclose(fit["gaussian"], math.sqrt(var))
    assert fit["poisson"] == 0.0 and fit["saltpepper"] == 0.0


def test_fit_with_no_used_level():
    from pssr2_amd.util import _noise_fit
    table = np.zeros((256, 5), dtype=np.int64)
    assert _same_fit(table) == dict(poisson=0.0, gaussian=0.0, gain=0.0, saltpepper=0.0, slope=0.0, intercept=0.0, alpha=0.0, beta=0.0, levels=0,
                                    found=False)
    _two_valued(table, 100, 30, 99, 103)                       # below min_count = 32
    _two_valued(table, 200, 30, 199, 201, zeros=10)            # ... and 10 of the 40 bright pixels are pepper
    _two_valued(table, 50, 20, 50, 50, full=20)                # ... and 20 of the 70 dark ones salt
    fit = _same_fit(table)
    assert not fit["found"] and fit["levels"] == 0 and math.isclose(fit["saltpepper"], 100 * (10 / 40 + 20 / 70))
    assert _noise_fit(table.tolist(), 32, 4.0)[:3] == (0.0, 0.0, 0.0)
    assert _same_fit(table, min_count=30)["levels"] == 2       # level 50 keeps 20 unsaturated pixels only


def test_fit_min_count_counts_unsaturated_pixels():
    table = np.zeros((256, 5), dtype=np.int64)
    _two_valued(table, 60, 32, 59, 61)
    _two_valued(table, 90, 32, 89, 91, zeros=1)                # 33 pixels, 32 of them unsaturated
    _two_valued(table, 120, 30, 119, 121, zeros=1, full=1)     # 32 pixels, 30 of them unsaturated
    assert _same_fit(table)["levels"] == 2
    assert _same_fit(table, min_count=33)["levels"] == 0 and _same_fit(table, min_count=30)["levels"] == 3
    one = np.zeros((256, 5), dtype=np.int64)
    one[77] = [1, 77, 77 * 77, 0, 0]                           # n' = 1 has no variance, whatever min_count
    assert not _same_fit(one, min_count=2)["found"]


def test_fit_guard_just_inside_and_just_outside():
    table = np.zeros((256, 5), dtype=np.int64)
    _two_valued(table, 10, 40, 8, 12)                          # mean 10, sd = 2 sqrt(40 / 39) = 2.0255: 10 / sd = 4.9371
    _two_valued(table, 245, 40, 243, 247)                      # the same 10 grey levels below 255
    _two_valued(table, 128, 40, 126, 130)
    assert 4.93 < 10 / (2 * math.sqrt(40 / 39)) < 4.94
    assert _same_fit(table, guard=4.93)["levels"] == 3
    assert _same_fit(table, guard=4.94)["levels"] == 1
    table[245] = 0
    assert _same_fit(table, guard=4.93)["levels"] == 2 and _same_fit(table, guard=4.94)["levels"] == 1


def test_fit_with_only_bright_or_only_dark_levels():
    bright = np.zeros((256, 5), dtype=np.int64)
    _two_valued(bright, 150, 96, 149, 151, zeros=4)
    _two_valued(bright, 200, 100, 198, 202, full=7)            # 255 on a bright level is not salt
    fit = _same_fit(bright)
    assert fit["found"] and math.isclose(fit["saltpepper"], 100 * 2 * (4 / 207))
    dark = np.zeros((256, 5), dtype=np.int64)
    _two_valued(dark, 30, 96, 29, 31, zeros=4)                 # 0 on a dark level is not pepper
    _two_valued(dark, 100, 100, 98, 102, full=7)
    fit = _same_fit(dark)
    assert fit["found"] and math.isclose(fit["saltpepper"], 100 * 2 * (7 / 207))
    both = bright + dark
    assert math.isclose(_same_fit(both)["saltpepper"], 100 * (4 / 207 + 7 / 207))


@pytest.mark.parametrize("planting", R.PLANTINGS, ids=str)
def test_planted_noise_is_recovered(scene, planting):
    from pssr2_amd.util import _noise_fit
    want = planted_model(*planting)
    for seed in SEEDS:
        table = R.table_ref(scene, R.plant(scene, *planting, seed)).sum(axis=0)
        got = dict(zip(FITTED, _noise_fit(table.tolist(), 32, 4.0)))
        assert got["found"] and got["levels"] >= 150
        if planting == (0, 0, 0, 0):                           # the noiseless pair: exactly nothing
            assert got == dict(want, alpha=1.0, levels=got["levels"], found=True)
            assert all(type(got[k]) is float and got[k] == 0.0 for k in ("poisson", "gaussian", "gain", "saltpepper", "slope", "intercept", "beta"))
            continue
        for name, bound in WORST[planting].items():
            print(planting, seed, name, got[name], want[name])
            assert abs(got[name] - want[name]) <= 2 * bound, (seed, name, got[name], want[name])


# ------------------------------------------------------------------------------------------------ Noise.crappifier
def _stages(c):
    return [(type(s).__name__, s.intensity, s.gain, s.spread) for s in c.crappifiers]


def _noise(**kw):
    from pssr2_amd.util import Noise
    base = dict(poisson=0.0, gaussian=0.0, gain=0.0, saltpepper=0.0, slope=0.0, intercept=0.0, alpha=1.0, beta=0.0, levels=9, found=True, table=None,
                sigma=0.0, margin=0)
    return Noise(**dict(base, **kw))


def test_crappifier_stages_and_their_order(scene):
    from pssr2_amd import MultiCrappifier
    from pssr2_amd.util import Noise, _noise_fit
    assert Noise._fields == R.FIELDS
    full = _noise(poisson=0.5, gaussian=4.0, gain=3.0, saltpepper=1.5, sigma=2.0).crappifier(scale=4)
    assert type(full) is MultiCrappifier and full.clip is True
    assert _stages(full) == [("Blur", 0.5, 0, 0), ("Poisson", 0.5, 3.0, 0), ("AdditiveGaussian", 4.0, 0, 0), ("SaltPepper", 0.015, 0, 0)]
    assert _stages(_noise(sigma=3.0).crappifier(scale=2)) == [("Blur", 1.5, 0, 0)] and _stages(_noise(sigma=3.0).crappifier(1)) == [("Blur", 3.0, 0, 0)]
    assert _stages(_noise(gain=-2.0).crappifier()) == [("Poisson", 0.0, -2.0, 0)]                # the gain travels with the Poisson stage
    assert _stages(_noise(gaussian=2.0, saltpepper=0.5).crappifier(scale=4)) == [("AdditiveGaussian", 2.0, 0, 0), ("SaltPepper", 0.005, 0, 0)]
    empty = _noise(alpha=0.0, levels=0, found=False).crappifier()
    assert type(empty) is MultiCrappifier and empty.crappifiers == () and empty.clip is True
    np.testing.assert_array_equal(empty.crappify(scene[:1]), scene[:1])
    for bad in (None, 0, 17, 2.0, True):
        with pytest.raises(ValueError, match="scale"):
            _noise(sigma=1.0).crappifier(scale=bad)
    # the plantings: whatever was measured as non-zero, in the order Poisson, AdditiveGaussian, SaltPepper
    for planting in R.PLANTINGS:
        fit = _noise_fit(R.table_ref(scene, R.plant(scene, *planting, 3)).sum(axis=0).tolist(), 32, 4.0)
        noise = Noise(*fit, None, 0.0, 0)
        want = [("Poisson", noise.poisson, noise.gain, 0)] if noise.poisson > 0 or noise.gain != 0 else []
        want += [("AdditiveGaussian", noise.gaussian, 0, 0)] if noise.gaussian > 0 else []
        want += [("SaltPepper", noise.saltpepper / 100, 0, 0)] if noise.saltpepper > 0 else []
        assert _stages(noise.crappifier()) == want
        assert len(want) == {(0, 0, 0, 0): 0, (1, -2, 6, 0.01): 3, (0.7, 0, 2, 0.02): 3}.get(planting, len(want))
        assert planting[3] == 0 or want[-1][0] == "SaltPepper"
    # a pool="item" result: one item at a time
    items = _noise(poisson=np.array([0.0, 1.0]), gaussian=np.array([2.0, 0.0]), gain=np.array([0.0, 0.5]), saltpepper=np.zeros(2),
                   sigma=np.array([0.0, 4.0]))
    assert _stages(items.crappifier(item=0)) == [("AdditiveGaussian", 2.0, 0, 0)]
    assert _stages(items.crappifier(scale=4, item=1)) == [("Blur", 1.0, 0, 0), ("Poisson", 1.0, 0.5, 0)]
    for bad in (None, 2, -1, 0.0):
        with pytest.raises(ValueError, match="item"):
            items.crappifier(scale=4, item=bad)
    with pytest.raises(ValueError, match="item"):
        _noise().crappifier(item=0)


# ------------------------------------------------------------------------------------------------ argument checks in Python
HR, LR = np.zeros((2, 1, 64, 80), dtype=np.uint8), np.zeros((2, 3, 16, 20), dtype=np.uint8)


@pytest.mark.parametrize("lr,hr,kw,error,word", [
    (LR, HR, dict(pool="image"), ValueError, "pool"),
    (LR, HR, dict(pool=None), ValueError, "pool"),
    (LR, HR, dict(min_count=1), ValueError, "min_count"),
    (LR, HR, dict(min_count=32.0), ValueError, "min_count"),
    (LR, HR, dict(min_count=True), ValueError, "min_count"),
    (LR, HR, dict(guard=0), ValueError, "guard"),
    (LR, HR, dict(guard=-4.0), ValueError, "guard"),
    (LR, HR, dict(guard=float("inf")), ValueError, "guard"),
    (LR, HR, dict(guard=float("nan")), ValueError, "guard"),
    (LR, HR, dict(guard="4"), ValueError, "guard"),
    (LR, HR, dict(rsf="search"), ValueError, "rsf"),
    (LR, HR, dict(rsf=-1.0), ValueError, "finite"),
    (LR, HR, dict(rsf=11.0), ValueError, "ceil"),
    (LR, HR, dict(rsf=[1.0]), ValueError, "one sigma per item"),
    (LR, HR, dict(rsf=True), ValueError, "numbers"),
    (LR[..., :14, :], HR[..., :56, :], dict(rsf="fit"), ValueError, "margin"),                      # R = 24 at s = 4: m = 7, h' = 0
    (LR[..., :14], HR[..., :56], dict(rsf=8.0), ValueError, "margin"),                               # w' = 0
    (LR, HR.astype(np.float32), {}, TypeError, "uint8"),
    (LR.astype(np.int16), HR, {}, TypeError, "uint8"),
    (LR, HR.astype(np.float32), dict(rsf=1.0), TypeError, "uint8"),
    (torch.zeros(2, 3, 16, 20, dtype=torch.uint8), torch.zeros(2, 1, 64, 80, dtype=torch.uint8), {}, RuntimeError, "no CPU fallback"),
    (torch.zeros(2, 3, 16, 20, dtype=torch.uint8), torch.zeros(2, 1, 64, 80, dtype=torch.uint8), dict(rsf=1.0), RuntimeError, "no CPU fallback"),
    (LR, np.zeros((2, 4, 64, 80), dtype=np.uint8), {}, ValueError, "4 planes"),
    (LR, HR[:1], {}, ValueError, "same number of images"),
    (LR, np.zeros((2, 1, 64, 81), dtype=np.uint8), {}, ValueError, "integer multiple"),
    (LR, np.zeros((2, 1, 16 * 17, 20 * 17), dtype=np.uint8), {}, ValueError, "integer multiple"),
    (LR, HR[0], {}, ValueError, "3-D"),
])
def test_estimate_noise_checks_its_arguments_before_the_device(lr, hr, kw, error, word):
    from pssr2_amd.util import estimate_noise
    with pytest.raises(error, match=word):
        estimate_noise(lr, hr, **kw)


def test_without_a_device_the_reason_is_given(monkeypatch):
    from pssr2_amd.util import estimate_noise
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for kw in ({}, dict(rsf=1.0), dict(rsf="fit", pool="item")):
        with pytest.raises(RuntimeError, match="HIP"):
            estimate_noise(LR, HR, **kw)


def test_level_moments_refuses_what_is_no_pair_of_device_planes():
    from pssr2_amd import ops
    a = torch.zeros(2, 8, 8, dtype=torch.uint8)
    for d, l in ((a, a), (a.float(), a), (a, a[:1]), (a.numpy(), a.numpy()), (a[0, 0], a[0, 0]), (a[None], a[None])):
        with pytest.raises(ValueError, match="uint8 device tensors"):
            ops.level_moments_u8(d, l)
    assert ops.LEVEL_MOMENTS == 5


def test_the_interface():
    import pssr2_amd
    from pssr2_amd import util as U
    params = inspect.signature(U.estimate_noise).parameters
    assert list(params) == ["lr", "hr", "rsf", "pool", "min_count", "guard", "to_numpy"]
    assert [params[k].default for k in ("rsf", "pool", "min_count", "guard", "to_numpy")] == [None, "all", 32, 4.0, True]
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("rsf", "pool", "min_count", "guard", "to_numpy"))
    assert pssr2_amd.estimate_noise is U.estimate_noise and U.NOISE_POOLS == ("all", "item")
    assert "1/12" in U.estimate_noise.__doc__ and "commute" in U.Noise.crappifier.__doc__ and "x0" in U.Noise.crappifier.__doc__
    # consistency_map(rsf=...) still has its own name in its messages
    with pytest.raises(ValueError, match="rsf"):
        U.consistency_map(LR, HR, rsf="search")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(RuntimeError, match=r"util\.consistency_map"):
            U.consistency_map(torch.zeros(2, 3, 16, 20, dtype=torch.uint8), torch.zeros(2, 1, 64, 80, dtype=torch.uint8), rsf=1.0)


# ------------------------------------------------------------------------------------------------ argument checks of the entry point
def _lib():
    path = ROOT / "pssr2_amd" / "libpssr_mi355.so"
    if not path.exists():
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(str(path))
    lib.pssr_last_error.restype = ctypes.c_char_p
    return lib


def test_level_moments_entry_point_validates_without_gpu():
    """Every check happens before the launch: an error code and a message, no crash, no device needed."""
    lib = _lib()
    assert lib.pssr_abi_version() == 5
    i, i64, p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    moments, ws = lib.pssr_level_moments_u8, lib.pssr_level_moments_workspace_bytes
    moments.argtypes = [p, p, p, i, i64, p, i64, p]
    ws.restype, ws.argtypes = i64, [i, i64]
    fake = 0x1000          # never dereferenced: every call below fails its checks

    def err(status, word):
        return status == -1 and word in lib.pssr_last_error()

    need = ws(2, 4096)
    assert need >= 2 * 256 * 5 * 8                                                               # a row of sums per plane at least
    for hole in range(3):
        ptrs = [None if k == hole else fake for k in range(3)]
        assert err(moments(*ptrs, 2, 4096, fake, need, None), b"null")
    assert err(moments(fake, fake, fake, 2, 4096, None, need, None), b"null")
    for bad in (0, -1):
        assert err(moments(fake, fake, fake, bad, 4096, fake, need, None), b"planes")
        assert ws(bad, 4096) == 0
    for bad in (0, -5, (1 << 28) + 1, 1 << 40):
        assert err(moments(fake, fake, fake, 2, bad, fake, 1 << 40, None), b"2^28")
        assert ws(2, bad) == 0
    for short in (need - 1, 0, -1):
        assert err(moments(fake, fake, fake, 2, 4096, fake, short, None), b"workspace")
    # the workspace grows with the planes, and a large plane is shared by several workgroups
    assert ws(4, 4096) == 2 * need and ws(1, 1 << 28) > ws(1, 1 << 14) >= 256 * 5 * 8 and ws(1, 1) == 256 * 5 * 8
