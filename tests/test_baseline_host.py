"""The classical baselines without a GPU: the restatement of B1 against real Pillow, the restatement of B2 against scalar loops, the
table, the parameters, the uint32 bounds, every Python check and the entry points' argument checks (include/pssr_mi355.h, B1 and B2)."""
import ctypes
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import _baseline_ref as R

ROOT = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------------------------------------ B1 against Pillow
def _fixture_cases(golden):
    g = golden("baseline_pil.npz")
    return g, sorted(k[:-3] for k in g.files if k.endswith("_in"))


def test_fixture_holds_the_cases_it_should(golden):
    g, names = _fixture_cases(golden)
    want = {f"{kind}_{h}x{w}" for h, w, _ in R.PIL_CASES for kind in ("rnd", "bin")} | {"checker", "one"}
    assert set(names) == want
    for h, w, r in R.PIL_CASES:
        assert g[f"rnd_{h}x{w}_in"].shape == (h, w) and int(g[f"rnd_{h}x{w}_r"]) == r
    assert g["checker_in"].tolist() == R.checkerboard(4, 4).tolist() and int(g["checker_r"]) == 8
    assert g["one_in"].shape == (1, 1) and int(g["one_r"]) == 8


@pytest.mark.parametrize("filter", R.FILTERS)
def test_upsample_restatement_equals_the_pillow_fixture(golden, filter):
    g, names = _fixture_cases(golden)
    for name in names:
        x, r = g[f"{name}_in"], int(g[f"{name}_r"])
        assert np.array_equal(R.upsample(x, r, filter), g[f"{name}_{filter}"]), (name, filter)


@pytest.mark.parametrize("filter", R.FILTERS)
def test_upsample_restatement_equals_live_pillow(filter):
    Image = pytest.importorskip("PIL.Image")
    resample = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}[filter]
    rng = np.random.default_rng(11)
    for h, w, r in R.PIL_CASES + ((4, 4, 8), (1, 1, 8), (7, 3, 1), (2, 70, 2)):
        for x in (rng.integers(0, 256, (h, w)).astype(np.uint8), (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8), R.checkerboard(h, w)):
            want = np.asarray(Image.fromarray(x, mode="L").resize((w * r, h * r), resample))
            assert np.array_equal(R.upsample(x, r, filter), want), (h, w, r, filter)


def test_bicubic_overshoot_is_clipped_and_scale_one_is_the_identity():
    x = R.checkerboard(4, 4)
    up = R.upsample(x, 8, "bicubic")
    assert up.min() == 0 and up.max() == 255
    for filter in R.FILTERS:
        assert np.array_equal(R.upsample(x, 1, filter), x)
        assert np.array_equal(R.upsample(np.full((3, 5), 200, np.uint8), 3, filter), np.full((9, 15), 200, np.uint8))
    assert max(len(k) for _, k in R.taps(16, 64, "bicubic")) <= 5 and max(len(k) for _, k in R.taps(16, 16, "bicubic")) <= 5


# ------------------------------------------------------------------------------------------------ B2: the table and the parameters
def test_nlm_lut_is_the_formula():
    from pssr2_amd import ops
    want = [int(np.rint(16383.0 * math.exp(-(q + 0.5) / 32.0))) for q in range(255)] + [0]
    assert list(ops.NLM_LUT) == want == R.nlm_lut().tolist()
    assert ops.NLM_LUT[0] == 16129 and min(ops.NLM_LUT[:255]) > 0
    # no entry sits close enough to a half for another libm to round it the other way
    assert min(abs((16383.0 * math.exp(-(q + 0.5) / 32.0)) % 1 - 0.5) for q in range(255)) > 1e-4
    assert ops.MAX_NLM_SEARCH == 10 and ops.UPSAMPLE_FILTERS == ("bilinear", "bicubic")


def test_nlm_params_hand_worked_values():
    from pssr2_amd import util
    # P = 3, h = 0.5: 32 * 2^q / 2.25; q = 6 gives 910.2 -> 910, q = 7 gives 1820 > 1023
    assert util._nlm_params(0.5, 0.0, 3) == (910, 6, 0) == R.nlm_params(0.5, 0.0, 3)
    # P = 5, h = 10: 32 * 2^q / 2500; q = 16 gives 838.9 -> 839, q = 17 gives 1678 > 1023
    assert util._nlm_params(10, 0, 5) == (839, 16, 0) == R.nlm_params(10, 0, 5)
    # bias = rint(2 * 9 * 400) = 7200; the largest h still has a shift to spare
    assert util._nlm_params(16, 20, 3) == R.nlm_params(16, 20, 3) and util._nlm_params(16, 20, 3)[2] == 7200
    for P in (3, 5, 7):
        for h in (0.5, 0.7, 8, 100, 255):
            qmul, qshift, bias = util._nlm_params(h, 12.0, P)
            assert (qmul, qshift, bias) == R.nlm_params(h, 12.0, P)
            assert 512 <= qmul <= 1023 and 0 <= qshift <= 31 and bias == int(np.rint(2 * P * P * 144.0))


# ------------------------------------------------------------------------------------------------ B2: the restatement
@pytest.mark.parametrize("shape", [(5, 6), (1, 4)])
@pytest.mark.parametrize("p, s", [(1, 1), (2, 3), (3, 2)])
def test_nlm_restatement_against_scalar_loops(shape, p, s):
    x = np.random.default_rng(shape[0] * 10 + p).integers(0, 256, shape).astype(np.uint8)
    for h, sigma in ((0.5, 0.0), (40.0, 0.0), (30.0, 12.0)):
        params = R.nlm_params(h, sigma, 2 * p + 1)
        assert np.array_equal(R.nlm(x, p, s, *params)[0], R.nlm_scalar(x, p, s, *params))


def test_nlm_of_a_constant_plane_is_the_plane():
    for v in (0, 77, 255):
        x = np.full((2, 9, 11), v, dtype=np.uint8)
        assert np.array_equal(R.nlm_denoise(x, h=8, patch_radius=2, search_radius=4), x)


def test_nlm_search_window_larger_than_the_plane_counts_in_plane_centres_only():
    x = np.random.default_rng(2).integers(0, 256, (3, 3)).astype(np.uint8)
    params = R.nlm_params(255, 0, 3)
    big, small = R.nlm(x, 1, 10, *params)[0], R.nlm(x, 1, 2, *params)[0]
    assert np.array_equal(big, small) and np.array_equal(big, R.nlm_scalar(x, 1, 10, *params))


def test_nlm_uint32_bounds_at_the_extremes():
    lim = 1 << 32
    # the largest ssd: a checkerboard against itself moved by one pixel, 49 * 255^2, times the largest qmul
    _, peak = R.nlm(R.checkerboard(16, 16), 3, 2, 1023, 0, 0)
    assert peak["ssd"] == 49 * 255 * 255 < 1 << 22 and peak["ssd_qmul"] == 49 * 255 * 255 * 1023 < lim
    # the largest numerator: all 255, every one of the 441 candidates at weight LUT[0]
    out, peak = R.nlm(np.full((24, 24), 255, np.uint8), 1, 10, 1023, 0, 0)
    lut0 = int(R.nlm_lut()[0])
    assert peak["num"] == 441 * lut0 * 255 + (441 * lut0 >> 1) < 441 * 16383 * 255 + 441 * 16383 // 2 < lim
    assert np.all(out == 255)


def test_nlm_of_a_checkerboard_keeps_only_the_self_weight():
    x = R.checkerboard(12, 13)
    # a candidate of the other colour differs in (nearly) every pixel of the patch: q clamps to 255 and its weight is 0; the candidates
    # that survive have the pixel's own value
    out = R.nlm_denoise(x, h=0.5, patch_radius=1, search_radius=3)
    assert np.array_equal(out, x)


def test_nlm_denoises_the_block_image():
    """The sanity floor of the definition: p = 1, s = 5, h = 16, sigma = 20 on 8 x 8 constant blocks with sigma = 20 noise gains at least
    4 dB against the clean image (half of what the prototype measured).  Measured with this restatement: 22.20 dB -> 30.52 dB, a gain
    of 8.32 dB."""
    clean, noisy = R.block_image()
    before, after = R.psnr(clean, noisy), R.psnr(clean, R.nlm_denoise(noisy, h=16, sigma=20, patch_radius=1, search_radius=5))
    print(f"block image: {before:.2f} dB -> {after:.2f} dB")
    assert after - before >= 4.0


# ------------------------------------------------------------------------------------------------ the Python checks
def test_python_checks_come_before_any_device_work():
    from pssr2_amd import util
    img = np.zeros((2, 1, 16, 32), dtype=np.uint8)
    for bad in (0, 9, 2.0, True, None):
        with pytest.raises(ValueError, match="scale"):
            util.upsample(img, bad)
    with pytest.raises(ValueError, match="filter"):
        util.upsample(img, 4, filter="lanczos")
    with pytest.raises(TypeError):
        util.upsample(img, 4, "bicubic")                 # filter is keyword-only
    with pytest.raises(TypeError):
        util.nlm_denoise(img)                            # h is required
    with pytest.raises(TypeError):
        util.nlm_denoise(img, 8)                         # and keyword-only
    for bad in (0.4, 256, -1, None, True, float("nan")):
        with pytest.raises(ValueError, match="h must"):
            util.nlm_denoise(img, h=bad)
    for bad in (-0.1, 300, None, float("nan")):
        with pytest.raises(ValueError, match="sigma"):
            util.nlm_denoise(img, h=8, sigma=bad)
    for bad in (0, 4, 1.0, True):
        with pytest.raises(ValueError, match="patch_radius"):
            util.nlm_denoise(img, h=8, patch_radius=bad)
    for bad in (0, 11, 7.0, None):
        with pytest.raises(ValueError, match="search_radius"):
            util.nlm_denoise(img, h=8, search_radius=bad)
    for fn in (lambda a: util.upsample(a, 4), lambda a: util.nlm_denoise(a, h=8)):
        with pytest.raises(RuntimeError, match="MI355X"):
            fn(torch.zeros(2, 1, 16, 32, dtype=torch.uint8))
        with pytest.raises(TypeError, match="uint8"):
            fn(img.astype(np.float32))
        for shape in ((16, 32), (1, 2, 1, 16, 32), (0, 1, 16, 32), (2, 1, 0, 32)):
            with pytest.raises(ValueError, match="lr"):
                fn(np.zeros(shape, dtype=np.uint8))


def test_ops_checks():
    from pssr2_amd import ops
    host = torch.zeros(1, 8, 8, dtype=torch.uint8)
    with pytest.raises(ValueError, match="uint8 device tensor"):
        ops.nlm_u8(host, 1, 1, 512, 4, 0)
    with pytest.raises(ValueError, match="uint8 device tensor"):
        ops.upsample_u8(host, 2, "bicubic")


def test_baseline_constructor_checks_and_empty_state():
    import pssr2_amd
    from pssr2_amd.baselines import Baseline
    assert pssr2_amd.Baseline is Baseline
    m = Baseline()
    assert (m.scale, m.channels, m.filter, m.denoise) == (4, 1, "bicubic", None)
    assert len(m.state_dict()) == 0 and list(m.parameters()) == [] and m.eval() is m and m.to("cpu") is m
    assert getattr(m, "_engine", None) is None           # the drivers' path for arbitrary modules, not the captured replay
    m = Baseline(2, 3, filter="bilinear", denoise={"h": 10, "patch_radius": 2})
    assert m._nlm == (2, 7) + R.nlm_params(10, 0.0, 5)
    for bad in (0, 9, 2.5, True):
        with pytest.raises(ValueError, match="scale"):
            Baseline(bad)
    for bad in (0, -1, 1.0, True):
        with pytest.raises(ValueError, match="channels"):
            Baseline(4, bad)
    with pytest.raises(ValueError, match="filter"):
        Baseline(4, filter="nearest")
    with pytest.raises(TypeError):
        Baseline(4, 1, "bicubic")                        # filter is keyword-only
    for bad in ({}, {"sigma": 3.0}, {"h": 8, "strength": 1}, "nlm", 8.0):
        with pytest.raises(ValueError, match="denoise"):
            Baseline(4, denoise=bad)
    with pytest.raises(ValueError, match="h must"):
        Baseline(4, denoise={"h": 0.1})
    with pytest.raises(ValueError, match="search_radius"):
        Baseline(4, denoise={"h": 8, "search_radius": 11})
    with pytest.raises(RuntimeError, match="MI355X"):
        Baseline(4)(torch.zeros(1, 1, 8, 8))


# ------------------------------------------------------------------------------------------------ argument checks of the entry points
def _lib():
    path = ROOT / "pssr2_amd" / "libpssr_mi355.so"
    if not path.exists():
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(str(path))
    lib.pssr_last_error.restype = ctypes.c_char_p
    return lib


def test_baseline_entry_points_validate_without_gpu():
    """PSSR_ERR_ARG from both entry points; nothing is launched, so no device is needed."""
    lib = _lib()
    i, p = ctypes.c_int, ctypes.c_void_p
    nlm, up = lib.pssr_nlm_u8, lib.pssr_upsample_u8
    nlm.argtypes = [p] * 2 + [i] * 8 + [p]
    up.argtypes = [p] * 2 + [i] * 5 + [p]
    fake, other = 0x1000, 0x2000          # never dereferenced: every call below fails its checks

    def err(status, word):
        return status == -1 and word in lib.pssr_last_error()

    # x, out, planes, H, W, p, s, qmul, qshift, bias
    good = (1, 8, 8, 2, 7, 512, 10, 0)
    assert err(nlm(None, other, *good, None), b"null") and err(nlm(fake, None, *good, None), b"null")
    assert err(nlm(fake, fake, *good, None), b"in place")
    for bad in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, -2)):
        assert err(nlm(fake, other, *bad, 2, 7, 512, 10, 0, None), b"positive")
    for bad in (0, 4, -1):
        assert err(nlm(fake, other, 1, 8, 8, bad, 7, 512, 10, 0, None), b"patch radius")
    for bad in (0, 11, -1):
        assert err(nlm(fake, other, 1, 8, 8, 2, bad, 512, 10, 0, None), b"search radius")
    for bad in (0, 1024, -5):
        assert err(nlm(fake, other, 1, 8, 8, 2, 7, bad, 10, 0, None), b"qmul")
    for bad in (-1, 32):
        assert err(nlm(fake, other, 1, 8, 8, 2, 7, 512, bad, 0, None), b"qshift")
    assert err(nlm(fake, other, 1, 8, 8, 2, 7, 512, 10, -1, None), b"bias")
    assert err(nlm(fake, other, 1, 16385, 16384, 2, 7, 512, 10, 0, None), b"2^28")
    # x, out, planes, h, w, r, filter
    assert err(up(None, other, 1, 8, 8, 4, 1, None), b"null") and err(up(fake, None, 1, 8, 8, 4, 1, None), b"null")
    assert err(up(fake, fake, 1, 8, 8, 4, 1, None), b"in place")
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-3, 8, 8)):
        assert err(up(fake, other, *bad, 4, 1, None), b"positive")
    for bad in (0, 9, -2):
        assert err(up(fake, other, 1, 8, 8, bad, 1, None), b"scale")
    for bad in (-1, 2):
        assert err(up(fake, other, 1, 8, 8, 4, bad, None), b"filter")
    assert err(up(fake, other, 1, 16385, 16384, 1, 0, None), b"2^28")
    assert err(up(fake, other, 1, 8192, 8192, 4, 0, None), b"output")
    table = (ctypes.c_int32 * 256)()
    assert lib.pssr_nlm_lut(table) == 0 and list(table) == R.nlm_lut().tolist()
    assert err(lib.pssr_nlm_lut(None), b"null")
