"""The classical baselines on the device: pssr_upsample_u8 and pssr_nlm_u8 against the restatement of tests/_baseline_ref.py and the
Pillow fixture, util.upsample / util.nlm_denoise, and the Baseline module through the drivers.  ``==`` only."""
import math
import re
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest
import torch

import _baseline_ref as R

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
PLANES_CAP = int(re.search(r"U8_PLANES_CAP\s*=\s*(\d+)", (ROOT / "pssr2_amd" / "csrc" / "u8_planes.h").read_text()).group(1))
UP_SHAPES = ((1, 1), (1, 9), (5, 7), (3, 40), (33, 17), (64, 64), (70, 130))
UP_SCALES = (1, 2, 3, 4, 5, 8)
NLM_SHAPES = ((1, 1), (1, 40), (3, 3), (17, 33), (64, 64), (70, 130))        # the tile is 32 x 8: 33, 70 and 130 are no multiples
NLM_PS = ((1, 1), (1, 5), (2, 7), (3, 10))
NLM_H, NLM_SIGMA = (0.5, 8, 255), (0, 12)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _off_by_one(a):
    """The same values on the device at a start address that is no multiple of 16 (nor of 2)."""
    a = np.ascontiguousarray(a)
    flat = torch.empty(a.size + 1, dtype=torch.uint8, device="cuda")
    flat[1:] = _dev(a).reshape(-1)
    t = flat[1:].view(a.shape)
    assert t.data_ptr() % 2 == 1 and t.is_contiguous()
    return t


def _diff(got, want):
    """The first few places where two arrays differ, for an assertion's message."""
    idx = np.argwhere(np.asarray(got) != np.asarray(want))[:6]
    return [(tuple(int(v) for v in i), int(got[tuple(i)]), int(want[tuple(i)])) for i in idx]


def _rand(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ upsample_u8
def _up_inputs(h, w):
    """[4, h, w]: random, all 0, all 255, the 0 / 255 checkerboard."""
    return np.stack([_rand((h, w), h * 1000 + w), np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8), R.checkerboard(h, w)])


@pytest.mark.parametrize("filter", R.FILTERS)
@pytest.mark.parametrize("shape", UP_SHAPES)
def test_upsample_u8_against_the_restatement(shape, filter):
    from pssr2_amd import ops
    x = _up_inputs(*shape)
    for r in UP_SCALES:
        got = ops.upsample_u8(_dev(x), r, filter).cpu().numpy()
        assert got.shape == (4, shape[0] * r, shape[1] * r)
        want = R.upsample(x, r, filter)
        assert np.array_equal(got, want), (shape, r, filter, _diff(got, want))


@pytest.mark.parametrize("filter", R.FILTERS)
def test_upsample_u8_equals_the_pillow_fixture(golden, filter):
    from pssr2_amd import ops
    g = golden("baseline_pil.npz")
    for name in sorted(k[:-3] for k in g.files if k.endswith("_in")):
        got = ops.upsample_u8(_dev(g[f"{name}_in"]), int(g[f"{name}_r"]), filter).cpu().numpy()
        assert np.array_equal(got, g[f"{name}_{filter}"]), (name, filter)


@pytest.mark.parametrize("filter", R.FILTERS)
def test_upsample_u8_planes_views_and_addresses(filter):
    from pssr2_amd import ops
    one = _rand((1, 33, 17), 1)
    assert np.array_equal(ops.upsample_u8(_dev(one), 3, filter).cpu().numpy(), R.upsample(one, 3, filter))
    three = _rand((3, 16, 48), 2)                                   # rows of whole 16-byte pieces
    want = R.upsample(three, 2, filter)
    assert np.array_equal(ops.upsample_u8(_dev(three), 2, filter).cpu().numpy(), want)
    assert np.array_equal(ops.upsample_u8(_off_by_one(three), 2, filter).cpu().numpy(), want)       # the same rows from an odd address
    many = _rand((PLANES_CAP + 6, 3, 3), 3)
    assert np.array_equal(ops.upsample_u8(_dev(many), 2, filter).cpu().numpy(), R.upsample(many, 2, filter))
    base = _dev(_rand((2, 40, 70), 4))
    view = base[:, 3:30, 5:61]                                      # a non-contiguous view is copied, not refused
    assert not view.is_contiguous()
    got = ops.upsample_u8(view, 4, filter)
    assert np.array_equal(got.cpu().numpy(), R.upsample(view.cpu().numpy(), 4, filter))
    assert torch.equal(got, ops.upsample_u8(view, 4, filter))       # two calls, the same bits
    batch = _dev(_rand((2, 3, 5, 7), 5))                            # leading axes are kept
    assert ops.upsample_u8(batch, 2, filter).shape == (2, 3, 10, 14)


# ------------------------------------------------------------------------------------------------ nlm_u8
def _params(P):
    return [R.nlm_params(h, sigma, P) for h in NLM_H for sigma in NLM_SIGMA]


def _ramp(h, w, seed):
    yy, xx = np.mgrid[:h, :w]
    noise = np.random.default_rng(seed).normal(0.0, 6.0, (h, w))
    return np.clip(np.rint(40 + 150 * (xx + yy) / max(h + w - 2, 1) + noise), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("p, s", NLM_PS)
@pytest.mark.parametrize("shape", NLM_SHAPES)
def test_nlm_u8_against_the_restatement(shape, p, s):
    """Random planes and a smooth ramp plus noise (weights spread over the table), every h and sigma of the set."""
    from pssr2_amd import ops
    x = np.stack([_rand(shape, shape[0] * 100 + p), _ramp(*shape, seed=s)])
    params = _params(2 * p + 1)
    for (want, _), prm in zip(R.nlm_multi(x, p, s, params), params):
        got = ops.nlm_u8(_dev(x), p, s, *prm).cpu().numpy()
        assert np.array_equal(got, want), (shape, p, s, prm, _diff(got, want))


@pytest.mark.parametrize("p, s", NLM_PS)
def test_nlm_u8_constant_planes_and_checkerboard_come_back(p, s):
    """Constant 0 and 255 (the largest sum wgt v) and the checkerboard (the largest ssd: q clamps, only candidates of the pixel's own
    value keep a weight): the output is the input."""
    from pssr2_amd import ops
    for shape in ((17, 33), (70, 130)):
        x = np.stack([np.zeros(shape, np.uint8), np.full(shape, 255, np.uint8), R.checkerboard(*shape)])
        for prm in (R.nlm_params(0.5, 0, 2 * p + 1), (1023, 0, 0)):
            assert np.array_equal(ops.nlm_u8(_dev(x), p, s, *prm).cpu().numpy(), x), (shape, p, s, prm)
        flat = x[:2]                                                 # every weight LUT[0]: 255 * (2s + 1)^2 * 16129 in the numerator
        assert np.array_equal(ops.nlm_u8(_dev(flat), p, s, *R.nlm_params(255, 12, 2 * p + 1)).cpu().numpy(), flat)


def test_nlm_u8_planes_views_and_addresses():
    from pssr2_amd import ops
    prm = R.nlm_params(8, 0, 5)
    one = _rand((1, 17, 33), 1)
    assert np.array_equal(ops.nlm_u8(_dev(one), 2, 3, *prm).cpu().numpy(), R.nlm(one, 2, 3, *prm)[0])
    three = _rand((3, 16, 48), 2)                                   # rows of whole 16-byte pieces
    want = R.nlm(three, 2, 3, *prm)[0]
    assert np.array_equal(ops.nlm_u8(_dev(three), 2, 3, *prm).cpu().numpy(), want)
    assert np.array_equal(ops.nlm_u8(_off_by_one(three), 2, 3, *prm).cpu().numpy(), want)           # the same rows from an odd address
    many = _rand((PLANES_CAP + 6, 3, 3), 3)
    assert np.array_equal(ops.nlm_u8(_dev(many), 2, 3, *prm).cpu().numpy(), R.nlm(many, 2, 3, *prm)[0])
    base = _dev(_rand((2, 40, 70), 4))
    view = base[:, 3:30, 5:61]
    assert not view.is_contiguous()
    got = ops.nlm_u8(view, 2, 3, *prm)
    assert np.array_equal(got.cpu().numpy(), R.nlm(view.cpu().numpy(), 2, 3, *prm)[0])
    assert torch.equal(got, ops.nlm_u8(view, 2, 3, *prm))           # two calls, the same bits


# ------------------------------------------------------------------------------------------------ util
@lru_cache(maxsize=None)
def _lr_batch():
    return _rand((2, 3, 16, 16), 21)


def test_util_upsample_and_nlm_denoise_inputs_and_outputs():
    from pssr2_amd import util
    x = _lr_batch()
    want_up = R.upsample(x, 4, "bicubic")
    want_nl = R.nlm_denoise(x, h=12, sigma=10, patch_radius=1, search_radius=3)
    kw = dict(h=12, sigma=10, patch_radius=1, search_radius=3)
    for src in (x, _dev(x)):
        got = util.upsample(src, 4)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want_up)
        got = util.upsample(src, 4, to_numpy=False)
        assert torch.is_tensor(got) and got.is_cuda and np.array_equal(got.cpu().numpy(), want_up)
        got = util.nlm_denoise(src, **kw)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want_nl)
        got = util.nlm_denoise(src, to_numpy=False, **kw)
        assert torch.is_tensor(got) and got.is_cuda and np.array_equal(got.cpu().numpy(), want_nl)
        assert np.array_equal(util.upsample(src[0], 4), want_up[0]) and np.array_equal(util.nlm_denoise(src[0], **kw), want_nl[0])      # 3-D
    assert np.array_equal(util.upsample(x, 2, filter="bilinear"), R.upsample(x, 2, "bilinear"))
    assert np.array_equal(util.nlm_denoise(x, h=9), R.nlm_denoise(x, h=9))                       # the defaults: p = 2, s = 7, sigma = 0


# ------------------------------------------------------------------------------------------------ Baseline
def _as_u8(y):
    """What the drivers make of a model's output: clip and truncate (pssr2_amd.predict._pred_tensor)."""
    from pssr2_amd.predict import _pred_tensor
    return _pred_tensor(y, y.shape[1]).cpu().numpy()        # all of the output's planes


def test_baseline_forward_is_the_two_launches():
    from pssr2_amd import ops
    from pssr2_amd.baselines import Baseline
    x = _lr_batch()[:, :1]
    lr = _dev(x).float()
    y = Baseline(4).cuda().eval()(lr)
    assert y.dtype == torch.float32 and y.shape == (2, 1, 64, 64)
    assert np.array_equal(_as_u8(y), ops.upsample_u8(_dev(x), 4, "bicubic").cpu().numpy())
    assert np.array_equal(_as_u8(y), R.upsample(x, 4, "bicubic"))
    assert np.array_equal(_as_u8(Baseline(2, filter="bilinear")(lr)), R.upsample(x, 2, "bilinear"))
    assert np.array_equal(_as_u8(Baseline(4)(_dev(x))), R.upsample(x, 4, "bicubic"))            # uint8 items, as the ensemble hands them
    kw = dict(h=12, sigma=10, patch_radius=1, search_radius=3)
    want = R.upsample(R.nlm_denoise(x, **kw), 4, "bicubic")
    assert np.array_equal(_as_u8(Baseline(4, denoise=kw)(lr)), want)
    # round half to even, then clip, in front of the kernels
    frac = torch.tensor([[-3.0, 0.5, 1.5, 2.5], [254.5, 255.5, 300.0, 99.49]], device="cuda").view(1, 1, 2, 4)
    assert np.array_equal(_as_u8(Baseline(1)(frac)), np.array([[0, 0, 2, 2], [254, 255, 255, 99]], dtype=np.uint8).reshape(1, 1, 2, 4))


def test_baseline_keeps_the_centre_frames():
    from pssr2_amd.baselines import Baseline
    x = _lr_batch()                                                  # n_frames = 3
    assert np.array_equal(_as_u8(Baseline(4)(_dev(x).float())), R.upsample(x[:, 1:2], 4, "bicubic"))
    assert np.array_equal(_as_u8(Baseline(2, 3)(_dev(x).float())), R.upsample(x, 2, "bicubic"))
    five = _rand((1, 5, 8, 8), 22)
    assert np.array_equal(_as_u8(Baseline(2, 3)(_dev(five).float())), R.upsample(five[:, 1:4], 2, "bicubic"))
    with pytest.raises(ValueError, match="frames"):
        Baseline(2, 3)(_dev(x[:, :2]).float())


class _Pairs(torch.utils.data.Dataset):
    """A paired dataset in memory: LR [1, 16, 16] random, HR [1, 64, 64], handed over as float32."""
    is_lr, extra_hr_files, lr_scale = False, None, 4

    def __init__(self, n=2):
        rng = np.random.default_rng(31)
        self.lrs = rng.integers(0, 256, size=(n, 1, 16, 16), dtype=np.uint8)
        self.hrs = rng.integers(0, 256, size=(n, 1, 64, 64), dtype=np.uint8)
        self.val_idx, self.crop_res = list(range(n)), 64

    def __len__(self):
        return len(self.lrs)

    def _get_name(self, i):
        return f"img{i}"

    def __getitem__(self, i):
        return torch.tensor(self.hrs[i]).float(), torch.tensor(self.lrs[i]).float()


@pytest.mark.parametrize("denoise", [None, dict(h=12, sigma=10, patch_radius=1, search_radius=3)])
def test_baseline_through_test_metrics_and_predict_images(denoise):
    from pssr2_amd.baselines import Baseline
    from pssr2_amd.predict import predict_images, test_metrics
    ds = _Pairs()
    lr = ds.lrs[0] if denoise is None else R.nlm_denoise(ds.lrs[0], **denoise)
    hat = R.upsample(lr, 4, "bicubic")
    err = float(((ds.hrs[0].astype(np.int64) - hat) ** 2).sum()) / hat.size
    got = test_metrics(Baseline(4, denoise=denoise), ds, device="cuda", metrics=("mse", "psnr"), norm=False, avg=False)
    assert got == {"mse": [err / 255 ** 2] * 2, "psnr": [10 * math.log10(255 ** 2 / err)] * 2}   # every iteration: dataset[0], as upstream
    preds = predict_images(Baseline(4, denoise=denoise), ds, device="cuda", batch_size=2, out_dir=None)
    assert np.array_equal(preds["img0"], hat)


def test_baseline_through_predict_sheet_equals_upsample_inside_the_tiles():
    """Each tile is enlarged on its own, so its clipped, renormalised border taps differ from those of the whole sheet: bicubic reaches 2
    LR pixels, and the two agree on every pixel at least 2 r from a tile edge (checked), not nearer (not asserted either way)."""
    from pssr2_amd import util
    from pssr2_amd.baselines import Baseline
    from pssr2_amd.predict import predict_sheet
    r, tile = 4, 16
    sheet = _rand((1, 32, 48), 41)
    got = predict_sheet(Baseline(r), sheet, tile_res=tile, overlap=0)
    whole = util.upsample(sheet, r)
    assert got.shape == whole.shape == (1, 32 * r, 48 * r)
    d = np.arange(48 * r) % (tile * r)
    inner = (d >= 2 * r) & (d < tile * r - 2 * r)
    mask = inner[:32 * r, None] & inner[None, :]
    assert mask.sum() == (2 * 3) * (tile * r - 4 * r) ** 2
    assert np.array_equal(got[0][mask], whole[0][mask])
    assert np.array_equal(got[0, :tile * r, :tile * r], R.upsample(sheet[0, :tile, :tile], r, "bicubic"))     # a tile is its own enlargement
