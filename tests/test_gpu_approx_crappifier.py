"""approximate_crappifier on the MI355X: the noise-profile kernels against numpy, the objective against the reference's recorded draws
and curve (tests/golden/paired.npz, paired_poisson.npz: tools/gen_golden_paired.py), the device paired dataset against the host one,
parameter recovery, and the paired datasets through the existing drivers."""
import math
import random
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
BINS = np.arange(-256, 256)
EDGE_VALUES = [-256.0, -256.5, -255.999, 254.999, 255.0, 255.0001, 1000.0, -1000.0, 0.0, -0.0, 0.999999, -1e-30]
NON_FINITE = [float("nan"), float("inf"), float("-inf")]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD / "paired.npz", allow_pickle=False)


def _bits(t):
    return t.view(torch.int64).cpu().numpy()


def _expected(a, b):
    """np.histogram and the exactly rounded sum (math.fsum) of the float32 profile a - b per image."""
    v = a.astype(np.float32) - b.astype(np.float32)
    assert v.dtype == np.float32
    flat = v.reshape(len(v), -1)
    hist = np.stack([np.histogram(row, BINS)[0] for row in flat])
    with np.errstate(invalid="ignore"):
        sums = np.array([math.fsum(row.astype(np.float64)) if np.all(np.isfinite(row)) else row.astype(np.float64).sum() for row in flat])
    return flat, hist, sums


# shapes: one strip and one workgroup per image; several workgroups per image (integer atomics + the fold launch), 3 channels; sizes that
# are not a multiple of the 16-value vector (scalar instantiation) with one and with two workgroups; many small images
SHAPES = [(5, 1, 64, 64), (3, 3, 96, 96), (3, 1, 37, 41), (4, 3, 50, 50), (300, 1, 32, 32)]


@pytest.mark.parametrize("shape", SHAPES)
def test_noise_profile_f32_vs_numpy(shape):
    from pssr2_amd import ops
    r = np.random.default_rng(sum(shape))
    a = (r.standard_normal(shape) * 40).astype(np.float32)
    b = r.integers(0, 256, shape, dtype=np.uint8)
    a += b                                                   # profiles around zero, like a crappified image
    per = int(np.prod(shape[1:]))
    # image 0: the edge values, injected as the profile itself (b = 0 there)
    flat_a, flat_b = a.reshape(shape[0], -1), b.reshape(shape[0], -1)
    flat_b[0, :len(EDGE_VALUES)] = 0
    flat_a[0, :len(EDGE_VALUES)] = EDGE_VALUES
    # image 1: the whole mass in three neighbouring bins
    flat_b[1] = 7
    flat_a[1] = (7 + r.choice(np.array([-0.5, 0.3, 1.7], dtype=np.float32), per)).astype(np.float32)
    # last image: NaN and both infinities as well (its sum is NaN)
    flat_b[-1, :3] = 0
    flat_a[-1, :3] = NON_FINITE
    v, hist, sums = _expected(a, b)
    assert np.count_nonzero(hist[1]) == 3 and hist[1].sum() == per

    got_hist, got_sum = ops.noise_profile(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    assert got_hist.dtype == torch.int32 and tuple(got_hist.shape) == (shape[0], 511) and got_sum.dtype == torch.float64
    assert np.array_equal(got_hist.cpu().numpy(), hist)                       # counts: exact
    got = got_sum.cpu().numpy()
    assert math.isnan(got[-1]) and math.isnan(sums[-1])
    # sums: the kernel adds n float32 values in f64 in a fixed order; against the exactly rounded sum every such order is within
    # (n - 1) * 2^-53 * sum|v| (the classical bound of recursive summation), and one more rounding for fsum's result
    for i in range(shape[0] - 1):
        bound = per * 2.0 ** -53 * float(np.abs(v[i].astype(np.float64)).sum())
        print(f"image {i}: sum {got[i]!r} exact {sums[i]!r} |diff| {abs(got[i] - sums[i]):.3e} bound {bound:.3e}")
        assert abs(got[i] - sums[i]) <= bound
    again_hist, again_sum = ops.noise_profile(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    assert torch.equal(again_hist, got_hist) and np.array_equal(_bits(again_sum), _bits(got_sum))        # same bits, NaN included


@pytest.mark.parametrize("shape", SHAPES)
def test_noise_profile_u8_is_exact(shape):
    from pssr2_amd import ops
    r = np.random.default_rng(sum(shape) + 1)
    a = r.integers(0, 256, shape, dtype=np.uint8)
    b = np.clip(a.astype(np.int64) + r.integers(-30, 31, shape), 0, 255).astype(np.uint8)
    a.reshape(shape[0], -1)[0, :4] = [0, 255, 255, 0]
    b.reshape(shape[0], -1)[0, :4] = [255, 0, 255, 0]            # profiles -255, 255, 0, 0
    v, hist, sums = _expected(a, b)
    got_hist, got_sum = ops.noise_profile(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    assert np.array_equal(got_hist.cpu().numpy(), hist)
    assert np.array_equal(got_sum.cpu().numpy(), (a.astype(np.int64) - b.astype(np.int64)).reshape(shape[0], -1).sum(axis=1).astype(np.float64))
    again_hist, again_sum = ops.noise_profile(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    assert torch.equal(again_hist, got_hist) and np.array_equal(_bits(again_sum), _bits(got_sum))


def test_noise_profile_argument_validation():
    from pssr2_amd import _lib as L, ops
    a = torch.zeros(2, 1, 8, 8, device="cuda")
    b = torch.zeros(2, 1, 8, 8, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        ops.noise_profile(a, b.float())
    with pytest.raises(ValueError):
        ops.noise_profile(a[:1], b)
    lib = L.lib()
    assert lib.pssr_noise_profile_f32(None, L.ptr(b), None, None, 2, 64, None, 0, None) != 0
    assert b"noise_profile_f32" in lib.pssr_last_error()
    assert lib.pssr_noise_profile_loss(None, None, None, None, 1, 64, 8, None, None, None, None) != 0
    assert b"noise_profile_loss" in lib.pssr_last_error()
    assert lib.pssr_noise_profile_workspace_bytes(4, 16384) == 4 * 4 * 8 and lib.pssr_noise_profile_workspace_bytes(4096, 16384) == 0


def test_noise_profile_loss_vs_numpy():
    from pssr2_amd import ops
    r = np.random.default_rng(2)
    images, per, width = 300, 4096, 64
    ph, th = r.multinomial(per, np.ones(511) / 511, images).astype(np.int32), r.multinomial(per, np.ones(511) / 511, images).astype(np.int32)
    ps, ts = r.standard_normal(images) * per, r.standard_normal(images) * per
    loss, mean, parts = ops.noise_profile_loss(*(torch.from_numpy(x).cuda() for x in (ph, ps, th, ts)), per, width, terms=True)
    dist = np.array([np.mean((t.astype(np.int64) - p.astype(np.int64)) ** 2) / (width ** 2) for p, t in zip(ph, th)])
    value = np.abs(ts / per - ps / per)
    assert np.array_equal(parts.cpu().numpy()[:, 0], dist) and np.array_equal(parts.cpu().numpy()[:, 1], value)
    assert np.array_equal(loss.cpu().numpy(), dist + value)
    # the mean: 300 f64 values added in a fixed tree, against fsum
    exact = math.fsum(dist + value) / images
    assert abs(float(mean.item()) - exact) <= images * 2.0 ** -53 * float(np.sum(dist + value)) / images + 2.0 ** -53 * exact


@pytest.mark.parametrize("tag", ["gaussian", "poisson"])
def test_objective_with_the_reference_draws(gold, tag):
    """The reference's own ``lr_hat`` arrays through the profile and loss kernels."""
    from pssr2_amd import ops
    d = gold if tag == "gaussian" else np.load(GOLD / "paired_poisson.npz", allow_pickle=False)
    order = d[f"obj/{tag}/order"]
    assert np.array_equal(ops.bilinear_down_u8(torch.from_numpy(gold["obj/hr"]).cuda(), 128, 128).cpu().numpy(), gold["obj/ds_hr"])
    ds_hr, lr = gold["obj/ds_hr"][order], gold["obj/lr"][order]
    lr_hat = d[f"obj/{tag}/lr_hat"]
    assert lr_hat.dtype == np.float32 and lr_hat.shape == ds_hr.shape == (8, 1, 128, 128)
    ds_dev = torch.from_numpy(ds_hr).cuda()
    pred = ops.noise_profile(torch.from_numpy(lr_hat).cuda(), ds_dev)
    target = ops.noise_profile(torch.from_numpy(lr).cuda(), ds_dev)
    n, width = 128 * 128, 128
    loss, mean, parts = ops.noise_profile_loss(*pred, *target, n, width, terms=True)
    parts, terms = parts.cpu().numpy(), d[f"obj/{tag}/terms"]
    assert np.array_equal(parts[:, 0], terms[:, 0])                      # histogram term: bit for bit
    # value term: the reference takes both means in float32 with numpy's pairwise summation; worst case per mean
    # 2 (ceil(log2 n) + 2) 2^-24 mean|v|.  The kernel's own f64 round-off (n 2^-53 mean|v|) is nine orders below that.
    depth = 2 * (math.ceil(math.log2(n)) + 2) * 2.0 ** -24
    bounds = []
    for i in range(8):
        vp = np.abs(lr_hat[i].astype(np.float32) - ds_hr[i].astype(np.float32)).astype(np.float64).mean()
        vt = np.abs(lr[i].astype(np.float32) - ds_hr[i].astype(np.float32)).astype(np.float64).mean()
        bounds.append(depth * (vp + vt))
        print(f"{tag} image {i}: value term {parts[i, 1]!r} reference {terms[i, 1]!r} |diff| {abs(parts[i, 1] - terms[i, 1]):.3e} bound {bounds[-1]:.3e}")
        assert abs(parts[i, 1] - terms[i, 1]) <= bounds[-1]
    value, ref = float(mean.item()), float(d[f"obj/{tag}/value"])
    print(f"{tag}: objective {value!r} reference {ref!r} |diff| {abs(value - ref):.3e} bound {np.mean(bounds):.3e}")
    assert abs(value - ref) <= float(np.mean(bounds)) + 8 * 2.0 ** -53 * ref


# ------------------------------------------------------------------------------------------ device paired dataset
def _same_items(dev_item, host_item):
    assert dev_item[0].is_cuda and dev_item[1].is_cuda and dev_item[0].dtype == torch.float32
    assert torch.equal(dev_item[0].cpu(), host_item[0]) and torch.equal(dev_item[1].cpu(), host_item[1])


@pytest.mark.parametrize("name", ["equal", "crop", "pad", "nonsq"])
def test_device_paired_dataset_equals_the_host_dataset(gold, name):
    from pssr2_amd.data import DevicePairedTileDataset, PairedArrayDataset
    hr, lr = gold[f"geo/{name}/hr_in"], gold[f"geo/{name}/lr_in"]
    host, dev = PairedArrayDataset(hr, lr, 32, 4), DevicePairedTileDataset(hr, lr, 32, 4)
    assert dev.val_idx == host.val_idx and len(dev) == len(host) and repr(dev).splitlines()[-1] == repr(host).splitlines()[-1]
    for i in range(len(host)):
        _same_items(dev[i], host[i])
        assert np.array_equal(dev[i][0].cpu().numpy(), gold[f"geo/{name}/hr"][i]) and np.array_equal(dev[i][1].cpu().numpy(), gold[f"geo/{name}/lr"][i])
    with pytest.raises(IndexError):
        dev[len(dev)]
    host, dev = PairedArrayDataset(hr, lr, 32, 4, val_split=0.25), DevicePairedTileDataset(hr, lr, 32, 4, val_split=0.25)
    for seed in gold["geo/draw_seeds"]:
        random.seed(int(seed))
        a = host[0]
        random.seed(int(seed))
        _same_items(dev[0], a)
    # whole batches: one host draw, the same rotation sequence as item-by-item access
    idx = [0, 1, len(host) - 1, 0, 1]
    random.seed(5)
    items = [host[i] for i in idx]
    state = random.getstate()
    random.seed(5)
    hr_b, lr_b = dev.device_pair_batch(dev.draw_pair_items(idx))
    assert random.getstate() == state
    assert torch.equal(hr_b.cpu(), torch.stack([a for a, _ in items])) and torch.equal(lr_b.cpu(), torch.stack([b for _, b in items]))
    random.seed(5)
    hr_u8, lr_u8 = dev.device_pair_batch(dev.draw_pair_items(idx), u8=True)
    assert hr_u8.dtype == torch.uint8 and torch.equal(hr_u8.float(), hr_b) and torch.equal(lr_u8.float(), lr_b)


def test_device_paired_dataset_centre_frames(gold):
    from pssr2_amd.data import DevicePairedTileDataset
    hr, lr = gold["frames/hr_in"], gold["frames/lr_in"]
    dev = DevicePairedTileDataset(np.stack([hr, hr]), np.stack([lr, lr]), 32, 4, n_frames=[3, 1], val_split=0.5)
    a, b = dev[1]
    assert np.array_equal(a.cpu().numpy(), gold["frames/plain_hr"]) and np.array_equal(b.cpu().numpy(), gold["frames/plain_lr"])
    random.seed(int(gold["frames/seed"]))
    a, b = dev[0]
    assert np.array_equal(a.cpu().numpy(), gold["frames/rot_hr"]) and np.array_equal(b.cpu().numpy(), gold["frames/rot_lr"])


# ------------------------------------------------------------------------------------------ the objective and the driver
def test_statistical_parity_with_the_reference_curve(gold):
    """16 device values at each of the 15 grid points against the reference's 16: the means agree within five standard errors
    (the generators differ, and 15 points are tested at once).  The device run is deterministic: fixed Philox seed, fixed subsets."""
    from pssr2_amd import AdditiveGaussian
    from pssr2_amd.data import PairedArrayDataset
    from pssr2_amd.train import _Crappifier_Objective
    ds = PairedArrayDataset(gold["obj/hr"], gold["obj/lr"], 256, 2)
    obj = _Crappifier_Objective(AdditiveGaussian, ds, 8, device="cuda", seed=0)
    assert np.array_equal(obj.ds_hr.cpu().numpy(), gold["obj/ds_hr"])
    curve = gold["obj/curve"]
    random.seed(0)
    bad = []
    for a, intensity in enumerate(gold["obj/curve_intensity"]):
        for b, gain in enumerate(gold["obj/curve_gain"]):
            dev = np.array([obj.sample([float(intensity), float(gain)]) for _ in range(16)])
            ref = curve[a, b]
            tol = 5 * math.sqrt((ref.std(ddof=1) ** 2 + dev.std(ddof=1) ** 2) / 16)
            diff = abs(dev.mean() - ref.mean())
            print(f"intensity {intensity} gain {gain}: device {dev.mean():.5f} +- {dev.std(ddof=1):.5f}  reference {ref.mean():.5f} +- "
                  f"{ref.std(ddof=1):.5f}  |diff| {diff:.5f} tolerance {tol:.5f}")
            if not diff <= tol:
                bad.append((int(intensity), int(gain), diff, tol))
    assert not bad, bad


@pytest.fixture(scope="module")
def em_pairs():
    """32 synthetic tiles of 512^2 and their LR = Pillow reduction to 128^2 + N(2, 9), rounded and clipped."""
    from pssr2_amd.data import _resize_bilinear_u8, synthetic_em_tile
    rng = np.random.RandomState(123)
    hr = np.stack([synthetic_em_tile(i, 512) for i in range(32)])
    ds = np.stack([_resize_bilinear_u8(t, 128) for t in hr])
    lr = np.clip(np.round(ds + rng.normal(2, 9, ds.shape)), 0, 255).astype(np.uint8)
    return hr, lr


@pytest.mark.parametrize("state", [0, 1, 2])
def test_recovers_the_noise_parameters(em_pairs, state):
    """AdditiveGaussian fitted to pairs made with N(2, 9).  The box comes from the reference's objective on this data (its floor is
    0.075 +- 0.007 at (9, 2); every edge of the box is at least ten standard deviations above it, intensity 8 - 10 within two)."""
    from pssr2_amd import AdditiveGaussian, approximate_crappifier
    from pssr2_amd.bayes import gp_minimize
    from pssr2_amd.data import PairedArrayDataset
    ds = PairedArrayDataset(*em_pairs, 512, 4)
    random.seed(state)
    res = approximate_crappifier(AdditiveGaussian, [(0, 20), (-5, 5)], ds, max_images=8, opt_kwargs=dict(n_calls=40, random_state=state),
                                 minimizer=gp_minimize)
    print(f"random_state {state}: x = {res.x}, fun = {res.fun:.5f}")
    assert len(res.func_vals) == 40 and res.fun == min(res.func_vals)
    assert 6 <= res.x[0] <= 12 and 1.5 <= res.x[1] <= 2.5


def test_same_seeds_same_run_and_the_errors(em_pairs):
    from pssr2_amd import AdditiveGaussian, Crappifier, MultiCrappifier, Poisson, approximate_crappifier
    from pssr2_amd.data import DevicePairedTileDataset, PairedArrayDataset
    hr, lr = em_pairs[0][:6, :, :128, :128], em_pairs[1][:6, :, :32, :32]
    ds = PairedArrayDataset(hr, lr, 128, 4)
    runs = []
    for dataset in (ds, ds, DevicePairedTileDataset(hr, lr, 128, 4)):       # the device dataset is used in place: the same numbers
        random.seed(4)
        runs.append(approximate_crappifier(AdditiveGaussian, [(0.0, 20.0), (-5.0, 5.0)], dataset, max_images=4, seed=3,
                                           opt_kwargs=dict(n_calls=14, random_state=2)))
    for other in runs[1:]:
        assert other.x_iters == runs[0].x_iters and np.array_equal(other.func_vals, runs[0].func_vals)
    random.seed(4)
    other = approximate_crappifier(AdditiveGaussian, [(0.0, 20.0), (-5.0, 5.0)], ds, max_images=4, seed=4, opt_kwargs=dict(n_calls=14, random_state=2))
    assert not np.array_equal(other.func_vals, runs[0].func_vals)             # another noise seed: other values

    class HostOnly(Crappifier):
        def __init__(self, *params):
            pass

        def crappify(self, image):
            return image

    with pytest.raises(NotImplementedError, match="device path"):
        approximate_crappifier(HostOnly, [(0.0, 1.0)], ds, opt_kwargs=dict(n_calls=3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        approximate_crappifier(AdditiveGaussian, [(0.0, 20.0)], ds, device="cpu")

    class Fractions(torch.utils.data.Dataset):
        val_idx, is_lr = [0, 1], False

        def __len__(self):
            return 2

        def __getitem__(self, i):
            return torch.full((1, 32, 32), 10.5), torch.full((1, 8, 8), 10.0)

    with pytest.raises(ValueError, match="not integers"):
        approximate_crappifier(AdditiveGaussian, [(0.0, 20.0)], Fractions())

    # a factory instead of a class; a single dimension that is not wrapped in a list; every sample of a rotating training dataset
    rot = PairedArrayDataset(hr, lr, 128, 4, val_split=0.5, split_seed=0)
    res = approximate_crappifier(lambda sigma, lam: MultiCrappifier(Poisson(lam), AdditiveGaussian(sigma, 2)), [(0.0, 20.0), (0.0, 1.0)], rot,
                                 opt_kwargs=dict(n_calls=12, random_state=0))
    assert len(res.x_iters) == 12 and np.all(np.isfinite(res.func_vals)) and rot.rotation is True
    res = approximate_crappifier(AdditiveGaussian, (0.0, 20.0), ds, max_images=100, opt_kwargs=dict(n_calls=11, random_state=0))
    assert len(res.x) == 1 and len(res.func_vals) == 11


def test_paired_datasets_through_the_drivers(em_pairs):
    """train_crappifier, test_metrics and predict_images take the host and the device paired dataset alike: same numbers."""
    from pssr2_amd.data import DevicePairedTileDataset, PairedArrayDataset
    from pssr2_amd.models import ResUNet
    from pssr2_amd.predict import predict_images, test_metrics
    from pssr2_amd.train import train_crappifier
    hr, lr = em_pairs[0][:8, :, :64, :64], em_pairs[1][:8, :, :16, :16]
    kw = dict(hr_res=64, lr_scale=4, val_split=0.25, rotation=False)
    sets = [DevicePairedTileDataset(hr, lr, **kw), PairedArrayDataset(hr, lr, **kw)]
    assert sets[0].val_idx == sets[1].val_idx == [6, 7]
    losses, metrics, preds = [], [], []
    for ds in sets:
        torch.manual_seed(0)
        random.seed(0)
        model = ResUNet(hidden=[8, 16], depth=1, scale=1)
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
        losses.append(train_crappifier(model, ds, 2, opt, epochs=2, device="cuda", log_frequency=1))
        torch.manual_seed(1)
        sr = ResUNet(hidden=[16, 32])
        metrics.append([test_metrics(sr, ds, device="cuda", norm=norm, avg=False) for norm in (True, False)])
        preds.append(predict_images(sr, ds, device="cuda", batch_size=2, norm=True, out_dir=None))
    assert len(losses[0][0]) == 6 and len(losses[0][1]) == 2 and np.all(np.isfinite(losses[0][0]))
    assert losses[0] == losses[1]
    assert metrics[0] == metrics[1] and metrics[0][0] != metrics[0][1]
    assert set(metrics[0][0]) == {"mse", "pixel", "psnr", "ssim"} and len(metrics[0][0]["mse"]) == 2
    assert list(preds[0]) == list(preds[1]) == ["image0", "image1"]         # predict_images names by position in val_idx, as upstream
    for k in preds[0]:
        assert preds[0][k].shape == (1, 64, 64) and np.array_equal(np.asarray(preds[0][k]), np.asarray(preds[1][k]))
