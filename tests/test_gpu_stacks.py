"""DeviceTileDataset over multi-frame tile stacks: items against the reference's recorded ones (tests/golden/stacks.npz) and the host
dataset, noise against the generator on host-cut slices and against the sheet dataset, and train_paired / predict_images /
preprocess_dataset over frame slices.  Everything here is bit-exact."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HR_RES, LR_SCALE = 32, 4
CONFIGS = {"f31": [3, 1], "f13": [1, 3], "f2": 2}
NAMES = ["im00", "im01", "im02", "im03"]


@pytest.fixture(scope="module")
def gold(golden):
    return golden("stacks.npz")


@pytest.fixture(scope="module")
def stacks(gold):
    return [gold[f"hr_in/{k}"] for k in range(4)]


@pytest.fixture(scope="module")
def deep():
    """Four (7, 32, 32) stacks: what a sheet dataset with hr_res 32 and no overlap cuts into the same items."""
    from pssr2_amd.data import synthetic_em_tile
    return [synthetic_em_tile(60 + k, 32, channels=7) for k in range(4)]


def _pair(host, dev, **kw):
    from pssr2_amd.data import ArrayDataset, DeviceTileDataset
    kw = dict(dict(hr_res=HR_RES, lr_scale=LR_SCALE, crappifier=None), **kw)
    return ArrayDataset(host, **kw), DeviceTileDataset(dev, **kw)


def _equal(dev, want):
    want = torch.as_tensor(np.asarray(want), dtype=torch.float32) if not torch.is_tensor(want) else want
    assert dev.dtype == torch.float32 and dev.is_cuda and dev.shape == want.shape
    assert torch.equal(dev.cpu(), want)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_device_items_equal_the_reference(gold, stacks, name):
    key = f"cfg/{name}"
    host, dev = _pair(stacks, stacks, names=NAMES, n_frames=CONFIGS[name], val_split=1)
    n = int(gold[f"{key}/len"])
    assert len(dev) == len(host) == n and dev.slices == host.slices == gold[f"{key}/slices"].tolist()
    for attr in ("val_idx", "crop_res", "is_lr", "hr_res", "lr_scale", "n_frames", "extra_hr_files"):
        assert getattr(dev, attr) == getattr(host, attr), attr
    assert [dev._get_name(i) for i in range(n)] == [host._get_name(i) for i in range(n)] == gold[f"{key}/names"].tolist()
    assert repr(dev).splitlines()[-1] == str(gold[f"{key}/repr"]).splitlines()[-1] and not hasattr(dev, "compact")
    assert isinstance(dev.images, list) and all(t.is_cuda and t.dtype == torch.uint8 for t in dev.images)
    rows = dev.draw_items(range(n))
    assert rows.shape == (n, 3) and rows.dtype == torch.int64 and rows.is_cuda
    hr, lr = dev.device_batch(rows)
    _equal(hr, np.stack([gold[f"{key}/hr/{i}"] for i in range(n)])), _equal(lr, np.stack([gold[f"{key}/lr/{i}"] for i in range(n)]))
    assert int(dev.tile_counter) == n
    for i in range(n):
        for a, b in (dev[i], dev.__getitem__(i, pp=True)):
            _equal(a, gold[f"{key}/hr/{i}"]), _equal(b, gold[f"{key}/lr/{i}"])
    with pytest.raises(IndexError, match=f"Tried to retrieve invalid image. Index {n} is not less than {n} total image frame slices."):
        dev[n]
    with pytest.raises(IndexError, match=f"Index {n} is not less than {n}"):
        dev.draw_items([0, n])
    with pytest.raises(IndexError):
        dev.draw_items([-1])                                # a row is an address: nothing before the first stack
    assert dev.draw_items([]).shape == (0, 3)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_device_rotation_draws_equal_the_reference(gold, stacks, name):
    cases = [(1, f"cfg/{name}/rot")] + ([(0, "cfg/f31/rot0")] if name == "f31" else [])
    for split_seed, key in cases:
        host, dev = _pair(stacks, stacks, n_frames=CONFIGS[name], val_split=0.25, split_seed=split_seed)
        idx = int(gold[f"{key}_idx"])
        assert dev.val_idx == host.val_idx and idx not in dev.val_idx
        order = [idx] + dev.val_idx + [idx]                 # two draws for each training index, none for a validation index
        for k, seed in enumerate(gold["draw_seeds"]):
            random.seed(int(seed))
            a, b = dev[idx]
            _equal(a, gold[f"{key}_hr"][k]), _equal(b, gold[f"{key}_lr"][k])
            assert random.random() == float(gold[f"{key}_state"][k])
            random.seed(int(seed))
            want = [host[i] for i in order]
            state = random.getstate()
            random.seed(int(seed))
            hr, lr = dev.device_batch(dev.draw_items(order))
            assert random.getstate() == state
            _equal(hr, torch.stack([w[0] for w in want])), _equal(lr, torch.stack([w[1] for w in want]))
            _equal(hr[0], gold[f"{key}_hr"][k])
        random.seed(3)
        state = random.getstate()
        hr, _ = dev.device_batch(dev.draw_items(order, pp=True))                # pp: no rotation, no draw
        assert random.getstate() == state
        _equal(hr[0], host.__getitem__(idx, pp=True)[0])


def test_device_lr_mode_equals_the_reference(gold, stacks):
    host, dev = _pair(stacks, stacks, hr_res=8, lr_scale=-1, n_frames=2, val_split=1)
    assert dev.is_lr and host.is_lr and len(dev) == len(host) == 6 and dev.lr_scale == 1
    _equal(dev.device_batch(dev.draw_items(range(6))), gold["lrmode/items"])
    for i in range(6):
        _equal(dev[i], gold["lrmode/items"][i])
    assert int(dev.tile_counter) == 0


def test_depths(gold, stacks):
    from pssr2_amd.data import DeviceTileDataset
    kw = dict(hr_res=HR_RES, lr_scale=LR_SCALE, crappifier=None, val_split=1)
    with pytest.raises(ValueError, match=r"DeviceTileDataset: n_frames=-1 needs stacks with the same number of frames \(a batch has one depth\); "
                                         r"found \[1, 2, 5, 7\]"):
        DeviceTileDataset(stacks, n_frames=-1, **kw)
    assert len(DeviceTileDataset(stacks, n_frames=[3, 1], **kw)) == 3          # (NotImplementedError before)
    cut = [s[:1] for s in stacks]                                               # a common depth: one item per file, sizes still differ
    host, dev = _pair(cut, cut, n_frames=-1, val_split=1)
    assert len(dev) == 4 and dev.depth == 1 and [dev._get_name(i) for i in range(4)] == [f"image{i}" for i in range(4)]
    hr, lr = dev.device_batch(dev.draw_items(range(4)))
    for i in range(4):
        _equal(hr[i], gold[f"cfg/all/hr/{i}"][:1]), _equal(lr[i], gold[f"cfg/all/lr/{i}"][:1])
        _equal(hr[i], host[i][0])
    # one shape: a single tensor in HBM, cut into slices all the same, also when it is already there
    one = np.stack([stacks[0][:, :24, :24], stacks[0][:, 4:28, 6:30]])
    for given in (one, torch.from_numpy(one).cuda()):
        host, dev = _pair(one, given, n_frames=[3, 1], val_split=1)
        assert torch.is_tensor(dev.images) and dev.images.shape == (2, 7, 24, 24) and len(dev) == 4 and dev._get_name(3) == "image1_1"
        hr, lr = dev.device_batch(dev.draw_items([3, 0, 2, 1]))
        for k, i in enumerate([3, 0, 2, 1]):
            _equal(hr[k], host[i][0]), _equal(lr[k], host[i][1])


def _host_cut(host, indices):
    """uint8 [b, m, hr_res, hr_res]: the host's frame slices after ``_gen_pair``'s crop / pad."""
    from pssr2_amd.data import _pad_image, _square_crop
    return torch.from_numpy(np.stack([_pad_image(_square_crop(host._slice(i), host.hr_res), host.hr_res) for i in indices])).cuda()


@pytest.mark.parametrize("name", ["f31", "f2"])
def test_crappified_batches_equal_the_generator_on_host_cut_slices(stacks, name):
    """HR exact; LR = DevicePairGenerator on the host-cut slices with the same seed and tile offset, then the centre frames."""
    from pssr2_amd.crappifiers import AdditiveGaussian
    from pssr2_amd.data import ArrayDataset, DevicePairGenerator, DeviceTileDataset, _slice_center
    nf = CONFIGS[name]
    host = ArrayDataset(stacks, hr_res=HR_RES, lr_scale=LR_SCALE, crappifier=None, n_frames=nf, rotation=False)
    dev = DeviceTileDataset(stacks, hr_res=HR_RES, lr_scale=LR_SCALE, crappifier=AdditiveGaussian(5, 0, 0), n_frames=nf, rotation=False, seed=7)
    gen = DevicePairGenerator(LR_SCALE, AdditiveGaussian(5, 0, 0), seed=7)
    offset, clean = 0, []
    for idx in ({"f31": [2, 0], "f2": [3, 0, 5, 1]}[name], {"f31": [1], "f2": [4, 2]}[name]):
        want_hr, want_lr = gen(_host_cut(host, idx), tile_offset=offset)
        if name == "f31":
            want_hr, want_lr = _slice_center(want_hr, 1), _slice_center(want_lr, 3)
        hr, lr = dev.device_batch(dev.draw_items(idx))
        assert hr.shape == want_hr.shape and lr.shape == want_lr.shape and torch.equal(hr, want_hr) and torch.equal(lr, want_lr)
        items = [host[i] for i in idx]
        assert torch.equal(hr.cpu(), torch.stack([a for a, _ in items]))
        clean.append(torch.equal(lr.cpu(), torch.stack([b for _, b in items])))
        offset += len(idx)
    assert not any(clean) and int(dev.tile_counter) == len(host)                # noise was added; the second batch drew from its own offset


def _sheet_twin(deep, **kw):
    from pssr2_amd.data import DeviceSlidingDataset, DeviceTileDataset
    tiles = DeviceTileDataset(deep, hr_res=HR_RES, lr_scale=LR_SCALE, **kw)
    sheets = DeviceSlidingDataset(deep, hr_res=HR_RES, lr_scale=LR_SCALE, overlap=0, slide=False, **kw)
    assert len(tiles) == len(sheets) and tiles.val_idx == sheets.val_idx and sheets.tiles == [1] * len(deep) and sheets.slices == tiles.slices
    return tiles, sheets


@pytest.mark.parametrize("nf", [[3, 1], 2])
def test_crappified_batches_equal_the_sheet_dataset(deep, nf):
    from pssr2_amd.crappifiers import AdditiveGaussian
    tiles, sheets = _sheet_twin(deep, crappifier=AdditiveGaussian(5, 0, 0), n_frames=nf, rotation=False, seed=7)
    n = len(tiles)
    assert n == 4 * (7 // max(nf if isinstance(nf, list) else [nf]))
    order = list(range(n))
    random.Random(2).shuffle(order)
    for idx in (order[:5], order[5:]):
        a, b = tiles.device_batch(tiles.draw_items(idx)), sheets.device_batch(sheets.draw_items(idx))
        assert a[0].shape == b[0].shape and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert int(tiles.tile_counter) == int(sheets.tile_counter) == n


def _train(ds, graph=True):
    from pssr2_amd import fastpath as FP
    from pssr2_amd.models import ResUNet
    from pssr2_amd.optim import FusedAdamW
    from pssr2_amd.train import train_paired
    if not graph:
        os.environ["PSSR_GRAPH"] = "0"
    try:
        torch.manual_seed(4)
        random.seed(9)
        model = ResUNet(channels=[3, 1], hidden=[16, 32]).cuda()
        assert bool(FP.supports(model, ds, "cuda")) == graph
        tl, vl = train_paired(model, ds, 2, torch.nn.MSELoss(), FusedAdamW(model.parameters(), lr=1e-3), epochs=2, device="cuda", log_frequency=1)
        stepper = getattr(model._engine, "last_train_stepper", None)
        if graph:
            assert stepper.dataset is ds and stepper.graph is not None and not stepper.eager_only and not stepper.host
        return tl, vl
    finally:
        os.environ.pop("PSSR_GRAPH", None)


@pytest.fixture(scope="module", params=["none", "gaussian"])
def trained(request, deep):
    """(losses over tile stacks, a factory of fresh twin datasets) per crappifier: the run the two comparisons below share."""
    from pssr2_amd.crappifiers import AdditiveGaussian

    def twins():
        cr = None if request.param == "none" else AdditiveGaussian(5, 0, 0)
        return _sheet_twin(deep, crappifier=cr, n_frames=[3, 1], val_split=0.25, split_seed=0, seed=3)
    tiles, _ = twins()
    assert len(tiles) == 8 and len(tiles.val_idx) == 2
    run = _train(tiles)
    print(f"train_paired over stacks ({request.param}): train {run[0]} val {run[1]}")
    assert len(run[0]) == 6 and len(run[1]) == 2 and all(np.isfinite(run[0])) and all(np.isfinite(run[1]))
    return run, twins


def test_train_paired_replay_equals_the_launch_by_launch_loop(trained):
    """The replayed run against the same run with PSSR_GRAPH=0, bit for bit: the same kernels with the same arguments, batches of frame
    slices and the optimizer's device-side step count included."""
    run, twins = trained
    eager = _train(twins()[0], graph=False)
    print(f"PSSR_GRAPH=0: train {eager[0]} val {eager[1]}")
    assert run == eager


def test_train_paired_over_stacks_equals_over_sheets(trained):
    run, twins = trained
    sheets = _train(twins()[1])
    print(f"over sheets: train {sheets[0]} val {sheets[1]}")
    assert run == sheets


def test_predict_images_over_lr_mode_slices(stacks):
    from pssr2_amd.data import DeviceTileDataset
    from pssr2_amd.models import ResUNet
    from pssr2_amd.predict import _pred_array, predict_images
    more = stacks + [np.ascontiguousarray(stacks[0][1:7, 2:, :]), stacks[1][:4]]
    ds = DeviceTileDataset(more, hr_res=8, lr_scale=-1, n_frames=[3, 1], val_split=1)
    assert ds.is_lr and ds.slices == [2, 1, 0, 0, 2, 1] and len(ds) == 6
    torch.manual_seed(6)
    model = ResUNet(channels=[3, 1], hidden=[16, 32]).cuda()
    got = predict_images(model, ds, device="cuda", batch_size=4, out_dir=None)                  # a full batch and a tail of two
    assert list(got) == ["image0_0", "image0_1", "image1_0", "image4_0", "image4_1", "image5_0"]
    model.eval()
    with torch.no_grad():
        for i, name in enumerate(got):
            item = ds[i]
            assert item.shape == (3, 8, 8)
            want = _pred_array(model(item[None]))[0]
            assert got[name].dtype == np.uint8 and got[name].shape == want.shape == (1, 32, 32) and np.array_equal(got[name], want), name


def test_preprocess_dataset_writes_the_host_files(stacks, tmp_path):
    from pssr2_amd.data import preprocess_dataset
    host, dev = _pair(stacks, stacks, names=NAMES, n_frames=2, val_split=0.25, split_seed=0)
    preprocess_dataset(host, preprocess_hr=True, out_dir=str(tmp_path / "host"))
    preprocess_dataset(dev, preprocess_hr=True, out_dir=str(tmp_path / "dev"), batch_size=4)    # a full batch and a tail of two
    for side in ("lr", "hr"):
        files = sorted(p.name for p in (tmp_path / "host" / side).iterdir())
        assert files == sorted(p.name for p in (tmp_path / "dev" / side).iterdir()) == sorted(f"{host._get_name(i)}.tif" for i in range(6))
        for f in files:
            assert (tmp_path / "dev" / side / f).read_bytes() == (tmp_path / "host" / side / f).read_bytes(), (side, f)
