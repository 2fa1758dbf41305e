"""pssr_gather_windows_u8 against numpy, the device sheet datasets against the host ones, and train_paired / the crappifier objective
over sheets against the same runs over pre-cut tiles.  Everything here is bit-exact."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HR_RES, OVERLAP, LR_SCALE = 32, 8, 4
ORIENTATIONS = [(rot, axis) for rot in (0, 1) for axis in (-1, 0, 1, 2, 3)]     # the reference draws six of them; axis 0 and "none" are the ABI's


@pytest.fixture(scope="module")
def gold(golden):
    return golden("sliding.npz")


@pytest.fixture(scope="module")
def sheets(gold):
    return [gold[f"hr_in/{k}"] for k in range(2)], [gold[f"lr_in/{k}"] for k in range(2)]


class _Bank:
    """Sheets as separate device allocations plus their pssr_sheet_desc table."""

    def __init__(self, arrays):
        from pssr2_amd import _lib as L
        self.arrays = arrays
        self.dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]
        descs = (L.SheetDesc * len(arrays))()
        for d, t, shape in zip(descs, self.dev, [a.shape for a in arrays]):
            d.base, (d.frames, d.h, d.w), d.reserved = t.data_ptr(), shape, 0
        assert C.sizeof(L.SheetDesc) == 24 and C.sizeof(L.WindowItem) == 24
        self.table = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).cuda()

    def gather(self, items, c, res):
        from pssr2_amd import _lib as L, ops
        rows = (L.WindowItem * len(items))(*[L.WindowItem(*it) for it in items])
        return ops.gather_windows_u8(self.table, len(self.arrays), torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8).cuda(), c, res).cpu().numpy()

    def expect(self, items, c, res):
        out = []
        for sheet, frame0, y0, x0, rot, axis in items:
            w = self.arrays[sheet][frame0:frame0 + c, y0:y0 + res, x0:x0 + res]
            w = np.rot90(w, axes=(1, 2)) if rot else w
            out.append(w if axis < 0 else np.flip(w, axis=(1, 2) if axis == 3 else axis))
        return np.stack(out)


def _check(bank, items, c, res):
    got, want = bank.gather(items, c, res), bank.expect(items, c, res)
    assert got.shape == want.shape == (len(items), c, res, res)
    bad = [it for it, a, b in zip(items, got, want) if not np.array_equal(a, b)]
    assert not bad, bad[:5]


@pytest.mark.parametrize("c", [1, 3])
def test_every_tile_in_every_orientation(sheets, c):
    """res 32, stride 24: x0 = 0 / 24 / 48 / 72 on pitches 90 and 121, so most rows are misaligned; c = 1 walks through the frames
    (non-zero frame0).  One launch holds the items of both sheets."""
    bank = _Bank(sheets[0])
    items = []
    for s, a in enumerate(sheets[0]):
        f, h, w = a.shape
        tiles = [(y, x) for y in range(0, h - 32 + 1, 24) for x in range(0, w - 32 + 1, 24)]
        assert len(tiles) == (9, 8)[s]
        for t, (y, x) in enumerate(tiles):
            items += [(s, (t + k) % (f - c + 1), y, x, rot, axis) for k, (rot, axis) in enumerate(ORIENTATIONS)]
    assert len(items) == 170 and any(it[1] for it in items)
    random.Random(0).shuffle(items)                         # the two sheets interleaved
    _check(bank, items, c, 32)


def test_scalar_instantiation(sheets):
    """res 20 is no multiple of 16: byte loads and stores."""
    bank = _Bank(sheets[0])
    items = [(s, f, y, x, rot, axis) for (s, f, y, x) in ((0, 0, 0, 0), (0, 4, 80, 70), (1, 1, 33, 101), (1, 2, 50, 7)) for rot, axis in ORIENTATIONS]
    _check(bank, items, 2, 20)


@pytest.mark.parametrize("c", [1, 2])
def test_block_remainder(c):
    """res 80: one full 64-block and a 16-wide remainder in each direction, on a (2, 100, 121) sheet."""
    sheet = np.random.default_rng(8).integers(0, 256, (2, 100, 121), dtype=np.uint8)
    bank = _Bank([sheet])
    items = [(0, 2 - c if y else 0, y, x, rot, axis) for (y, x) in ((0, 0), (20, 41), (7, 13)) for rot, axis in ORIENTATIONS]
    _check(bank, items, c, 80)


def test_misaligned_output_takes_the_scalar_path(sheets):
    from pssr2_amd import _lib as L
    bank = _Bank(sheets[0])
    items = [(1, 1, 24, 48, rot, axis) for rot, axis in ORIENTATIONS]
    rows = (L.WindowItem * len(items))(*[L.WindowItem(*it) for it in items])
    table = torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8).cuda()
    buf = torch.full((len(items) * 2 * 32 * 32 + 16,), 7, dtype=torch.uint8, device="cuda")
    L.check(L.lib().pssr_gather_windows_u8(L.ptr(bank.table), 2, L.ptr(table), len(items), C.c_void_p(buf.data_ptr() + 3), 2, 32, L.stream_ptr()),
            "pssr_gather_windows_u8")
    got = buf.cpu().numpy()
    assert np.array_equal(got[3:-13].reshape(len(items), 2, 32, 32), bank.expect(items, 2, 32))
    assert (got[:3] == 7).all() and (got[-13:] == 7).all()


def test_items_outside_their_sheet_are_zero_filled(sheets):
    """The kernel's guard, with tables that understate what is allocated, so that every address a failing guard would touch still lies
    inside an allocation: the descriptor covers frames 1..3 of the six of sheet 0, and the launch is told of one descriptor, the middle
    one of three."""
    from pssr2_amd import _lib as L
    backing = torch.from_numpy(sheets[0][0]).cuda()
    f, h, w = backing.shape
    descs = (L.SheetDesc * 3)(*[L.SheetDesc(backing.data_ptr() + h * w, 3, h, w, 0)] * 3)
    table = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).cuda()
    good = (0, 1, 20, 40, 1, 3)
    for res in (32, 20):
        # sheet index past / before the table, frame range past / before the sheet, window one row / column over each edge
        bad = [(1, 0, 0, 0, 0, -1), (-1, 0, 0, 0, 0, -1), (0, 2, 0, 0, 0, -1), (0, -1, 0, 0, 0, -1), (0, 0, h - res + 1, 0, 0, -1),
               (0, 0, 0, w - res + 1, 0, -1), (0, 1, -1, 0, 0, -1), (0, 1, 0, -1, 0, -1)]
        items = [good] + bad + [good]
        rows = (L.WindowItem * len(items))(*[L.WindowItem(*it) for it in items])
        rows = torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8).cuda()
        out = torch.full((len(items), 2, res, res), 9, dtype=torch.uint8, device="cuda")
        L.check(L.lib().pssr_gather_windows_u8(C.c_void_p(table.data_ptr() + 24), 1, L.ptr(rows), len(items), L.ptr(out), 2, res, L.stream_ptr()),
                "pssr_gather_windows_u8")
        got = out.cpu().numpy()
        want = np.flip(np.rot90(sheets[0][0][2:4, 20:20 + res, 40:40 + res], axes=(1, 2)), axis=(1, 2))
        assert np.array_equal(got[0], want) and np.array_equal(got[-1], want)
        assert not got[1:-1].any()


# --------------------------------------------------------------------------------------------- datasets
def _host_batch(ds, indices):
    items = [ds[i] for i in indices]
    if ds.is_lr:
        return torch.stack(items)
    return torch.stack([a for a, _ in items]), torch.stack([b for _, b in items])


def _equal(dev, host):
    assert dev.dtype == torch.float32 and dev.is_cuda and dev.shape == host.shape
    assert torch.equal(dev.cpu(), host)


@pytest.mark.parametrize("name", ["single", "slide31", "pairs2"])
def test_device_items_equal_host_items(sheets, name):
    from pssr2_amd.data import DeviceSlidingDataset, SlidingSheetDataset
    cfg = {"single": dict(n_frames=-1), "slide31": dict(n_frames=[3, 1], slide=True), "pairs2": dict(n_frames=2, slide=False)}[name]
    hr = [s[:1] for s in sheets[0]] if name == "single" else sheets[0]
    kw = dict(hr_res=HR_RES, lr_scale=LR_SCALE, crappifier=None, overlap=OVERLAP, rotation=False, **cfg)
    host, dev = SlidingSheetDataset(hr, **kw), DeviceSlidingDataset(hr, **kw)
    n = len(host)
    assert len(dev) == n == {"single": 17, "slide31": 52, "pairs2": 43}[name] and dev.val_idx == host.val_idx and dev.tiles == host.tiles
    assert [dev._get_name(i) for i in range(n)] == [host._get_name(i) for i in range(n)] and not hasattr(dev, "compact")
    rows = dev.draw_items(range(n))
    assert rows.shape == (n, 3) and rows.dtype == torch.int64 and rows.is_cuda
    want, got = _host_batch(host, range(n)), dev.device_batch(rows)
    _equal(got[0], want[0]), _equal(got[1], want[1])
    assert int(dev.tile_counter) == n
    for i in (0, n // 2, n - 1):                            # __getitem__ goes through the same two calls
        a, b = dev[i]
        _equal(a, want[0][i]), _equal(b, want[1][i])


def test_device_lr_mode_equals_host(sheets):
    from pssr2_amd.data import DeviceSlidingDataset, SlidingSheetDataset
    kw = dict(hr_res=HR_RES, lr_scale=-1, overlap=OVERLAP, n_frames=2, val_split=1)
    host, dev = SlidingSheetDataset(sheets[0], **kw), DeviceSlidingDataset(sheets[0], **kw)
    assert dev.is_lr and len(dev) == len(host) == 43
    _equal(dev.device_batch(dev.draw_items(range(43))), _host_batch(host, range(43)))
    _equal(dev[7], host[7])


def test_device_rotation_draws_equal_host_draws(sheets):
    """Training indices under one random.seed: the device dataset draws index by index in the host's order."""
    from pssr2_amd.data import DeviceSlidingDataset, SlidingSheetDataset
    kw = dict(hr_res=HR_RES, lr_scale=LR_SCALE, crappifier=None, overlap=OVERLAP, n_frames=[3, 1], slide=True, val_split=0.25, split_seed=0)
    host, dev = SlidingSheetDataset(sheets[0], **kw), DeviceSlidingDataset(sheets[0], **kw)
    idx = [i for i in range(len(host)) if i not in host.val_idx][:20] + host.val_idx[:4]
    random.seed(21)
    want = _host_batch(host, idx)
    random.seed(21)
    rows = dev.draw_items(idx)
    assert len(set(rows[:, 2].tolist())) > 1          # (rot, flip_axis) packed in the third int64: several orientations drawn
    got = dev.device_batch(rows)
    _equal(got[0], want[0]), _equal(got[1], want[1])


def test_host_validation(sheets):
    from pssr2_amd.data import DevicePairedSlidingDataset, DeviceSlidingDataset
    kw = dict(hr_res=HR_RES, lr_scale=LR_SCALE, crappifier=None, overlap=OVERLAP)
    dev = DeviceSlidingDataset(sheets[0], n_frames=2, **kw)
    with pytest.raises(IndexError, match="Tried to retrieve invalid image. Index 43 is not less than 43 total image frame slices."):
        dev.draw_items([0, 43])
    with pytest.raises(IndexError):
        dev[43]
    assert dev.draw_items([]).shape == (0, 3)
    with pytest.raises(ValueError, match="same number of frames"):
        DeviceSlidingDataset(sheets[0], n_frames=-1, **kw)
    with pytest.raises(NotImplementedError, match="transforms"):
        DeviceSlidingDataset(sheets[0], transforms=[torch.nn.Identity()], **kw)
    with pytest.raises(ValueError, match="leaves sheet 0"):
        dev.bank.check(0, 5, 0, 0, 2, 32)
    paired = DevicePairedSlidingDataset(*sheets, hr_res=HR_RES, lr_scale=LR_SCALE, overlap=OVERLAP, n_frames=2)
    with pytest.raises(IndexError):
        paired.draw_pair_items([43])
    # an LR folder that is too small for the windows the HR side counts: caught on the host, nothing is launched
    small = DevicePairedSlidingDataset(sheets[0], [s[:, :12, :12] for s in sheets[1]], hr_res=HR_RES, lr_scale=LR_SCALE, overlap=OVERLAP, n_frames=2)
    with pytest.raises(ValueError, match="leaves sheet 0"):
        small.draw_pair_items([8 * 3])


def test_crappified_batches_equal_the_generator_on_host_cut_windows(sheets):
    """HR exact; LR = DevicePairGenerator on the host-cut windows with the same seed and tile offset (the same kernels: bitwise)."""
    from pssr2_amd.crappifiers import AdditiveGaussian
    from pssr2_amd.data import DevicePairGenerator, DeviceSlidingDataset, SlidingSheetDataset
    kw = dict(hr_res=HR_RES, lr_scale=LR_SCALE, overlap=OVERLAP, n_frames=2, rotation=False)
    host = SlidingSheetDataset(sheets[0], crappifier=None, **kw)
    dev = DeviceSlidingDataset(sheets[0], crappifier=AdditiveGaussian(5, 0, 0), seed=7, **kw)
    gen = DevicePairGenerator(LR_SCALE, AdditiveGaussian(5, 0, 0), seed=7)
    offset, clean = 0, []
    for idx in ([3, 30, 12, 41, 0], [8, 9, 42]):
        windows = torch.from_numpy(np.stack([host._window(i) for i in idx])).cuda()
        want_hr, want_lr = gen(windows, tile_offset=offset)
        hr, lr = dev.device_batch(dev.draw_items(idx))
        assert torch.equal(hr, want_hr) and torch.equal(lr, want_lr)
        assert torch.equal(hr.cpu(), _host_batch(host, idx)[0])
        clean.append(torch.equal(lr.cpu(), _host_batch(host, idx)[1]))
        offset += len(idx)
    assert not any(clean) and int(dev.tile_counter) == 8            # noise was added, and the second batch drew from its own offset


def test_train_paired_replays_over_sheets_like_over_tiles():
    """Two 1 x 96 x 96 sheets, nine windows each, against a DeviceTileDataset of the same 18 windows pre-cut in dataset order."""
    from pssr2_amd import fastpath as FP
    from pssr2_amd.data import DeviceSlidingDataset, DeviceTileDataset, synthetic_em_tile
    from pssr2_amd.models import ResUNet
    from pssr2_amd.optim import FusedAdamW
    from pssr2_amd.train import train_paired
    sheet_arrays = [synthetic_em_tile(40 + k, 96) for k in range(2)]
    kw = dict(hr_res=32, lr_scale=4, crappifier=None, val_split=0.2, rotation=False, split_seed=0)
    over_sheets = DeviceSlidingDataset(sheet_arrays, overlap=0, **kw)
    assert over_sheets.tiles == [9, 9] and len(over_sheets.val_idx) == 3
    tiles = np.stack([s[:, y:y + 32, x:x + 32] for s in sheet_arrays for y in (0, 32, 64) for x in (0, 32, 64)])
    over_tiles = DeviceTileDataset(tiles, **kw)
    over_tiles.val_idx = list(over_sheets.val_idx)
    runs = []
    for ds in (over_sheets, over_tiles):
        torch.manual_seed(4)
        random.seed(9)
        model = ResUNet(hidden=[16, 32]).cuda()
        assert FP.supports(model, ds, "cuda")
        tl, vl = train_paired(model, ds, 2, torch.nn.MSELoss(), FusedAdamW(model.parameters(), lr=1e-3), epochs=2, device="cuda", log_frequency=1)
        stepper = model._engine.last_train_stepper
        assert stepper.dataset is ds and stepper.graph is not None and not stepper.eager_only and not stepper.host
        runs.append((tl, vl))
    assert len(runs[0][0]) == 16 and len(runs[0][1]) == 2 and all(np.isfinite(runs[0][0]))
    assert runs[0] == runs[1]


# --------------------------------------------------------------------------------------------- real pairs
def test_device_paired_items_equal_host_items(sheets):
    from pssr2_amd.data import DevicePairedSlidingDataset, PairedSlidingArrayDataset
    kw = dict(hr_res=HR_RES, lr_scale=LR_SCALE, overlap=OVERLAP, n_frames=[1, 3], slide=True)
    host, dev = PairedSlidingArrayDataset(*sheets, **kw), DevicePairedSlidingDataset(*sheets, **kw)
    assert len(dev) == len(host) == 52 and dev.val_idx == host.val_idx and repr(dev).splitlines()[-1] == repr(host).splitlines()[-1]
    want, got = _host_batch(host, range(52)), dev.device_pair_batch(dev.draw_pair_items(range(52)))
    assert got[0].shape == (52, 3, 32, 32) and got[1].shape == (52, 1, 8, 8)
    _equal(got[0], want[0]), _equal(got[1], want[1])
    a, b = dev[51]
    _equal(a, want[0][51]), _equal(b, want[1][51])
    u8 = dev.device_pair_batch(dev.draw_pair_items([4, 5]), u8=True)
    assert u8[0].dtype == torch.uint8 and torch.equal(u8[0].float(), got[0][4:6]) and torch.equal(u8[1].float(), got[1][4:6])
    host, dev = PairedSlidingArrayDataset(*sheets, val_split=0.25, **kw), DevicePairedSlidingDataset(*sheets, val_split=0.25, **kw)
    idx = [i for i in range(52) if i not in host.val_idx][:16]
    random.seed(33)
    want = _host_batch(host, idx)
    random.seed(33)
    got = dev.device_pair_batch(dev.draw_pair_items(idx))
    _equal(got[0], want[0]), _equal(got[1], want[1])


def test_objective_over_sheets_equals_objective_over_precut_pairs(sheets):
    from pssr2_amd import AdditiveGaussian
    from pssr2_amd.data import DevicePairedSlidingDataset, DevicePairedTileDataset, PairedSlidingArrayDataset
    from pssr2_amd.train import _Crappifier_Objective
    kw = dict(hr_res=HR_RES, lr_scale=LR_SCALE, overlap=OVERLAP, n_frames=2)
    host = PairedSlidingArrayDataset(*sheets, **kw)
    hr, lr = _host_batch(host, range(len(host)))
    over_tiles = DevicePairedTileDataset(hr.to(torch.uint8), lr.to(torch.uint8), HR_RES, LR_SCALE, n_frames=2)
    over_sheets = DevicePairedSlidingDataset(*sheets, **kw)
    values = []
    for ds in (over_sheets, over_tiles):
        obj = _Crappifier_Objective(AdditiveGaussian, ds, 8, device="cuda", seed=5)
        random.seed(17)
        values.append([obj.sample(p) for p in ([9.0, 2.0], [3.0, -1.0])])
    assert np.isfinite(values[0]).all() and values[0][0] != values[0][1]
    assert values[0] == values[1]
