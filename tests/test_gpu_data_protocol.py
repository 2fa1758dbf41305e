"""The four HBM-resident dataset classes against their host classes over the inputs of tools/gen_golden_data_protocol.py
(``crappifier=None``, ``rotation=True``, ``val_split=0.5``: training and validation items): items one by one and as one batch, the
``random`` stream they leave, names / ``len`` / ``val_idx`` / ``repr``, empty index lists, the host's index checks, no ``compact``."""
import importlib.util
import random
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("gen_golden_data_protocol", ROOT / "tools" / "gen_golden_data_protocol.py")
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def _case(tool, name):
    """(host dataset, device dataset, is it a paired class)."""
    import pssr2_amd.data as D
    split = dict(val_split=0.5, split_seed=0, rotation=True)
    tile, sheet = dict(**tool.COMMON, crappifier=None, **split), dict(**tool.COMMON, crappifier=None, overlap=tool.OVERLAP, **split)
    pair, pair_sheet = dict(**tool.COMMON, **split), dict(**tool.COMMON, overlap=tool.OVERLAP, **split)
    host, dev, args, kw = {
        "tile/ragged_f31": (D.ArrayDataset, D.DeviceTileDataset, (tool.ragged_stacks(),), dict(tile, n_frames=[3, 1])),
        "tile/array_all": (D.ArrayDataset, D.DeviceTileDataset, (tool.uniform_stacks(),), dict(tile, n_frames=-1)),
        "pair/all": (D.PairedArrayDataset, D.DevicePairedTileDataset, tool.paired_stacks(), dict(pair, n_frames=-1)),
        "pair/f31": (D.PairedArrayDataset, D.DevicePairedTileDataset, tool.paired_stacks(), dict(pair, n_frames=[3, 1])),
        "sheet/f2": (D.SlidingSheetDataset, D.DeviceSlidingDataset, (tool.sheets(),), dict(sheet, n_frames=2)),
        "sheet/f21_slide": (D.SlidingSheetDataset, D.DeviceSlidingDataset, (tool.sheets(),), dict(sheet, n_frames=[2, 1], slide=True)),
        "pair_sheet/f2": (D.PairedSlidingArrayDataset, D.DevicePairedSlidingDataset, (tool.sheets(), tool.lr_sheets()), dict(pair_sheet, n_frames=2)),
        "pair_sheet/f12_slide": (D.PairedSlidingArrayDataset, D.DevicePairedSlidingDataset, (tool.sheets(), tool.lr_sheets()),
                                 dict(pair_sheet, n_frames=[1, 2], slide=True)),
    }[name]
    return host(*args, **kw), dev(*args, **kw), name.startswith("pair")


CASES = ["tile/ragged_f31", "tile/array_all", "pair/all", "pair/f31", "sheet/f2", "sheet/f21_slide", "pair_sheet/f2", "pair_sheet/f12_slide"]


def _equal(got, want, dtype=torch.float32):
    assert got.is_cuda and got.dtype == dtype and got.shape == want.shape
    assert torch.equal(got.cpu().float(), want)


@pytest.mark.parametrize("name", CASES)
def test_device_class_equals_its_host_class(tool, name):
    host, dev, paired = _case(tool, name)
    n = len(host)
    order = list(range(n))
    assert len(dev) == n and dev.val_idx == host.val_idx and 0 < len(host.val_idx) < n
    assert [dev._get_name(i) for i in order] == [host._get_name(i) for i in order]
    assert repr(dev) == repr(host).replace(type(host).__name__, type(dev).__name__)
    assert getattr(dev, "compact", None) is None and host.compact is False
    assert type(host) in type(dev).__mro__

    random.seed(7)
    want = [host[i] for i in order]
    state = random.getstate()
    hr, lr = torch.stack([a for a, _ in want]), torch.stack([b for _, b in want])
    assert any(not torch.equal(a, host.__getitem__(i, pp=True)[0]) for i, (a, _) in enumerate(want))        # items were rotated

    random.seed(7)
    for i in order:
        a, b = dev[i]
        _equal(a, want[i][0]), _equal(b, want[i][1])
    assert random.getstate() == state

    random.seed(7)
    if paired:
        tables = dev.draw_pair_items(order)
        assert random.getstate() == state
        assert all(t.shape == (n, 3) and t.dtype == torch.int64 and t.is_cuda for t in tables)
        got, got_u8 = dev.device_pair_batch(tables), dev.device_pair_batch(tables, u8=True)
        _equal(got_u8[0], hr, torch.uint8), _equal(got_u8[1], lr, torch.uint8)
    else:
        rows = dev.draw_items(order)
        assert random.getstate() == state
        assert rows.shape == (n, 3) and rows.dtype == torch.int64 and rows.is_cuda
        got = dev.device_batch(rows)
    _equal(got[0], hr), _equal(got[1], lr)

    # empty orders and the host's index checks: no row of these ever reaches a kernel
    draw = dev.draw_pair_items if paired else dev.draw_items
    random.seed(7)
    state = random.getstate()
    if paired:
        empty = draw([])
        assert all(t.shape == (0, 3) and t.dtype == torch.int64 for t in empty)
        for u8 in (False, True):
            sides = dev.device_pair_batch(empty, u8=u8)
            assert [tuple(s.shape) for s in sides] == [(0,) + tuple(hr.shape[1:]), (0,) + tuple(lr.shape[1:])]
            assert all(s.dtype == torch.uint8 and s.is_cuda for s in sides)
    else:
        assert draw([]).shape == (0, 3) and draw([]).dtype == torch.int64
    message = f"Tried to retrieve invalid image. Index {n} is not less than {n} total image frame slices."
    with pytest.raises(IndexError, match=message):
        draw([0, n])
    with pytest.raises(IndexError, match=message):
        dev[n]
    with pytest.raises(IndexError):
        draw([-1])
    assert random.getstate() == state           # an index outside the dataset is refused before anything is drawn
    with pytest.raises(NotImplementedError, match=f"{type(dev).__name__} applies no host transforms"):
        type(dev)(*([tool.sheets()] * (2 if paired else 1)), transforms=[torch.nn.Identity()])


def test_sheet_windows_are_checked_on_the_host(tool):
    """``ValueError`` from the host's half of the bounds check, for a window the LR sheets are too small for."""
    import pssr2_amd.data as D
    small = [s[:, :5, :5] for s in tool.lr_sheets()]
    dev = D.DevicePairedSlidingDataset(tool.sheets(), small, **tool.COMMON, overlap=tool.OVERLAP, n_frames=2)
    with pytest.raises(ValueError, match="leaves sheet 0"):
        dev.draw_pair_items([len(dev) // 2 - 1])
    with pytest.raises(ValueError, match="same number of frames"):
        D.DeviceSlidingDataset(tool.sheets(), **tool.COMMON, overlap=tool.OVERLAP, n_frames=-1)
