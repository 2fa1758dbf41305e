"""Write tests/golden/data_protocol.json: what every host dataset class of pssr2_amd/data.py answers, recorded from this package itself.

TEST INFRASTRUCTURE ONLY.  Unlike the other gen_golden tools this one needs no reference checkout: it characterises the package's own
behaviour at one commit, so that a refactor of data.py can be compared with the commit before it.  ``records()`` is also what
tests/test_data_protocol.py runs; the test compares its result with the committed file for equality.

Per case (``cases()``: every host class over the small inputs below, ``hr_res=16, lr_scale=4, overlap=4``, ``crappifier=None`` but for
one ``AdditiveGaussian`` case under ``np.random.seed(3)``) the record holds ``len``, ``val_idx``, ``repr``, every name, what the
constructor printed and warned (and whether the warning points at the caller's file), and for ``compact`` False and True: a SHA-256
over dtype, shape and bytes of every item -- visited under ``random.seed(7)`` in index order, then in one fixed permutation, then once
more with ``pp=True`` -- and a SHA-256 of ``random.getstate()`` after the three passes.  ``errors`` holds type and message of every
constructor and index error, with several faults at once where the order of the checks matters.  Folder names are replaced by ``{TMP}``.

Left out on purpose: ``ResourceWarning`` (whether a reader leaves its files to the garbage collector is not protocol), and for
``SlidingArrayDataset`` what its constructor prints, its ``repr`` and the text of its ``IndexError``.

    python tools/gen_golden_data_protocol.py
"""
from __future__ import annotations

import contextlib
import hashlib
import io
import json
import random
import sys
import tempfile
import warnings
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
OUT = ROOT / "tests" / "golden" / "data_protocol.json"

HR_RES, LR_SCALE, OVERLAP = 16, 4, 4
STACK_SHAPES = ((3, 20, 24), (5, 16, 16))
SHEET_SHAPES = ((4, 40, 36), (2, 33, 50))
COMMON = dict(hr_res=HR_RES, lr_scale=LR_SCALE)


def _noise(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def uniform_stacks():
    """uint8 [4, 3, 20, 24]: the one-array input."""
    return _noise(11, (4,) + STACK_SHAPES[0])


def ragged_stacks():
    """Four stacks, two of each shape: the list input (``n_frames=[3, 1]``: one slice per file)."""
    return [_noise(20 + i, STACK_SHAPES[i % 2]) for i in range(4)]


def paired_stacks():
    """uint8 HR [4, 3, 20, 24] and LR [4, 3, 5, 6]."""
    return uniform_stacks(), _noise(12, (4, 3, 5, 6))


def sheets():
    return [_noise(30 + i, s) for i, s in enumerate(SHEET_SHAPES)]


def lr_sheets():
    return [_noise(40 + i, (f, h // LR_SCALE, w // LR_SCALE)) for i, (f, h, w) in enumerate(SHEET_SHAPES)]


def write_tifs(folder, images, stem="im"):
    from PIL import Image
    folder.mkdir(parents=True, exist_ok=True)
    for i, st in enumerate(images):
        pages = [Image.fromarray(f) for f in st]
        pages[0].save(folder / f"{stem}{i:02d}.tif", save_all=True, append_images=pages[1:])
    return folder


def folders(tmp):
    """The folders of the file classes, written once per ``tmp``."""
    out = {"stacks": tmp / "stacks", "hr": tmp / "hr", "lr": tmp / "lr", "sheets": tmp / "sheets", "lr_sheets": tmp / "lr_sheets",
           "empty": tmp / "empty", "one": tmp / "one", "uneven": tmp / "uneven", "missing": tmp / "missing"}
    if not out["stacks"].exists():
        write_tifs(out["stacks"], ragged_stacks())
        hr, lr = paired_stacks()
        write_tifs(out["hr"], hr)
        write_tifs(out["lr"], lr)
        write_tifs(out["sheets"], sheets())
        write_tifs(out["lr_sheets"], lr_sheets())
        write_tifs(out["one"], sheets()[:1])
        write_tifs(out["uneven"], ragged_stacks())
        out["empty"].mkdir()
    return out


def cases(tmp):
    """name -> function that builds the dataset."""
    import pssr2_amd.data as D
    from pssr2_amd.crappifiers import AdditiveGaussian
    p = folders(tmp)
    split = dict(val_split=0.5, split_seed=0)
    sliding = dict(**COMMON, crappifier=None, overlap=OVERLAP, **split)
    pair_sliding = dict(**COMMON, overlap=OVERLAP, **split)
    return {
        "ArrayDataset/array": lambda: D.ArrayDataset(uniform_stacks(), **COMMON, crappifier=None, **split),
        "ArrayDataset/array_gaussian": lambda: D.ArrayDataset(uniform_stacks(), **COMMON, crappifier=AdditiveGaussian(13), **split),
        "ArrayDataset/array_lr": lambda: D.ArrayDataset(uniform_stacks(), hr_res=HR_RES, lr_scale=-1, crappifier=None, val_split=1),
        "ArrayDataset/ragged_f31": lambda: D.ArrayDataset(ragged_stacks(), **COMMON, crappifier=None, n_frames=[3, 1], **split),
        "ImageDataset/f31": lambda: D.ImageDataset(p["stacks"], **COMMON, crappifier=None, n_frames=[3, 1], **split),
        "PairedArrayDataset/all": lambda: D.PairedArrayDataset(*paired_stacks(), **COMMON, **split),
        "PairedArrayDataset/f31": lambda: D.PairedArrayDataset(*paired_stacks(), **COMMON, n_frames=[3, 1], **split),
        "PairedImageDataset/f13": lambda: D.PairedImageDataset(p["hr"], p["lr"], **COMMON, n_frames=[1, 3], **split),
        "SlidingArrayDataset": lambda: D.SlidingArrayDataset(sheets(), hr_res=HR_RES, overlap=OVERLAP),
        "SlidingSheetDataset/f2": lambda: D.SlidingSheetDataset(sheets(), **sliding, n_frames=2),
        "SlidingSheetDataset/f21_slide": lambda: D.SlidingSheetDataset(sheets(), **sliding, n_frames=[2, 1], slide=True),
        "SlidingSheetDataset/lr": lambda: D.SlidingSheetDataset(sheets(), hr_res=HR_RES, lr_scale=-1, crappifier=None, overlap=OVERLAP, val_split=1),
        "SlidingDataset/f21": lambda: D.SlidingDataset(p["sheets"], **sliding, n_frames=[2, 1]),
        "PairedSlidingArrayDataset/f2": lambda: D.PairedSlidingArrayDataset(sheets(), lr_sheets(), **pair_sliding, n_frames=2),
        "PairedSlidingArrayDataset/f12_slide": lambda: D.PairedSlidingArrayDataset(sheets(), lr_sheets(), **pair_sliding, n_frames=[1, 2], slide=True),
        "PairedSlidingDataset/f2": lambda: D.PairedSlidingDataset(p["sheets"], p["lr_sheets"], **pair_sliding, n_frames=2),
    }


def error_cases(tmp):
    """name -> function that must raise; where two faults are given at once the name says which check comes first."""
    import pssr2_amd.data as D
    p = folders(tmp)
    f32 = lambda a: np.asarray(a, dtype=np.float32)                                           # noqa: E731
    past = lambda make: (lambda: (lambda ds: ds[len(ds)])(make()))                            # noqa: E731
    c = cases(tmp)
    hr, lr = paired_stacks()
    return {
        "ArrayDataset/float": lambda: D.ArrayDataset(f32(uniform_stacks())),
        "ArrayDataset/ragged_float": lambda: D.ArrayDataset([f32(s) for s in ragged_stacks()]),
        "ArrayDataset/ragged_4d": lambda: D.ArrayDataset([ragged_stacks()[0][None], ragged_stacks()[1]]),
        "ArrayDataset/index": past(c["ArrayDataset/array"]),
        "ArrayDataset/ragged_index": past(c["ArrayDataset/ragged_f31"]),
        "ImageDataset/no_path": lambda: D.ImageDataset(p["missing"], extension="png", extra_path="x"),
        "ImageDataset/empty_path": lambda: D.ImageDataset(""),
        "ImageDataset/no_files_before_extra_path": lambda: D.ImageDataset(p["stacks"], extension="png", extra_path="x"),
        "ImageDataset/extra_path": lambda: D.ImageDataset(p["stacks"], extra_path="x"),
        "ImageDataset/index": past(c["ImageDataset/f31"]),
        "PairedArrayDataset/float": lambda: D.PairedArrayDataset(hr, f32(lr)),
        "PairedArrayDataset/5d": lambda: D.PairedArrayDataset(hr[None], lr),
        "PairedArrayDataset/mismatch": lambda: D.PairedArrayDataset(hr, lr[:3]),
        "PairedArrayDataset/index": past(c["PairedArrayDataset/all"]),
        "PairedImageDataset/no_hr_path": lambda: D.PairedImageDataset(p["missing"], p["lr"]),
        "PairedImageDataset/no_lr_path": lambda: D.PairedImageDataset(p["hr"], p["missing"], extension="png"),
        "PairedImageDataset/no_hr_files": lambda: D.PairedImageDataset(p["empty"], p["lr"]),
        "PairedImageDataset/no_lr_files": lambda: D.PairedImageDataset(p["hr"], p["empty"]),
        "PairedImageDataset/mismatch": lambda: D.PairedImageDataset(p["hr"], p["one"]),
        "PairedImageDataset/uneven": lambda: D.PairedImageDataset(p["uneven"], p["lr"]),
        "PairedImageDataset/index": past(c["PairedImageDataset/f13"]),
        "SlidingArrayDataset/index": past(c["SlidingArrayDataset"]),
        "SlidingSheetDataset/float": lambda: D.SlidingSheetDataset([f32(s) for s in sheets()], hr_res=16, overlap=16),
        "SlidingSheetDataset/4d": lambda: D.SlidingSheetDataset([s[None] for s in sheets()]),
        "SlidingSheetDataset/stride": lambda: D.SlidingSheetDataset(sheets(), hr_res=16, overlap=16),
        "SlidingSheetDataset/stride_none": lambda: D.SlidingSheetDataset(sheets(), hr_res=0, overlap=None),
        "SlidingSheetDataset/index": past(c["SlidingSheetDataset/f2"]),
        "SlidingDataset/no_path_before_czi": lambda: D.SlidingDataset(p["missing"], extension="czi"),
        "SlidingDataset/czi_before_files": lambda: D.SlidingDataset(p["empty"], extension="CZI", extra_path="x"),
        "SlidingDataset/no_files_before_extra_path": lambda: D.SlidingDataset(p["empty"], extra_path="x", hr_res=16, overlap=16),
        "SlidingDataset/extra_path_before_stride": lambda: D.SlidingDataset(p["sheets"], extra_path="x", hr_res=16, overlap=16),
        "SlidingDataset/stride": lambda: D.SlidingDataset(p["sheets"], hr_res=16, overlap=16),
        "SlidingDataset/index": past(c["SlidingDataset/f21"]),
        "PairedSlidingArrayDataset/float": lambda: D.PairedSlidingArrayDataset(sheets(), [f32(s) for s in lr_sheets()]),
        "PairedSlidingArrayDataset/mismatch_before_stride": lambda: D.PairedSlidingArrayDataset(sheets(), lr_sheets()[:1], hr_res=16, overlap=16),
        "PairedSlidingArrayDataset/stride": lambda: D.PairedSlidingArrayDataset(sheets(), lr_sheets(), hr_res=16, overlap=16),
        "PairedSlidingArrayDataset/index": past(c["PairedSlidingArrayDataset/f2"]),
        "PairedSlidingDataset/no_hr_path": lambda: D.PairedSlidingDataset(p["missing"], p["lr_sheets"], extension="czi"),
        "PairedSlidingDataset/no_lr_path_before_czi": lambda: D.PairedSlidingDataset(p["sheets"], p["missing"], extension="czi"),
        "PairedSlidingDataset/czi": lambda: D.PairedSlidingDataset(p["sheets"], p["lr_sheets"], extension="czi"),
        "PairedSlidingDataset/no_hr_files": lambda: D.PairedSlidingDataset(p["empty"], p["lr_sheets"]),
        "PairedSlidingDataset/no_lr_files": lambda: D.PairedSlidingDataset(p["sheets"], p["empty"]),
        "PairedSlidingDataset/mismatch_before_stride": lambda: D.PairedSlidingDataset(p["sheets"], p["one"], hr_res=16, overlap=16),
        "PairedSlidingDataset/stride": lambda: D.PairedSlidingDataset(p["sheets"], p["lr_sheets"], hr_res=16, overlap=16),
        "PairedSlidingDataset/index": past(c["PairedSlidingDataset/f2"]),
    }


def warning_cases(tmp):
    """name -> function whose construction warns."""
    import pssr2_amd.data as D
    p = folders(tmp)
    return {
        "PairedImageDataset/same_path": lambda: D.PairedImageDataset(p["hr"], p["hr"], **COMMON),
        "PairedSlidingDataset/same_path": lambda: D.PairedSlidingDataset(p["sheets"], str(p["sheets"]), **COMMON, overlap=OVERLAP),
        "SlidingSheetDataset/lr_split": lambda: D.SlidingSheetDataset(sheets(), hr_res=HR_RES, lr_scale=-1, crappifier=None, overlap=OVERLAP),
        "SlidingDataset/lr_split": lambda: D.SlidingDataset(p["sheets"], hr_res=HR_RES, lr_scale=-1, crappifier=None, overlap=OVERLAP),
    }


def item_digest(item):
    h = hashlib.sha256()
    for t in item if isinstance(item, (tuple, list)) else (item,):
        a = np.ascontiguousarray(t.detach().cpu().numpy())
        h.update(f"{a.dtype}{a.shape}".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def permutation(n):
    return random.Random(11).sample(range(n), n)


def visits(n):
    """(index, pp) of the three passes."""
    return [(i, False) for i in range(n)] + [(i, False) for i in permutation(n)] + [(i, True) for i in range(n)]


def get_item(ds, idx, pp):
    # SlidingArrayDataset's __getitem__ had no ``pp`` when the fixture was recorded; its items are validation items either way
    return ds.__getitem__(idx, pp=True) if pp and type(ds).__name__ != "SlidingArrayDataset" else ds[idx]


def state_digest():
    return hashlib.sha256(repr(random.getstate()).encode()).hexdigest()


def _construct(make, tmp):
    """(dataset, printed text, [(warning text, points at this file)])."""
    out = io.StringIO()
    with contextlib.redirect_stdout(out), warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        ds = make()
    return ds, out.getvalue(), [[str(w.message).replace(str(tmp), "{TMP}"), Path(w.filename).name == Path(__file__).name] for w in caught
                                  if not issubclass(w.category, ResourceWarning)]


def record(name, make, tmp):
    ds, printed, warned = _construct(make, tmp)
    rec = {"len": len(ds), "val_idx": [int(i) for i in ds.val_idx], "names": [ds._get_name(i) for i in range(len(ds))], "warnings": warned}
    if name != "SlidingArrayDataset":
        rec["printed"], rec["repr"] = printed, repr(ds).replace(str(tmp), "{TMP}")
    for compact in (False, True):
        ds = _construct(make, tmp)[0]
        ds.compact = compact
        np.random.seed(3)
        random.seed(7)
        rec[f"items_compact_{compact}"] = [item_digest(get_item(ds, i, pp)) for i, pp in visits(len(ds))]
        rec[f"random_state_compact_{compact}"] = state_digest()
    return rec


def record_error(name, make, tmp):
    try:
        _construct(make, tmp)
    except Exception as e:                                      # noqa: BLE001 -- the type is part of the record
        if name == "SlidingArrayDataset/index":
            return type(e).__name__
        return f"{type(e).__name__}: {e}".replace(str(tmp), "{TMP}")
    return None


def records(tmp):
    tmp = Path(tmp)
    return {"cases": {name: record(name, make, tmp) for name, make in cases(tmp).items()},
            "errors": {name: record_error(name, make, tmp) for name, make in error_cases(tmp).items()},
            "warnings": {name: _construct(make, tmp)[2] for name, make in warning_cases(tmp).items()}}


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        out = records(tmp)
    OUT.write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
    for name, rec in out["cases"].items():
        print(name, "len", rec["len"], "val", len(rec["val_idx"]))
    print("wrote", OUT.name, OUT.stat().st_size // 1024, "KiB")
    assert OUT.stat().st_size < 100 * 1024, OUT
