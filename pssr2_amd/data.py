"""Datasets and pair generation with the reference's protocol (pssr/data.py).

Two ways to produce (HR, LR) training pairs from uint8 HR tiles:

* host path — ``_gen_pair`` exactly as the reference orders it (crop, reflect-pad, rot90/flip, Pillow
  BILINEAR reduction, crappifier on numpy, round-half-even + clip): used by ``ImageDataset`` /
  ``ArrayDataset.__getitem__`` so that DataLoader workers and user crappifier subclasses keep working;
* device path — ``DevicePairGenerator``: whole batches of uint8 HR tiles resident in HBM go through
  the HIP kernels (bit-exact Pillow reduction, Philox noise, fused round/clip), removing the
  ~1 ms/tile host stage that would otherwise cap multi-GPU training.

File decoding (tif/czi) is out of scope: ``ImageDataset`` reads what Pillow reads.

Image sheets (the reference's ``SlidingDataset`` / ``PairedSlidingDataset``) follow the same three steps: ``SlidingSheetDataset`` /
``PairedSlidingArrayDataset`` over sheets in memory, the file classes on top of them (Pillow, multi-page tifs included), and
``DeviceSlidingDataset`` / ``DevicePairedSlidingDataset`` with the sheets in HBM and the windows cut by ``pssr_gather_windows_u8``.
"""
from __future__ import annotations

import glob
import random
import warnings
from pathlib import Path

import numpy as np
import torch
from torch.utils.data import Dataset

from .crappifiers import Crappifier, Poisson
from .util import _force_list


# --------------------------------------------------------------------------------------- geometry
def _square_crop(image, max_res):
    h, w = image.shape[-2:]
    if [h, w] == [max_res] * 2:
        return image
    size = min(h, w, max_res)
    sx, sy = (h - size) // 2, (w - size) // 2
    return image[:, sx:sx + size, sy:sy + size]


def _pad_image(image, res):
    if image.shape[-1] < res:
        p = res - image.shape[-1]
        return np.stack([np.pad(ch, [[0, p], [0, p]], mode="reflect") for ch in image])
    return image


def _slice_center(image, n_frames):
    center, half = image.shape[-3] // 2, n_frames // 2
    if n_frames % 2 == 0:
        return image[..., center - half:center + half, :, :]
    return image[..., center - half:center + half + 1, :, :]


def _tensor_ready(image, transforms, compact=False):
    """float32 tensor of an image (pssr/data.py:497-505).  ``compact``: uint8 instead -- what the drivers of this package ask their own
    datasets for while they feed a captured graph from a DataLoader (every value here is an integer in [0, 255]: uint8 pixels, or the
    rounded and clipped crappifier output); the conversion to float32 then happens on the device, and the worker -> pin-memory thread ->
    PCIe path moves a quarter of the bytes."""
    if compact and transforms is None:
        u8 = np.ascontiguousarray(image).astype(np.uint8)
        if image.dtype == np.uint8 or np.array_equal(u8, image):        # (a crappifier that returned NaN / a value outside [0, 255]: float32 as always)
            return torch.from_numpy(u8)
    t = torch.tensor(np.ascontiguousarray(image).astype(np.float32), dtype=torch.float)
    if transforms is not None:
        for tr in transforms:
            t = tr(t)
    return t


def _resize_bilinear_u8(hr, lr_res):
    """Per-frame ``PIL.Image.resize(BILINEAR)`` (pssr/data.py:483)."""
    from PIL import Image
    return np.stack([np.asarray(Image.fromarray(ch).resize([lr_res] * 2, Image.Resampling.BILINEAR)) for ch in hr])


def _gen_pair(hr, hr_res, lr_scale, rotation, crappifier, transforms, n_frames, compact=False):
    """Training pair from one uint8 HR stack [C, H, W] (pssr/data.py:471-495)."""
    hr = _pad_image(_square_crop(hr, hr_res), hr_res)
    if rotation:
        hr = np.rot90(hr, axes=(1, 2)) if rotation[0] else hr
        hr = np.flip(hr, axis=rotation[1])
    lr = _resize_bilinear_u8(np.ascontiguousarray(hr), hr_res // lr_scale).astype(np.float32)
    if crappifier is not None:
        lr = crappifier.crappify(lr) if issubclass(type(crappifier), Crappifier) else crappifier(lr)
        lr = np.clip(lr.round(), 0, 255)
    if n_frames is not None and n_frames[0] != n_frames[1]:
        if not n_frames[1] > hr.shape[-3]:
            hr = _slice_center(hr, n_frames[1])
        if not n_frames[0] > lr.shape[-3]:
            lr = _slice_center(lr, n_frames[0])
    return _tensor_ready(hr, transforms, compact), _tensor_ready(lr, transforms, compact)


def _transform_pair(hr, lr, hr_res, lr_res, rotation, transforms, n_frames, compact=False):
    """Item of a real (HR, LR) pair (pssr/data.py:497-516): each side gets ``_gen_pair``'s geometry at its own resolution, one
    (rot90, flip) draw serves both, and no crappifier runs."""
    sides = []
    for image, res in ((hr, hr_res), (lr, lr_res)):
        image = _pad_image(_square_crop(image, res), res)
        if rotation:
            image = np.flip(np.rot90(image, axes=(1, 2)) if rotation[0] else image, axis=rotation[1])
        sides.append(image)
    hr, lr = sides
    if n_frames is not None and n_frames[0] != n_frames[1]:
        if not n_frames[1] > hr.shape[-3]:
            hr = _slice_center(hr, n_frames[1])
        if not n_frames[0] > lr.shape[-3]:
            lr = _slice_center(lr, n_frames[0])
    return _tensor_ready(hr, transforms, compact), _tensor_ready(lr, transforms, compact)


def _ready_lr(lr, lr_res, transforms, compact=False):
    return _tensor_ready(_pad_image(_square_crop(lr, lr_res), lr_res), transforms, compact)


def _n_tiles(image, size, stride):
    x, y = image.shape[-2:]
    return max(0, (x - size) // stride + 1), max(0, (y - size) // stride + 1)


def _sliding_tile(image, size, stride, tile_idx):
    _, ty = _n_tiles(image, size, stride)
    sx, sy = tile_idx // ty * stride, tile_idx % ty * stride
    return image[..., sx:sx + size, sy:sy + size]


def _get_n_frames(n_frames):
    if n_frames in [None, -1, [-1]]:
        return None
    n_frames = _force_list(n_frames)
    return n_frames * 2 if len(n_frames) == 1 else n_frames


def _get_val_idx(slices, split, seed, tiles=None):
    """Validation frame indices (pssr/data.py:708-730): numpy legacy shuffle under ``seed``."""
    if tiles is not None:
        slices = [s for s, t in zip(slices, tiles) for _ in range(t)]
    order = list(range(len(slices)))
    if seed is not None and split < 1:
        np.random.seed(seed)
        np.random.shuffle(order)
    chosen = set(order[-max(1, int(split * len(slices))):])
    val, pos = [], 0
    for i, s in enumerate(slices):
        if i in chosen:
            val.extend(range(pos, pos + s))
        pos += s
    return val


def _invert_idx(idx, idx_len):
    r = np.arange(idx_len)
    return r[np.logical_not(np.isin(r, idx))]


class _RandomIterIdx:
    """Sampler of pssr/data.py:737-752; ``rank``/``world`` shard the epoch for data-parallel runs and
    ``shuffle_seed`` makes the (otherwise unseeded) training shuffle identical on every rank."""

    def __init__(self, idx, seed=False, rank=0, world=1, shuffle_seed=None):
        self.idx, self.seed, self.rank, self.world, self.shuffle_seed = idx, seed, rank, world, shuffle_seed
        self.epoch = 0

    def __iter__(self):
        order = list(self.idx.copy()) if not isinstance(self.idx, list) else self.idx.copy()
        if self.seed:
            np.random.seed(0)
            np.random.shuffle(order)
        elif self.shuffle_seed is not None:
            random.Random(self.shuffle_seed + self.epoch).shuffle(order)
        else:
            random.shuffle(order)
        self.epoch += 1
        if self.world > 1:
            n = len(order) // self.world * self.world if len(order) >= self.world else len(order)
            order = order[:n][self.rank::self.world] if n >= self.world else order
        yield from order

    def __len__(self):
        n = len(self.idx)
        return n // self.world if self.world > 1 and n >= self.world else n


# --------------------------------------------------------------------------------------- datasets
def _tile_stacks(images, who, keep_tensors=False):
    """The stacks of a tile dataset: one uint8 array / tensor [N, C, H, W] (``[N, H, W]``: one frame each) as it came, or a sequence of uint8
    stacks [C_i, H_i, W_i] (2-D: one frame) of any depths and sizes -- stacked into one array when every shape agrees, else a list."""
    if torch.is_tensor(images):
        single = images if keep_tensors else images.cpu().numpy()
    elif isinstance(images, np.ndarray) and images.dtype != object:
        single = images
    else:
        stacks = [s if torch.is_tensor(s) and keep_tensors else (s.cpu().numpy() if torch.is_tensor(s) else np.asarray(s)) for s in images]
        if len(stacks) and len({tuple(s.shape) for s in stacks}) == 1:
            single = torch.stack(stacks) if torch.is_tensor(stacks[0]) else np.stack(stacks)
        else:
            stacks = [s[None] if s.ndim == 2 else s for s in stacks]
            if any(s.ndim != 3 or str(s.dtype).split(".")[-1] != "uint8" for s in stacks):
                raise ValueError(f"{who} expects uint8 images")
            return stacks
    if single.ndim == 3:
        single = single[:, None]
    if str(single.dtype).split(".")[-1] != "uint8":
        raise ValueError(f"{who} expects uint8 images")
    return single


def _stack_shapes(images):
    """(frames, H, W) per file of what ``_tile_stacks`` returned."""
    return [tuple(s.shape) for s in images] if isinstance(images, list) else [tuple(images.shape[1:])] * len(images)


def _stack_slices(shapes, n_frames):
    """Frame slices per file (pssr/data.py:70-74): 1 with ``n_frames=-1``, else ``frames // max(n_frames)`` -- none for a file that is too shallow."""
    return [1 if n_frames is None else s[0] // max(n_frames) for s in shapes]


def _max_extent(shapes):
    return max((max(s[-2:]) for s in shapes), default=0)


class ArrayDataset(Dataset):
    """In-memory HR stacks (uint8 [N, C, H, W], or a sequence of stacks [C_i, H_i, W_i] of differing depths and sizes) with the attribute
    protocol the drivers consume (``val_idx``, ``extra_hr_files``, ``crop_res``, ``lr_scale``, ``is_lr``, ``hr_res``, ``n_frames``,
    ``_get_name``).  With ``n_frames`` every stack is cut into ``frames // max(n_frames)`` consecutive frame slices, each one item
    (pssr/data.py:70-74, 100-110, 566-577, 649-660): item ``idx`` is slice ``k`` of file ``f``, ``(f, k) = _get_image_idx(idx, slices)``,
    frames ``[k * m, k * m + m)`` with ``m = max(n_frames)``, named ``{name}_{k}``; the validation split is taken over files.
    ``images`` stays the single array when every stack has one shape, else it is the list."""

    def __init__(self, images, hr_res=512, lr_scale=4, crappifier=Poisson(), val_split=0.1, rotation=True, split_seed=0,
                 transforms=None, names=None, n_frames=-1):
        self.images = _tile_stacks(images, "ArrayDataset")
        lr_scale = None if lr_scale == -1 else lr_scale
        self.n_frames = _get_n_frames(n_frames)
        shapes = _stack_shapes(self.images)
        self.slices = _stack_slices(shapes, self.n_frames)
        max_size = _max_extent(shapes)
        self.val_idx = _get_val_idx(self.slices, val_split, split_seed)
        self.crop_res = min(hr_res, max_size)
        self.is_lr = lr_scale is None or max_size <= hr_res // lr_scale
        self.hr_res, self.lr_scale = hr_res, lr_scale if lr_scale is not None else 1
        self.crappifier, self.rotation, self.transforms = crappifier, rotation, transforms
        self.extra_hr_files = None
        self.compact = False        # True while train_paired feeds a captured graph from this dataset: uint8 items (see _tensor_ready)
        self.names = names if names is not None else [f"image{i}" for i in range(len(self.images))]

    def __len__(self):
        return sum(self.slices)

    def _slice(self, idx):
        """Host stack [frames, H, W] of a dataset index: the whole file with ``n_frames=-1``, else ``max(n_frames)`` frames of it."""
        if self.n_frames is None:
            return self.images[idx]
        image_idx, k = _get_image_idx(idx, self.slices)
        m = max(self.n_frames)
        return self.images[image_idx][k * m:k * m + m]

    def __getitem__(self, idx, pp=False):
        if idx >= len(self):
            raise IndexError(f"Tried to retrieve invalid image. Index {idx} is not less than {len(self)} total image frame slices.")
        is_val = idx in self.val_idx or pp        # pp: preprocess_dataset's items are never rotated (pssr/data.py:103)
        rot = [bool(random.getrandbits(1)), random.choice((1, 2, (1, 2)))] if self.rotation and not is_val else False
        hr = self._slice(idx)
        if self.is_lr:
            return _ready_lr(hr, self.hr_res // self.lr_scale, self.transforms, getattr(self, "compact", False))
        return _gen_pair(hr, self.hr_res, self.lr_scale, rot, self.crappifier, self.transforms, self.n_frames, getattr(self, "compact", False))

    def _res_line(self):
        return f"low-res: {self.hr_res // self.lr_scale}" if self.is_lr else f"high-res: {self.hr_res}, low-res: {self.hr_res // self.lr_scale}"

    def __repr__(self):
        return f"{type(self).__name__} of {len(self.images)} images with {len(self)} total frame slices\n{self._res_line()}"

    def _get_name(self, idx):
        if self.n_frames is None:
            return self.names[idx]
        image_idx, k = _get_image_idx(idx, self.slices)
        return f"{self.names[image_idx]}_{k}"


class ImageDataset(ArrayDataset):
    """Folder of pre-tiled images (anything Pillow opens; every page of a multi-page tif is a frame), reference arguments
    (pssr/data.py:13).  Files may differ in size and depth: each is cropped / padded on its own, and with ``n_frames`` each is cut into
    its own ``frames // max(n_frames)`` frame slices (``n_frames=[5, 1]``: five LR frames in, the centre HR frame out), see
    :class:`ArrayDataset`.  ``crop_res`` and ``is_lr`` come from the largest extent over all files.  czi sheets and ``extra_path``
    (upstream's branch for it cannot run) are not built."""

    def __init__(self, path, hr_res=512, lr_scale=4, crappifier=Poisson(), n_frames=-1, extension="tif", val_split=0.1,
                 rotation=True, split_seed=0, extra_path=None, extra_scale=1, transforms=None):
        self.path = Path(path) if type(path) is str else path
        if not path or not self.path.exists():
            raise FileNotFoundError(f'Path "{self.path}" does not exist.')
        files = sorted(f.split(str(self.path), maxsplit=1)[-1].strip("/") for f in glob.glob(f"{self.path}/**/*.{extension}", recursive=True))
        if not files:
            raise FileNotFoundError(f'No .{extension} files exist in path "{self.path}".')
        if extra_path is not None:
            raise NotImplementedError("extra_path is not supported by pssr2_amd.ImageDataset")
        super().__init__(_read_sheets(self.path, files), hr_res, lr_scale, crappifier, val_split, rotation, split_seed, transforms,
                         [f.split(".")[0] for f in files], n_frames)
        self.hr_files = files

    def __repr__(self):
        return f'ImageDataset from path "{self.path}"\n{len(self.hr_files)} files with {len(self)} total frame slices\n{self._res_line()}'


def _paired_stacks(hr_images, lr_images, who, keep_tensors=False):
    out = []
    for images in (hr_images, lr_images):
        if not torch.is_tensor(images):
            images = np.asarray(images)
        elif not keep_tensors:
            images = images.cpu().numpy()
        if images.ndim == 3:
            images = images[:, None]
        if images.ndim != 4 or str(images.dtype).split(".")[-1] != "uint8":
            raise ValueError(f"{who} expects uint8 images [N, C, H, W]")
        out.append(images)
    if len(out[0]) != len(out[1]):
        raise ValueError(f"Mismatch between amounts of high-low-resolution images. Found {len(out[0])} high-resolution and "
                         f"{len(out[1])} low-resolution images.")
    return out


class PairedArrayDataset(Dataset):
    """Real (HR, LR) pairs in memory, uint8 [N, C, H, W] and [N, c, h, w]: the reference's ``PairedImageDataset`` (pssr/data.py:268-346)
    without the files -- its defaults (``val_split=1``: every item is a validation item; ``split_seed=None``: the last images), its
    attribute protocol and its item geometry (``_transform_pair``), for ``train_crappifier``, ``approximate_crappifier``,
    ``test_metrics`` and ``predict_images(norm=True)``.  Every pair is one item: with ``n_frames=[lr, hr]`` of different lengths the
    centre frames of the two stacks are taken, as ``_transform_pair`` does."""
    _keep_tensors = False

    def __init__(self, hr_images, lr_images, hr_res=512, lr_scale=4, n_frames=-1, val_split=1, rotation=True, split_seed=None,
                 transforms=None, names=None):
        self.hr_images, self.lr_images = _paired_stacks(hr_images, lr_images, type(self).__name__, self._keep_tensors)
        self.n_frames = _get_n_frames(n_frames)
        self.slices = [1] * len(self.hr_images)
        self.val_idx = _get_val_idx(self.slices, val_split, split_seed)
        self.is_lr = False
        self.crop_res = min(hr_res, max(self.hr_images.shape[-2:]))
        self.extra_hr_files = None
        self.hr_res, self.lr_scale, self.rotation, self.transforms = hr_res, lr_scale, rotation, transforms
        self.compact = False        # see ArrayDataset.compact
        self.names = list(names) if names is not None else [f"image{i}" for i in range(len(self.hr_images))]

    def __len__(self):
        return sum(self.slices)

    def _draw_rotation(self, idx, pp=False):
        if self.rotation and not (idx in self.val_idx or pp):
            return [bool(random.getrandbits(1)), random.choice((1, 2, (1, 2)))]      # the reference's draws, in its order
        return False

    def __getitem__(self, idx, pp=False):
        if idx >= len(self):
            raise IndexError(f"Tried to retrieve invalid image. Index {idx} is not less than {len(self)} total image frame slices.")
        return _transform_pair(self.hr_images[idx], self.lr_images[idx], self.hr_res, self.hr_res // self.lr_scale,
                               self._draw_rotation(idx, pp), self.transforms, self.n_frames, getattr(self, "compact", False))

    def __repr__(self):
        return (f"{type(self).__name__} of {len(self.hr_images)} paired images with {len(self)} total frame slices\n"
                f"high-res: {self.hr_res}, low-res: {self.hr_res // self.lr_scale}")

    def _get_name(self, idx):
        return self.names[idx] + ("_0" if self.n_frames is not None else "")


def _read_folder(path, files):
    from PIL import Image
    stacks = []
    for f in files:
        im = Image.open(Path(path, f))
        frames = []
        for k in range(getattr(im, "n_frames", 1)):
            im.seek(k)
            frames.append(np.asarray(im.convert("L"), dtype=np.uint8))
        stacks.append(np.stack(frames))
    if len({st.shape for st in stacks}) != 1:
        raise ValueError(f'pssr2_amd.PairedImageDataset needs equally sized images in "{path}"')
    return np.stack(stacks)


class PairedImageDataset(PairedArrayDataset):
    """Two folders of pre-tiled images (anything Pillow opens) holding the high- and low-resolution side of each pair in the same sorted
    order: reference arguments, errors and warning (pssr/data.py:268-346).  The files of a side must be equally sized; tif stacks
    sliced into several items per file and sheets are outside this build's scope."""

    def __init__(self, hr_path, lr_path, hr_res=512, lr_scale=4, n_frames=-1, extension="tif", val_split=1, rotation=True,
                 split_seed=None, transforms=None):
        self.hr_path = Path(hr_path) if type(hr_path) is str else hr_path
        self.lr_path = Path(lr_path) if type(lr_path) is str else lr_path
        for path in (self.hr_path, self.lr_path):
            if not path or not path.exists():
                raise FileNotFoundError(f'Path "{path}" does not exist.')
        if self.hr_path == self.lr_path:
            warnings.warn("hr_path is equal to lr_path! Consider using ImageDataset instead.", stacklevel=2)
        found = []
        for path in (self.hr_path, self.lr_path):
            files = sorted(f.split(str(path), maxsplit=1)[-1].strip("/") for f in glob.glob(f"{path}/**/*.{extension}", recursive=True))
            if not files:
                raise FileNotFoundError(f'No .{extension} files exist in path "{path}".')
            found.append(files)
        self.hr_files, self.lr_files = found
        if len(self.hr_files) != len(self.lr_files):
            raise FileNotFoundError(f"Mismatch between amounts of high-low-resolution images. Found {len(self.hr_files)} high-resolution "
                                    f"and {len(self.lr_files)} low-resolution images.")
        super().__init__(_read_folder(self.hr_path, self.hr_files), _read_folder(self.lr_path, self.lr_files), hr_res, lr_scale, n_frames,
                         val_split, rotation, split_seed, transforms, [f.split(".")[0] for f in self.lr_files])
        self.mode = "L"

    def __repr__(self):
        return (f'PairedImageDataset from paths "{self.hr_path}" and "{self.lr_path}"\n{len(self.hr_files)} paired files with {len(self)} '
                f"total frame slices\nhigh-res: {self.hr_res}, low-res: {self.hr_res // self.lr_scale}")


class SlidingArrayDataset(Dataset):
    """LR-mode sliding window over in-memory sheets (pssr/data.py:132-266 with ``lr_scale=-1``): tiles are
    row-major, ``stride = hr_res - overlap``, trailing remainders are dropped."""

    def __init__(self, sheets, hr_res=128, overlap=32, names=None, transforms=None):
        self.sheets = [np.asarray(s if np.asarray(s).ndim == 3 else np.asarray(s)[None]) for s in sheets]
        self.hr_res, self.lr_scale, self.stride = hr_res, 1, hr_res - overlap
        self.tiles = [int(np.prod(_n_tiles(s, hr_res, self.stride))) for s in self.sheets]
        self.val_idx = list(range(sum(self.tiles)))
        self.crop_res, self.is_lr, self.extra_hr_files, self.n_frames = hr_res, True, None, None
        self.names = names if names is not None else [f"sheet{i}" for i in range(len(self.sheets))]
        self.transforms = transforms
        self.compact = False        # see ArrayDataset.compact

    def __len__(self):
        return sum(self.tiles)

    def _locate(self, idx):
        for s, t in enumerate(self.tiles):
            if idx < t:
                return s, idx
            idx -= t
        raise IndexError(idx)

    def __getitem__(self, idx):
        s, t = self._locate(idx)
        return _tensor_ready(_sliding_tile(self.sheets[s], self.hr_res, self.stride, t), self.transforms, getattr(self, "compact", False))

    def _get_name(self, idx):
        s, t = self._locate(idx)
        return f"{self.names[s]}_{t}_0"


# --------------------------------------------------------------------------------------- sheets
def _get_image_idx(idx, slices, tiles=None):
    """(sheet, index inside the sheet) of a dataset index (pssr/data.py:697-706)."""
    tiles = [1] * len(slices) if tiles is None else tiles
    for image_idx, (s, t) in enumerate(zip(slices, tiles)):
        if idx < s * t:
            return image_idx, idx
        idx -= s * t
    return None


def _window_origin(sheet, size, stride, n_frames, n_slices, idx, slide):
    """(frame0, y0, x0) of the window ``_sliding_window`` cuts for the in-sheet index ``idx`` (pssr/data.py:629-660): tiles row-major,
    ``tile = idx // n_slices``; frame slice ``idx % n_slices``, times ``n_frames`` unless the stack is slid over."""
    _, ty = _n_tiles(sheet, size, stride)
    tile = idx // n_slices
    frame0 = 0 if n_frames is None else idx % n_slices * (1 if slide else n_frames)
    return frame0, tile // ty * stride, tile % ty * stride


def _sliding_window(sheet, size, stride, n_frames, n_slices, idx, slide):
    frame0, y0, x0 = _window_origin(sheet, size, stride, n_frames, n_slices, idx, slide)
    window = sheet[..., y0:y0 + size, x0:x0 + size]
    return window if n_frames is None else window[frame0:frame0 + n_frames]


def _sheet_list(sheets, who, keep_tensors=False):
    out = []
    for s in sheets:
        if not torch.is_tensor(s):
            s = np.asarray(s)
        elif not keep_tensors:
            s = s.cpu().numpy()
        if s.ndim == 2:
            s = s[None]
        if s.ndim != 3 or str(s.dtype).split(".")[-1] != "uint8":
            raise ValueError(f"{who} expects uint8 sheets [F, H, W]")
        out.append(s)
    return out


def _tiles_slices(sheets, size, stride, n_frames, slide):
    """Windows per sheet and frame slices per window (pssr/data.py:205-210)."""
    tiles, slices = [], []
    for s in sheets:
        tx, ty = _n_tiles(s, size, stride)
        tiles.append(tx * ty)
        slices.append(1 if n_frames is None else ((s.shape[0] - max(n_frames) + 1) if slide else (s.shape[0] // max(n_frames))))
    return tiles, slices


def _in_val(dataset, idx):
    # ``idx in dataset.val_idx`` as upstream, with the list hashed once per assignment / length change (see DeviceTileDataset._draw_rotation)
    key = (id(dataset.val_idx), len(dataset.val_idx))
    if key != getattr(dataset, "_val_key", None):
        dataset._val_set, dataset._val_key = set(dataset.val_idx), key
    return idx in dataset._val_set


def _check_stride(hr_res, overlap):
    overlap = 0 if overlap is None else overlap
    if not hr_res > overlap:
        raise ValueError(f"hr_res must be greater than overlap. Given values are {hr_res} and {overlap} respectively.")
    return hr_res - overlap


class SlidingSheetDataset(Dataset):
    """Training dataset over in-memory image sheets (uint8 [F, H, W] each, 2-D accepted, of any sizes): the reference's
    ``SlidingDataset`` (pssr/data.py:132-266) without the files.  Same arithmetic -- ``stride = hr_res - overlap``, whole windows only,
    row-major; per sheet ``tiles`` windows times ``slices`` frame slices (``frames - max(n_frames) + 1`` with ``slide``, else
    ``frames // max(n_frames)``); the validation split is taken over windows (``_get_val_idx(slices, split, seed, tiles)``); item
    ``idx`` of a sheet is window ``idx // slices``, frame slice ``idx % slices`` -- the same attribute protocol, names
    (``{name}_{window}_{slice}``), ``__getitem__(idx, pp=False)`` and LR mode (``lr_scale=-1``, ``hr_res`` = LR resolution)."""

    def __init__(self, sheets, hr_res=512, lr_scale=4, crappifier=Poisson(), overlap=128, n_frames=-1, slide=False, val_split=0.1,
                 rotation=True, split_seed=0, transforms=None, names=None):
        self.sheets = _sheet_list(sheets, type(self).__name__, getattr(self, "_keep_tensors", False))
        self.stride = _check_stride(hr_res, overlap)
        lr_scale = None if lr_scale == -1 else lr_scale
        self.n_frames, self.slide = _get_n_frames(n_frames), slide
        self.tiles, self.slices = _tiles_slices(self.sheets, hr_res, self.stride, self.n_frames, slide)
        self.val_idx = _get_val_idx(self.slices, val_split, split_seed, self.tiles)
        self.crop_res = hr_res
        self.is_lr = lr_scale is None
        if self.is_lr:
            print("LR mode is enabled, dataset will load only unmodified low-resolution images.")
            if val_split < 1:
                warnings.warn("val_split is less than 1, not all low-resolution images will be used in prediciton.", stacklevel=2)
        self.hr_res, self.lr_scale = hr_res, lr_scale if lr_scale is not None else 1
        self.crappifier, self.rotation, self.transforms = crappifier, rotation, transforms
        self.extra_hr_files = None
        self.compact = False        # see ArrayDataset.compact
        self.names = list(names) if names is not None else [f"sheet{i}" for i in range(len(self.sheets))]

    def __len__(self):
        return sum(t * s for t, s in zip(self.tiles, self.slices))

    def _check_idx(self, idx):
        if idx >= len(self):
            raise IndexError(f"Tried to retrieve invalid image. Index {idx} is not less than {len(self)} total image frame slices.")

    def _draw_rotation(self, idx, pp=False):
        if self.rotation and not (_in_val(self, idx) or pp):
            return [bool(random.getrandbits(1)), random.choice((1, 2, (1, 2)))]      # the reference's draws, in its order
        return False

    def _window(self, idx):
        """Host window [frames, hr_res, hr_res] of a dataset index, ``max(n_frames)`` frames deep."""
        image_idx, local = _get_image_idx(idx, self.slices, self.tiles)
        return _sliding_window(self.sheets[image_idx], self.hr_res, self.stride, max(self.n_frames) if self.n_frames is not None else None,
                               self.slices[image_idx], local, self.slide)

    def __getitem__(self, idx, pp=False):
        self._check_idx(idx)
        hr, rot, compact = self._window(idx), self._draw_rotation(idx, pp), getattr(self, "compact", False)
        if self.is_lr:
            return _ready_lr(hr, self.hr_res, self.transforms, compact)
        return _gen_pair(hr, self.hr_res, self.lr_scale, rot, self.crappifier, self.transforms, self.n_frames, compact)

    def _res_line(self):
        return f"low-res: {self.hr_res}" if self.is_lr else f"high-res: {self.hr_res}, low-res: {self.hr_res // self.lr_scale}"

    def __repr__(self):
        return f"{type(self).__name__} of {len(self.sheets)} sheets with {len(self)} total frame slices\n{self._res_line()}"

    def _get_name(self, idx):
        image_idx, local = _get_image_idx(idx, self.slices, self.tiles)
        return f"{self.names[image_idx]}_{local // self.slices[image_idx]}_{local % self.slices[image_idx]}"


def _sheet_files(path, extension):
    path = Path(path) if type(path) is str else path
    if not path or not path.exists():
        raise FileNotFoundError(f'Path "{path}" does not exist.')
    if extension.lower() == "czi":
        raise NotImplementedError("czi sheets are not supported by pssr2_amd (czifile is not a dependency): export them to tif")
    files = sorted(f.split(str(path), maxsplit=1)[-1].strip("/") for f in glob.glob(f"{path}/**/*.{extension}", recursive=True))
    if not files:
        raise FileNotFoundError(f'No .{extension} files exist in path "{path}".')
    return path, files


def _read_sheets(path, files):
    """Every file as a uint8 stack [F, H, W] through Pillow (multi-page tifs: one frame per page), sizes free."""
    from PIL import Image
    sheets = []
    for f in files:
        with Image.open(Path(path, f)) as im:
            frames = []
            for k in range(getattr(im, "n_frames", 1)):
                im.seek(k)
                frames.append(np.asarray(im.convert("L"), dtype=np.uint8))
        sheets.append(np.stack(frames))
    return sheets


class SlidingDataset(SlidingSheetDataset):
    """Folder of image sheets: reference arguments, errors and warning (pssr/data.py:132-266).  Files are read through Pillow
    (multi-page tifs included).  ``preload`` is accepted for compatibility: the sheets are held in host memory either way.  czi files
    (``extension="czi"``, with them ``stack``) and ``extra_path`` raise ``NotImplementedError``."""

    def __init__(self, path, hr_res=512, lr_scale=4, crappifier=Poisson(), overlap=128, n_frames=-1, slide=False, stack="TZ",
                 extension="tif", preload=True, val_split=0.1, rotation=True, split_seed=0, extra_path=None, extra_scale=1,
                 transforms=None):
        self.path, self.hr_files = _sheet_files(path, extension)
        if extra_path is not None:
            raise NotImplementedError("extra_path is not supported by pssr2_amd.SlidingDataset")
        self.stack, self.mode, self.preload, self.extra_path, self.extra_scale = stack.upper(), "L", preload, None, extra_scale
        _check_stride(hr_res, overlap)          # before any file is read, as upstream
        super().__init__(_read_sheets(self.path, self.hr_files), hr_res, lr_scale, crappifier, overlap, n_frames, slide, val_split, rotation,
                         split_seed, transforms, [f.split(".")[0] for f in self.hr_files])

    def __repr__(self):
        return f'SlidingDataset from path "{self.path}"\n{len(self.hr_files)} files with {len(self)} total frame slices\n{self._res_line()}'


class PairedSlidingArrayDataset(Dataset):
    """Real (HR, LR) sheet pairs in memory (uint8 [F, H, W] / [f, h, w] each): the reference's ``PairedSlidingDataset``
    (pssr/data.py:348-444) without the files -- its defaults (``val_split=1``, ``split_seed=None``), attribute protocol and item geometry
    (``_transform_pair``), for ``train_crappifier``, ``approximate_crappifier`` and ``test_metrics``.  Windows, slices and the split are
    counted on the HR sheets.  As upstream, the LR side runs its own sliding window with ``hr_res // lr_scale`` and
    ``stride // lr_scale`` and takes its windows-per-row from the LR sheet, not from the HR sheet; and with ``n_frames=[lr, hr]`` each
    side takes its own number of frames from the slice's first frame on."""

    def __init__(self, hr_sheets, lr_sheets, hr_res=512, lr_scale=4, overlap=128, n_frames=-1, slide=False, val_split=1, rotation=True,
                 split_seed=None, transforms=None, names=None):
        keep = getattr(self, "_keep_tensors", False)
        self.hr_sheets, self.lr_sheets = _sheet_list(hr_sheets, type(self).__name__, keep), _sheet_list(lr_sheets, type(self).__name__, keep)
        if len(self.hr_sheets) != len(self.lr_sheets):
            raise ValueError(f"Mismatch between amounts of high-low-resolution images. Found {len(self.hr_sheets)} high-resolution and "
                             f"{len(self.lr_sheets)} low-resolution images.")
        self.stride = _check_stride(hr_res, overlap)
        self.n_frames, self.slide = _get_n_frames(n_frames), slide
        self.tiles, self.slices = _tiles_slices(self.hr_sheets, hr_res, self.stride, self.n_frames, slide)
        self.val_idx = _get_val_idx(self.slices, val_split, split_seed, self.tiles)
        self.is_lr, self.crop_res, self.extra_hr_files = False, hr_res, None
        self.hr_res, self.lr_scale, self.rotation, self.transforms = hr_res, lr_scale, rotation, transforms
        self.compact = False        # see ArrayDataset.compact
        self.names = list(names) if names is not None else [f"sheet{i}" for i in range(len(self.hr_sheets))]

    __len__ = SlidingSheetDataset.__len__
    _check_idx = SlidingSheetDataset._check_idx
    _draw_rotation = SlidingSheetDataset._draw_rotation
    _get_name = SlidingSheetDataset._get_name

    def _side_args(self, idx):
        """Per side (HR, LR): (sheet, size, stride, frames, slices of the sheet, in-sheet index, slide) as ``_sliding_window`` takes them."""
        image_idx, local = _get_image_idx(idx, self.slices, self.tiles)
        nf = self.n_frames
        return ((self.hr_sheets[image_idx], self.hr_res, self.stride, nf[1] if nf is not None else None, self.slices[image_idx], local, self.slide),
                (self.lr_sheets[image_idx], self.hr_res // self.lr_scale, self.stride // self.lr_scale, nf[0] if nf is not None else None,
                 self.slices[image_idx], local, self.slide))

    def __getitem__(self, idx, pp=False):
        self._check_idx(idx)
        hr_args, lr_args = self._side_args(idx)
        return _transform_pair(_sliding_window(*hr_args), _sliding_window(*lr_args), self.hr_res, self.hr_res // self.lr_scale,
                               self._draw_rotation(idx, pp), self.transforms, self.n_frames, getattr(self, "compact", False))

    def __repr__(self):
        return (f"{type(self).__name__} of {len(self.hr_sheets)} paired sheets with {len(self)} total frame slices\n"
                f"high-res: {self.hr_res}, low-res: {self.hr_res // self.lr_scale}")


class PairedSlidingDataset(PairedSlidingArrayDataset):
    """Two folders of image sheets holding the high- and low-resolution side of each pair in the same sorted order: reference
    arguments, errors and warning (pssr/data.py:348-444); items are named after the LR files.  Files as in :class:`SlidingDataset`
    (Pillow; ``preload`` accepted, sheets held in host memory either way; czi raises ``NotImplementedError``)."""

    def __init__(self, hr_path, lr_path, hr_res=512, lr_scale=4, overlap=128, n_frames=-1, slide=False, stack="TZ", extension="tif",
                 preload=True, val_split=1, rotation=True, split_seed=None, transforms=None):
        for path in (hr_path, lr_path):
            path = Path(path) if type(path) is str else path
            if not path or not path.exists():
                raise FileNotFoundError(f'Path "{path}" does not exist.')
        if (Path(hr_path) if type(hr_path) is str else hr_path) == (Path(lr_path) if type(lr_path) is str else lr_path):
            warnings.warn("hr_path is equal to lr_path! Consider using SlidingDataset instead.", stacklevel=2)
        (self.hr_path, self.hr_files), (self.lr_path, self.lr_files) = _sheet_files(hr_path, extension), _sheet_files(lr_path, extension)
        if len(self.hr_files) != len(self.lr_files):
            raise FileNotFoundError(f"Mismatch between amounts of high-low-resolution images. Found {len(self.hr_files)} high-resolution "
                                    f"and {len(self.lr_files)} low-resolution images.")
        self.stack, self.mode, self.preload = stack.upper(), "L", preload
        _check_stride(hr_res, overlap)
        super().__init__(_read_sheets(self.hr_path, self.hr_files), _read_sheets(self.lr_path, self.lr_files), hr_res, lr_scale, overlap,
                         n_frames, slide, val_split, rotation, split_seed, transforms, [f.split(".")[0] for f in self.lr_files])

    def __repr__(self):
        return (f'PairedSlidingDataset from paths "{self.hr_path}" and "{self.lr_path}"\n{len(self.hr_files)} paired files with {len(self)} '
                f"total frame slices\nhigh-res: {self.hr_res}, low-res: {self.hr_res // self.lr_scale}")


def _save_stack(path, stack):
    """uint8 [C, H, W] as a tif with one page per frame through Pillow, as ``predict_images`` writes its outputs."""
    from PIL import Image
    frames = [Image.fromarray(f) for f in np.ascontiguousarray(stack)]
    frames[0].save(path, save_all=len(frames) > 1, append_images=frames[1:])


def preprocess_dataset(dataset: Dataset, preprocess_hr: bool = False, out_dir: str = "preprocess", *, batch_size: int = 64):
    r"""Saves the processed frame slices of a dataset -- cropping / padding and crappification as its arguments specify, rotation
    disabled -- to ``{out_dir}/lr/{name}.tif`` and, with ``preprocess_hr``, ``{out_dir}/hr/{name}.tif`` for every index
    (pssr/data.py:446-467: same arguments and file names; multi-page tifs through Pillow instead of tifffile).

    Host datasets go item by item through ``dataset.__getitem__(idx, pp=True)``, as upstream.  Datasets that make their batches on the
    MI355X (``draw_items`` + ``device_batch``, or ``draw_pair_items`` + ``device_pair_batch``) go ``batch_size`` items at a time: one
    draw with ``pp=True``, the batch method, ``pssr_clip_u8`` (exact: these classes apply no transforms, every value is an integer in
    [0, 255]) and one device-to-host copy per batch and side; their Philox tile counter advances as for any other batch.  An LR-mode
    dataset has no pairs and raises ``ValueError`` (upstream fails there while unpacking the item)."""
    import os
    if getattr(dataset, "is_lr", False):
        raise ValueError("Dataset must be paired with high-low-resolution images for preprocessing: an LR-mode dataset has no pairs.")
    if batch_size < 1:
        raise ValueError(f"batch_size must be positive, got {batch_size}")
    os.makedirs(f"{out_dir}/lr", exist_ok=True)
    if preprocess_hr:
        os.makedirs(f"{out_dir}/hr", exist_ok=True)

    def save(idx, hr, lr):
        name = dataset._get_name(idx)
        _save_stack(f"{out_dir}/lr/{name}.tif", lr)
        if preprocess_hr:
            _save_stack(f"{out_dir}/hr/{name}.tif", hr)

    if hasattr(dataset, "draw_items") and hasattr(dataset, "device_batch"):
        draw, batch = dataset.draw_items, dataset.device_batch
    elif hasattr(dataset, "draw_pair_items") and hasattr(dataset, "device_pair_batch"):
        draw, batch = dataset.draw_pair_items, dataset.device_pair_batch
    else:
        for idx in range(len(dataset)):
            hr, lr = dataset.__getitem__(idx, pp=True)
            save(idx, np.asarray(hr, dtype=np.uint8) if preprocess_hr else None, np.asarray(lr, dtype=np.uint8))
        return

    from . import ops

    def to_host(x):
        x = x.contiguous().float()
        out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
        ops.clip_u8(x, out)
        return out.cpu().numpy()

    for first in range(0, len(dataset), batch_size):
        indices = list(range(first, min(first + batch_size, len(dataset))))
        hr, lr = batch(draw(indices, pp=True))
        hr, lr = to_host(hr) if preprocess_hr else None, to_host(lr)
        for k, idx in enumerate(indices):
            save(idx, hr[k] if preprocess_hr else None, lr[k])


def synthetic_em_tile(index, res=512, channels=1):
    """Seeded synthetic EM-like uint8 tile: band-limited noise + white noise."""
    rng = np.random.default_rng(1234 + index)
    out = []
    for _ in range(channels):
        white = rng.standard_normal((res, res))
        f = np.fft.rfft2(white)
        ky, kx = np.fft.fftfreq(res)[:, None], np.fft.rfftfreq(res)[None, :]
        smooth = np.fft.irfft2(f * np.exp(-2 * (np.pi * 3.0) ** 2 * (kx ** 2 + ky ** 2)), s=(res, res))
        smooth /= smooth.std() + 1e-12
        out.append(np.clip(128 + 48 * smooth + 8 * rng.standard_normal((res, res)), 0, 255).astype(np.uint8))
    return np.stack(out)


# --------------------------------------------------------------------------------------- device path
class DevicePairGenerator:
    """(HR, LR) batches from uint8 HR tiles already resident in HBM, entirely with HIP kernels."""

    def __init__(self, lr_scale=4, crappifier=Poisson(), seed=0, tile_counter=None):
        self.lr_scale, self.crappifier, self.seed = lr_scale, crappifier, seed
        self.tile_counter = tile_counter      # optional device uint64 added to tile_offset in-kernel (hipGraph replay)

    def _stage(self, x, spec, seed, tile_offset, flags):
        from . import ops
        kind, intensity, gain, spread = spec
        if kind == "gaussian":
            return ops.crappify_gaussian(x, intensity, gain, spread, seed, tile_offset, flags, tile_counter=self.tile_counter)
        if kind == "poisson":
            return ops.crappify_poisson(x, intensity, gain, spread, seed, tile_offset, flags, tile_counter=self.tile_counter)
        if kind == "blur":
            if spread > 0:      # per-tile sigma from the tile's Philox stream
                return ops.gaussian_blur_tiles(x, intensity, spread, gain, seed, tile_offset, flags, tile_counter=self.tile_counter)
            return ops.gaussian_blur(x, intensity, gain, flags)
        if kind == "saltpepper":
            return ops.crappify_saltpepper(x, intensity, gain, spread, seed, tile_offset, flags, tile_counter=self.tile_counter)
        raise NotImplementedError(kind)

    def __call__(self, hr_u8: torch.Tensor, tile_offset: int = 0):
        """hr_u8: uint8 [B, C, H, W] on the device.  Returns float32 (hr, lr) like ``_gen_pair``."""
        from . import ops
        if not hr_u8.is_cuda or hr_u8.dtype != torch.uint8:
            raise RuntimeError("DevicePairGenerator needs a uint8 tensor on the MI355X")
        hr_u8 = hr_u8.contiguous()
        b, c, h, w = hr_u8.shape
        lr = ops.u8_to_f32(ops.bilinear_down_u8(hr_u8, h // self.lr_scale, w // self.lr_scale))
        cr = self.crappifier
        if cr is not None:
            spec = cr.device_spec()
            if isinstance(spec, list):
                clip = ops.CLIP if spec[0][0] == "clip" else 0
                stages = spec[1:]
                for i, st in enumerate(stages):
                    last = i == len(stages) - 1
                    lr = self._stage(lr, st, self.seed + 7919 * i, tile_offset, ops.ROUND_CLIP if last and clip else (clip if not last else 0))
                if not clip:
                    lr = self._stage(lr, ("gaussian", 0.0, 0.0, 0.0), 0, 0, ops.ROUND_CLIP)
            else:
                lr = self._stage(lr, spec, self.seed, tile_offset, ops.ROUND_CLIP)
        return ops.u8_to_f32(hr_u8), lr

    def from_stacks(self, stacks, hr_res, rotations=None, tile_offset: int = 0):
        """On-device ``_gen_pair`` (pssr/data.py:471-495) for a batch of uint8 stacks [C, H, W] resident in HBM: centred
        crop / reflect pad to ``hr_res``, rot90 / flip with the (host-drawn, reference-order) ``rotations``, then the
        Pillow-exact reduction and the crappifier.  Returns float32 (hr, lr)."""
        from . import ops
        rotations = [False] * len(stacks) if rotations is None else rotations
        return self(ops.gen_pair_geometry_u8(stacks, rotations, hr_res), tile_offset)


def _gather_rows(entries, device):
    """int64 [n, 3] device rows (= n ``pssr_gather_item``) from (src address, sh, sw, ``False`` / ``[rot, axis]`` draw) entries."""
    import struct
    buf = bytearray()
    for src, h, w, rot in entries:
        axis = -1
        if rot:
            axis = 3 if isinstance(rot[1], (tuple, list)) else int(rot[1])
        buf += struct.pack("<Qiiii", src, h, w, int(bool(rot and rot[0])), axis)
    if not buf:                        # an empty order (val_split = 0, a rank without validation items): torch.frombuffer rejects b""
        return torch.zeros(0, 3, dtype=torch.int64, device=device)
    return torch.frombuffer(buf, dtype=torch.int64).view(-1, 3).to(device)


def _gather_table(images, indices, rotations):
    """int64 [n, 3] device rows (= n ``pssr_gather_item``) that point at ``images[i]`` with the given ``False`` / ``[rot, axis]`` draws."""
    c, h, w = images.shape[1:]
    base, stride = images.data_ptr(), c * h * w
    return _gather_rows([(base + int(i) * stride, h, w, rot) for i, rot in zip(indices, rotations)], images.device)


class DeviceTileDataset(Dataset):
    """``ArrayDataset`` whose uint8 HR stacks live in HBM: same constructor arguments, same attribute protocol
    (``val_idx``, ``extra_hr_files``, ``crop_res``, ``lr_scale``, ``is_lr``, ``hr_res``, ``n_frames``, ``_get_name``) and the same
    ``__getitem__`` contract (float32 CHW tensors, here already on the device), so ``train_paired`` / ``predict_images`` /
    ``test_metrics`` take it like any dataset.  In addition it can produce whole batches without touching the host
    (``draw_items`` + ``device_batch``): ``_gen_pair``'s crop / reflect pad / rot90 / flip (host-drawn in the reference's order,
    applied by one gather kernel), the Pillow-exact reduction and the crappifier (device Philox streams) as HIP launches whose
    only per-step inputs are device tensors -- which is what lets ``train_paired`` replay a whole training step as one hipGraph
    (pssr2_amd/fastpath.py).  Noise comes from the device generator: statistically, not bitwise, the numpy stream of the host path.

    Stacks of differing depths and sizes (a sequence of [C_i, H_i, W_i]) each stay their own tensor in HBM.  With ``n_frames`` an item is
    a frame slice of its file exactly as in ``ArrayDataset`` -- for the gather kernel that is an address (``k * m * H_i * W_i`` bytes into
    the stack) and the file's own size, so a batch mixes slices of files of any sizes; with ``n_frames=[lr, hr]`` the centre frames of
    each side are taken after the generator, as ``_gen_pair`` does.  ``n_frames=-1`` needs one depth over all files (a batch has one)."""

    def __init__(self, images, hr_res=512, lr_scale=4, crappifier=Poisson(), val_split=0.1, rotation=True, split_seed=0,
                 transforms=None, names=None, n_frames=-1, device="cuda", seed=0):
        if transforms is not None:
            raise NotImplementedError("DeviceTileDataset applies no host transforms")
        images = _tile_stacks(images, "DeviceTileDataset", keep_tensors=True)
        if isinstance(images, list):
            self.images = [torch.as_tensor(s).to(device).contiguous() for s in images]
        else:
            self.images = torch.as_tensor(images).to(device).contiguous()
        lr_scale = None if lr_scale == -1 else lr_scale
        self.n_frames = _get_n_frames(n_frames)
        shapes = _stack_shapes(self.images)
        self.slices = _stack_slices(shapes, self.n_frames)
        self.depth = max(self.n_frames) if self.n_frames is not None else _uniform_frames(shapes, "DeviceTileDataset", "stacks")
        max_size = _max_extent(shapes)
        self.val_idx = _get_val_idx(self.slices, val_split, split_seed)
        self.crop_res = min(hr_res, max_size)
        self.is_lr = lr_scale is None or max_size <= hr_res // lr_scale
        self.hr_res, self.lr_scale = hr_res, lr_scale if lr_scale is not None else 1
        self.crappifier, self.rotation, self.transforms = crappifier, rotation, None
        self.extra_hr_files = None
        self.names = names if names is not None else [f"image{i}" for i in range(len(self.images))]
        self._val_set, self._val_key = set(self.val_idx), None
        self.device = self.images[0].device if isinstance(self.images, list) else self.images.device
        self.tile_counter = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.gen = DevicePairGenerator(self.lr_scale, crappifier, seed=seed, tile_counter=self.tile_counter)
        self._item_bytes = 24             # struct pssr_gather_item {src, sh, sw, rot, flip_axis}
        # per dataset index (file, slice k, address of the slice's first frame, the file's H, W), in _get_image_idx's order: every read of
        # the gather kernel, depth frames of H x W bytes from that address, lies inside the file's stack since (k + 1) * depth <= frames
        if isinstance(self.images, list):
            bases = [s.data_ptr() for s in self.images]
        else:
            bases = [self.images.data_ptr() + f * self.images[0].numel() for f in range(len(self.images))]
        self._where = [(f, k, base + k * self.depth * h * w, h, w)
                       for f, (base, (_, h, w), n) in enumerate(zip(bases, shapes, self.slices)) for k in range(n)]

    def __len__(self):
        return len(self._where)

    def _get_name(self, idx):
        if self.n_frames is None:
            return self.names[idx]
        f, k = self._where[idx][:2]
        return f"{self.names[f]}_{k}"

    def _res_line(self):
        return f"low-res: {self.hr_res // self.lr_scale}" if self.is_lr else f"high-res: {self.hr_res}, low-res: {self.hr_res // self.lr_scale}"

    def __repr__(self):
        return f"{type(self).__name__} of {len(self.images)} images with {len(self)} total frame slices\n{self._res_line()}"

    def _draw_rotation(self, idx, pp=False):
        # ``idx in self.val_idx`` as upstream (pssr/data.py:103), with the list hashed once per assignment / length change: users enlarge
        # val_idx after training to predict every image
        key = (id(self.val_idx), len(self.val_idx))
        if key != self._val_key:
            self._val_set, self._val_key = set(self.val_idx), key
        if self.rotation and not (idx in self._val_set or pp):
            return [bool(random.getrandbits(1)), random.choice((1, 2, (1, 2)))]      # the reference's draws, in its order
        return False

    def draw_items(self, indices, pp=False):
        """Gather table (int64 [n, 3] on the device = n ``pssr_gather_item``) for these dataset indices, drawing the training
        rotations exactly as ``__getitem__`` would for the same sequence of indices (none with ``pp``).  An index outside the dataset
        raises ``IndexError`` before anything is drawn: a row is an address the kernel reads from."""
        indices = [int(i) for i in indices]
        for i in indices:
            if not 0 <= i < len(self):
                raise IndexError(f"Tried to retrieve invalid image. Index {i} is not less than {len(self)} total image frame slices.")
        return _gather_rows([self._where[i][2:] + (self._draw_rotation(i, pp),) for i in indices], self.device)

    def device_batch(self, items):
        """items: int64 [b, 3] device rows of ``draw_items``.  Returns float32 (hr, lr) on the device, or lr alone in LR mode.  No
        host synchronisation, no host-side data: capturable in a hipGraph (the Philox tile counter advances on the device)."""
        from . import _lib as L, ops
        b, c = items.shape[0], self.depth
        res = self.hr_res // self.lr_scale if self.is_lr else self.hr_res
        out = torch.empty(b, c, res, res, dtype=torch.uint8, device=self.device)
        L.check(L.lib().pssr_gen_pair_geometry_u8(L.ptr(items), b, L.ptr(out), c, res, L.stream_ptr()), "pssr_gen_pair_geometry_u8")
        if self.is_lr:
            return ops.u8_to_f32(out)
        hr, lr = self.gen(out)
        ops.counter_add(self.tile_counter, b)
        nf = self.n_frames
        if nf is not None and nf[0] != nf[1]:           # centre frames of each side, as _gen_pair
            if not nf[1] > hr.shape[-3]:
                hr = _slice_center(hr, nf[1]).contiguous()
            if not nf[0] > lr.shape[-3]:
                lr = _slice_center(lr, nf[0]).contiguous()
        return hr, lr

    def __getitem__(self, idx, pp=False):
        if idx >= len(self):
            raise IndexError(f"Tried to retrieve invalid image. Index {idx} is not less than {len(self)} total image frame slices.")
        out = self.device_batch(self.draw_items([idx], pp))
        return out[0] if self.is_lr else (out[0][0], out[1][0])


class DevicePairedTileDataset(PairedArrayDataset):
    """``PairedArrayDataset`` whose two uint8 stacks live in HBM: same arguments, attributes and item values (float32 CHW tensors, here on
    the device), so the drivers take it like any dataset whose items need no host-to-device copy.  Whole batches come from one host
    draw (``draw_pair_items``: the reference's rotation draws, index by index) and two launches of the ``_gen_pair`` gather kernel
    (``device_pair_batch``: one table per side, the same (rot, flip) per item).  These are deliberately not DeviceTileDataset's
    ``draw_items`` / ``device_batch``: the hipGraph replay of ``train_paired`` (pssr2_amd/fastpath.py) does not cover real pairs."""
    _keep_tensors = True        # stacks already in HBM stay there

    def __init__(self, hr_images, lr_images, hr_res=512, lr_scale=4, n_frames=-1, val_split=1, rotation=True, split_seed=None,
                 transforms=None, names=None, device="cuda"):
        if transforms is not None:
            raise NotImplementedError("DevicePairedTileDataset applies no host transforms")
        super().__init__(hr_images, lr_images, hr_res, lr_scale, n_frames, val_split, rotation, split_seed, None, names)
        self.hr_images = torch.as_tensor(self.hr_images).to(device).contiguous()
        self.lr_images = torch.as_tensor(self.lr_images).to(device).contiguous()
        if not self.hr_images.is_cuda:
            raise RuntimeError("DevicePairedTileDataset keeps its images on an MI355X (HIP) device; there is no CPU fallback")
        del self.compact            # items are float32 device tensors: the host feed has nothing to compact

    def draw_pair_items(self, indices, pp=False):
        """(HR table, LR table) for these dataset indices: the training rotations are drawn exactly as ``__getitem__`` would draw them
        for the same sequence of indices, and each draw is written to both tables."""
        indices = [int(i) for i in indices]
        for i in indices:
            if i >= len(self):
                raise IndexError(f"Tried to retrieve invalid image. Index {i} is not less than {len(self)} total image frame slices.")
        rots = [self._draw_rotation(i, pp) for i in indices]
        return _gather_table(self.hr_images, indices, rots), _gather_table(self.lr_images, indices, rots)

    def device_pair_batch(self, tables, u8=False):
        """tables: ``draw_pair_items``' result.  float32 (uint8 with ``u8``) (hr [b, C, R, R], lr [b, c, r, r]) on the device, no host
        synchronisation."""
        from . import _lib as L, ops
        out = []
        for table, images, res, keep in zip(tables, (self.hr_images, self.lr_images), (self.hr_res, self.hr_res // self.lr_scale), (1, 0)):
            b, c = table.shape[0], images.shape[1]
            side = torch.empty(b, c, res, res, dtype=torch.uint8, device=images.device)
            if b:
                L.check(L.lib().pssr_gen_pair_geometry_u8(L.ptr(table), b, L.ptr(side), c, res, L.stream_ptr()), "pssr_gen_pair_geometry_u8")
            if self.n_frames is not None and self.n_frames[0] != self.n_frames[1] and not self.n_frames[keep] > c:
                side = _slice_center(side, self.n_frames[keep]).contiguous()
            out.append(side if u8 or not b else ops.u8_to_f32(side))
        return tuple(out)

    def __getitem__(self, idx, pp=False):
        hr, lr = self.device_pair_batch(self.draw_pair_items([idx], pp))
        return hr[0], lr[0]


def _window_rows(entries):
    """int64 [n, 3] rows (= n ``pssr_window_item``) from (sheet, frame0, y0, x0, rotation draw) entries; host tensor."""
    import struct
    buf = bytearray()
    for sheet, frame0, y0, x0, rot in entries:
        axis = -1
        if rot:
            axis = 3 if isinstance(rot[1], (tuple, list)) else int(rot[1])
        buf += struct.pack("<iiiiii", sheet, frame0, y0, x0, int(bool(rot and rot[0])), axis)
    if not buf:                        # an empty order: torch.frombuffer rejects b""
        return torch.zeros(0, 3, dtype=torch.int64)
    return torch.frombuffer(buf, dtype=torch.int64).view(-1, 3)


class _SheetBank:
    """uint8 sheets [F, H, W] in HBM and their device table of ``pssr_sheet_desc`` {base, frames, h, w, reserved}."""

    def __init__(self, sheets, device, who):
        import struct
        self.sheets = [torch.as_tensor(s).to(device).contiguous() for s in sheets]
        if not self.sheets or not all(s.is_cuda for s in self.sheets):
            raise RuntimeError(f"{who} keeps its sheets on an MI355X (HIP) device; there is no CPU fallback")
        self.device = self.sheets[0].device
        buf = bytearray()
        for s in self.sheets:
            buf += struct.pack("<Qiiii", s.data_ptr(), *s.shape, 0)
        self.table = torch.frombuffer(buf, dtype=torch.int64).view(-1, 3).to(self.device)

    def check(self, sheet, frame0, y0, x0, c, res):
        """The host's half of the bounds check (the kernel zero-fills what fails its own): no launch with a window outside its sheet."""
        f, h, w = self.sheets[sheet].shape
        if not (0 <= frame0 and frame0 + c <= f and 0 <= y0 and y0 + res <= h and 0 <= x0 and x0 + res <= w):
            raise ValueError(f"window (frames {frame0}:{frame0 + c}, rows {y0}:{y0 + res}, columns {x0}:{x0 + res}) leaves sheet {sheet} "
                             f"of shape {(f, h, w)}")

    def gather(self, items, c, res):
        from . import ops
        return ops.gather_windows_u8(self.table, len(self.sheets), items, c, res)


def _uniform_frames(sheets, who, what="sheets"):
    frames = {int(getattr(s, "shape", s)[0]) for s in sheets}          # sheets, or their shapes
    if len(frames) != 1:
        raise ValueError(f"{who}: n_frames=-1 needs {what} with the same number of frames (a batch has one depth); found {sorted(frames)}")
    return frames.pop()


class DeviceSlidingDataset(SlidingSheetDataset):
    """``SlidingSheetDataset`` whose sheets live in HBM: same arguments, attributes and item values (float32 CHW tensors, here on the
    device).  Like ``DeviceTileDataset`` it makes whole batches without touching the host -- ``draw_items`` (the reference's rotation
    draws, index by index, and each window's origin: one ``pssr_window_item`` per index) and ``device_batch`` (one window gather out of
    the sheets, then the Pillow-exact reduction and the crappifier on device Philox streams) -- so ``train_paired`` replays a whole
    training step over sheets as one hipGraph (pssr2_amd/fastpath.py).  With ``n_frames=-1`` every sheet must have the same number of
    frames (a batch has one depth); host transforms are not applied."""
    _keep_tensors = True        # sheets already in HBM stay there

    def __init__(self, sheets, hr_res=512, lr_scale=4, crappifier=Poisson(), overlap=128, n_frames=-1, slide=False, val_split=0.1,
                 rotation=True, split_seed=0, transforms=None, names=None, device="cuda", seed=0):
        if transforms is not None:
            raise NotImplementedError("DeviceSlidingDataset applies no host transforms")
        super().__init__(sheets, hr_res, lr_scale, crappifier, overlap, n_frames, slide, val_split, rotation, split_seed, None, names)
        self.depth = max(self.n_frames) if self.n_frames is not None else _uniform_frames(self.sheets, type(self).__name__)
        self.bank = _SheetBank(self.sheets, device, type(self).__name__)
        self.sheets = self.bank.sheets
        del self.compact            # items are float32 device tensors: the host feed has nothing to compact
        self.tile_counter = torch.zeros(1, dtype=torch.int64, device=self.bank.device)
        self.gen = DevicePairGenerator(self.lr_scale, crappifier, seed=seed, tile_counter=self.tile_counter)
        self._item_bytes = 24             # struct pssr_window_item {sheet, frame0, y0, x0, rot, flip_axis}

    def draw_items(self, indices, pp=False):
        """Window table (int64 [n, 3] on the device = n ``pssr_window_item``) for these dataset indices, drawing the training rotations
        exactly as ``__getitem__`` would for the same sequence of indices.  Every window is checked against its sheet here."""
        entries = []
        for idx in indices:
            idx = int(idx)
            self._check_idx(idx)
            image_idx, local = _get_image_idx(idx, self.slices, self.tiles)
            origin = _window_origin(self.sheets[image_idx], self.hr_res, self.stride, None if self.n_frames is None else self.depth,
                                    self.slices[image_idx], local, self.slide)
            self.bank.check(image_idx, *origin, self.depth, self.hr_res)
            entries.append((image_idx, *origin, self._draw_rotation(idx, pp)))
        return _window_rows(entries).to(self.bank.device)

    def device_batch(self, items):
        """items: int64 [b, 3] device rows of ``draw_items``.  Returns float32 (hr, lr) on the device, or lr alone in LR mode.  No host
        synchronisation, no host-side data: capturable in a hipGraph (the Philox tile counter advances on the device)."""
        from . import ops
        out = self.bank.gather(items, self.depth, self.hr_res)
        if self.is_lr:
            return ops.u8_to_f32(out)
        hr, lr = self.gen(out)
        ops.counter_add(self.tile_counter, items.shape[0])
        nf = self.n_frames
        if nf is not None and nf[0] != nf[1]:           # centre frames of each side, as _gen_pair
            if not nf[1] > hr.shape[-3]:
                hr = _slice_center(hr, nf[1]).contiguous()
            if not nf[0] > lr.shape[-3]:
                lr = _slice_center(lr, nf[0]).contiguous()
        return hr, lr

    def __getitem__(self, idx, pp=False):
        out = self.device_batch(self.draw_items([idx], pp))
        return out[0] if self.is_lr else (out[0][0], out[1][0])


class DevicePairedSlidingDataset(PairedSlidingArrayDataset):
    """``PairedSlidingArrayDataset`` whose sheets live in HBM: same arguments, attributes and item values (float32 CHW tensors, here on
    the device).  Whole batches come from one host draw (``draw_pair_items``) and two window gathers (``device_pair_batch``: one sheet
    table and one item table per side, the same (rot, flip) per item), as ``DevicePairedTileDataset`` does for pre-cut pairs."""
    _keep_tensors = True

    def __init__(self, hr_sheets, lr_sheets, hr_res=512, lr_scale=4, overlap=128, n_frames=-1, slide=False, val_split=1, rotation=True,
                 split_seed=None, transforms=None, names=None, device="cuda"):
        if transforms is not None:
            raise NotImplementedError("DevicePairedSlidingDataset applies no host transforms")
        super().__init__(hr_sheets, lr_sheets, hr_res, lr_scale, overlap, n_frames, slide, val_split, rotation, split_seed, None, names)
        who, nf = type(self).__name__, self.n_frames
        self.depths = (nf[1], nf[0]) if nf is not None else (_uniform_frames(self.hr_sheets, who), _uniform_frames(self.lr_sheets, who))
        self.banks = (_SheetBank(self.hr_sheets, device, who), _SheetBank(self.lr_sheets, device, who))
        self.hr_sheets, self.lr_sheets = self.banks[0].sheets, self.banks[1].sheets
        del self.compact

    def draw_pair_items(self, indices, pp=False):
        """(HR table, LR table) for these dataset indices: the training rotations are drawn exactly as ``__getitem__`` would draw them for
        the same sequence of indices, and each draw is written to both tables.  Every window is checked against its sheet here."""
        entries = ([], [])
        for idx in indices:
            idx = int(idx)
            self._check_idx(idx)
            image_idx, _ = _get_image_idx(idx, self.slices, self.tiles)
            rot = self._draw_rotation(idx, pp)
            for side, bank, depth, (sheet, size, stride, frames, n_slices, local, slide) in zip(entries, self.banks, self.depths, self._side_args(idx)):
                origin = _window_origin(sheet, size, stride, frames, n_slices, local, slide)
                bank.check(image_idx, *origin, depth, size)
                side.append((image_idx, *origin, rot))
        return tuple(_window_rows(side).to(bank.device) for side, bank in zip(entries, self.banks))

    def device_pair_batch(self, tables, u8=False):
        """tables: ``draw_pair_items``' result.  float32 (uint8 with ``u8``) (hr [b, C, R, R], lr [b, c, r, r]) on the device, no host
        synchronisation.  Each side is gathered at its own depth (``n_frames[1]`` / ``n_frames[0]``), which ``_transform_pair``'s
        centre-frame slicing leaves as it is."""
        from . import ops
        out = []
        for table, bank, depth, res in zip(tables, self.banks, self.depths, (self.hr_res, self.hr_res // self.lr_scale)):
            if table.shape[0]:
                side = bank.gather(table, depth, res)
            else:
                side = torch.empty(0, depth, res, res, dtype=torch.uint8, device=bank.device)
            out.append(side if u8 or not table.shape[0] else ops.u8_to_f32(side))
        return tuple(out)

    def __getitem__(self, idx, pp=False):
        hr, lr = self.device_pair_batch(self.draw_pair_items([idx], pp))
        return hr[0], lr[0]
