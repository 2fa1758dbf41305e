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

Layout: four families (tile, paired tile, sheet, paired sheet), each an in-memory class, a folder class on top of it and an HBM-resident
class that derives from it.  What they share is written once: ``_ItemProtocol`` (index check, rotation draw, ``val_idx`` membership through
``_in_val``, ``compact``, ``__repr__``), ``_center_frames``, ``_u8_stack`` (input normalisation), ``_find_files`` / ``_find_paired_files`` /
``_read_sheets`` (folders), ``_pack_rows`` (kernel tables), and for the device classes ``_DeviceItems`` with ``_DeviceSynthesis`` (pairs
synthesised from HR: everything after the uint8 gather) and ``_DevicePairs`` (real pairs).  ``SlidingArrayDataset`` is
``SlidingSheetDataset`` in LR mode under a short signature: unlike its earlier stand-alone form it prints upstream's LR-mode line and
refuses sheets that are not uint8.
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


def _center_frames(sides, n_frames):
    """``n_frames=[lr, hr]`` of different lengths (pssr/data.py:488-492): the centre ``hr`` / ``lr`` frames of the (HR, LR) arrays or tensors
    [..., C, H, W]; a side that has fewer frames stays whole.  Views: the device callers make them contiguous."""
    if n_frames is None or n_frames[0] == n_frames[1]:
        return tuple(sides)
    return tuple(side if n > side.shape[-3] else _slice_center(side, n) for side, n in zip(sides, n_frames[::-1]))


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
    hr, lr = _center_frames((hr, lr), n_frames)
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
    hr, lr = _center_frames((hr, lr), n_frames)
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


# --------------------------------------------------------------------------------------- dataset inputs
def _u8_stack(x, ndim, message, keep_tensors=False):
    """One input of a dataset as the classes hold it: a numpy array (a tensor as it is with ``keep_tensors``: the device classes) of
    ``ndim`` axes [..., frames, H, W], an input without the frame axis taken as one frame each.  Anything else, and anything but uint8,
    raises ``ValueError(message)``."""
    if not torch.is_tensor(x):
        x = np.asarray(x)
    elif not keep_tensors:
        x = x.cpu().numpy()
    if x.ndim == ndim - 1:
        x = x[..., None, :, :]
    if x.ndim != ndim or str(x.dtype).split(".")[-1] != "uint8":          # numpy's and torch's spelling of the dtype
        raise ValueError(message)
    return x


def _tile_stacks(images, who, keep_tensors=False):
    """The stacks of a tile dataset: one uint8 array / tensor [N, C, H, W] (``[N, H, W]``: one frame each) as it came, or a sequence of uint8
    stacks [C_i, H_i, W_i] (2-D: one frame) of any depths and sizes -- stacked into one array when every shape agrees, else a list."""
    message = f"{who} expects uint8 images"
    if torch.is_tensor(images) or (isinstance(images, np.ndarray) and images.dtype != object):
        return _u8_stack(images, 4, message, keep_tensors)
    stacks = [_u8_stack(s, 3, message, keep_tensors) for s in images]
    if len(stacks) and len({tuple(s.shape) for s in stacks}) == 1:
        return torch.stack(stacks) if torch.is_tensor(stacks[0]) else np.stack(stacks)
    return stacks


def _check_paired(hr, lr, error=ValueError):
    if len(hr) != len(lr):
        raise error(f"Mismatch between amounts of high-low-resolution images. Found {len(hr)} high-resolution and {len(lr)} low-resolution images.")
    return hr, lr


def _check_register(register, who):
    """``register=None`` or a search radius for ``util.register_pairs``; a radius needs a HIP device, and says so before anything is read."""
    if register is None:
        return
    from .util import _check_radius
    _check_radius(register, f"{who}: register")
    if not torch.cuda.is_available():
        raise RuntimeError(f"{who}: register={register} aligns the stacks on an MI355X (HIP) device, and none is available; there is no CPU fallback")


def _paired_stacks(hr_images, lr_images, who, keep_tensors=False):
    return _check_paired(*(_u8_stack(images, 4, f"{who} expects uint8 images [N, C, H, W]", keep_tensors) for images in (hr_images, lr_images)))


def _sheet_list(sheets, who, keep_tensors=False):
    return [_u8_stack(s, 3, f"{who} expects uint8 sheets [F, H, W]", keep_tensors) for s in sheets]


def _stack_shapes(images):
    """(frames, H, W) per file of what ``_tile_stacks`` returned."""
    return [tuple(s.shape) for s in images] if isinstance(images, list) else [tuple(images.shape[1:])] * len(images)


def _stack_slices(shapes, n_frames):
    """Frame slices per file (pssr/data.py:70-74): 1 with ``n_frames=-1``, else ``frames // max(n_frames)`` -- none for a file that is too shallow."""
    return [1 if n_frames is None else s[0] // max(n_frames) for s in shapes]


def _max_extent(shapes):
    return max((max(s[-2:]) for s in shapes), default=0)


def _tiles_slices(sheets, size, stride, n_frames, slide):
    """Windows per sheet and frame slices per window (pssr/data.py:205-210)."""
    tiles, slices = [], []
    for s in sheets:
        tx, ty = _n_tiles(s, size, stride)
        tiles.append(tx * ty)
        slices.append(1 if n_frames is None else ((s.shape[0] - max(n_frames) + 1) if slide else (s.shape[0] // max(n_frames))))
    return tiles, slices


def _check_stride(hr_res, overlap):
    overlap = 0 if overlap is None else overlap
    if not hr_res > overlap:
        raise ValueError(f"hr_res must be greater than overlap. Given values are {hr_res} and {overlap} respectively.")
    return hr_res - overlap


# --------------------------------------------------------------------------------------- folders
def _existing_path(path):
    given, path = path, Path(path) if type(path) is str else path
    if not given or not path.exists():
        raise FileNotFoundError(f'Path "{path}" does not exist.')
    return path


def _find_files(path, extension, sheets=False):
    """(folder, its ``.extension`` files at any depth, relative and sorted), with the reference's errors in its order; ``sheets``: the sheet
    classes, which upstream reads czi files for and this package does not."""
    path = _existing_path(path)
    if sheets and extension.lower() == "czi":
        raise NotImplementedError("czi sheets are not supported by pssr2_amd (czifile is not a dependency): export them to tif")
    files = sorted(f.split(str(path), maxsplit=1)[-1].strip("/") for f in glob.glob(f"{path}/**/*.{extension}", recursive=True))
    if not files:
        raise FileNotFoundError(f'No .{extension} files exist in path "{path}".')
    return path, files


def _find_paired_files(hr_path, lr_path, extension, instead, sheets=False):
    """((HR folder, files), (LR folder, files)) of a two-folder dataset (pssr/data.py:294-306, 384-396): both folders exist, the warning
    for one folder given twice (raised for the caller of the dataset's constructor), the files of each side, as many on both."""
    hr_path, lr_path = _existing_path(hr_path), _existing_path(lr_path)
    if hr_path == lr_path:
        warnings.warn(f"hr_path is equal to lr_path! Consider using {instead} instead.", stacklevel=3)
    hr, lr = _find_files(hr_path, extension, sheets), _find_files(lr_path, extension, sheets)
    _check_paired(hr[1], lr[1], FileNotFoundError)
    return hr, lr


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


def _file_names(files):
    return [f.split(".")[0] for f in files]


# --------------------------------------------------------------------------------------- item protocol
def _get_image_idx(idx, slices, tiles=None):
    """(sheet, index inside the sheet) of a dataset index (pssr/data.py:697-706)."""
    tiles = [1] * len(slices) if tiles is None else tiles
    for image_idx, (s, t) in enumerate(zip(slices, tiles)):
        if idx < s * t:
            return image_idx, idx
        idx -= s * t
    return None


def _in_val(dataset, idx):
    # ``idx in dataset.val_idx`` as upstream (pssr/data.py:103), with the list hashed once per assignment / length change: users enlarge
    # val_idx after training to predict every image
    key = (id(dataset.val_idx), len(dataset.val_idx))
    if key != getattr(dataset, "_val_key", None):
        dataset._val_set, dataset._val_key = set(dataset.val_idx), key
    return idx in dataset._val_set


class _ItemProtocol(Dataset):
    """What every dataset family shares of the reference's item protocol: the index check, the rotation draw, ``extra_hr_files`` and
    ``compact``, ``__repr__``.  A family sets ``hr_res``, ``lr_scale``, ``is_lr``, ``rotation``, ``transforms``, ``val_idx`` and ``names``
    (``_set_protocol``) and writes ``__len__``, ``_get_name``, ``_summary`` and ``_item``."""
    _keep_tensors = False           # True in the device classes: inputs already in HBM stay there
    _host_items = True              # False in the device classes: their items are float32 device tensors, so the host feed has nothing to
                                    # compact and they have no ``compact`` attribute at all (the drivers ask ``getattr(dataset, "compact", None)``)

    def _set_protocol(self, hr_res, lr_scale, rotation, transforms, names, stem, count):
        self.hr_res, self.lr_scale, self.rotation, self.transforms = hr_res, lr_scale, rotation, transforms
        self.extra_hr_files = None
        if self._host_items:
            self.compact = False        # True while a driver feeds a captured graph from this dataset: uint8 items (see _tensor_ready)
        self.names = list(names) if names is not None else [f"{stem}{i}" for i in range(count)]

    def _check_idx(self, idx, row=False):
        """``row``: the index becomes a row that a kernel reads addresses from, so nothing before the first item either."""
        if idx >= len(self) or (row and idx < 0):
            raise IndexError(f"Tried to retrieve invalid image. Index {idx} is not less than {len(self)} total image frame slices.")

    def _draw_rotation(self, idx, pp=False):
        """``False`` for a validation item and for ``pp`` (preprocess_dataset's items are never rotated, pssr/data.py:103), else the
        reference's two draws in its order -- also in LR mode, where they go unused."""
        if self.rotation and not (_in_val(self, idx) or pp):
            return [bool(random.getrandbits(1)), random.choice((1, 2, (1, 2)))]
        return False

    def __getitem__(self, idx, pp=False):
        self._check_idx(idx)
        return self._item(idx, self._draw_rotation(idx, pp))

    def _res_line(self):
        return f"low-res: {self.hr_res // self.lr_scale}" if self.is_lr else f"high-res: {self.hr_res}, low-res: {self.hr_res // self.lr_scale}"

    def __repr__(self):
        return f"{self._summary()} with {len(self)} total frame slices\n{self._res_line()}"


# --------------------------------------------------------------------------------------- tiles
class ArrayDataset(_ItemProtocol):
    """In-memory HR stacks (uint8 [N, C, H, W], or a sequence of stacks [C_i, H_i, W_i] of differing depths and sizes) with the attribute
    protocol the drivers consume (``val_idx``, ``extra_hr_files``, ``crop_res``, ``lr_scale``, ``is_lr``, ``hr_res``, ``n_frames``,
    ``_get_name``).  With ``n_frames`` every stack is cut into ``frames // max(n_frames)`` consecutive frame slices, each one item
    (pssr/data.py:70-74, 100-110, 566-577, 649-660): item ``idx`` is slice ``k`` of file ``f``, ``(f, k) = _get_image_idx(idx, slices)``,
    frames ``[k * m, k * m + m)`` with ``m = max(n_frames)``, named ``{name}_{k}``; the validation split is taken over files.
    ``images`` stays the single array when every stack has one shape, else it is the list."""

    def __init__(self, images, hr_res=512, lr_scale=4, crappifier=Poisson(), val_split=0.1, rotation=True, split_seed=0,
                 transforms=None, names=None, n_frames=-1):
        self.images = _tile_stacks(images, type(self).__name__, self._keep_tensors)
        lr_scale = None if lr_scale == -1 else lr_scale
        self.n_frames = _get_n_frames(n_frames)
        shapes = _stack_shapes(self.images)
        self.slices = _stack_slices(shapes, self.n_frames)
        max_size = _max_extent(shapes)
        self.val_idx = _get_val_idx(self.slices, val_split, split_seed)
        self.crop_res = min(hr_res, max_size)
        self.is_lr = lr_scale is None or max_size <= hr_res // lr_scale
        self.crappifier = crappifier
        self._set_protocol(hr_res, lr_scale if lr_scale is not None else 1, rotation, transforms, names, "image", len(self.images))

    def __len__(self):
        return sum(self.slices)

    def _slice(self, idx):
        """Host stack [frames, H, W] of a dataset index: the whole file with ``n_frames=-1``, else ``max(n_frames)`` frames of it."""
        if self.n_frames is None:
            return self.images[idx]
        image_idx, k = _get_image_idx(idx, self.slices)
        m = max(self.n_frames)
        return self.images[image_idx][k * m:k * m + m]

    def _item(self, idx, rot):
        hr = self._slice(idx)
        if self.is_lr:
            return _ready_lr(hr, self.hr_res // self.lr_scale, self.transforms, self.compact)
        return _gen_pair(hr, self.hr_res, self.lr_scale, rot, self.crappifier, self.transforms, self.n_frames, self.compact)

    def _summary(self):
        return f"{type(self).__name__} of {len(self.images)} images"

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
        self.path, self.hr_files = _find_files(path, extension)
        if extra_path is not None:
            raise NotImplementedError("extra_path is not supported by pssr2_amd.ImageDataset")
        super().__init__(_read_sheets(self.path, self.hr_files), hr_res, lr_scale, crappifier, val_split, rotation, split_seed, transforms,
                         _file_names(self.hr_files), n_frames)

    def _summary(self):
        return f'ImageDataset from path "{self.path}"\n{len(self.hr_files)} files'


class PairedArrayDataset(_ItemProtocol):
    """Real (HR, LR) pairs in memory, uint8 [N, C, H, W] and [N, c, h, w]: the reference's ``PairedImageDataset`` (pssr/data.py:268-346)
    without the files -- its defaults (``val_split=1``: every item is a validation item; ``split_seed=None``: the last images), its
    attribute protocol and its item geometry (``_transform_pair``), for ``train_crappifier``, ``approximate_crappifier``,
    ``test_metrics`` and ``predict_images(norm=True)``.  Every pair is one item: with ``n_frames=[lr, hr]`` of different lengths the
    centre frames of the two stacks are taken, as ``_transform_pair`` does.

    ``register=R`` (keyword-only, not in the reference; also on ``PairedImageDataset`` and ``DevicePairedTileDataset``): the two sides are
    separate acquisitions a few HR pixels apart, so ``util.register_pairs(radius=R)`` runs once over the whole stacks at construction
    (it needs a HIP device), the class holds the aligned stacks without their margin, and ``shifts`` [N, 2] / ``scores`` [N] say what was
    found.  ``None``: the stacks as they came."""

    def __init__(self, hr_images, lr_images, hr_res=512, lr_scale=4, n_frames=-1, val_split=1, rotation=True, split_seed=None,
                 transforms=None, names=None, *, register=None):
        _check_register(register, type(self).__name__)
        self.hr_images, self.lr_images = _paired_stacks(hr_images, lr_images, type(self).__name__, self._keep_tensors)
        self.shifts = self.scores = None
        if register is not None:
            self._register(register)
        self.n_frames = _get_n_frames(n_frames)
        self.slices = [1] * len(self.hr_images)
        self.val_idx = _get_val_idx(self.slices, val_split, split_seed)
        self.is_lr = False
        self.crop_res = min(hr_res, max(self.hr_images.shape[-2:]))
        self._set_protocol(hr_res, lr_scale, rotation, transforms, names, "image", len(self.hr_images))

    __len__ = ArrayDataset.__len__

    def _register(self, radius):
        """``register=radius``: the stacks become the aligned, cropped stacks of one ``util.register_pairs`` call over all of them."""
        from .util import register_pairs
        reg = register_pairs(self.hr_images, self.lr_images, radius=radius, to_numpy=not self._keep_tensors)
        self.hr_images, self.lr_images, self.shifts, self.scores = reg.hr, reg.lr, reg.shift, reg.score

    def _item(self, idx, rot):
        return _transform_pair(self.hr_images[idx], self.lr_images[idx], self.hr_res, self.hr_res // self.lr_scale, rot, self.transforms,
                               self.n_frames, self.compact)

    def _summary(self):
        return f"{type(self).__name__} of {len(self.hr_images)} paired images"

    def _get_name(self, idx):
        return self.names[idx] + ("_0" if self.n_frames is not None else "")


class PairedImageDataset(PairedArrayDataset):
    """Two folders of pre-tiled images (anything Pillow opens) holding the high- and low-resolution side of each pair in the same sorted
    order: reference arguments, errors and warning (pssr/data.py:268-346).  The files of a side must be equally sized; tif stacks
    sliced into several items per file and sheets are outside this build's scope."""

    def __init__(self, hr_path, lr_path, hr_res=512, lr_scale=4, n_frames=-1, extension="tif", val_split=1, rotation=True,
                 split_seed=None, transforms=None, *, register=None):
        _check_register(register, type(self).__name__)
        (self.hr_path, self.hr_files), (self.lr_path, self.lr_files) = _find_paired_files(hr_path, lr_path, extension, "ImageDataset")
        sides = []
        for path, files in ((self.hr_path, self.hr_files), (self.lr_path, self.lr_files)):
            stacks = _read_sheets(path, files)
            if len({st.shape for st in stacks}) != 1:
                raise ValueError(f'pssr2_amd.PairedImageDataset needs equally sized images in "{path}"')
            sides.append(np.stack(stacks))
        super().__init__(*sides, hr_res, lr_scale, n_frames, val_split, rotation, split_seed, transforms, _file_names(self.lr_files),
                         register=register)
        self.mode = "L"

    def _summary(self):
        return f'PairedImageDataset from paths "{self.hr_path}" and "{self.lr_path}"\n{len(self.hr_files)} paired files'


# --------------------------------------------------------------------------------------- sheets
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


class _SheetIndex(_ItemProtocol):
    """Windows times frame slices per sheet (``tiles``, ``slices``): what the two sheet families count and name their items by."""

    def __len__(self):
        return sum(t * s for t, s in zip(self.tiles, self.slices))

    def _get_name(self, idx):
        image_idx, local = _get_image_idx(idx, self.slices, self.tiles)
        return f"{self.names[image_idx]}_{local // self.slices[image_idx]}_{local % self.slices[image_idx]}"


class SlidingSheetDataset(_SheetIndex):
    """Training dataset over in-memory image sheets (uint8 [F, H, W] each, 2-D accepted, of any sizes): the reference's
    ``SlidingDataset`` (pssr/data.py:132-266) without the files.  Same arithmetic -- ``stride = hr_res - overlap``, whole windows only,
    row-major; per sheet ``tiles`` windows times ``slices`` frame slices (``frames - max(n_frames) + 1`` with ``slide``, else
    ``frames // max(n_frames)``); the validation split is taken over windows (``_get_val_idx(slices, split, seed, tiles)``); item
    ``idx`` of a sheet is window ``idx // slices``, frame slice ``idx % slices`` -- the same attribute protocol, names
    (``{name}_{window}_{slice}``), ``__getitem__(idx, pp=False)`` and LR mode (``lr_scale=-1``, ``hr_res`` = LR resolution)."""

    def __init__(self, sheets, hr_res=512, lr_scale=4, crappifier=Poisson(), overlap=128, n_frames=-1, slide=False, val_split=0.1,
                 rotation=True, split_seed=0, transforms=None, names=None):
        self.sheets = _sheet_list(sheets, type(self).__name__, self._keep_tensors)
        self.stride = _check_stride(hr_res, overlap)
        self.n_frames, self.slide = _get_n_frames(n_frames), slide
        self.tiles, self.slices = _tiles_slices(self.sheets, hr_res, self.stride, self.n_frames, slide)
        self.val_idx = _get_val_idx(self.slices, val_split, split_seed, self.tiles)
        self.crop_res = hr_res
        self.is_lr = lr_scale in (-1, None)
        if self.is_lr:
            print("LR mode is enabled, dataset will load only unmodified low-resolution images.")
            if val_split < 1:
                warnings.warn("val_split is less than 1, not all low-resolution images will be used in prediciton.", stacklevel=2)
        self.crappifier = crappifier
        self._set_protocol(hr_res, 1 if self.is_lr else lr_scale, rotation, transforms, names, "sheet", len(self.sheets))

    def _window(self, idx):
        """Host window [frames, hr_res, hr_res] of a dataset index, ``max(n_frames)`` frames deep."""
        image_idx, local = _get_image_idx(idx, self.slices, self.tiles)
        return _sliding_window(self.sheets[image_idx], self.hr_res, self.stride, max(self.n_frames) if self.n_frames is not None else None,
                               self.slices[image_idx], local, self.slide)

    def _item(self, idx, rot):
        hr = self._window(idx)
        if self.is_lr:
            return _ready_lr(hr, self.hr_res, self.transforms, self.compact)
        return _gen_pair(hr, self.hr_res, self.lr_scale, rot, self.crappifier, self.transforms, self.n_frames, self.compact)

    def _summary(self):
        return f"{type(self).__name__} of {len(self.sheets)} sheets"


class SlidingArrayDataset(SlidingSheetDataset):
    """LR-mode sliding window over in-memory sheets, every tile a validation item: ``SlidingSheetDataset(lr_scale=-1, val_split=1)`` under
    the short signature ``predict_images`` is given sheets with (tiles row-major, ``stride = hr_res - overlap``, trailing remainders
    dropped, names ``{name}_{tile}_0``)."""

    def __init__(self, sheets, hr_res=128, overlap=32, names=None, transforms=None):
        super().__init__(sheets, hr_res, -1, None, overlap, val_split=1, transforms=transforms, names=names)


class SlidingDataset(SlidingSheetDataset):
    """Folder of image sheets: reference arguments, errors and warning (pssr/data.py:132-266).  Files are read through Pillow
    (multi-page tifs included).  ``preload`` is accepted for compatibility: the sheets are held in host memory either way.  czi files
    (``extension="czi"``, with them ``stack``) and ``extra_path`` raise ``NotImplementedError``."""

    def __init__(self, path, hr_res=512, lr_scale=4, crappifier=Poisson(), overlap=128, n_frames=-1, slide=False, stack="TZ",
                 extension="tif", preload=True, val_split=0.1, rotation=True, split_seed=0, extra_path=None, extra_scale=1,
                 transforms=None):
        self.path, self.hr_files = _find_files(path, extension, sheets=True)
        if extra_path is not None:
            raise NotImplementedError("extra_path is not supported by pssr2_amd.SlidingDataset")
        self.stack, self.mode, self.preload, self.extra_path, self.extra_scale = stack.upper(), "L", preload, None, extra_scale
        _check_stride(hr_res, overlap)          # before any file is read, as upstream
        super().__init__(_read_sheets(self.path, self.hr_files), hr_res, lr_scale, crappifier, overlap, n_frames, slide, val_split, rotation,
                         split_seed, transforms, _file_names(self.hr_files))

    def _summary(self):
        return f'SlidingDataset from path "{self.path}"\n{len(self.hr_files)} files'


class PairedSlidingArrayDataset(_SheetIndex):
    """Real (HR, LR) sheet pairs in memory (uint8 [F, H, W] / [f, h, w] each): the reference's ``PairedSlidingDataset``
    (pssr/data.py:348-444) without the files -- its defaults (``val_split=1``, ``split_seed=None``), attribute protocol and item geometry
    (``_transform_pair``), for ``train_crappifier``, ``approximate_crappifier`` and ``test_metrics``.  Windows, slices and the split are
    counted on the HR sheets.  As upstream, the LR side runs its own sliding window with ``hr_res // lr_scale`` and
    ``stride // lr_scale`` and takes its windows-per-row from the LR sheet, not from the HR sheet; and with ``n_frames=[lr, hr]`` each
    side takes its own number of frames from the slice's first frame on."""

    def __init__(self, hr_sheets, lr_sheets, hr_res=512, lr_scale=4, overlap=128, n_frames=-1, slide=False, val_split=1, rotation=True,
                 split_seed=None, transforms=None, names=None):
        who = type(self).__name__
        self.hr_sheets, self.lr_sheets = _check_paired(_sheet_list(hr_sheets, who, self._keep_tensors), _sheet_list(lr_sheets, who, self._keep_tensors))
        self.stride = _check_stride(hr_res, overlap)
        self.n_frames, self.slide = _get_n_frames(n_frames), slide
        self.tiles, self.slices = _tiles_slices(self.hr_sheets, hr_res, self.stride, self.n_frames, slide)
        self.val_idx = _get_val_idx(self.slices, val_split, split_seed, self.tiles)
        self.is_lr, self.crop_res = False, hr_res
        self._set_protocol(hr_res, lr_scale, rotation, transforms, names, "sheet", len(self.hr_sheets))

    def _side_args(self, idx):
        """Per side (HR, LR): (sheet, size, stride, frames, slices of the sheet, in-sheet index, slide) as ``_sliding_window`` takes them."""
        image_idx, local = _get_image_idx(idx, self.slices, self.tiles)
        nf = self.n_frames
        return ((self.hr_sheets[image_idx], self.hr_res, self.stride, nf[1] if nf is not None else None, self.slices[image_idx], local, self.slide),
                (self.lr_sheets[image_idx], self.hr_res // self.lr_scale, self.stride // self.lr_scale, nf[0] if nf is not None else None,
                 self.slices[image_idx], local, self.slide))

    def _item(self, idx, rot):
        hr_args, lr_args = self._side_args(idx)
        return _transform_pair(_sliding_window(*hr_args), _sliding_window(*lr_args), self.hr_res, self.hr_res // self.lr_scale, rot,
                               self.transforms, self.n_frames, self.compact)

    def _summary(self):
        return f"{type(self).__name__} of {len(self.hr_sheets)} paired sheets"


class PairedSlidingDataset(PairedSlidingArrayDataset):
    """Two folders of image sheets holding the high- and low-resolution side of each pair in the same sorted order: reference
    arguments, errors and warning (pssr/data.py:348-444); items are named after the LR files.  Files as in :class:`SlidingDataset`
    (Pillow; ``preload`` accepted, sheets held in host memory either way; czi raises ``NotImplementedError``)."""

    def __init__(self, hr_path, lr_path, hr_res=512, lr_scale=4, overlap=128, n_frames=-1, slide=False, stack="TZ", extension="tif",
                 preload=True, val_split=1, rotation=True, split_seed=None, transforms=None):
        (self.hr_path, self.hr_files), (self.lr_path, self.lr_files) = _find_paired_files(hr_path, lr_path, extension, "SlidingDataset", sheets=True)
        self.stack, self.mode, self.preload = stack.upper(), "L", preload
        _check_stride(hr_res, overlap)
        super().__init__(_read_sheets(self.hr_path, self.hr_files), _read_sheets(self.lr_path, self.lr_files), hr_res, lr_scale, overlap,
                         n_frames, slide, val_split, rotation, split_seed, transforms, _file_names(self.lr_files))

    def _summary(self):
        return f'PairedSlidingDataset from paths "{self.hr_path}" and "{self.lr_path}"\n{len(self.hr_files)} paired files'


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
        kind, intensity, gain, spread, *more = spec       # a fifth field: ScanPhase's jitter
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
        if kind == "scanphase":     # a row table from the tile's Philox stream, then the resampling of the rows
            tiles, h = x.shape[0], x.shape[-2]
            table = ops.scan_rows_table(tiles, x.numel() // (tiles * h * x.shape[-1]), h, intensity, spread, more[0], seed, tile_offset,
                                        tile_counter=self.tile_counter)
            return ops.shift_rows_f32(x, table, gain, flags)
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


def _pack_rows(head, entries):
    """int64 [n, 3] host rows, one 24-byte kernel item per entry: its leading fields as the struct format ``head`` says, then the rot90 flag
    and the flip axis (-1: none, 3: both) of its ``False`` / ``[rot, axis]`` draw.  One ``struct.pack`` over all entries."""
    import struct
    flat = []
    for entry in entries:
        rot = entry[-1]
        flat += entry[:-1]
        flat += (1 if rot[0] else 0, 3 if isinstance(rot[1], (tuple, list)) else int(rot[1])) if rot else (0, -1)
    if not flat:                       # an empty order (val_split = 0, a rank without validation items): torch.frombuffer rejects b""
        return torch.zeros(0, 3, dtype=torch.int64)
    buf = bytearray(24 * len(entries))
    struct.pack_into("<" + (head + "ii") * len(entries), buf, 0, *flat)
    return torch.frombuffer(buf, dtype=torch.int64).view(-1, 3)


def _gather_rows(entries, device):
    """int64 [n, 3] device rows (= n ``pssr_gather_item`` {src, sh, sw, rot, flip_axis}) from (src address, sh, sw, draw) entries."""
    return _pack_rows("Qii", entries).to(device)


def _window_rows(entries):
    """int64 [n, 3] rows (= n ``pssr_window_item`` {sheet, frame0, y0, x0, rot, flip_axis}) from (sheet, frame0, y0, x0, draw) entries; host tensor."""
    return _pack_rows("iiii", entries)


def _gather_table(images, indices, rotations):
    """int64 [n, 3] device rows (= n ``pssr_gather_item``) that point at ``images[i]`` with the given ``False`` / ``[rot, axis]`` draws."""
    c, h, w = images.shape[1:]
    base, stride = images.data_ptr(), c * h * w
    return _gather_rows([(base + int(i) * stride, h, w, rot) for i, rot in zip(indices, rotations)], images.device)


def _gen_pair_geometry_u8(items, depth, res, device):
    """uint8 [b, depth, res, res]: one launch of the ``_gen_pair`` gather kernel over the int64 [b, 3] device rows ``items``."""
    from . import _lib as L
    out = torch.empty(items.shape[0], depth, res, res, dtype=torch.uint8, device=device)
    L.check(L.lib().pssr_gen_pair_geometry_u8(L.ptr(items), items.shape[0], L.ptr(out), depth, res, L.stream_ptr()), "pssr_gen_pair_geometry_u8")
    return out


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


class _DeviceItems:
    """What the four HBM-resident classes put in front of their host class: inputs stay tensors, items are float32 device tensors (no
    ``compact``), no host transforms, and every index is checked before it becomes a row of a kernel's table."""
    _keep_tensors, _host_items = True, False

    def _no_transforms(self, transforms):
        if transforms is not None:
            raise NotImplementedError(f"{type(self).__name__} applies no host transforms")

    def _row_indices(self, indices):
        """The indices as ints; one outside the dataset raises ``IndexError`` before anything is drawn: a row is an address the kernel reads from."""
        indices, n = [int(i) for i in indices], len(self)
        for i in indices:
            if not 0 <= i < n:
                self._check_idx(i, row=True)
        return indices


class _DeviceSynthesis(_DeviceItems):
    """The half that ``DeviceTileDataset`` and ``DeviceSlidingDataset`` share: everything after their uint8 HR batch [b, depth, R, R] is
    gathered (``_gather_u8`` over the rows of their ``draw_items``)."""

    def _set_generator(self, device, seed):
        self.tile_counter = torch.zeros(1, dtype=torch.int64, device=device)
        self.gen = DevicePairGenerator(self.lr_scale, self.crappifier, seed=seed, tile_counter=self.tile_counter)

    def device_batch(self, items):
        """items: int64 [b, 3] device rows of ``draw_items``.  Returns float32 (hr, lr) on the device, or lr alone in LR mode.  No
        host synchronisation, no host-side data: capturable in a hipGraph (the Philox tile counter advances on the device)."""
        from . import ops
        out = self._gather_u8(items)
        if self.is_lr:
            return ops.u8_to_f32(out)
        pair = self.gen(out)
        ops.counter_add(self.tile_counter, items.shape[0])
        hr, lr = _center_frames(pair, self.n_frames)           # centre frames of each side, as _gen_pair
        return hr.contiguous(), lr.contiguous()

    def __getitem__(self, idx, pp=False):
        out = self.device_batch(self.draw_items([idx], pp))
        return out[0] if self.is_lr else (out[0][0], out[1][0])


class _DevicePairs(_DeviceItems):
    """The half that the two paired device classes share: ``device_pair_batch`` around their ``_gather_u8(side, table, depth, res)``;
    ``depths``: frames per side (HR, LR) of what that gathers."""

    def device_pair_batch(self, tables, u8=False):
        """tables: ``draw_pair_items``' result.  float32 (uint8 with ``u8``, and for an empty table) (hr [b, C, R, R], lr [b, c, r, r]) on
        the device, no host synchronisation; with ``n_frames=[lr, hr]`` the centre frames of each side, as ``_transform_pair``."""
        from . import ops
        sides = []
        for side, (table, depth, res) in enumerate(zip(tables, self.depths, (self.hr_res, self.hr_res // self.lr_scale))):
            if table.shape[0]:
                sides.append(self._gather_u8(side, table, depth, res))
            else:
                sides.append(torch.empty(0, depth, res, res, dtype=torch.uint8, device=table.device))
        sides = [s.contiguous() for s in _center_frames(sides, self.n_frames)]
        return tuple(s if u8 or not s.shape[0] else ops.u8_to_f32(s) for s in sides)

    def __getitem__(self, idx, pp=False):
        hr, lr = self.device_pair_batch(self.draw_pair_items([idx], pp))
        return hr[0], lr[0]


class DeviceTileDataset(_DeviceSynthesis, ArrayDataset):
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
        self._no_transforms(transforms)
        super().__init__(images, hr_res, lr_scale, crappifier, val_split, rotation, split_seed, None, names, n_frames)
        if isinstance(self.images, list):
            self.images = [torch.as_tensor(s).to(device).contiguous() for s in self.images]
        else:
            self.images = torch.as_tensor(self.images).to(device).contiguous()
        shapes = _stack_shapes(self.images)
        self.depth = max(self.n_frames) if self.n_frames is not None else _uniform_frames(shapes, type(self).__name__, "stacks")
        self.device = self.images[0].device if isinstance(self.images, list) else self.images.device
        self._set_generator(self.device, seed)
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

    def draw_items(self, indices, pp=False):
        """Gather table (int64 [n, 3] on the device = n ``pssr_gather_item``) for these dataset indices, drawing the training
        rotations exactly as ``__getitem__`` would for the same sequence of indices (none with ``pp``)."""
        return _gather_rows([self._where[i][2:] + (self._draw_rotation(i, pp),) for i in self._row_indices(indices)], self.device)

    def _gather_u8(self, items):
        return _gen_pair_geometry_u8(items, self.depth, self.hr_res // self.lr_scale if self.is_lr else self.hr_res, self.device)


class DevicePairedTileDataset(_DevicePairs, PairedArrayDataset):
    """``PairedArrayDataset`` whose two uint8 stacks live in HBM: same arguments, attributes and item values (float32 CHW tensors, here on
    the device), so the drivers take it like any dataset whose items need no host-to-device copy.  Whole batches come from one host
    draw (``draw_pair_items``: the reference's rotation draws, index by index) and two launches of the ``_gen_pair`` gather kernel
    (``device_pair_batch``: one table per side, the same (rot, flip) per item).  These are deliberately not DeviceTileDataset's
    ``draw_items`` / ``device_batch``: the hipGraph replay of ``train_paired`` (pssr2_amd/fastpath.py) does not cover real pairs."""

    def __init__(self, hr_images, lr_images, hr_res=512, lr_scale=4, n_frames=-1, val_split=1, rotation=True, split_seed=None,
                 transforms=None, names=None, device="cuda", *, register=None):
        self._no_transforms(transforms)
        self._device = device           # where ``register=`` aligns the stacks, before the class holds them
        super().__init__(hr_images, lr_images, hr_res, lr_scale, n_frames, val_split, rotation, split_seed, None, names, register=register)
        self.hr_images = torch.as_tensor(self.hr_images).to(device).contiguous()
        self.lr_images = torch.as_tensor(self.lr_images).to(device).contiguous()
        if not self.hr_images.is_cuda:
            raise RuntimeError("DevicePairedTileDataset keeps its images on an MI355X (HIP) device; there is no CPU fallback")
        self.depths = (self.hr_images.shape[1], self.lr_images.shape[1])

    def _register(self, radius):
        self.hr_images, self.lr_images = (torch.as_tensor(x).to(self._device) for x in (self.hr_images, self.lr_images))
        super()._register(radius)

    def draw_pair_items(self, indices, pp=False):
        """(HR table, LR table) for these dataset indices: the training rotations are drawn exactly as ``__getitem__`` would draw them
        for the same sequence of indices, and each draw is written to both tables."""
        indices = self._row_indices(indices)
        rots = [self._draw_rotation(i, pp) for i in indices]
        return _gather_table(self.hr_images, indices, rots), _gather_table(self.lr_images, indices, rots)

    def _gather_u8(self, side, table, depth, res):
        return _gen_pair_geometry_u8(table, depth, res, table.device)


class DeviceSlidingDataset(_DeviceSynthesis, SlidingSheetDataset):
    """``SlidingSheetDataset`` whose sheets live in HBM: same arguments, attributes and item values (float32 CHW tensors, here on the
    device).  Like ``DeviceTileDataset`` it makes whole batches without touching the host -- ``draw_items`` (the reference's rotation
    draws, index by index, and each window's origin: one ``pssr_window_item`` per index) and ``device_batch`` (one window gather out of
    the sheets, then the Pillow-exact reduction and the crappifier on device Philox streams) -- so ``train_paired`` replays a whole
    training step over sheets as one hipGraph (pssr2_amd/fastpath.py).  With ``n_frames=-1`` every sheet must have the same number of
    frames (a batch has one depth); host transforms are not applied."""

    def __init__(self, sheets, hr_res=512, lr_scale=4, crappifier=Poisson(), overlap=128, n_frames=-1, slide=False, val_split=0.1,
                 rotation=True, split_seed=0, transforms=None, names=None, device="cuda", seed=0):
        self._no_transforms(transforms)
        super().__init__(sheets, hr_res, lr_scale, crappifier, overlap, n_frames, slide, val_split, rotation, split_seed, None, names)
        self.depth = max(self.n_frames) if self.n_frames is not None else _uniform_frames(self.sheets, type(self).__name__)
        self.bank = _SheetBank(self.sheets, device, type(self).__name__)
        self.sheets = self.bank.sheets
        self._set_generator(self.bank.device, seed)

    def draw_items(self, indices, pp=False):
        """Window table (int64 [n, 3] on the device = n ``pssr_window_item``) for these dataset indices, drawing the training rotations
        exactly as ``__getitem__`` would for the same sequence of indices.  Every window is checked against its sheet here."""
        entries = []
        for idx in self._row_indices(indices):
            image_idx, local = _get_image_idx(idx, self.slices, self.tiles)
            origin = _window_origin(self.sheets[image_idx], self.hr_res, self.stride, None if self.n_frames is None else self.depth,
                                    self.slices[image_idx], local, self.slide)
            self.bank.check(image_idx, *origin, self.depth, self.hr_res)
            entries.append((image_idx, *origin, self._draw_rotation(idx, pp)))
        return _window_rows(entries).to(self.bank.device)

    def _gather_u8(self, items):
        return self.bank.gather(items, self.depth, self.hr_res)


class DevicePairedSlidingDataset(_DevicePairs, PairedSlidingArrayDataset):
    """``PairedSlidingArrayDataset`` whose sheets live in HBM: same arguments, attributes and item values (float32 CHW tensors, here on
    the device).  Whole batches come from one host draw (``draw_pair_items``) and two window gathers (``device_pair_batch``: one sheet
    table and one item table per side, the same (rot, flip) per item), as ``DevicePairedTileDataset`` does for pre-cut pairs.  Each side
    is gathered at its own depth (``n_frames[1]`` / ``n_frames[0]``), which the centre-frame slicing leaves as it is."""

    def __init__(self, hr_sheets, lr_sheets, hr_res=512, lr_scale=4, overlap=128, n_frames=-1, slide=False, val_split=1, rotation=True,
                 split_seed=None, transforms=None, names=None, device="cuda"):
        self._no_transforms(transforms)
        super().__init__(hr_sheets, lr_sheets, hr_res, lr_scale, overlap, n_frames, slide, val_split, rotation, split_seed, None, names)
        who, nf = type(self).__name__, self.n_frames
        self.depths = (nf[1], nf[0]) if nf is not None else (_uniform_frames(self.hr_sheets, who), _uniform_frames(self.lr_sheets, who))
        self.banks = (_SheetBank(self.hr_sheets, device, who), _SheetBank(self.lr_sheets, device, who))
        self.hr_sheets, self.lr_sheets = self.banks[0].sheets, self.banks[1].sheets

    def draw_pair_items(self, indices, pp=False):
        """(HR table, LR table) for these dataset indices: the training rotations are drawn exactly as ``__getitem__`` would draw them for
        the same sequence of indices, and each draw is written to both tables.  Every window is checked against its sheet here."""
        entries = ([], [])
        for idx in self._row_indices(indices):
            image_idx, _ = _get_image_idx(idx, self.slices, self.tiles)
            rot = self._draw_rotation(idx, pp)
            for side, bank, depth, (sheet, size, stride, frames, n_slices, local, slide) in zip(entries, self.banks, self.depths, self._side_args(idx)):
                origin = _window_origin(sheet, size, stride, frames, n_slices, local, slide)
                bank.check(image_idx, *origin, depth, size)
                side.append((image_idx, *origin, rot))
        return tuple(_window_rows(side).to(bank.device) for side, bank in zip(entries, self.banks))

    def _gather_u8(self, side, table, depth, res):
        return self.banks[side].gather(table, depth, res)
