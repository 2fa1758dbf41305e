"""``predict_images`` with the reference's signature (pssr/predict.py:11-83): batched no-grad forward,
clip + uint8 truncation on the device (csrc/elementwise.hip: pssr_clip_u8), crop, dict or file output; ``predict_collage``
(pssr/predict.py:85-142) with its picture composed in HBM (csrc/collage.hip: pssr_collage_rows_u8); ``predict_sheet``; ``test_metrics``."""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn as nn
from torch.utils.data import DataLoader, Dataset

from . import distributed as D
from . import ops
from .data import _get_n_frames, _slice_center
from .util import _get_callbacks

try:
    from tqdm import tqdm
except ImportError:                                   # pragma: no cover
    def tqdm(it, **kw):
        return it


def _pred_array(data: torch.Tensor, n_frames: int = 1):
    """``np.clip(x, 0, 255).astype(np.uint8)`` (truncation) + centre-frame slice (pssr/predict.py:245-246)."""
    if not data.is_cuda:
        raise RuntimeError("pssr2_amd.predict runs on an MI355X (HIP) device only; there is no CPU fallback")
    x = data.detach().contiguous().float()
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    ops.clip_u8(x, out)
    return _slice_center(out.cpu().numpy(), n_frames)


def _pred_tensor(data: torch.Tensor, n_frames: int = 1):
    """``_pred_array`` that leaves the uint8 result in HBM (for the device-side normalisation and metrics)."""
    if not data.is_cuda:
        raise RuntimeError("pssr2_amd.predict runs on an MI355X (HIP) device only; there is no CPU fallback")
    x = data.detach().contiguous().float()
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    ops.clip_u8(x, out)
    return _slice_center(out, n_frames)


def _check_ensemble(ensemble, device, spread=False):
    """The keyword checks of ``predict_images`` / ``test_metrics``, before model, dataset or device are touched."""
    if ensemble not in ops.ENSEMBLES:
        raise ValueError(f"ensemble must be one of {ops.ENSEMBLES}. Given {ensemble!r}.")
    if spread and ensemble == 1:
        raise ValueError("spread=True compares the members of a self-ensemble: with ensemble=1 there is nothing to compare.")
    if ensemble > 1 and torch.device(device).type != "cuda":
        raise RuntimeError("pssr2_amd.predict runs on an MI355X (HIP) device only; there is no CPU fallback")


def _ensemble_pred(model: nn.Module, lr: torch.Tensor, ensemble: int, batch_size: int, spread: bool = False):
    """The ensembled uint8 prediction of a device batch ``lr`` [n, m, s, s] (uint8 or float32): ``mean`` or ``(mean, spread)``, uint8
    [n, C, S, S] in HBM (include/pssr_mi355.h: ``mean = floor(sum_d q_d / E)``, ``spread = max_d q_d - min_d q_d`` of the quantised members
    turned back).  One ``pssr_dihedral_batch_*`` launch makes the ``n * E`` members, item ``i * E + d = T_d(lr[i])``; one
    ``pssr_ensemble_reduce_u8`` launch reduces their float32 predictions.

    Chunk rule: the members go through the model in sequence order in consecutive chunks of at most ``batch_size`` items,
    ``[0, batch_size), [batch_size, 2 * batch_size), ...``, the last one shorter; a chunk may span images.  A model whose result depends
    on the batch composition (any bf16 model here: the tiling follows the batch) is reproduced bit for bit only with the same chunks."""
    if lr.dim() != 4 or lr.shape[-1] != lr.shape[-2]:
        raise ValueError(f"ensemble > 1 rotates the items, which must be square [n, m, s, s]; got {tuple(lr.shape)}")
    if not lr.is_cuda:
        raise RuntimeError("pssr2_amd.predict runs on an MI355X (HIP) device only; there is no CPU fallback")
    lr = lr.detach().contiguous()
    members = ops.dihedral_batch(lr if lr.dtype == torch.uint8 else lr.float(), ensemble)
    ys = None
    for g0 in range(0, len(members), batch_size):
        y = model(members[g0:g0 + batch_size])
        if y.dim() != 4 or y.shape[-1] != y.shape[-2]:
            raise ValueError(f"ensemble > 1 turns the predictions back, which must be square; the model returned {tuple(y.shape)}")
        if ys is None:
            ys = torch.empty(len(members), *y.shape[1:], dtype=torch.float32, device=y.device)
        ys[g0:g0 + len(y)] = y
    return ops.ensemble_reduce_u8(ys, ensemble, spread)


def _check_consistency(consistency, fit, device):
    """The ``consistency`` / ``fit`` keyword checks of the drivers, before model, dataset or device are touched."""
    if fit not in ops.FITS:
        raise ValueError(f"fit must be one of {ops.FITS}. Given {fit!r}.")
    if consistency and torch.device(device).type != "cuda":
        raise RuntimeError("pssr2_amd.predict runs on an MI355X (HIP) device only; there is no CPU fallback")


def _score_items(lr: torch.Tensor, hat: torch.Tensor, crop_res: int, scale: int, fit: str, rsf: bool = False):
    """``util.consistency_map`` of a device batch for ``predict_images`` / ``test_metrics``: the cropped uint8 predictions ``hat``
    [n, C, H', W'] (not normalised, in HBM) against their LR items ``lr`` [n, m, h, w] cut to ``crop_res // scale`` as the predictions were
    cut to ``crop_res`` (``scale``: the model's).  A float item is quantised as a prediction is (``ops.clip_u8``); the datasets hand out
    integers, for which that is the identity.  ``rsf=True``: ``util.estimate_rsf`` of the same two batches instead."""
    from .util import consistency_map, estimate_rsf
    if scale < 1 or crop_res % scale:
        raise ValueError(f"consistency=True compares the cropped prediction with the LR item cut to crop_res // scale: the crop ({crop_res}) "
                         f"must be a multiple of the model's scale ({scale}).")
    if lr.dtype != torch.uint8:
        x = lr.detach().contiguous().float()
        lr = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
        ops.clip_u8(x, lr)
    cut = crop_res // scale
    if rsf:
        return estimate_rsf(lr[:, :, :cut, :cut].contiguous(), hat.contiguous())
    return consistency_map(lr[:, :, :cut, :cut].contiguous(), hat.contiguous(), fit=fit)


def predict_images(model: nn.Module, dataset: Dataset, device: str = "cpu", batch_size=None, out_dir: str = "preds", norm: bool = False,
                   prefix: str = None, dataloader_kwargs=None, callbacks=None, *, ensemble: int = 1, spread: bool = False,
                   consistency: bool = False, fit: str = "affine"):
    r"""Predicts high-resolution images for ``dataset.val_idx``; returns ``{name: uint8 [C,H,W]}`` when
    ``out_dir`` is None, else writes ``{out_dir}/{prefix_}{name}.tif`` through Pillow.

    ``ensemble=E`` (1, 2, 4 or 8; keyword-only, the reference has none) is ``predict_sheet``'s geometric self-ensemble for tiles: every item
    is also predicted rotated / flipped, the quantised predictions are turned back and their floored integer mean is the prediction
    (``_ensemble_pred``: two launches per batch beside the ``E`` times larger forward pass; ``batch_size`` also bounds the member chunks).
    It takes the ordinary loop (no captured graph), needs square items and a square output, and multiplies the model evaluations by
    ``E``.  ``spread=True`` also gives the per-pixel ``max - min`` of the members, where the network disagrees with itself: written as
    ``{out_dir}/{prefix_}{name}_spread.tif``, or with ``out_dir=None`` returned as a second dict, ``(preds, spreads)``, with the same keys.
    ``norm`` normalises the ensembled prediction (not the spread); the crop applies to both.  The defaults are the call without them.

    ``consistency=True`` (keyword-only; ``fit`` as ``util.consistency_map``) scores every prediction against its own LR item, for which no
    ground truth is needed: the (ensembled) uint8 prediction, cropped but before ``norm``, against the item cut to ``crop // scale`` (a
    crop that the model's scale does not divide is a ``ValueError``).  It takes the ordinary loop as ``ensemble > 1`` does and adds
    ``consistency_map``'s few small launches and its two copies to the host per batch.  The maps are written as ``{out_dir}/{prefix_}{name}_consistency.tif``; with ``out_dir=None`` a dict
    ``name -> Consistency`` (``map`` uint8 [C, h, w] for the [C, H, W] handed out, ``alpha, beta, rse, rsp`` float64 [C]) is appended to the
    returned tuple, after ``spreads`` when both are asked for."""
    _check_ensemble(ensemble, device, spread)
    _check_consistency(consistency, fit, device)
    dataloader_kwargs = {} if dataloader_kwargs is None else dataloader_kwargs
    batch_size = 1 if batch_size is None else batch_size
    if norm and dataset.is_lr:
        raise ValueError("Dataset must be paired with high-low-resolution images for normalization.")
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    callbacks, callback_locals = _get_callbacks(callbacks)
    rank, world = D.rank_world()

    model.to(device)
    model.eval()
    idx = list(dataset.val_idx)
    if world > 1:                                     # contiguous chunk per rank keeps output naming intact
        per = (len(idx) + world - 1) // world
        first = rank * per
        idx = idx[first:first + per]
    else:
        first = 0
    # device-made batches replayed as a hipGraph when the dataset offers them (pssr2_amd/fastpath.py); ``dataset.device_outputs``
    # (an extension of such datasets) keeps the uint8 predictions in HBM: the dict then holds device tensors
    from . import fastpath
    fast = ensemble == 1 and not consistency and fastpath.supports(model, dataset, device) and not dataloader_kwargs and len(idx) > 0
    host_fast = ensemble == 1 and not consistency and not fast and fastpath.supports_host(model, dataset, device) and len(idx) > 0
    keep_dev = bool(getattr(dataset, "device_outputs", False)) and not out_dir and not norm
    compact = False
    if host_fast:
        # host batches (any dataset through a DataLoader): one captured forward over a static input buffer per (dataset, batch size)
        cache = model._engine._eval_steppers
        evaler = cache.get((id(dataset), batch_size, "host"))
        if evaler is None or evaler.dataset is not dataset:
            if len(cache) >= 4:
                cache.pop(next(iter(cache)))
            evaler = cache[(id(dataset), batch_size, "host")] = fastpath.EvalStepper(model, dataset, batch_size, device, to_u8=True, weights_move=False,
                                                                                     host=True)
        evaler.begin()
        # a dataset of this package hands the replay uint8 items (pssr2_amd/data.py: _tensor_ready); taken back when the loop below ends
        compact = getattr(dataset, "compact", None) is False and os.environ.get("PSSR_HOST_COMPACT", "1") != "0"
        if compact:
            dataset.compact = True
        dataloader = DataLoader(dataset, batch_size, sampler=idx, **dataloader_kwargs)
    elif fast:
        # one stepper (and one captured graph) per (dataset, batch size): a second call over the same dataset only replays
        cache = model._engine._eval_steppers
        evaler = cache.get((id(dataset), batch_size))
        if evaler is None or evaler.dataset is not dataset or len(idx) > evaler.cur.table.shape[0]:
            if len(cache) >= 4:           # each stepper pins a captured graph and its memory pool: keep the most recent few
                cache.pop(next(iter(cache)))
            evaler = cache[(id(dataset), batch_size)] = fastpath.EvalStepper(model, dataset, batch_size, device, to_u8=True, weights_move=False)
        dataloader = range(evaler.begin(idx))
    else:
        dataloader = DataLoader(dataset, batch_size, sampler=idx, **dataloader_kwargs)
    outs, spreads, scores, cur_idx = {}, {}, {}, first
    from .train import _restore_compact
    from .util import Consistency
    with torch.no_grad(), _restore_compact(dataset, host_fast and compact):
        for item in tqdm(dataloader, disable=rank != 0):
            if fast or host_fast:
                hr_dev, lr, _, _, u8 = evaler.step() if fast else evaler.step((item,) if dataset.is_lr else tuple(item))
                hr_hat = u8.clone() if keep_dev else _slice_center(u8.cpu().numpy(), 1)      # u8 is the graph's static output buffer
            else:
                lr = item if dataset.is_lr else item[1]
                lr = lr.to(device)
                if ensemble > 1:
                    reduced = _ensemble_pred(model, lr, ensemble, batch_size, spread)
                    hr_hat, dif = reduced if spread else (reduced, None)
                    hat_dev = _slice_center(hr_hat, 1) if consistency else None
                    hr_hat = _slice_center(hr_hat.cpu().numpy(), 1)
                elif consistency:
                    hat_dev = _pred_tensor(model(lr))
                    hr_hat = hat_dev.cpu().numpy()
                else:
                    hr_hat = _pred_array(model(lr))
            if norm:      # pssr/predict.py:63-64: intensities matched to the ground truth of the paired dataset
                from .util import normalize_preds
                _, hr_hat = normalize_preds(_pred_array(hr_dev if (fast or host_fast) else item[0].to(device)), hr_hat)
            crop_res = dataset.crop_res if not dataset.is_lr else dataset.crop_res * (hr_hat.shape[-1] // lr.shape[-1])
            if consistency:       # the prediction as it is handed out, but before norm
                cons = _score_items(lr, hat_dev[:, :, :crop_res, :crop_res], crop_res, hat_dev.shape[-1] // lr.shape[-1], fit)
            hr_hat = hr_hat[:, :, :crop_res, :crop_res]
            if spread:
                dif = _slice_center(dif.cpu().numpy(), 1)[:, :, :crop_res, :crop_res]
            for batch_idx, image_idx in enumerate(range(cur_idx, min(cur_idx + batch_size, first + len(idx)))):
                name = dataset._get_name(image_idx)
                if out_dir:
                    from PIL import Image
                    frames = [Image.fromarray(f) for f in hr_hat[batch_idx]]
                    frames[0].save(f"{out_dir}/{prefix + '_' if prefix else ''}{name}.tif", save_all=len(frames) > 1, append_images=frames[1:])
                    if spread:
                        frames = [Image.fromarray(f) for f in dif[batch_idx]]
                        frames[0].save(f"{out_dir}/{prefix + '_' if prefix else ''}{name}_spread.tif", save_all=len(frames) > 1,
                                       append_images=frames[1:])
                    if consistency:
                        frames = [Image.fromarray(f) for f in cons.map[batch_idx]]
                        frames[0].save(f"{out_dir}/{prefix + '_' if prefix else ''}{name}_consistency.tif", save_all=len(frames) > 1,
                                       append_images=frames[1:])
                else:
                    outs[name] = hr_hat[batch_idx]
                    if spread:
                        spreads[name] = dif[batch_idx]
                    if consistency:
                        scores[name] = Consistency(*(v[batch_idx] for v in cons))
                for i, callback in enumerate(callbacks):
                    callback(locals()) if callback_locals[i] else callback()
            cur_idx += batch_size
    if out_dir is None:
        if consistency:
            return (outs, spreads, scores) if spread else (outs, scores)
        return (outs, spreads) if spread else outs


def _center_crop_view(t: torch.Tensor, rows: int, cols: int):
    """[1, rows', cols'] view of the centre frame ``C // 2`` of a [1, C, H, W] tensor cut to at most ``rows`` x ``cols`` (numpy slicing:
    a smaller image stays as it is), without a copy."""
    return t[:, t.shape[1] // 2, :rows, :cols]


def _collage_row(canvas: torch.Tensor, row: int, lr: torch.Tensor, hr_hat: torch.Tensor, hr, norm: bool, crop_res: int, lr_scale: int):
    """One collage row on the device: ``_collage_preds(lr, hr_hat, hr, norm, 1, crop_res, lr_scale)`` (pssr/predict.py:213-232) written
    into rows ``row * crop_res ...`` of the uint8 device ``canvas``.  ``lr`` / ``hr_hat`` / ``hr`` (None in LR mode): float32 device
    tensors [1, C, H, W].  Centre frame of each, LR cut to ``crop_res // lr_scale`` and prediction / HR to ``crop_res``; with ``norm``
    prediction and HR go through ``normalize_preds`` and LR through ``normalize_preds`` against the normalised HR (all three stay in
    HBM); LR is enlarged to the prediction's size by Pillow's NEAREST map; one ``pssr_collage_rows_u8`` launch places the panels.
    Without ``norm`` that launch reads the float32 tensors directly (clip + truncation as ``_pred_array``)."""
    tensors = [lr, hr_hat] + ([] if hr is None else [hr])
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError("pssr2_amd.predict runs on an MI355X (HIP) device only; there is no CPU fallback")
        if t.dim() != 4 or t.shape[0] != 1:
            raise ValueError(f"_collage_row takes single items [1, C, H, W], got {tuple(t.shape)}")
    views = [_center_crop_view(t.detach().float(), res, res) for t, res in zip(tensors, [crop_res // lr_scale, crop_res, crop_res])]
    h, w = views[1].shape[1:]
    if hr is not None and views[2].shape != views[1].shape:
        raise ValueError(f"Cropped prediction and high-resolution image differ in size ({tuple(views[1].shape[1:])} and "
                         f"{tuple(views[2].shape[1:])}): the model's scale does not match the dataset's lr_scale. (The reference resizes "
                         "and pastes such panels; pssr2_amd does not.)")
    if (h, w) != (crop_res, crop_res):
        raise ValueError(f"The cropped prediction is {h}x{w} but a collage row is crop_res = {crop_res} pixels high and each panel as wide.")
    if norm:
        u8 = []
        for v in views:
            v = v.contiguous()
            out = torch.empty(v.shape, dtype=torch.uint8, device=v.device)
            ops.clip_u8(v, out)
            u8.append(out)
        lr_u8, hat_u8, hr_u8 = u8
        hr_u8, hat_u8 = ops.normalize_preds_u8(hr_u8, hat_u8)
        if lr_u8.shape == hr_u8.shape:
            _, lr_u8 = ops.normalize_preds_u8(hr_u8, lr_u8)
        else:
            _, lr_u8 = ops.normalize_preds_resized_u8(hr_u8, lr_u8)
        views = [lr_u8, hat_u8, hr_u8]
    sh, sw = views[0].shape[1:]
    tables = (None, None) if (sh, sw) == (h, w) else (ops.nearest_table(sh, h, canvas.device), ops.nearest_table(sw, w, canvas.device))
    ops.collage_rows_u8([(views[0], *tables)] + views[1:], canvas, row)


def predict_collage(model: nn.Module, dataset: Dataset, device: str = "cpu", norm: bool = True, n_images: int = None, prefix: str = None,
                    out_dir: str = "preds", callbacks=None):
    r"""Saves ``{out_dir}/{prefix_}collage_{n_images}.png``: vertically stacked rows of the low-resolution input (enlarged, nearest
    neighbour), the prediction and the high-resolution image side by side (pssr/predict.py:85-142: same arguments, order of the
    images, file name and pixel values).  In LR mode there is no high-resolution panel.  Only the centre frame of each item is shown;
    only validation images are used; rows for which no validation item exists stay black.

    Items are predicted one by one as upstream.  Clipping, (``norm``) the two ``normalize_preds`` passes, the nearest-neighbour
    enlargement and the placement of the panels run on the MI355X (csrc/collage.hip); the canvas lives in HBM and comes to the host
    once, to be saved through Pillow as mode ``"L"``.

    Two deviations: upstream's callback loop overwrites the row counter that ends its outer loop, so with callbacks it may stop early
    or late; here the loop ends after ``n_images`` rows whatever the callbacks.  And ``collage`` in the locals a callback receives is
    the uint8 device canvas, not a PIL image.  Panels of different sizes (a model whose scale is not the dataset's ``lr_scale``) raise
    ``ValueError``; upstream pastes them as they are."""
    if norm and dataset.is_lr:
        raise ValueError("Dataset must be paired with high-low-resolution images for normalization.")
    if torch.device(device).type != "cuda":
        raise RuntimeError("pssr2_amd.predict runs on an MI355X (HIP) device only; there is no CPU fallback")
    from .data import _RandomIterIdx
    callbacks, callback_locals = _get_callbacks(callbacks)
    n_images = min(50, len(dataset)) if n_images is None else n_images

    model.to(device)
    model.eval()

    crop_res = dataset.crop_res
    collage = torch.zeros(crop_res * n_images, crop_res * (2 if dataset.is_lr else 3), dtype=torch.uint8, device=device)
    with torch.no_grad():
        # only shuffled if val_split < 1 (pssr/predict.py:119-120)
        order = _RandomIterIdx(dataset.val_idx, seed=True) if len(dataset.val_idx) < len(dataset) else dataset.val_idx
        for idx, data_idx in enumerate(order):
            if idx >= n_images:
                break
            if dataset.is_lr:
                hr, lr = None, dataset[data_idx].to(device).unsqueeze(0)
            else:
                hr, lr = dataset[data_idx]
                hr, lr = hr.to(device).unsqueeze(0), lr.to(device).unsqueeze(0)
            hr_hat = model(lr)
            _collage_row(collage, idx, lr, hr_hat, hr, norm, crop_res, dataset.lr_scale)
            for i, callback in enumerate(callbacks):
                callback(locals()) if callback_locals[i] else callback()

    from PIL import Image
    os.makedirs(out_dir, exist_ok=True)
    Image.fromarray(collage.cpu().numpy()).save(f"{out_dir}/{prefix + '_' if prefix else ''}collage_{n_images}.png")


def _sheet_grid(h: int, w: int, tile: int, stride: int, cover: bool):
    """``(n_rows, n_cols)`` of the windows ``predict_sheet`` cuts: whole windows only (pssr/data.py:629-638), or with ``cover`` the
    smallest grid whose windows reach the bottom and the right edge of the sheet (extended by reflection, so no axis may be 1 long)."""
    if cover:
        if h < 2 or w < 2:
            raise ValueError(f"cover=True extends the sheet by reflection, which an axis of length 1 does not have (sheet {h}x{w})")
        return tuple(-(-max(n - tile, 0) // stride) + 1 for n in (h, w))
    if h < tile or w < tile:
        raise ValueError(f"sheet {h}x{w} is smaller than one tile ({tile})")
    return (h - tile) // stride + 1, (w - tile) // stride + 1


def _slice_plan(frames: int, n_frames, slide: bool):
    """``(m, step, n_slices)``: frame slice ``k`` of a stack of ``frames`` is frames ``[k * step, k * step + m)`` with
    ``m = max(n_frames)`` as in the sheet datasets' LR mode (``frames - m + 1`` slices with ``slide``, else ``frames // m``);
    ``n_frames=-1``: one slice of all frames."""
    n_frames = _get_n_frames(n_frames)
    if n_frames is None:
        return frames, frames, 1
    m = max(n_frames)
    n_slices = frames - m + 1 if slide else frames // m
    if m < 1 or n_slices < 1:
        raise ValueError(f"A stack of {frames} frames holds no slice of n_frames = {m} frames.")
    return m, 1 if slide else m, n_slices


def predict_sheet(model: nn.Module, sheet, tile_res: int = 128, overlap: int = 32, margin: int = 0, batch_size: int = 128,
                  device: str = "cuda", to_numpy: bool = True, *, n_frames=-1, slide: bool = False, cover: bool = False,
                  blend: str = "average", ensemble: int = 1, spread: bool = False, consistency: bool = False, fit: str = "affine"):
    r"""Whole-sheet prediction entirely on the device: what ``predict_images`` on a ``SlidingDataset`` in LR mode
    (pssr/data.py:132-266, pssr/predict.py:11-83) followed by ``reassemble_sheets`` (pssr/util.py:54-137) computes, without
    the per-tile host round trips.  ``sheet``: uint8 array or tensor [C, H, W] (or [H, W]) of the low-resolution image.
    Tiles of ``tile_res`` LR pixels with ``overlap`` are cut on the device, predicted in batches, truncated to uint8
    (``_pred_array``), and stitched with overlap averaging and ``margin`` trimming (in LR pixels times the model's scale,
    as upstream).  Returns uint8 [C_out, H', W'] with H' = (n_rows*(tile_res-overlap)+overlap)*scale.

    ``cover=True`` predicts the whole sheet whatever its size: the tile grid is the smallest that reaches the bottom and the right edge,
    the tiles beyond them read the sheet reflected there (``np.pad(mode="reflect")``, by address arithmetic: no padded copy is made),
    and the result is cut to ``H * scale`` x ``W * scale``.  It equals ``predict_sheet`` of the sheet padded that way on the host, cut;
    ``margin`` trims the inner edges of that extended grid.  A sheet smaller than a tile is fine, an axis of length 1 is not.

    ``n_frames=m`` or ``[lr, hr]`` (with ``slide`` as in the sheet datasets) reads ``sheet`` as a stack [F, H, W] and runs the model on
    every frame slice ``[k * step, k * step + max(n_frames))``: returns uint8 [S, C_out, H', W'], slice ``k`` first.  The tiles of all
    slices form one slice-major sequence cut into batches of ``batch_size`` (a batch may span slices), and one launch stitches them.

    ``blend="linear"`` feathers the overlaps (the reference has only the plain average, whose value jumps wherever the set of covering
    tiles changes): on each axis a tile's weight ramps 1, 2, ... up to ``T = max(overlap * scale - 2 * margin, 0) + 1`` from every inner
    edge (after ``margin`` trimming) and stays ``T`` inside and at the sheet's border; a pixel's weight is the product of the two axes, and
    the result is the floored weighted mean, in integers.  ``ensemble=E`` (1, 2, 4 or 8) is the geometric self-ensemble: every tile is also
    predicted rotated / flipped (member ``d``: ``np.rot90(a[..., ::-1] if d & 4 else a, d & 3)``), each prediction is turned back and the
    ``E`` of them are averaged inside the same integer division.  It multiplies the model evaluations by ``E``; ``batch_size`` then counts
    items (tile x member).  Every combination but ``blend="average", ensemble=1`` (which runs exactly the kernels it always ran) takes
    ``pssr_dihedral_tiles_u8`` / ``pssr_clip_u8_dihedral`` / ``pssr_blend_stack_u8`` and keeps all member predictions in HBM until the one
    stitching launch: ``n_tiles * E * C_out * (tile_res * scale) ** 2`` bytes, about 1 GB for ``ensemble=8`` on a 2048 x 2048 sheet at 4x
    with the default tiles.

    ``spread=True`` returns ``(sheet, spread)``: next to the sheet, which it leaves as it is, a uint8 map of the same shape with the
    ``max - min`` of all predictions of each pixel -- every member of every tile that covers it with a non-zero weight -- from one more
    launch (``pssr_spread_stack_u8``) over the predictions the call already holds, on the plain, covered, stacked and blended paths alike.
    With ``ensemble=1`` and an overlap it shows where neighbouring tiles disagree at the seams; without either it is zero.

    ``consistency=True`` also scores the returned sheet against the low-resolution region it covers, ``sheet[..., :H' // scale, :W' // scale]``
    of each slice's frames (``util.consistency_map`` with ``fit``; no ground truth is needed, and unlike the spread it sees a structure that
    every member invents alike): after whichever stitch ran, one fused reduction + moments launch and one map launch over what the call
    already holds in HBM, one fit per output plane of the whole sheet.  Returns ``(sheet, cons)``, or ``(sheet, spread, cons)`` with
    ``spread=True``; ``cons`` is a ``Consistency`` with ``map`` uint8 [C_out, h', w'] and ``alpha, beta, rse, rsp`` float64 [C_out] ([S, ...]
    for stacks).  A model with more output planes than the slice has frames is a ``ValueError``."""
    if fit not in ops.FITS:
        raise ValueError(f"fit must be one of {ops.FITS}. Given {fit!r}.")
    if blend not in ops.BLENDS:
        raise ValueError(f"blend must be one of {sorted(ops.BLENDS)}. Given {blend!r}.")
    if ensemble not in ops.ENSEMBLES:
        raise ValueError(f"ensemble must be one of {ops.ENSEMBLES}. Given {ensemble!r}.")
    if margin > overlap:
        raise ValueError(f"The value of margin cannot be greater than overlap. Given {margin} and {overlap} respectively.")
    sheet = torch.as_tensor(np.asarray(sheet) if not torch.is_tensor(sheet) else sheet)
    if sheet.dim() == 2:
        sheet = sheet[None]
    if sheet.dtype != torch.uint8:
        raise ValueError("predict_sheet expects a uint8 sheet (the reference's uint8 tif path)")
    sheet = sheet.to(device).contiguous()
    c, h, w = sheet.shape
    stride = tile_res - overlap
    n_rows, n_cols = _sheet_grid(h, w, tile_res, stride, cover)
    m, step, n_slices = _slice_plan(c, n_frames, slide)
    # the plain call keeps the kernels it has always used (pssr_sliding_tiles_u8 / pssr_patch_tiles_u8); stacks and covered sheets take
    # the slice-major, reflecting pair (pssr_stack_tiles_u8 / pssr_patch_stack_u8); a blend or an ensemble takes the dihedral, weighted
    # form of that pair (pssr_dihedral_tiles_u8 / pssr_clip_u8_dihedral / pssr_blend_stack_u8), which subsumes both
    stacked = _get_n_frames(n_frames) is not None
    mixed = blend != "average" or ensemble != 1
    plain = not cover and not stacked and not mixed
    n_items = n_slices * n_rows * n_cols * ensemble
    model.to(device)
    model.eval()
    preds = None
    with torch.no_grad():
        for t0 in range(0, n_items, batch_size):
            nt = min(batch_size, n_items - t0)
            if plain:
                lr = ops.sliding_tiles_u8(sheet, tile_res, stride, t0, nt)
            elif mixed:
                lr = ops.dihedral_tiles_u8(sheet, m, step, tile_res, stride, n_rows, n_cols, ensemble, t0, nt)
            else:
                lr = ops.stack_tiles_u8(sheet, m, step, tile_res, stride, n_rows, n_cols, t0, nt)
            y = model(lr).contiguous().float()
            if preds is None:
                preds = torch.empty(n_items, *y.shape[1:], dtype=torch.uint8, device=y.device)
            if mixed:
                ops.clip_u8_dihedral(y, preds[t0:t0 + nt], ensemble, t0)
            else:
                ops.clip_u8(y, preds[t0:t0 + nt])
    scale = preds.shape[-1] // tile_res
    # upstream passes overlap*lr_scale and the raw margin to _patch_images (pssr/util.py:99)
    if plain:
        out = ops.patch_tiles_u8(preds, n_rows, n_cols, overlap * scale, margin)
    else:
        out_h, out_w = ((h, w) if cover else (n_rows * stride + overlap, n_cols * stride + overlap))
        if mixed:
            out = ops.blend_stack_u8(preds, n_slices, n_rows, n_cols, overlap * scale, margin, out_h * scale, out_w * scale, blend, ensemble)
        else:
            out = ops.patch_stack_u8(preds, n_slices, n_rows, n_cols, overlap * scale, margin, out_h * scale, out_w * scale)
        out = out if stacked else out[0]
    extra = ()
    if consistency:
        from .util import Consistency, consistency_map
        hat = out if stacked else out[None]
        lh, lw = hat.shape[-2] // scale, hat.shape[-1] // scale
        lr = torch.stack([sheet[k * step:k * step + m, :lh, :lw] for k in range(n_slices)])
        cons = consistency_map(lr, hat, fit=fit, to_numpy=to_numpy)
        extra = (cons if stacked else Consistency(*(v[0] for v in cons)),)
    if spread:
        out_h, out_w = ((h, w) if cover else (n_rows * stride + overlap, n_cols * stride + overlap))
        dif = ops.spread_stack_u8(preds, n_slices, n_rows, n_cols, overlap * scale, margin, out_h * scale, out_w * scale, ensemble)
        dif = dif if stacked else dif[0]
        return ((out.cpu().numpy(), dif.cpu().numpy()) if to_numpy else (out, dif)) + extra
    if consistency:
        return (out.cpu().numpy() if to_numpy else out,) + extra
    return out.cpu().numpy() if to_numpy else out


def test_metrics(model: nn.Module, dataset: Dataset, device: str = "cpu", metrics=("mse", "pixel", "psnr", "ssim"), avg: bool = True,
                 norm: bool = True, callbacks=None, *, ensemble: int = 1, fit: str = "affine"):
    r"""Image restoration metrics of predicted vs ground truth images over ``dataset.val_idx`` (pssr/predict.py:144-211): same
    arguments and return value.  Prediction, uint8 cast, (``norm``) intensity normalisation and the per-image statistics all run on
    the MI355X (csrc/metrics.hip): the squared-difference sum is an exact integer and ``ssim`` is scikit-image's
    ``structural_similarity(data_range=255)`` (uniform 7x7 windows, sample covariance, interior mean) evaluated from exact integer
    window sums; only two doubles per image come back to the host.  Like the reference (pssr/predict.py:180) every iteration
    evaluates ``dataset[0]``.

    ``ensemble=E`` (keyword-only) scores ``predict_images(ensemble=E)``'s prediction: the ensembled uint8 image (``_ensemble_pred``, its
    ``E`` members in one chunk) takes the place of the quantised model output, everything after it is the same.

    ``metrics`` may also name ``"rse"`` and ``"rsp"`` (not in the default tuple): the two summary numbers of ``util.consistency_map``
    (with ``fit``) of the cropped prediction, before ``norm``, against the item's own LR side -- the resolution-scaled error in grey
    levels and the Pearson correlation, which need no ground truth -- per image the mean over its planes.

    ``metrics`` may name ``"frc"`` too (not in the default tuple either): the resolution that the prediction reached, in HR pixels --
    ``util.frc`` with its defaults (one block per plane, Hann window, the 1/7 threshold) of the cropped uint8 prediction, before ``norm``,
    against the cropped ground truth, the image's planes pooled.  A call that does not name it launches what it launched before.

    ``"rsf"`` (not in the default tuple either) reports how much sharper the prediction is than the optics behind its LR side: the width
    ``sigma``, in HR pixels, of the Gaussian resolution-scaling function that ``util.estimate_rsf`` (default candidates, one choice per image)
    finds between the cropped uint8 prediction, before ``norm``, and the item's own LR side, cut as for ``"rse"``.  No ground truth is needed.

    ``"decorr"`` (not in the default tuple either) is the resolution of the prediction alone, in HR pixels: ``util.decorr`` with its defaults
    (one block per plane, Hann window, ten high-pass filters, the image's planes pooled) of the cropped uint8 prediction, before ``norm``.
    Unlike ``"frc"`` it does not look at the ground truth: it measures the detail the prediction holds, not its agreement with anything.

    ``"frc_x"``, ``"frc_y"``, ``"decorr_x"`` and ``"decorr_y"`` (none in the default tuple) are the directional forms of those two:
    ``util.frc_sectors`` and ``util.decorr_sectors`` with ``sectors=2`` and otherwise their defaults, on the same images; ``_x`` is sector 0,
    the resolution of detail along a scan line, ``_y`` sector 1, the resolution from line to line.  One sums call per method and item,
    however many of the four are named."""
    import math
    from .util import pixel_metric
    _check_ensemble(ensemble, device)
    _check_consistency(False, fit, device)
    callbacks, callback_locals = _get_callbacks(callbacks)
    image_range = 255
    metrics = [metrics] if type(metrics) is str else list(metrics)
    out = {m: [] for m in metrics}
    sectored = [m for m in ("frc", "decorr") if f"{m}_x" in out or f"{m}_y" in out]
    if ("frc" in out or "rsf" in out or "decorr" in out or sectored) and torch.device(device).type != "cuda":                   # as _check_ensemble: before model, dataset or device are touched
        raise RuntimeError("pssr2_amd.predict runs on an MI355X (HIP) device only; there is no CPU fallback")
    model.to(device)
    model.eval()

    with torch.no_grad():
        for _ in tqdm(dataset.val_idx):
            hr, lr = dataset[0]
            hr, lr = hr.to(device).unsqueeze(0), lr.to(device).unsqueeze(0)
            if ensemble > 1:
                hr_hat = _ensemble_pred(model, lr, ensemble, ensemble)
                hr_dev, hat_dev = _pred_tensor(hr), _slice_center(hr_hat, 1)
            else:
                hr_hat = model(lr)
                hr_dev, hat_dev = _pred_tensor(hr), _pred_tensor(hr_hat)
            crop_res = dataset.crop_res if not dataset.is_lr else dataset.crop_res * (hr_hat.shape[-1] // lr.shape[-1])
            hr_dev, hat_dev = hr_dev[:, :, :crop_res, :crop_res].contiguous(), hat_dev[:, :, :crop_res, :crop_res].contiguous()
            if "rse" in out or "rsp" in out:
                cons = _score_items(lr, hat_dev, crop_res, hr_hat.shape[-1] // lr.shape[-1], fit)
                for name in ("rse", "rsp"):
                    if name in out:
                        out[name].extend(sum(v.tolist()) / len(v) for v in getattr(cons, name))
            if "frc" in out:
                from .util import frc
                out["frc"].extend(frc(hat_dev, hr_dev).resolution.tolist())
            if "decorr" in out:
                from .util import decorr
                out["decorr"].extend(decorr(hat_dev).resolution.tolist())
            for method in sectored:
                from . import util
                res = (util.frc_sectors(hat_dev, hr_dev) if method == "frc" else util.decorr_sectors(hat_dev)).resolution
                for s, axis in enumerate("xy"):
                    if f"{method}_{axis}" in out:
                        out[f"{method}_{axis}"].extend(res[:, s].tolist())
            if "rsf" in out:
                out["rsf"].extend(_score_items(lr, hat_dev, crop_res, hr_hat.shape[-1] // lr.shape[-1], fit, rsf=True).sigma.tolist())
            if norm:
                hr_dev, hat_dev = ops.normalize_preds_u8(hr_dev, hat_dev)
            n, c, h, w = hr_dev.shape
            if "ssim" in out and c > 1:
                raise ValueError("ssim: multi-channel images form a volume thinner than the 7x7x7 window (scikit-image raises here too)")
            stats = ops.image_metrics_u8(hr_dev, hat_dev).reshape(n, c, 2).cpu()
            for i in range(n):
                err = float(stats[i, :, 0].sum()) / (c * h * w)           # mean squared error at uint8 scale (exact sum)
                mse = err / image_range ** 2
                if "mse" in out:
                    out["mse"].append(mse)
                if "pixel" in out:
                    out["pixel"].append(pixel_metric(mse, image_range))
                if "psnr" in out:
                    out["psnr"].append(10 * math.log10(image_range ** 2 / err) if err > 0 else float("inf"))
                if "ssim" in out:
                    out["ssim"].append(float(stats[i, 0, 1]))
            if any(callback_locals):
                hr, hr_hat = hr_dev.cpu().numpy(), hat_dev.cpu().numpy()       # the arrays the reference's callbacks see
            for i, callback in enumerate(callbacks):
                callback(locals()) if callback_locals[i] else callback()
    return {m: (sum(v) / len(v) if avg else v) for m, v in out.items()}


test_metrics.__test__ = False      # a library function, not a pytest test (the reference's conftest deselects it the same way)
