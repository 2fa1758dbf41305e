"""``train_paired`` with the reference's signature, return value and loop semantics
(pssr/train.py:19-166), running the model / loss / optimizer kernels of libpssr_mi355.so.

Additions with no reference counterpart (documented in DESIGN.md): when ``torch.distributed`` is
initialised the training indices are sharded per rank with a rank-identical shuffle, gradients are
mean-all-reduced (overlapped with backward through ``Engine.attach_reducer``), validation loss is
averaged over ranks, and only rank 0 writes checkpoints / collages.
"""
from __future__ import annotations

import os
import random

import torch
import torch.nn as nn
from torch.utils.data import DataLoader, Dataset

from . import distributed as D
from .data import _invert_idx, _RandomIterIdx
from .util import _get_callbacks, _psnr_metric, pixel_metric

try:
    from tqdm import tqdm
except ImportError:                                   # pragma: no cover
    def tqdm(it, **kw):
        return it


def _metric_ssim(hr_hat, hr, image_range):
    from .util import ssim
    try:
        return float(ssim(hr_hat.detach(), hr, data_range=image_range))
    except Exception:
        return float("nan")


def _collage(lr, hr_hat, hr, crop_res, lr_scale):
    """Small PIL collage of (LR | prediction | HR) rows for ``collage_dir`` (pssr/train.py:155-158, 316-318).  A prediction smaller
    than HR (train_crappifier's LR-sized ``lr_hat``) is enlarged to HR size by nearest neighbour, as pssr/predict.py:227-230 does."""
    import numpy as np
    from PIL import Image
    rows = []
    for i in range(min(len(lr), 4)):
        up = np.kron(np.clip(lr[i, lr.shape[1] // 2].numpy(), 0, 255), np.ones((lr_scale, lr_scale)))
        pred = np.clip(hr_hat[i, hr_hat.shape[1] // 2].numpy(), 0, 255)
        if pred.shape != tuple(hr.shape[-2:]):
            ry, rx = hr.shape[-2] // pred.shape[0], hr.shape[-1] // pred.shape[1]
            pred = np.kron(pred, np.ones((ry, rx)))
        tiles = [up, pred, np.clip(hr[i, hr.shape[1] // 2].numpy(), 0, 255)]
        rows.append(np.concatenate([t[:crop_res, :crop_res] for t in tiles], axis=1))
    return Image.fromarray(np.concatenate(rows, axis=0).astype(np.uint8))


class _restore_compact:
    """Takes the dataset out of compact (uint8 item) mode when the driver leaves, however it leaves."""

    def __init__(self, dataset, active):
        self.dataset, self.active = dataset, active

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self.active:
            self.dataset.compact = False
        return False


def train_paired(model: nn.Module, dataset: Dataset, batch_size: int, loss_fn: nn.Module, optim: torch.optim.Optimizer, epochs: int,
                 device: str = "cpu", scheduler=None, log_frequency: int = 50, checkpoint_dir: str = None, collage_dir: str = None,
                 clamp: bool = False, dataloader_kwargs=None, callbacks=None):
    r"""Trains ``model`` on paired high-/low-resolution data; returns ``(train_losses, val_losses)``."""
    dataloader_kwargs = {} if dataloader_kwargs is None else dataloader_kwargs
    callbacks, callback_locals = _get_callbacks(callbacks)
    image_range = 255
    rank, world = D.rank_world()

    train_idx = _invert_idx(dataset.val_idx, len(dataset))
    train_sampler = _RandomIterIdx(train_idx, rank=rank, world=world, shuffle_seed=0 if world > 1 else None)
    val_sampler = _RandomIterIdx(dataset.val_idx, seed=True, rank=rank, world=world)
    include_metric = type(scheduler) == torch.optim.lr_scheduler.ReduceLROnPlateau

    model.to(device)
    engine = getattr(model, "_engine", None)
    # hipGraph replay of whole steps when the dataset makes its batches on the device (pssr2_amd/fastpath.py); everything else
    # (host datasets, DataLoader workers, user crappifier subclasses, ``extra`` losses) takes the reference's loop below
    from . import fastpath
    fast = fastpath.supports(model, dataset, device) and not dataloader_kwargs
    # host datasets (the reference's own ImageDataset / SlidingDataset through a DataLoader, workers and all): the same replay over
    # static input buffers, fed by one asynchronous host-to-device copy per batch
    host_fast = not fast and fastpath.supports_host(model, dataset, device)
    # a dataset of this package feeding the replay hands over uint8 items (every value is an integer in [0, 255]); the feed converts on the
    # device.  The flag travels to the DataLoader workers with the dataset and is taken back when the driver returns
    compact = host_fast and getattr(dataset, "compact", None) is False and os.environ.get("PSSR_HOST_COMPACT", "1") != "0"
    if compact:
        dataset.compact = True
    if fast:
        train_dataloader = val_dataloader = None
    else:
        train_dataloader = DataLoader(dataset, batch_size, sampler=train_sampler, **dataloader_kwargs)
        val_dataloader = DataLoader(dataset, batch_size, sampler=val_sampler, **dataloader_kwargs)
    if world > 1:
        D.broadcast_module(model)
        if engine is not None and engine.reducer is None and not fast and not host_fast:
            engine.attach_reducer()

    # fp16 storage (model.compute_dtype = torch.float16) needs loss scaling; f32 / bf16 do not
    scaler = None
    if getattr(model, "compute_dtype", None) == torch.float16:
        from .optim import LossScaler
        scaler = LossScaler()

    # one optimizer arithmetic however the steps are issued: the replay keeps FusedAdamW's step count and rate on the device (the bias
    # correction then comes from the device's powf, which differs from the host's in the last place for some step counts); the loop
    # below does the same, so that PSSR_GRAPH=0 gives the replay's bits
    from .optim import FusedAdamW
    if isinstance(optim, FusedAdamW) and torch.device(device).type == "cuda":
        optim.device_state = True

    stepper = evaler = None
    if fast:
        stepper = fastpath.TrainStepper(model, dataset, batch_size, loss_fn, optim, clamp, image_range, scaler, len(train_sampler), device)
        evaler = fastpath.EvalStepper(model, dataset, batch_size, device, loss_fn=loss_fn, clamp=clamp, image_range=image_range)
    elif host_fast:
        stepper = fastpath.TrainStepper(model, dataset, batch_size, loss_fn, optim, clamp, image_range, scaler, 0, device, host=True)
        evaler = fastpath.EvalStepper(model, dataset, batch_size, device, loss_fn=loss_fn, clamp=clamp, image_range=image_range, host=True)

    train_losses, val_losses = [], []
    # world > 1: an exception on one rank (a callback's, say) ends every rank within seconds (pssr2_amd/distributed.py: failure_watch)
    with _restore_compact(dataset, compact), D.failure_watch("train_paired"):
        for epoch in range(epochs):
            model.train()
            if rank == 0:
                print(f"Epoch {epoch}:")
            if fast:
                progress = tqdm(range(stepper.begin_epoch(list(train_sampler))), disable=rank != 0)
            else:
                progress = tqdm(train_dataloader, disable=rank != 0)
            for batch_idx, data in enumerate(progress):
                if fast:
                    hr, lr, hr_hat, loss = stepper.step()
                elif host_fast:
                    hr, lr, hr_hat, loss = stepper.step(data)
                else:
                    if dataset.extra_hr_files is None:
                        hr, lr = data
                    else:
                        (hr, lr), extra = data
                        extra = extra.to(device)
                    hr, lr = hr.to(device), lr.to(device)

                    hr_hat = model(lr)
                    if clamp:
                        hr_hat = torch.clamp(hr_hat, 0, image_range)
                    loss = loss_fn(hr_hat / image_range, hr / image_range) if dataset.extra_hr_files is None \
                        else loss_fn(hr_hat / image_range, hr / image_range, extra / image_range)
                    (scaler.scale(loss) if scaler is not None else loss).backward()
                    if world > 1 and engine is None:
                        D.allreduce_mean_([p.grad for p in model.parameters() if p.grad is not None])
                    if scaler is not None:
                        scaler.step(optim, list(model.parameters()))
                    else:
                        optim.step()
                    optim.zero_grad()

                if batch_idx % log_frequency == 0 or batch_idx == len(progress) - 1:
                    train_losses.append(loss.item())
                    mse = nn.functional.mse_loss(hr_hat.detach() / image_range, hr / image_range)
                    if rank == 0 and hasattr(progress, "set_description"):
                        progress.set_description(f"pixel[{pixel_metric(mse.item(), image_range):.2f}], psnr[{_psnr_metric(mse):.2f}], "
                                                 f"ssim[{_metric_ssim(hr_hat, hr, image_range):.3f}]")
                if batch_idx == max(len(progress), 2) - 2:
                    last_full = [lr.cpu(), hr_hat.detach().cpu(), hr.cpu()]       # accessible from callbacks via locals
                for idx, callback in enumerate(callbacks):
                    callback(locals()) if callback_locals[idx] else callback()
            if fast or host_fast:
                stepper.finish()

            model.eval()
            if rank == 0:
                print(f"Epoch {epoch} validation...")
            val_loss = []
            if fast:
                progress = tqdm(range(evaler.begin(list(val_sampler))), disable=rank != 0)
            else:
                if host_fast:
                    evaler.begin()
                progress = tqdm(val_dataloader, disable=rank != 0)
            with torch.no_grad():
                for batch_idx, data in enumerate(progress):
                    if fast:
                        hr, lr, hr_hat, loss, _ = evaler.step()
                    elif host_fast:
                        hr, lr, hr_hat, loss, _ = evaler.step(tuple(data))
                    else:
                        if dataset.extra_hr_files is None:
                            hr, lr = data
                        else:
                            (hr, lr), extra = data
                            extra = extra.to(device)
                        hr, lr = hr.to(device), lr.to(device)
                        hr_hat = model(lr)
                        if clamp:
                            hr_hat = torch.clamp(hr_hat, 0, image_range)
                        loss = loss_fn(hr_hat / image_range, hr / image_range) if dataset.extra_hr_files is None \
                            else loss_fn(hr_hat / image_range, hr / image_range, extra / image_range)
                        val_loss.append(loss.detach().float().reshape(1))            # stays on device: one sync per epoch
                    if batch_idx == max(len(progress), 2) - 2:
                        last_full_val = [lr.cpu(), hr_hat.cpu(), hr.cpu()]
            if fast or host_fast:
                stat = evaler.mean_loss_stat()
                engine.mark_weights_changed()
            else:
                stat = torch.stack([torch.cat(val_loss).sum(), torch.tensor(float(len(val_loss)), device=val_loss[0].device)]) \
                    if val_loss else torch.zeros(2, device=device)
            if world > 1:
                torch.distributed.all_reduce(stat)
            val_loss = (stat[0] / stat[1].clamp(min=1)).item()
            val_losses.append(val_loss)
            if rank == 0:
                print(f"Epoch {epoch} validation loss: {val_loss:4f}\n")

            if checkpoint_dir and epoch < epochs - 1 and rank == 0:
                os.makedirs(checkpoint_dir, exist_ok=True)
                torch.save(model.state_dict(), f"{checkpoint_dir}/checkpoint{epoch}_{model.__class__.__name__}_{val_loss:.4f}.pth")
            if collage_dir and rank == 0:
                os.makedirs(collage_dir, exist_ok=True)
                _collage(*last_full_val, crop_res=dataset.crop_res, lr_scale=dataset.lr_scale).save(f"{collage_dir}/epoch{epoch}_loss{val_loss:.4f}.png")
            if scheduler:
                scheduler.step(val_loss) if include_metric else scheduler.step()
                if hasattr(optim, "sync_device_lr"):
                    optim.sync_device_lr()

    return train_losses, val_losses


def _crappifier_loss(lr, lr_hat, ds_hr, hist_fn, ssim_loss, clamp: bool = False):
    """pssr/train.py:388-402 on the device: ``mse(hist_fn(lr_hat - ds_hr), hist_fn(lr - ds_hr)) / W_lr**2 * ssim_loss(lr_hat - ds_hr,
    lr - ds_hr)`` as one autograd node (util._CrappifierLossFunction).  ``clamp``: ``lr_hat`` is clamped to [0, 255] on load, which is
    what pssr/train.py:238-239 does before the call."""
    from .models import GradHist
    from .util import SSIMLoss, _CrappifierLossFunction
    if not isinstance(hist_fn, GradHist) or not isinstance(ssim_loss, SSIMLoss):
        raise TypeError("the device crappifier loss takes a pssr2_amd GradHist and a pssr2_amd SSIMLoss")
    hist_cfg = (hist_fn.bins, hist_fn.range[0], hist_fn.range[1], float(hist_fn.sigma))
    ssim_cfg = (ssim_loss.win, float(ssim_loss.mix), bool(ssim_loss.ms), ssim_loss.K[0], ssim_loss.K[1], 1.0, ssim_loss.weights)
    return _CrappifierLossFunction.apply(lr, lr_hat, ds_hr, hist_cfg, ssim_cfg, bool(clamp))


def _clip_grad_value(model, clip):
    """nn.utils.clip_grad_value_(model.parameters(), clip) (pssr/train.py:243-244).  A pssr2_amd model keeps every gradient in its
    engine's flat buffer: one pssr_clamp_f32 launch over it (its alignment padding holds zeros, which stay zeros)."""
    from . import ops
    engine = getattr(model, "_engine", None)
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    if not grads:
        return
    flat = engine._flat_grad if engine is not None else None
    if flat is not None and len(grads) == len(engine._gviews) and all(g.data_ptr() == v.data_ptr() for g, v in zip(grads, engine._gviews)):
        ops.clamp_f32(flat, -clip, clip, out=flat)
    elif engine is not None:
        for g in grads:
            ops.clamp_f32(g, -clip, clip, out=g)
    else:                                               # a foreign nn.Module
        nn.utils.clip_grad_value_(model.parameters(), clip)


def train_crappifier(model: nn.Module, dataset: Dataset, batch_size: int, optim: torch.optim.Optimizer, epochs: int, sigma: int = 5,
                     clip: float = 3, device: str = "cpu", scheduler=None, log_frequency: int = 50, checkpoint_dir: str = None,
                     collage_dir: str = None, clamp: bool = False, dataloader_kwargs=None, callbacks=None):
    r"""EXPERIMENTAL, NOT CURRENTLY RECOMMENDED FOR MOST WORKFLOWS!

    Trains an :class:`nn.Module` model as a crappifier on high-low-resolution paired data (pssr/train.py:168-322).
    The model must output an image the same size as the input/have a `scale` value of 1.
    This is not necessary if you are using a :class:`Crappifier` instance as your crappifier.

    Same arguments, defaults and return value ``(train_losses, val_losses)`` as the reference; ``callbacks`` (documented and read
    by the reference's body, missing from its signature) is the trailing keyword.  The loss (GradHist distance x SSIM of the noise
    profiles) runs as HIP kernels (util._CrappifierLossFunction), the strided subsample ``hr[:, :, ::s, ::s]`` and the gradient
    clipping too.  A pssr2_amd model must have ``scale == 1`` (``ValueError`` before the first step) and an f32 or bf16
    ``compute_dtype``; fp16 storage (which needs a loss scaler) and multi-process runs raise ``NotImplementedError``.
    """
    from . import ops
    from .models import GradHist
    from .util import SSIMLoss
    rec = getattr(model, "reconstruction", None)
    if rec is not None and getattr(rec, "scale", 1) != 1:
        raise ValueError(f"train_crappifier needs a model with scale 1 (its output has the input's size); got scale={rec.scale}")
    if getattr(model, "compute_dtype", None) == torch.float16:
        raise NotImplementedError("train_crappifier with fp16 storage needs a loss scaler, which this driver does not have; "
                                  "use compute_dtype torch.float32 or torch.bfloat16")
    rank, world = D.rank_world()
    if world > 1:
        raise NotImplementedError("train_crappifier runs on one process; multi-GPU training of a crappifier is not implemented")
    dataloader_kwargs = {} if dataloader_kwargs is None else dataloader_kwargs
    callbacks, callback_locals = _get_callbacks(callbacks)
    image_range = 255

    train_dataloader = DataLoader(dataset, batch_size, sampler=_RandomIterIdx(_invert_idx(dataset.val_idx, len(dataset))), **dataloader_kwargs)
    val_dataloader = DataLoader(dataset, batch_size, sampler=_RandomIterIdx(dataset.val_idx, seed=True), **dataloader_kwargs)
    include_metric = type(scheduler) == torch.optim.lr_scheduler.ReduceLROnPlateau

    model.to(device)

    hist_fn = GradHist(sigma=sigma)
    ssim_loss = SSIMLoss(ms=False)

    def _subsample(hr, lr):
        scale = int(hr.shape[-1] / lr.shape[-1])
        hr = hr.to(device).float().contiguous()
        if not hr.is_cuda:
            raise RuntimeError("pssr2_amd.train_crappifier runs on an MI355X (HIP) device only; there is no CPU fallback")
        return ops.subsample(hr, scale)

    def _clamped(t):
        return ops.clamp_f32(t.detach().contiguous(), 0, image_range) if clamp else t

    train_losses, val_losses = [], []
    for epoch in range(epochs):
        model.train()
        print(f"Epoch {epoch}:")

        progress = tqdm(train_dataloader)
        for batch_idx, (hr, lr) in enumerate(progress):
            ds_hr = _subsample(hr, lr)

            lr_hat = model(ds_hr)
            loss = _crappifier_loss(lr.to(device), lr_hat, ds_hr, hist_fn, ssim_loss, clamp=clamp)
            loss.backward()

            if clip is not None and clip > 0:
                _clip_grad_value(model, clip)

            optim.step()
            optim.zero_grad()

            if batch_idx % log_frequency == 0 or batch_idx == len(progress) - 1:
                train_losses.append(loss.item())
                if hasattr(progress, "set_description"):
                    progress.set_description(f"loss[{loss.item():.4f}]")

            if batch_idx == max(len(progress), 2) - 2:
                last_full = [lr.cpu(), _clamped(lr_hat).detach().cpu(), hr.cpu()]      # accessible from callbacks via locals

            for idx, callback in enumerate(callbacks):
                callback(locals()) if callback_locals[idx] else callback()

        model.eval()
        print(f"Epoch {epoch} validation...")

        val_loss = []
        progress = tqdm(val_dataloader)
        with torch.no_grad():
            for batch_idx, (hr, lr) in enumerate(progress):
                ds_hr = _subsample(hr, lr)
                lr_hat = model(ds_hr)
                loss = _crappifier_loss(lr.to(device), lr_hat, ds_hr, hist_fn, ssim_loss, clamp=clamp)
                val_loss.append(loss.detach().reshape(1))            # stays on the device: one sync per epoch

                if batch_idx == max(len(progress), 2) - 2:
                    last_full_val = [lr.cpu(), _clamped(lr_hat).cpu(), hr.cpu()]

        val_loss = [float(v) for v in torch.cat(val_loss).cpu()]
        val_loss = sum(val_loss) / len(val_loss)
        val_losses.append(val_loss)
        print(f"Epoch {epoch} validation loss: {val_loss:4f}\n")

        if checkpoint_dir and epoch < epochs - 1:
            os.makedirs(checkpoint_dir, exist_ok=True)
            torch.save(model.state_dict(), f"{checkpoint_dir}/checkpoint{epoch}_{model.__class__.__name__}_{val_loss:.4f}.pth")

        if collage_dir:
            collage = _collage(*last_full_val, crop_res=dataset.crop_res, lr_scale=dataset.lr_scale)
            os.makedirs(collage_dir, exist_ok=True)
            collage.save(f"{collage_dir}/epoch{epoch}_loss{val_loss:.4f}.png")

        if scheduler:
            scheduler.step(val_loss) if include_metric else scheduler.step()
            if hasattr(optim, "sync_device_lr"):
                optim.sync_device_lr()

    return train_losses, val_losses


def _crappify_unrounded(x, crappifier, seed, tile_offset):
    """``crappifier.crappify`` on the device for float32 tiles [n, C, h, w], as the objective calls it (pssr/train.py:368): no rounding
    and no final clip to [0, 255] (kernel flags 0); a ``MultiCrappifier(clip=True)`` clips after each of its stages, as its ``crappify``
    does.  Tile ``i`` draws from the Philox stream (seed, tile_offset + i)."""
    from . import ops
    from .data import DevicePairGenerator
    spec = crappifier.device_spec()             # NotImplementedError for a subclass without a device path
    stage = DevicePairGenerator(crappifier=None)._stage
    if not isinstance(spec, list):
        return stage(x, spec, seed, tile_offset, 0)
    flags = ops.CLIP if spec[0][0] == "clip" else 0
    for i, st in enumerate(spec[1:]):
        if isinstance(st, list):
            raise NotImplementedError("nested MultiCrappifier has no MI355X device path")
        x = stage(x, st, seed + 7919 * i, tile_offset, flags)
    return x


class _Crappifier_Objective:
    """The noise-profile objective of ``approximate_crappifier`` (pssr/train.py:348-386) on the device.

    Once, at construction: every pair goes to HBM as uint8 (a ``DevicePairedTileDataset`` / ``DevicePairedSlidingDataset`` is gathered
    in place; any other paired dataset is read item by item), HR is reduced to the LR size by the Pillow-exact kernel, and the histogram and sum of the real
    profile ``lr - ds_hr`` are taken per pair -- none of this depends on the parameters, while the reference redoes it on every call.
    Per ``sample(params)``: the reference's ``random.shuffle`` of the indices and its first ``n_samples``; ``crappifier(*params)`` run
    through its device path (Philox seed ``seed``, tile offset advancing by ``n_samples`` per call); one profile launch over
    ``lr_hat``; the loss kernels; one float64 comes back.

    Deviations: items are materialised without the training rotation (the statistic is invariant under a joint rot90 / flip of the
    pair but for the rounding of the reduction); the noise is the device generator's, so values agree with the reference
    statistically, not bit for bit; the two means are taken in float64 (float32 upstream)."""

    def __init__(self, crappifier, dataset, n_samples, device="cuda", seed=0):
        from . import ops
        from .data import DevicePairedSlidingDataset, DevicePairedTileDataset
        if torch.device(device).type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("pssr2_amd.approximate_crappifier runs on an MI355X (HIP) device only; there is no CPU fallback")
        if getattr(dataset, "is_lr", False):
            raise ValueError("Dataset must be paired with high-low-resolution images.")
        self.crappifier, self.dataset, self.n_samples, self.seed = crappifier, dataset, n_samples, int(seed)
        self.calls = 0
        n = len(dataset)
        if n == 0 or n_samples <= 0:
            raise ValueError("approximate_crappifier needs at least one pair")
        if isinstance(dataset, (DevicePairedTileDataset, DevicePairedSlidingDataset)):
            hr, lr = dataset.device_pair_batch(dataset.draw_pair_items(range(n), pp=True), u8=True)
            hr, lr = hr.to(device), lr.to(device)
        else:
            hr, lr = self._read_items(dataset, device)
        if hr.shape[1] != lr.shape[1]:
            raise ValueError(f"the objective compares equal stacks: HR items have {hr.shape[1]} frames, LR items {lr.shape[1]}")
        self.lr_shape = tuple(lr.shape[1:])
        self.ds_hr = ops.bilinear_down_u8(hr.contiguous(), lr.shape[-2], lr.shape[-1])          # pssr/train.py:365
        self.target_hist, self.target_sum = ops.noise_profile(lr.contiguous(), self.ds_hr)       # pssr/train.py:373, 377, 382
        self.per_image = self.ds_hr[0].numel()

    @staticmethod
    def _read_items(dataset, device):
        rotation = getattr(dataset, "rotation", None)
        if rotation:
            dataset.rotation = False
        try:
            sides = ([], [])
            for i in range(len(dataset)):
                for side, item in zip(sides, dataset[i]):
                    item = torch.as_tensor(item)
                    if item.dtype != torch.uint8:
                        u8 = item.to(torch.uint8)
                        if not torch.equal(u8.to(item.dtype), item):          # NaN, fractions and values outside [0, 255] all fail
                            raise ValueError(f"item {i} of the dataset holds values that are not integers in [0, 255]; the objective "
                                             "works on uint8 images")
                        item = u8
                    side.append(item.cpu())
        finally:
            if rotation:
                dataset.rotation = rotation
        return torch.stack(sides[0]).to(device), torch.stack(sides[1]).to(device)

    def sample(self, params):
        from . import ops
        sample_idx = list(range(len(self.dataset)))
        random.shuffle(sample_idx)
        idx = torch.tensor(sample_idx[:self.n_samples], device=self.ds_hr.device)
        ds_hr = self.ds_hr.index_select(0, idx)
        lr_hat = _crappify_unrounded(ops.u8_to_f32(ds_hr), self.crappifier(*params), self.seed, self.calls * self.n_samples)
        self.calls += 1
        pred_hist, pred_sum = ops.noise_profile(lr_hat, ds_hr)
        _, mean = ops.noise_profile_loss(pred_hist, pred_sum, self.target_hist.index_select(0, idx), self.target_sum.index_select(0, idx),
                                         self.per_image, self.lr_shape[-1])
        return float(mean.item())


def approximate_crappifier(crappifier, space, dataset: Dataset, max_images=None, opt_kwargs=None, *, device: str = "cuda", seed: int = 0,
                           minimizer=None):
    r"""Approximates :class:`Crappifier` parameters from ground truth paired images by Bayesian optimisation of a noise-profile
    objective (pssr/train.py:324-346): same arguments and return value (the optimiser's result: ``x``, ``fun``, ``x_iters``,
    ``func_vals``).  ``crappifier`` is a class or any callable that builds a :class:`Crappifier` from ``*params``; it needs a device
    path (``device_spec``), and the objective runs on the MI355X (:class:`_Crappifier_Objective`).

    Keyword-only additions: ``device``; ``seed`` of the device noise generator; ``minimizer`` (a callable with ``gp_minimize``'s
    interface).  Without it ``skopt.gp_minimize`` is used when scikit-optimize is installed, else ``pssr2_amd.bayes.gp_minimize``.
    """
    space = [space] if type(space) is not list else space
    n_samples = len(dataset) if max_images is None else min(max_images, len(dataset))
    opt_kwargs = {} if opt_kwargs is None else opt_kwargs
    if minimizer is None:
        try:
            from skopt import gp_minimize as minimizer
        except ImportError:
            from .bayes import gp_minimize as minimizer
    objective = _Crappifier_Objective(crappifier, dataset, n_samples, device=device, seed=seed).sample
    return minimizer(objective, space, **opt_kwargs)
