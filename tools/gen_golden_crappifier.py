"""Write tests/golden/crappifier.npz from the GENUINE reference (runs only where the reference checkout exists).

TEST INFRASTRUCTURE ONLY, like oracle/gen_golden.py, whose ``import_reference`` it uses (absent third-party modules stubbed).  Records:

* ``GradHist`` (pssr/models/_blocks.py:94-112) outputs and input gradients (autograd, fixed upstream gradient) for the default
  configuration (512 bins, range +-256, sigma 5) and a wide one (64 bins, +-32, sigma 0.5), on inputs that include values outside the
  range, and a 3-channel case.  The reference's forward sizes its padding rows by H*W (``np.prod(x.shape[2:])``), which only
  matches its flattened C*H*W for C = 1; the 3-channel histogram is therefore taken of the same values viewed as [B, 1, C*H, W],
  which is the per-image histogram over all channels the kernels compute;
* ``pssr.train._crappifier_loss`` value and d/d lr_hat (plain, and with lr_hat clamped to [0, 255] first as pssr/train.py:238 does),
  with ``ssim_loss`` a shim over ``oracle.loss_ref.ssim_loss(..., ms=False)`` (pytorch_msssim is absent);
* a 2-epoch ``pssr.train.train_crappifier`` trace (``ResUNet(hidden=[8, 16], depth=1, scale=1)``, AdamW, an in-memory paired dataset
  of 64^2 HR / 16^2 LR, fixed seeds, learning rate ``TRACE_LR``, ``SSIMLoss`` patched to the same shim): ``train_losses``, ``val_losses``, ``sd0/*``, ``sd1/*``.
  The reference's body reads a ``callbacks`` argument its signature lacks (an UnboundLocalError as published); the run compiles the
  reference's own function text at generation time with that one trailing keyword added (``callbacks=None``) and nothing else changed.

    python tools/gen_golden_crappifier.py
"""
from __future__ import annotations

import inspect
import random
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
OUT = ROOT / "tests" / "golden" / "crappifier.npz"
# The trace's learning rate.  At 1e-3 the reference's own run moves its 4th loss by 1.1e-4 and its first validation loss by 3e-4
# (relative) when the initial weights are scaled by 1 + 1e-7: Adam's sign-like first updates of near-zero gradients amplify round-off
# past the trace's rtol 1e-4 whoever computes it.  At 1e-4 that sensitivity is <= 5e-5.
TRACE_LR = 1e-4


def _hist_case(GH, out, name, x, bins, rng_, sigma, view=None):
    m = GH(bins=bins, range=rng_, sigma=sigma)
    xt = torch.tensor(x, requires_grad=True)
    h = m(xt.reshape(view) if view is not None else xt)
    g = torch.tensor(np.random.default_rng(11).standard_normal(h.shape).astype(np.float32))
    (h * g).sum().backward()
    out[f"{name}_x"], out[f"{name}_g"] = x, g.numpy()
    out[f"{name}_h"], out[f"{name}_dx"] = h.detach().numpy(), xt.grad.numpy()
    out[f"{name}_cfg"] = np.array([bins, rng_[0], rng_[1], sigma], dtype=np.float64)


def gen_hist(out):
    from pssr.models._blocks import GradHist
    r = np.random.default_rng(3)
    x = (r.standard_normal((4, 1, 24, 24)) * 20).astype(np.float32)
    x.reshape(-1)[:8] = [300, -300, 256, -256, 255.5, -255.5, 1000, -1000]          # outside / at the edges of the range
    _hist_case(GradHist, out, "def", x, 512, (-256, 256), 5)
    x = (r.standard_normal((3, 1, 17, 19)) * 15).astype(np.float32)
    x.reshape(-1)[:4] = [40, -40, 33, -70]
    _hist_case(GradHist, out, "wide", x, 64, (-32, 32), 0.5)
    x = (r.standard_normal((2, 3, 11, 13)) * 25).astype(np.float32)
    _hist_case(GradHist, out, "c3", x, 512, (-256, 256), 5, view=(2, 1, 33, 13))


class _ShimSSIM(torch.nn.Module):
    """SSIMLoss(ms=False) of the reference through the oracle's restatement of pytorch_msssim."""

    def __init__(self, channels=1, mix=.8, win_size=11, win_sigma=1.5, ms=True, kwargs=None):
        super().__init__()
        self.mix, self.win_size, self.win_sigma, self.ms = mix, win_size, win_sigma, ms

    def forward(self, a, b):
        from oracle import loss_ref
        return loss_ref.ssim_loss(a, b, mix=self.mix, win_size=self.win_size, win_sigma=self.win_sigma, ms=self.ms)


def gen_loss(out):
    import pssr.train as T
    from pssr.models._blocks import GradHist
    r = np.random.default_rng(5)
    ds = np.clip(r.standard_normal((2, 1, 24, 24)) * 40 + 120, 0, 255).round().astype(np.float32)
    lr = np.clip(ds + r.standard_normal(ds.shape) * 13, 0, 255).round().astype(np.float32)
    lr_hat = (ds + r.standard_normal(ds.shape) * 6).astype(np.float32)
    out["loss_ds"], out["loss_lr"], out["loss_lr_hat"] = ds, lr, lr_hat
    for tag, arr, clamp in (("plain", lr_hat, False), ("clamp", None, True)):
        if arr is None:          # crosses 0 and 255
            arr = (ds + r.standard_normal(ds.shape) * 60).astype(np.float32)
            arr.reshape(-1)[:4] = [-20, 300, 0, 255]
            out["loss_lr_hat_clamp"] = arr
        x = torch.tensor(arr, requires_grad=True)
        xin = torch.clamp(x, 0, 255) if clamp else x
        L = T._crappifier_loss(torch.tensor(lr), xin, torch.tensor(ds), GradHist(sigma=5), _ShimSSIM(ms=False))
        L.backward()
        out[f"loss_{tag}_value"], out[f"loss_{tag}_grad"] = np.array(L.item()), x.grad.numpy()


def gen_trace(out):
    import pssr.train as T
    from pssr.models.resunet import ResUNet
    T.SSIMLoss = _ShimSSIM
    src = inspect.getsource(T.train_crappifier).replace("dataloader_kwargs = None\n", "dataloader_kwargs = None, callbacks = None\n", 1)
    assert src.count("callbacks = None") == 1
    ns = {}
    exec(compile(src, T.__file__, "exec"), T.__dict__, ns)
    train_crappifier = ns["train_crappifier"]

    r = np.random.default_rng(21)
    base = r.standard_normal((6, 1, 8, 8)) * 40 + 120
    hrs = np.clip(np.kron(base, np.ones((8, 8))) + r.standard_normal((6, 1, 64, 64)) * 3, 0, 255).round().astype(np.float32)
    lrs = np.clip(hrs[:, :, ::4, ::4] + r.standard_normal((6, 1, 16, 16)) * 13, 0, 255).round().astype(np.float32)

    class DS(torch.utils.data.Dataset):
        val_idx, crop_res, lr_scale = [4, 5], 64, 4

        def __len__(self):
            return 6

        def __getitem__(self, i):
            return torch.tensor(hrs[i]), torch.tensor(lrs[i])

    torch.manual_seed(5)
    random.seed(5)
    np.random.seed(5)
    model = ResUNet(hidden=[8, 16], depth=1, scale=1)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    opt = torch.optim.AdamW(model.parameters(), lr=TRACE_LR)
    random.seed(6)
    tl, vl = train_crappifier(model, DS(), 2, opt, epochs=2, log_frequency=1)
    out["trace_hrs"], out["trace_lrs"] = hrs, lrs
    out["train_losses"], out["val_losses"], out["trace_lr"] = np.array(tl), np.array(vl), np.array(TRACE_LR)
    for k, v in sd0.items():
        out[f"sd0/{k}"] = v.numpy()
    for k, v in model.state_dict().items():
        out[f"sd1/{k}"] = v.numpy()


if __name__ == "__main__":
    from oracle.gen_golden import import_reference
    torch.set_num_threads(1)   # deterministic summation order for the fixtures
    import_reference()
    out = {}
    gen_hist(out)
    gen_loss(out)
    gen_trace(out)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT.name, OUT.stat().st_size // 1024, "KiB")
