"""GradHist (csrc/hist.hip), the fused crappifier loss, scale-1 ResUNet and train_crappifier on the device, against float64
restatements written here and the reference's own outputs (tests/golden/crappifier.npz, tools/gen_golden_crappifier.py)."""
import random
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).parent / "golden"
DEF, WIDE = (512, (-256, 256), 5), (64, (-32, 32), 0.5)


def _restated(x, g, bins, rng, sigma, dtype):
    """GradHist forward / backward written out (pssr/models/_blocks.py:94-112) in ``dtype``, centres as the reference's fp32
    tensor, chunked over pixels."""
    B = x.shape[0]
    xf = x.reshape(B, -1).to(dtype)
    delta = float(rng[1] - rng[0]) / float(bins)
    c = (float(rng[0]) + delta * (torch.arange(bins).float() + 0.5)).to(x.device, dtype)
    h = torch.zeros(B, bins, dtype=dtype, device=x.device)
    dx = torch.zeros_like(xf)
    gg = g.to(dtype)
    G = torch.cat([gg[:, 1:], torch.zeros(B, 1, dtype=dtype, device=x.device)], 1) - gg          # g[k+1] [k+1 < bins] - g[k]
    for i in range(0, xf.shape[1], 2048):
        s = torch.sigmoid((xf[:, None, i:i + 2048] - c[:, None]) * sigma)                         # [B, bins, n]
        ones = torch.ones(B, 1, s.shape[-1], dtype=dtype, device=x.device)
        h += (torch.cat([ones, s[:, :-1]], 1) - s).sum(-1)
        dx[:, i:i + 2048] = sigma * (s * (1 - s) * G[:, :, None]).sum(1)
    return h, dx.reshape(x.shape)


def _run(x, g, cfg):
    from pssr2_amd.models import GradHist
    bins, rng, sigma = cfg
    xt = x.clone().requires_grad_(True)
    h = GradHist(bins=bins, range=rng, sigma=sigma)(xt)
    h.backward(g)
    return h.detach(), xt.grad


def _check(h, dx, h_ref, dx_ref):
    err_h = ((h.double() - h_ref.double()).abs().amax(1) / h_ref.double().abs().amax(1)).max().item()
    err_dx = ((dx.double() - dx_ref.double()).abs().max() / dx_ref.double().abs().max()).item()
    return err_h, err_dx


def _inputs(shape, std, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=gen) * std
    x.view(-1)[::97] = torch.round(x.view(-1)[::97])            # integer profile values sit on bin edges
    x.view(-1)[:6] = torch.tensor([3.0 * std * 40, -3.0 * std * 40, 1e4, -1e4, 0.0, 0.5])       # far outside the range
    return x.cuda()


@pytest.mark.parametrize("cfg,shape,std", [(DEF, (4, 1, 128, 128), 13.0), (WIDE, (4, 1, 128, 128), 10.0),
                                           (DEF, (2, 3, 37, 53), 20.0), (WIDE, (2, 3, 37, 53), 8.0)])
def test_gradhist_vs_float64(cfg, shape, std):
    x = _inputs(shape, std, 1)
    g = torch.randn(shape[0], cfg[0], generator=torch.Generator().manual_seed(2)).cuda()
    h, dx = _run(x, g, cfg)
    h64, dx64 = _restated(x, g, *cfg, torch.float64)
    e_h, e_dx = _check(h, dx, h64, dx64)
    h32, dx32 = _restated(x, g, *cfg, torch.float32)
    e_h32, e_dx32 = _check(h32, dx32, h64, dx64)
    print(f"{cfg} {shape}: HIP fwd {e_h:.2e} bwd {e_dx:.2e}; torch fp32 fwd {e_h32:.2e} bwd {e_dx32:.2e}")
    assert e_h <= 1e-5 and e_dx <= 1e-4, (e_h, e_dx)
    assert e_h32 <= 1e-5 and e_dx32 <= 1e-4, (e_h32, e_dx32)          # the bounds hold for a plain fp32 evaluation too


@pytest.mark.parametrize("name", ["def", "wide", "c3"])
def test_gradhist_vs_reference_fixture(name):
    d = np.load(GOLD / "crappifier.npz")
    bins, lo, hi, sigma = d[f"{name}_cfg"]
    h, dx = _run(torch.tensor(d[f"{name}_x"]).cuda(), torch.tensor(d[f"{name}_g"]).cuda(), (int(bins), (lo, hi), float(sigma)))
    e_h, e_dx = _check(h.cpu(), dx.cpu(), torch.tensor(d[f"{name}_h"]), torch.tensor(d[f"{name}_dx"]))
    assert e_h <= 1e-5 and e_dx <= 1e-4, (e_h, e_dx)


def test_gradhist_bit_reproducible():
    x = _inputs((16, 1, 128, 128), 13.0, 3)
    g = torch.randn(16, 512, generator=torch.Generator().manual_seed(4)).cuda()
    h0, dx0 = _run(x, g, DEF)
    h1, dx1 = _run(x, g, DEF)
    assert torch.equal(h0, h1) and torch.equal(dx0, dx1)


def test_gradhist_two_pairs_in_one_launch():
    """pssr_gradhist_fwd histograms a - b of two pairs on load (clamping the first pair's a when asked)."""
    from pssr2_amd import ops
    a0, b0, a1, b1 = (_inputs((3, 1, 40, 33), 60.0, s) + 128 for s in (5, 6, 7, 8))
    h0, h1 = ops.gradhist_fwd([(a0, b0), (a1, b1)], 512, -256.0, 256.0, 5.0, clamp_first=True)
    r0, _ = _restated(a0.clamp(0, 255) - b0, torch.zeros(3, 512).cuda(), *DEF, torch.float64)
    r1, _ = _restated(a1 - b1, torch.zeros(3, 512).cuda(), *DEF, torch.float64)
    assert _check(h0, torch.ones(1), r0, torch.ones(1))[0] <= 1e-5
    assert _check(h1, torch.ones(1), r1, torch.ones(1))[0] <= 1e-5


@pytest.mark.parametrize("tag", ["plain", "clamp"])
def test_crappifier_loss_vs_reference_fixture(tag):
    from pssr2_amd.models import GradHist
    from pssr2_amd.train import _crappifier_loss
    from pssr2_amd.util import SSIMLoss
    d = np.load(GOLD / "crappifier.npz")
    lr, ds = torch.tensor(d["loss_lr"]).cuda(), torch.tensor(d["loss_ds"]).cuda()
    x = torch.tensor(d["loss_lr_hat" if tag == "plain" else "loss_lr_hat_clamp"]).cuda().requires_grad_(True)
    L = _crappifier_loss(lr, x, ds, GradHist(sigma=5), SSIMLoss(ms=False), clamp=tag == "clamp")
    L.backward()
    ref_v, ref_g = float(d[f"loss_{tag}_value"]), torch.tensor(d[f"loss_{tag}_grad"])
    assert abs(L.item() - ref_v) <= 1e-4 * abs(ref_v), (L.item(), ref_v)
    err = ((x.grad.cpu().double() - ref_g.double()).abs().max() / ref_g.abs().max()).item()
    assert err <= 1e-4, err
    if tag == "clamp":
        raw = x.detach().cpu()
        assert (x.grad.cpu()[(raw < 0) | (raw > 255)] == 0).all()


def test_resunet_scale1_vs_oracle():
    """scale 1 = blocked order with blk = 0 and no shuffle: outputs (train / eval), running statistics and every parameter gradient
    against the oracle's f64 graph (with the HIP path's ReLU decisions, as tests/test_gpu_model.py does)."""
    from oracle import model_ref as M
    from pssr2_amd.models import ResUNet
    from test_gpu_model import engine_relu_masks
    torch.manual_seed(3)
    model = ResUNet(hidden=[16, 32], depth=1, scale=1).cuda()
    sd0 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    gen = torch.Generator().manual_seed(9)
    x = torch.rand(2, 1, 32, 32, generator=gen) * 255
    target = torch.rand(2, 1, 32, 32, generator=gen) * 255

    def make64():
        return {k: (v.double().requires_grad_(True) if "running" not in k else v.double()) if v.dtype.is_floating_point else v
                for k, v in sd0.items()}

    model.eval()
    with torch.no_grad():
        y_eval = model(x.cuda()).cpu()
    y_eval64, _ = M.resunet_forward(x.double(), make64(), 2, 1, 1, train=False)
    assert y_eval.shape == x.shape
    np.testing.assert_allclose(y_eval.numpy(), y_eval64.detach().numpy(), rtol=2e-4, atol=2e-3)

    model.train()
    y = model(x.cuda())
    plain64, rec = make64(), {}
    y64p, stats64 = M.resunet_forward(x.double(), plain64, 2, 1, 1, train=True, record=rec)
    np.testing.assert_allclose(y.detach().cpu().numpy(), y64p.detach().numpy(), rtol=2e-4, atol=3e-3)
    sd = model.state_dict()
    for k, v in stats64.items():
        np.testing.assert_allclose(sd[k].cpu().numpy(), v.detach().numpy(), rtol=1e-4, atol=1e-5, err_msg=k)
    torch.nn.functional.mse_loss(y / 255, target.cuda() / 255).backward()
    masks = engine_relu_masks(model)
    p64 = make64()
    y64, _ = M.resunet_forward(x.double(), p64, 2, 1, 1, train=True, masks=masks)
    torch.nn.functional.mse_loss(y64 / 255, target.double() / 255).backward()
    bad = []
    for pname, prm in model.named_parameters():
        truth, got = p64[pname].grad, prm.grad.cpu().double()
        scale = truth.abs().max().item()
        if scale < 1e-7:
            assert got.abs().max().item() <= 1e-6, pname
            continue
        if (got - truth).abs().max().item() / scale > 2e-4:
            bad.append((pname, (got - truth).abs().max().item() / scale))
    assert not bad, bad


class _TraceDS(torch.utils.data.Dataset):
    val_idx, crop_res, lr_scale = [4, 5], 64, 4

    def __init__(self, hrs, lrs):
        self.hrs, self.lrs = hrs, lrs

    def __len__(self):
        return 6

    def __getitem__(self, i):
        return torch.tensor(self.hrs[i]), torch.tensor(self.lrs[i])


def test_train_crappifier_reproduces_the_reference_trace():
    from pssr2_amd.models import ResUNet
    from pssr2_amd.train import train_crappifier
    d = np.load(GOLD / "crappifier.npz")
    model = ResUNet(hidden=[8, 16], depth=1, scale=1)
    model.load_state_dict({k[4:]: torch.from_numpy(np.asarray(d[k])) for k in d.files if k.startswith("sd0/")})
    opt = torch.optim.AdamW(model.parameters(), lr=float(d["trace_lr"]))
    random.seed(6)
    tl, vl = train_crappifier(model, _TraceDS(d["trace_hrs"], d["trace_lrs"]), 2, opt, epochs=2, device="cuda", log_frequency=1)
    assert len(tl) == len(d["train_losses"]) and len(vl) == len(d["val_losses"]) == 2
    np.testing.assert_allclose(tl, d["train_losses"], rtol=1e-4)
    np.testing.assert_allclose(vl, d["val_losses"], rtol=1e-4)
    sd = model.state_dict()
    for k in d.files:
        if not k.startswith("sd1/"):
            continue
        # as tests/test_gpu_fastpath.py: a conv bias in front of a batch-statistics BatchNorm has an exactly zero gradient; the
        # reference's autograd leaves round-off there which Adam turns into +-lr steps, the engine leaves the slot zero (no effect on
        # any output: the BatchNorm removes them)
        parts = k[4:].split(".")
        if parts[-1] == "bias" and "conv" in parts and parts[parts.index("conv") + 1] in ("0", "3"):
            continue
        np.testing.assert_allclose(sd[k[4:]].cpu().numpy(), d[k], rtol=2e-3, atol=2e-4, err_msg=k)


def test_train_crappifier_learns_the_noise_distribution():
    """A scale-1 ResUNet trained on AdditiveGaussian(13) pairs: the histogram distance D of its noise profile to the real one ends well
    below where it started."""
    from pssr2_amd.crappifiers import AdditiveGaussian
    from pssr2_amd.data import synthetic_em_tile
    from pssr2_amd.models import GradHist, ResUNet
    from pssr2_amd.train import train_crappifier
    rng = np.random.default_rng(0)
    hrs, lrs = [], []
    crap = AdditiveGaussian(13)
    for i in range(40):
        hr = np.asarray(synthetic_em_tile(i, res=64), dtype=np.float32).reshape(1, 64, 64)
        ds = hr[:, ::2, ::2]
        np.random.seed(i)
        lrs.append(np.clip(np.round(crap.crappify(ds.copy())), 0, 255).astype(np.float32).reshape(ds.shape))
        hrs.append(hr)

    class DS(torch.utils.data.Dataset):
        val_idx, crop_res, lr_scale = list(range(32, 40)), 64, 2

        def __len__(self):
            return 40

        def __getitem__(self, i):
            return torch.tensor(hrs[i]), torch.tensor(lrs[i])

    hist = GradHist(sigma=5)

    def dist(model):
        model.train()                   # batch statistics: the untrained model's running statistics say nothing
        with torch.no_grad():
            hr = torch.tensor(np.stack(hrs[32:])).cuda()
            lr = torch.tensor(np.stack(lrs[32:])).cuda()
            ds = hr[:, :, ::2, ::2].contiguous()
            ph, th = hist(model(ds) - ds), hist(lr - ds)
            return (torch.nn.functional.mse_loss(ph, th) / lr.shape[-1] ** 2).item()

    torch.manual_seed(0)
    random.seed(0)
    model = ResUNet(hidden=[16, 32, 64], scale=1).cuda()
    d0 = dist(model)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    train_crappifier(model, DS(), 4, opt, epochs=40, device="cuda", log_frequency=1000)
    d1 = dist(model)
    print(f"noise-histogram distance D: {d0:.4f} -> {d1:.4f} ({d1 / d0:.3f})")
    assert d1 < 0.5 * d0, (d0, d1)


def test_clamp_keeps_nan_like_clip_grad_value():
    """Gradient clipping over the engine's flat buffer: the values of nn.utils.clip_grad_value_, NaN kept."""
    from pssr2_amd import ops
    x = torch.tensor([-5.0, -3.0, 0.5, 3.0, 7.0, float("nan"), float("inf"), -float("inf")], device="cuda")
    got = ops.clamp_f32(x, -3.0, 3.0)
    prm = torch.nn.Parameter(torch.zeros_like(x))
    prm.grad = x.clone()
    torch.nn.utils.clip_grad_value_([prm], 3.0)
    ref = prm.grad
    assert torch.isnan(got[5])
    assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(got[~torch.isnan(ref)], ref[~torch.isnan(ref)])


def _small_pairs(n, res, lr_scale, seed):
    from pssr2_amd.crappifiers import AdditiveGaussian
    from pssr2_amd.data import synthetic_em_tile
    hrs, lrs = [], []
    crap = AdditiveGaussian(13)
    for i in range(n):
        hr = np.asarray(synthetic_em_tile(seed + i, res=res), dtype=np.float32).reshape(1, res, res)
        ds = hr[:, ::lr_scale, ::lr_scale]
        np.random.seed(seed + i)
        lrs.append(np.clip(np.round(crap.crappify(ds.copy())), 0, 255).astype(np.float32).reshape(ds.shape))
        hrs.append(hr)
    return hrs, lrs


class _PairDS(torch.utils.data.Dataset):
    def __init__(self, hrs, lrs, val_idx, lr_scale):
        self.hrs, self.lrs, self.val_idx = hrs, lrs, val_idx
        self.crop_res, self.lr_scale = hrs[0].shape[-1], lr_scale

    def __len__(self):
        return len(self.hrs)

    def __getitem__(self, i):
        return torch.tensor(self.hrs[i]), torch.tensor(self.lrs[i])


def test_train_crappifier_checkpoints_collages_callbacks(tmp_path):
    """The driver's side outputs with lr_scale 4: one checkpoint per epoch but the last, one collage per epoch (LR-sized predictions
    enlarged to HR size), callbacks with the loop's locals, a clamp run."""
    from PIL import Image
    from pssr2_amd.models import ResUNet
    from pssr2_amd.train import train_crappifier
    hrs, lrs = _small_pairs(6, 64, 4, 100)
    torch.manual_seed(0)
    model = ResUNet(hidden=[8, 16], depth=1, scale=1)
    seen = []
    tl, vl = train_crappifier(model, _PairDS(hrs, lrs, [4, 5], 4), 2, torch.optim.AdamW(model.parameters(), lr=1e-3), 2, device="cuda",
                              log_frequency=1, checkpoint_dir=str(tmp_path / "ck"), collage_dir=str(tmp_path / "col"), clamp=True,
                              callbacks=[lambda loc: seen.append((loc["batch_idx"], tuple(loc["lr_hat"].shape)))])
    assert len(tl) == 4 and len(vl) == 2 and all(np.isfinite(tl)) and all(np.isfinite(vl))
    assert seen == [(0, (2, 1, 16, 16)), (1, (2, 1, 16, 16))] * 2
    cks = list((tmp_path / "ck").glob("checkpoint0_ResUNet_*.pth"))
    assert len(cks) == 1 and not list((tmp_path / "ck").glob("checkpoint1_*"))
    assert "encoder.0.conv.0.weight" in torch.load(cks[0], weights_only=True)
    cols = sorted((tmp_path / "col").glob("epoch*_loss*.png"))
    assert len(cols) == 2 and Image.open(cols[0]).size == (192, 128)


def test_train_crappifier_bf16_model():
    """bf16 storage: the fused loss and the driver run, every loss stays finite and the validation loss falls."""
    from pssr2_amd.models import ResUNet
    from pssr2_amd.train import train_crappifier
    hrs, lrs = _small_pairs(24, 64, 2, 200)
    torch.manual_seed(1)
    random.seed(1)
    model = ResUNet(hidden=[16, 32, 64], scale=1)
    model.compute_dtype = torch.bfloat16
    tl, vl = train_crappifier(model, _PairDS(hrs, lrs, list(range(20, 24)), 2), 4, torch.optim.AdamW(model.parameters(), lr=1e-3), 12,
                              device="cuda", log_frequency=1)
    print(f"bf16 train_crappifier: validation loss {vl[0]:.4f} -> {vl[-1]:.4f}")
    assert all(np.isfinite(tl)) and all(np.isfinite(vl))
    assert vl[-1] < 0.7 * vl[0], vl
