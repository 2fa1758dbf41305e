"""SwinIR on the MI355X with the fused window-attention kernel: the fixture cases of tests/golden/swinir.npz (float64 outputs and
gradients of the reference, tools/gen_golden_swinir.py), bf16 autocast against the torch composition, the drivers, the fall-back.

Bounds.  float32: 4x the reference's own float32-vs-float64 distance recorded per case, as in tests/test_swinir_host.py.  bf16
autocast: the yardstick is the composition path's distance from the float64 fixture on the same device; the fused path, which keeps S
and P in float32, may be at most 2x as far."""
import numpy as np
import pytest
import torch

from _swinir_cases import CASES, SEED, case_cotangent, case_input, fill_state, rel_err, run_case

pytestmark = pytest.mark.gpu
FACTOR = 4.0


@pytest.fixture(scope="module")
def gold(golden):
    return golden("swinir.npz")


@pytest.fixture
def fused_calls(monkeypatch):
    """Counts the launches of the two ops."""
    from pssr2_amd import ops
    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = ops.window_attn_fwd, ops.window_attn_bwd

    def count_fwd(*a, **k):
        calls["fwd"] += 1
        return fwd(*a, **k)

    def count_bwd(*a, **k):
        calls["bwd"] += 1
        return bwd(*a, **k)

    monkeypatch.setattr(ops, "window_attn_fwd", count_fwd)
    monkeypatch.setattr(ops, "window_attn_bwd", count_bwd)
    return calls


def _errors(gold, name, y, grads):
    err_out = rel_err(y.float().cpu().numpy(), gold[f"{name}/y"])
    errs = {k: rel_err(g.float().cpu().numpy(), gold[f"{name}/g/{k}"]) for k, g in grads.items() if f"{name}/g/{k}" in gold.files}
    worst = max(errs, key=errs.get)
    return err_out, errs[worst], worst


@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_matches_the_float64_reference(gold, fused_calls, name):
    from pssr2_amd import SwinIR
    kwargs = CASES[name][0]
    y, grads = run_case(SwinIR(**kwargs, fused_attention=True), name, torch.float32, "cuda")
    blocks = sum(kwargs["depths"])
    assert fused_calls == {"fwd": blocks, "bwd": blocks}
    err_out, err_grad, worst = _errors(gold, name, y, grads)
    print(f"case {name}: output {err_out:.3g} (yardstick {float(gold[f'{name}/err_out']):.3g}), gradients {err_grad:.3g} at {worst} "
          f"(yardstick {float(gold[f'{name}/err_grad']):.3g})")
    assert err_out <= FACTOR * float(gold[f"{name}/err_out"])
    assert err_grad <= FACTOR * float(gold[f"{name}/err_grad"]), worst


def _run_autocast(model, name):
    model = fill_state(model, SEED[name]).cuda().train()
    x = torch.from_numpy(case_input(name)).float().cuda()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = model(x)
    ct = torch.from_numpy(case_cotangent(name, y.shape)).cuda()
    (y.float() * ct.float()).sum().backward()
    return y.detach(), {k: p.grad.detach() for k, p in model.named_parameters()}


def test_bf16_autocast_fused_against_composition(gold, fused_calls):
    from pssr2_amd import SwinIR
    kwargs = CASES["a"][0]
    comp = _errors(gold, "a", *_run_autocast(SwinIR(**kwargs, fused_attention=False), "a"))
    assert fused_calls["fwd"] == 0
    fused = _errors(gold, "a", *_run_autocast(SwinIR(**kwargs, fused_attention=True), "a"))
    assert fused_calls == {"fwd": 2, "bwd": 2}
    print(f"bf16 autocast: output fused {fused[0]:.3g} / composition {comp[0]:.3g}; gradients fused {fused[1]:.3g} at {fused[2]} / "
          f"composition {comp[1]:.3g} at {comp[2]}")
    assert fused[0] <= 2 * comp[0]
    assert fused[1] <= 2 * comp[1], fused[2]


def _tiles():
    """Eight smooth 32 x 32 tiles and their 2 x 2 box-averaged 16 x 16 partners, uint8."""
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:32, 0:32]
    hr = np.stack([127 + 100 * np.sin(yy * rng.uniform(0.2, 0.5) + rng.uniform(0, 3)) * np.cos(xx * rng.uniform(0.2, 0.5) + rng.uniform(0, 3))
                   for _ in range(8)])[:, None]
    lr = hr.reshape(8, 1, 16, 2, 16, 2).mean((3, 5))
    return hr.round().astype(np.uint8), lr.round().astype(np.uint8)


def test_drivers_take_the_model(fused_calls):
    from pssr2_amd import PairedArrayDataset, SSIMLoss, SwinIR, predict_images, train_paired
    from pssr2_amd.predict import test_metrics as metrics_of
    torch.manual_seed(0)
    hr, lr = _tiles()
    ds = PairedArrayDataset(hr, lr, 32, 2, val_split=0.25, rotation=False)
    model = SwinIR(**CASES["a"][0])
    optim = torch.optim.AdamW(model.parameters(), lr=2e-3)
    train_losses, val_losses = train_paired(model, ds, 2, SSIMLoss(ms=False), optim, 2, device="cuda", log_frequency=1)
    assert len(train_losses) == 6 and len(val_losses) == 2
    assert np.isfinite(train_losses).all() and np.isfinite(val_losses).all()
    assert np.mean(train_losses[3:]) < np.mean(train_losses[:3]) and val_losses[1] < val_losses[0]
    assert fused_calls["fwd"] >= 2 * 8 and fused_calls["bwd"] == 2 * 6           # 16 x 16 is not input_resolution: no mask tensor needed
    preds = predict_images(model, ds, device="cuda", batch_size=2, out_dir=None)
    assert len(preds) == len(ds.val_idx) == 2 and all(p.shape == (1, 32, 32) and p.dtype == np.uint8 for p in preds.values())
    res = metrics_of(model, ds, device="cuda")
    assert set(res) == {"mse", "pixel", "psnr", "ssim"} and all(np.isfinite(v) for v in res.values())


def test_unsupported_window_falls_back(fused_calls):
    """window_size=12 is 144 tokens per window: the block takes the torch composition and matches fused_attention=False bit for bit."""
    from pssr2_amd import SwinIR
    kwargs = dict(image_size=24, channels=1, scale=2, embed_dim=16, depths=[2], num_heads=[2], window_size=12,
                  upsampler="pixelshuffledirect", drop_path_rate=0)
    x = torch.rand(1, 1, 24, 24, device="cuda")
    outs = []
    for fused in (True, False):
        model = fill_state(SwinIR(**kwargs, fused_attention=fused), 11).cuda().train()
        y = model(x)
        y.sum().backward()
        outs.append((y.detach(), model.layers[0].residual_group.blocks[1].attn.relative_position_bias_table.grad))
    assert fused_calls == {"fwd": 0, "bwd": 0}
    assert torch.allclose(outs[0][0], outs[1][0], rtol=0, atol=0) and torch.allclose(outs[0][1], outs[1][1], rtol=1e-5, atol=1e-7)
