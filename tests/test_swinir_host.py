"""SwinIR on the CPU (the torch composition path) against tests/golden/swinir.npz, which tools/gen_golden_swinir.py wrote from the
reference: interface, state_dict, float64 outputs and gradients, checkpoints, errors.

Bound: the fixture records, per case, how far the reference's own float32 run lies from its float64 run (max |f32 - f64| / max |f64|,
for the output and as the maximum over the gradient tensors).  That is one float32 evaluation's distance from the truth; ours is
another float32 evaluation with other summation orders, so 4x the recorded figure is allowed.  A wrong index, mask or bias shows at
1e-2 and above."""
import inspect

import numpy as np
import pytest
import torch

from _swinir_cases import CASES, SEED, fill_state, rel_err, run_case

FACTOR = 4.0


@pytest.fixture(scope="module")
def gold(golden):
    return golden("swinir.npz")


def test_exported_with_the_reference_signature(gold):
    import pssr2_amd
    from pssr2_amd.swinir import SwinIR
    assert pssr2_amd.SwinIR is SwinIR
    sig = inspect.signature(SwinIR.__init__)
    names = [n for n in sig.parameters if n != "self"]
    ref_names = list(gold["sig_names"])
    assert names[:len(ref_names)] == ref_names
    assert [repr(sig.parameters[n].default) for n in ref_names] == list(gold["sig_defaults"])
    extra = names[len(ref_names):]
    assert extra == ["fused_attention"] and sig.parameters["fused_attention"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["fused_attention"].default is True


@pytest.mark.parametrize("name", sorted(CASES))
def test_state_dict_keys_and_shapes(gold, name):
    from pssr2_amd import SwinIR
    sd = SwinIR(**CASES[name][0]).state_dict()
    assert list(sd) == list(gold[f"{name}/keys"])
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == list(gold[f"{name}/shapes"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_composition_matches_the_float64_reference(gold, name):
    from pssr2_amd import SwinIR
    y, grads = run_case(SwinIR(**CASES[name][0]), name, torch.float32, "cpu")
    err_out = rel_err(y.numpy(), gold[f"{name}/y"])
    errs = {k: rel_err(g.numpy(), gold[f"{name}/g/{k}"]) for k, g in grads.items() if f"{name}/g/{k}" in gold.files}
    assert len(errs) >= len(grads) - 4 and len(errs) > 10
    worst = max(errs, key=errs.get)
    print(f"case {name}: output {err_out:.3g} (yardstick {float(gold[f'{name}/err_out']):.3g}), gradients {errs[worst]:.3g} at {worst} "
          f"(yardstick {float(gold[f'{name}/err_grad']):.3g})")
    assert err_out <= FACTOR * float(gold[f"{name}/err_out"])
    assert errs[worst] <= FACTOR * float(gold[f"{name}/err_grad"]), worst


def test_eval_equals_train_at_zero_drop_rates():
    from pssr2_amd import SwinIR
    model = fill_state(SwinIR(**CASES["a"][0]), SEED["a"])
    x = torch.rand(1, 1, 16, 24)
    with torch.no_grad():
        y_train = model.train()(x)
        y_eval = model.eval()(x)
    assert torch.equal(y_train, y_eval)


def test_checkpoint_round_trip(tmp_path):
    from pssr2_amd import SwinIR
    kwargs = CASES["b"][0]
    a = fill_state(SwinIR(**kwargs), 7)
    torch.save(a.state_dict(), tmp_path / "swinir.pth")
    b = SwinIR(**kwargs)
    missing = b.load_state_dict(torch.load(tmp_path / "swinir.pth"), strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    x = torch.rand(1, 3, 12, 12)
    with torch.no_grad():
        assert torch.equal(a.eval()(x), b.eval()(x))


def test_activation_checkpointing_and_stochastic_depth_run():
    from pssr2_amd import SwinIR
    from pssr2_amd.swinir import DropPath
    kwargs = dict(CASES["a"][0], use_checkpoint=True, drop_path_rate=0.5)
    model = SwinIR(**kwargs).train()
    y = model(torch.rand(2, 1, 16, 24))
    y.sum().backward()
    assert y.shape == (2, 1, 32, 48) and all(p.grad is not None for p in model.parameters())
    drop = DropPath(0.25).train()
    torch.manual_seed(0)
    out = drop(torch.ones(64, 3, 2))
    kept = out[:, 0, 0] != 0
    assert 0 < int(kept.sum()) < 64 and torch.allclose(out[kept], torch.full_like(out[kept], 1 / 0.75))
    assert (out[~kept] == 0).all()
    assert torch.equal(drop.eval()(torch.ones(4, 2)), torch.ones(4, 2))
    assert torch.equal(DropPath(0.0).train()(torch.ones(4, 2)), torch.ones(4, 2))


def test_constructor_errors():
    from pssr2_amd import SwinIR
    from pssr2_amd.swinir import SwinTransformerBlock, Upsample
    with pytest.raises(ValueError, match="depths and num_heads"):
        SwinIR(depths=[2, 2], num_heads=[2])
    with pytest.raises(ValueError, match="not supported"):
        SwinIR(image_size=16, scale=5, embed_dim=12, depths=[1], num_heads=[2])
    with pytest.raises(ValueError, match="not supported"):
        Upsample(6, 8)
    with pytest.raises(ValueError, match="shift_size"):
        SwinTransformerBlock(16, (32, 32), 2, window_size=8, shift_size=8)


@pytest.mark.parametrize("upsampler,scale,shape", [("nearest+conv", 4, (1, 1, 64, 64)), ("nearest+conv", 2, (1, 1, 32, 32)),
                                                   ("pixelshuffle", 3, (1, 1, 48, 48)), (None, 1, (1, 1, 16, 16))])
def test_upsampler_settings(upsampler, scale, shape):
    from pssr2_amd import SwinIR
    model = SwinIR(image_size=16, scale=scale, embed_dim=16, depths=[2], num_heads=[2], window_size=8, upsampler=upsampler).eval()
    with torch.no_grad():
        assert model(torch.rand(1, 1, 16, 16)).shape == shape
        # 13 x 11 is padded to 16 x 16 and the result cropped back
        assert model(torch.rand(1, 1, 13, 11)).shape[2:] == (13 * scale, 11 * scale)
