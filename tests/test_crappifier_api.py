"""train_crappifier / GradHist API without a GPU: the reference's signature and defaults (pssr/train.py:168-183,
pssr/models/_blocks.py:96), GradHist's constructor check, the scale-1 requirement and the no-CPU-fallback rule."""
import inspect

import pytest
import torch

# pssr/train.py:168-183, hard-coded; ``callbacks`` is read by the reference's body and documented in its docstring
REFERENCE_PARAMS = [("model", inspect.Parameter.empty), ("dataset", inspect.Parameter.empty), ("batch_size", inspect.Parameter.empty),
                    ("optim", inspect.Parameter.empty), ("epochs", inspect.Parameter.empty), ("sigma", 5), ("clip", 3), ("device", "cpu"),
                    ("scheduler", None), ("log_frequency", 50), ("checkpoint_dir", None), ("collage_dir", None), ("clamp", False),
                    ("dataloader_kwargs", None)]


def test_train_crappifier_signature_matches_reference():
    import pssr2_amd
    from pssr2_amd.train import train_crappifier
    assert pssr2_amd.train_crappifier is train_crappifier
    params = list(inspect.signature(train_crappifier).parameters.values())
    assert [(p.name, p.default) for p in params[:len(REFERENCE_PARAMS)]] == REFERENCE_PARAMS
    assert [(p.name, p.default) for p in params[len(REFERENCE_PARAMS):]] == [("callbacks", None)]
    assert "EXPERIMENTAL" in train_crappifier.__doc__


def test_gradhist_signature_and_assert():
    import pssr2_amd
    from pssr2_amd.models import GradHist
    assert pssr2_amd.GradHist is GradHist
    params = inspect.signature(GradHist.__init__).parameters
    assert [(n, p.default) for n, p in params.items()][1:] == [("bins", 512), ("range", (-256, 256)), ("sigma", 5)]
    with pytest.raises(AssertionError):
        GradHist(range=(4, 4))
    with pytest.raises(AssertionError):
        GradHist(range=(5, -5))
    h = GradHist(bins=8, range=(-4, 4))
    assert h.delta == 1.0 and torch.equal(h.centers, torch.arange(8).float() - 3.5)


def test_scale_other_than_one_raises_before_a_step():
    from pssr2_amd.models import ResUNet
    from pssr2_amd.train import train_crappifier
    model = ResUNet(hidden=[8, 16], depth=1, scale=2)

    class DS(torch.utils.data.Dataset):
        val_idx, crop_res, lr_scale = [1], 16, 2

        def __len__(self):
            return 2

        def __getitem__(self, i):
            raise AssertionError("no item may be read")

    with pytest.raises(ValueError, match="scale"):
        train_crappifier(model, DS(), 1, torch.optim.SGD(model.parameters(), lr=0.1), 1)


def test_fp16_model_raises_not_implemented():
    from pssr2_amd.models import ResUNet
    from pssr2_amd.train import train_crappifier
    model = ResUNet(hidden=[8, 16], depth=1, scale=1)
    model.compute_dtype = torch.float16
    with pytest.raises(NotImplementedError, match="loss scaler"):
        train_crappifier(model, None, 1, torch.optim.SGD(model.parameters(), lr=0.1), 1)


def test_cpu_tensors_raise():
    from pssr2_amd.models import GradHist
    from pssr2_amd.train import _crappifier_loss
    from pssr2_amd.util import SSIMLoss
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GradHist()(torch.zeros(2, 1, 16, 16))
    x = torch.zeros(2, 1, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _crappifier_loss(x, x.clone().requires_grad_(True), x, GradHist(), SSIMLoss(ms=False))


def test_gradhist_rejects_bin_counts_the_kernels_do_not_take():
    from pssr2_amd.models import GradHist
    GradHist(bins=8192)
    with pytest.raises(ValueError, match="bins"):
        GradHist(bins=8193)
    with pytest.raises(ValueError, match="bins"):
        GradHist(bins=0)


def test_collage_of_lr_sized_predictions():
    """train_crappifier's collage: the prediction is LR-sized; it is enlarged to HR size by nearest neighbour (pssr/predict.py:227-230)."""
    import numpy as np
    from pssr2_amd.train import _collage
    lr = torch.rand(2, 1, 16, 16) * 255
    lr_hat = torch.rand(2, 1, 16, 16) * 255
    hr = torch.rand(2, 1, 64, 64) * 255
    img = np.asarray(_collage(lr, lr_hat, hr, crop_res=64, lr_scale=4))
    assert img.shape == (128, 192)
    expect = np.kron(lr_hat[0, 0].numpy(), np.ones((4, 4))).astype(np.uint8)
    assert np.array_equal(img[:64, 64:128], expect)
    # an HR-sized prediction (train_paired) is placed as it is
    img = np.asarray(_collage(lr, hr, hr, crop_res=64, lr_scale=4))
    assert img.shape == (128, 192) and np.array_equal(img[:64, 64:128], hr[0, 0].numpy().astype(np.uint8))
