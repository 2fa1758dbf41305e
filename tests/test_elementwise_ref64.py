"""The element-wise references (tests/_elementwise_ref64.py) against torch's own operators and autograd, on the CPU in f64: both
sides are f64 runs of one algebra and agree to rounding."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _elementwise_ref64 as R

TOL = 1e-12


def _close(got, want, scale=None):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    assert got.shape == want.shape
    den = want.abs().max().item() if scale is None else scale
    assert (got - want).abs().max().item() <= TOL * max(den, 1e-300), ((got - want).abs().max().item(), den)


def _image(n, c, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, c, h, w), generator=g).double()


def _bn_params(c, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(c, generator=g, dtype=torch.float64) + 0.5, torch.randn(c, generator=g, dtype=torch.float64),
            torch.randn(c, generator=g, dtype=torch.float64), torch.rand(c, generator=g, dtype=torch.float64) + 0.5)


@pytest.mark.parametrize("shape", [(3, 5, 6, 7), (1, 2, 1, 9), (4, 1, 3, 3)])
def test_batchnorm_chain_vs_torch(shape):
    """nchw_stats -> bn_finalize -> relu_bwd_stats (mask all ones) -> bn_bwd_coefs -> bn_bwd_apply is F.batch_norm(training=True) and
    its backward: output, running statistics, dx, dgamma, dbeta."""
    n, c, h, w = shape
    ps, pb, eps, mom = 1 / 128, -1.0, 1e-5, 0.1
    x = _image(n, c, h, w, sum(shape))
    gamma, beta, rm0, rv0 = _bn_params(c, 1)
    count = n * h * w
    s1, s2 = R.nchw_stats(x, ps, pb)
    fin = R.bn_finalize(s1, s2, count, gamma, beta, eps, mom, running=(rm0, rv0))
    xin = (x * ps + pb).requires_grad_(True)
    gt, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm, rv = rm0.clone(), rv0.clone()
    y = F.batch_norm(xin, rm, rv, gt, bt, training=True, momentum=mom, eps=eps)
    _close(xin.detach() * fin["scale"][None, :, None, None] + fin["shift"][None, :, None, None], y.detach())
    _close(fin["running_mean"], rm)
    _close(fin["running_var"], rv)
    _close(fin["mean"], xin.detach().mean((0, 2, 3)))
    _close(fin["var"], xin.detach().var((0, 2, 3), unbiased=False))
    gy = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    y.backward(gy)
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(count, c)
    dz, b1, b2 = R.relu_bwd_stats(flat(gy), torch.ones(count, c), flat(xin.detach()), fin["mean"], fin["invstd"])
    assert torch.equal(dz, flat(gy))
    co = R.bn_bwd_coefs(b1, b2, count, gamma, fin["mean"], fin["invstd"])
    dx = R.bn_bwd_apply(dz, flat(xin.detach()), co["A"], co["B"], co["C"])
    _close(dx, flat(xin.grad), scale=flat(gy).abs().max().item() * gamma.max().item() * fin["invstd"].max().item())
    _close(co["dgamma"], gt.grad, scale=gy.abs().sum().item())
    _close(co["dbeta"], bt.grad, scale=gy.abs().sum().item())


def test_bn_finalize_defaults_count_one_and_clamp():
    """No gamma / beta means 1 / 0; count == 1 keeps the biased variance for the running update; a negative variance is clamped."""
    s1, s2 = torch.tensor([3.0, -2.0]), torch.tensor([9.0 - 1e-6, 5.0])
    fin = R.bn_finalize(s1, s2, 1.0, eps=1e-5, momentum=0.25, running=(torch.tensor([1.0, 1.0]), torch.tensor([2.0, 2.0])))
    assert fin["var"][0] == 0.0 and fin["invstd"][0] == 1.0 / np.sqrt(1e-5)
    _close(fin["var"][1:], torch.tensor([1.0]))
    _close(fin["scale"], fin["invstd"])
    _close(fin["shift"], -fin["mean"] * fin["invstd"])
    _close(fin["running_var"], torch.tensor([1.5, 1.75]))
    _close(fin["running_mean"], torch.tensor([1.5, 0.25]))
    assert "running_mean" not in R.bn_finalize(s1, s2, 4.0)


def test_bn_eval_affine_vs_torch():
    n, c = 3, 5
    gamma, beta, rm, rv = _bn_params(c, 3)
    x = torch.randn(n, c, 4, 4, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    scale, shift = R.bn_eval_affine(gamma, beta, rm, rv, 1e-5)
    _close(x * scale[None, :, None, None] + shift[None, :, None, None], F.batch_norm(x, rm, rv, gamma, beta, training=False, eps=1e-5))


@pytest.mark.parametrize("shape", [(2, 1, 5, 7, 16), (1, 3, 6, 5, 32), (1, 1, 4, 4, 48)])
def test_input_im2col_vs_unfold(shape):
    n, c, h, w, xc = shape
    x = _image(n, c, h, w, sum(shape))
    scale, shift, _, _ = _bn_params(c, 5)
    got = R.input_im2col(x, scale, shift, xc)
    xn = (x / 128 - 1) * scale[None, :, None, None] + shift[None, :, None, None]
    want = F.unfold(xn, 3, padding=1).view(n, c * 9, h, w).permute(0, 2, 3, 1)
    _close(got[..., :9 * c], want)
    assert (got[..., 9 * c:] == 0).all()
    # a padding tap is zero, not `shift`: the tap above the first row
    assert (got[:, 0, :, 1] == 0).all() and (want[:, 0, :, 1] == 0).all()


def _patchify(x0, pk):
    n, c, h, w = x0.shape
    return x0.reshape(n, c, h // pk, pk, w // pk, pk).permute(0, 2, 4, 1, 3, 5).reshape(n, h // pk, w // pk, c * pk * pk)


@pytest.mark.parametrize("case", [(2, 1, 5, 7, 16, 1, 0), (2, 3, 8, 12, 32, 2, 0), (2, 3, 8, 12, 32, 0, 2), (2, 3, 8, 12, 32, 1, 4),
                                  (1, 2, 4, 6, 32, 2, 2)])
def test_input_norm_bwd_vs_autograd(case):
    """The fold of one or two im2col gradients and a patch gradient onto the normalised input is what autograd gives through
    F.unfold(padding=1) and a reshape / permute patchify; the two reduced sums follow."""
    n, c, h, w, xc, ncol, pk = case
    g = torch.Generator().manual_seed(sum(case))
    x = _image(n, c, h, w, 7)
    _, mean, _, invstd = _bn_params(c, 8)
    dxcols = [torch.randn(n, h, w, xc, generator=g, dtype=torch.float64) for _ in range(ncol)]
    pc = c * pk * pk + 3
    dpatch = torch.randn(n, h // pk, w // pk, pc, generator=g, dtype=torch.float64) if pk else None
    x0 = torch.randn(n, c, h, w, generator=g, dtype=torch.float64).requires_grad_(True)
    obj = x0.sum() * 0
    for d in dxcols:
        obj = obj + (F.unfold(x0, 3, padding=1).view(n, c * 9, h, w).permute(0, 2, 3, 1) * d[..., :9 * c]).sum()
    if pk:
        obj = obj + (_patchify(x0, pk) * dpatch[..., :c * pk * pk]).sum()
    (want,) = torch.autograd.grad(obj, x0)
    got, s1, s2 = R.input_norm_bwd(dxcols, dpatch, pk, x, mean, invstd)
    _close(got, want)
    xhat = (x / 128 - 1 - mean[None, :, None, None]) * invstd[None, :, None, None]
    _close(s1, want.sum((0, 2, 3)), scale=want.abs().sum().item())
    _close(s2, (want * xhat).sum((0, 2, 3)), scale=(want * xhat).abs().sum().item())


@pytest.mark.parametrize("hw", [(6, 10), (5, 7), (5, 6), (6, 5), (4, 4), (2, 3)])
@pytest.mark.parametrize("skip", [True, False])
def test_maxpool2_vs_torch(hw, skip):
    """Forward with floor, backward with the first maximum of tied windows (post-ReLU data: a third zeros, whole windows of zeros
    included), odd trailing rows / columns left to the skip gradient."""
    h, w = hw
    n, c = 2, 4
    g = torch.Generator().manual_seed(h * 16 + w)
    act = torch.relu(torch.randn(n, h, w, c, generator=g, dtype=torch.float64) + 0.43)
    act[0, :2, :2] = 0.0                                                   # one window all tied
    act[1, 0, 0], act[1, 1, 1] = 2.5, 2.5                                  # tie between the first and the last tap
    assert 0.15 < (act == 0).double().mean() < 0.5
    dpool = torch.randn(n, h // 2, w // 2, c, generator=g, dtype=torch.float64)
    dskip = torch.randn(n, h, w, c, generator=g, dtype=torch.float64) if skip else None
    av = act.permute(0, 3, 1, 2).clone().requires_grad_(True)
    pooled = F.max_pool2d(av, 2)
    assert torch.equal(R.maxpool2(act), pooled.detach().permute(0, 2, 3, 1))
    pooled.backward(dpool.permute(0, 3, 1, 2))
    want = av.grad.permute(0, 2, 3, 1) + (dskip if skip else 0.0)
    got = R.maxpool2_bwd(act, dpool, dskip)
    assert torch.equal(got, want)
    if h % 2:
        assert torch.equal(got[:, -1], dskip[:, -1] if skip else torch.zeros(n, w, c, dtype=torch.float64))
    if w % 2:
        assert torch.equal(got[:, :, -1], dskip[:, :, -1] if skip else torch.zeros(n, h, c, dtype=torch.float64))


def test_relu_mask_channel_sum_and_layout():
    g = torch.Generator().manual_seed(11)
    dout, y = torch.randn(9, 4, generator=g), torch.randn(9, 4, generator=g)
    out = torch.relu(torch.randn(9, 4, generator=g))
    mean, invstd = torch.randn(4, generator=g), torch.rand(4, generator=g) + 0.5
    dz, s1, s2 = R.relu_bwd_stats(dout, out, y, mean, invstd)
    assert torch.equal(dz, dout.double() * (out > 0))
    _close(s1, dz.sum(0))
    _close(s2, torch.einsum("pc,pc->c", dz, (y.double() - mean.double()) * invstd.double()))
    _close(R.channel_sum(y), y.double().sum(0))
    x = torch.randn(2, 3, 4, 5, generator=g)
    o = R.nchw_to_nhwc(x, 8, 1 / 3)
    assert o.dtype == torch.float32 and torch.equal(o[..., :3], (x * np.float32(1 / 3)).permute(0, 2, 3, 1)) and (o[..., 3:] == 0).all()


def test_clip_u8_and_stripe_fold():
    v = np.array([-1e10, -0.0, 0.49, 0.5, 0.999, 254.999, 255, 255.5, 256, 1e10, np.inf, -np.inf], dtype=np.float32)
    assert R.clip_u8(v).tolist() == [0, 0, 0, 0, 0, 254, 255, 255, 255, 255, 255, 0]
    src = np.arange(12, dtype=np.float64).reshape(3, 4) * 2.0 ** -20
    assert np.array_equal(R.stripe_fold(src), (src[0] + src[1] + src[2]).astype(np.float32))
    old = np.full(4, 0.1, dtype=np.float32)
    assert np.array_equal(R.stripe_fold(src, old), old + src.sum(0).astype(np.float32))
