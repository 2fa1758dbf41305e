"""The references of tests/_rdnet_ref64.py against torch in float64: F.conv2d(groups=C, padding=3) and its autograd, F.layer_norm and
its autograd, t * relu6(fc(mean(t)) + 3) / 6 * gamma and its autograd, F.unfold.  Runs on the CPU."""
import pytest
import torch
import torch.nn.functional as F

import _rdnet_ref64 as R

F64 = torch.float64


def _gen(*seed):
    return torch.Generator().manual_seed(sum(int(s) * (i + 1) for i, s in enumerate(seed)) + 4321)


def _close(got, want, what=""):
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12 * float(want.abs().max()) + 1e-300, msg=lambda m: f"{what}: {m}")


@pytest.mark.parametrize("shape,ps,pc", [((2, 1, 6, 10), 2, 16), ((1, 3, 8, 12), 4, 64), ((3, 3, 9, 6), 3, 32)])
def test_patchify(shape, ps, pc):
    n, c, h, w = shape
    g = _gen(*shape, ps)
    x = torch.rand(shape, generator=g, dtype=F64) * 255
    scale, shift = torch.rand(c, generator=g, dtype=F64) + 0.5, torch.randn(c, generator=g, dtype=F64)
    got = R.patchify(x, ps, pc, scale, shift, 1 / 128, -1.0)
    v = (x / 128 - 1.0) * scale.view(1, c, 1, 1) + shift.view(1, c, 1, 1)
    want = F.unfold(v, ps, stride=ps).view(n, c * ps * ps, h // ps, w // ps).permute(0, 2, 3, 1)
    _close(got[..., :c * ps * ps], want, "patchify")
    assert (got[..., c * ps * ps:] == 0).all() and got.shape == (n, h // ps, w // ps, pc)


@pytest.mark.parametrize("c", [1, 5, 12])
def test_dw_pack(c):
    w = torch.randn(c, 1, 7, 7, generator=_gen(c))
    p, pf = R.dw_pack(w), R.dw_pack(w, flip=True)
    assert p.dtype == w.dtype and p.shape == (49, c)
    assert torch.equal(p, w.view(c, 49).t()) and torch.equal(pf, torch.flip(w, (2, 3)).view(c, 49).t())
    assert p[8, c - 1] == w[c - 1, 0, 1, 1] and pf[8, c - 1] == w[c - 1, 0, 5, 5]


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shape", [(2, 3, 3, 5), (1, 5, 9, 13), (2, 4, 6, 2), (1, 2, 11, 7)])
def test_dwconv7(shape, bias):
    """Forward, input gradient and weight gradient, h and w below 7 included; the sums of |terms| are the same sums of |inputs|."""
    n, c, h, w = shape
    g = _gen(*shape)
    x = torch.randn(shape, generator=g, dtype=F64, requires_grad=True)
    wt = torch.randn(c, 1, 7, 7, generator=g, dtype=F64, requires_grad=True)
    b = torch.randn(c, generator=g, dtype=F64) if bias else None
    want = F.conv2d(x, wt, b, padding=3, groups=c)
    dy = torch.randn(shape, generator=g, dtype=F64)
    want.backward(dy)
    got, mag = R.dwconv7(x.detach(), wt.detach(), b)
    _close(got, want.detach(), "dwconv7")
    _close(mag, F.conv2d(x.detach().abs(), wt.detach().abs(), None if b is None else b.abs(), padding=3, groups=c), "dwconv7 |terms|")
    dx, dmag = R.dwconv7_dgrad(dy, wt.detach())
    _close(dx, x.grad, "dgrad")
    assert (dmag >= dx.abs() * (1 - 1e-12)).all()
    # the input gradient is the forward with the kernel rotated by 180 degrees: what the flipped pack feeds the same kernel
    _close(dx, R.dwconv7(dy, torch.flip(wt.detach(), (2, 3)))[0], "dgrad as a forward")
    dw, wmag = R.dwconv7_wgrad(dy, x.detach())
    _close(dw, wt.grad.view(c, 49), "wgrad")
    assert (wmag >= dw.abs() * (1 - 1e-12)).all()


@pytest.mark.parametrize("shape", [(2, 5, 3, 5), (1, 12, 4, 6), (3, 7, 2, 2)])
def test_layernorm2d(shape):
    n, c, h, w = shape
    g = _gen(*shape, 2)
    x = (torch.randn(shape, generator=g, dtype=F64) * 2 + 0.5).requires_grad_(True)
    gamma = (torch.rand(c, generator=g, dtype=F64) + 0.5).requires_grad_(True)
    beta = torch.randn(c, generator=g, dtype=F64).requires_grad_(True)
    eps = 1e-6
    want = F.layer_norm(x.permute(0, 2, 3, 1), (c,), gamma, beta, eps).permute(0, 3, 1, 2)
    dy = torch.randn(shape, generator=g, dtype=F64)
    want.backward(dy)
    out, mean, rstd = R.layernorm2d_fwd(x.detach(), gamma.detach(), beta.detach(), eps)
    _close(out, want.detach(), "out")
    _close(mean, x.detach().mean(1), "mean")
    _close(rstd, 1 / torch.sqrt(x.detach().var(1, unbiased=False) + eps), "rstd")
    dx, dgamma, dbeta, ag, ab = R.layernorm2d_bwd(dy, x.detach(), gamma.detach(), mean, rstd)
    _close(dx, x.grad, "dx")
    _close(dgamma, gamma.grad, "dgamma")
    _close(dbeta, beta.grad, "dbeta")
    assert (ag >= dgamma.abs() * (1 - 1e-12)).all() and torch.equal(ab, dy.abs().sum((0, 2, 3)))


@pytest.mark.parametrize("shape,c_pad", [((2, 5, 4, 6), 8), ((1, 3, 2, 2), 3), ((1, 12, 6, 4), 16)])
def test_s2d(shape, c_pad):
    """The layout is the one in which a 2x2 stride-2 conv is a 1x1 conv: channel (dy * 2 + dx) * c_pad + ch of F.unfold's patch."""
    n, c, h, w = shape
    v = torch.randn(shape, generator=_gen(*shape, c_pad), dtype=F64)
    t = R.s2d_fold(v, c_pad, fill=-7.0)
    assert t.shape == (n, h // 2, w // 2, 4 * c_pad)
    patches = F.unfold(v, 2, stride=2).view(n, c, 4, h // 2, w // 2)                       # [n, ch, dy * 2 + dx, oy, ox]
    t5 = t.view(n, h // 2, w // 2, 4, c_pad)
    assert torch.equal(t5[..., :c], patches.permute(0, 3, 4, 2, 1)) and (t5[..., c:] == -7.0).all()
    assert torch.equal(R.s2d_unfold(t, c, c_pad), v)
    # LayerNorm into the s2d layout followed by a 1x1 conv over 4 c_pad channels = LayerNorm followed by the 2x2 stride-2 conv
    g = _gen(c_pad)
    wt = torch.randn(6, c, 2, 2, generator=g, dtype=F64)
    w1 = torch.zeros(6, 4, c_pad, dtype=F64)
    w1[:, :, :c] = wt.permute(0, 2, 3, 1).reshape(6, 4, c)
    got = R.s2d_fold(v, c_pad) @ w1.view(6, 4 * c_pad).t()
    _close(got.permute(0, 3, 1, 2), F.conv2d(v, wt, stride=2), "transition conv")


@pytest.mark.parametrize("gate", [True, False])
@pytest.mark.parametrize("shape", [(3, 5, 3, 5), (2, 12, 1, 1), (4, 7, 2, 3)])
def test_ese_layerscale(shape, gate):
    """t * relu6(fc(mean(t)) + 3) / 6 * gamma and its autograd through image_channel_dot, ese_gate, scale_nc and ese_bwd, composed as
    the model composes them; u is scaled so that all three regions of the hard sigmoid occur."""
    n, c, h, w = shape
    hw = h * w
    g = _gen(*shape, gate)
    t = torch.randn(shape, generator=g, dtype=F64, requires_grad=True)
    wfc = (torch.randn(c, c, generator=g, dtype=F64) * 4).requires_grad_(True)
    bfc = (torch.randn(c, generator=g, dtype=F64) * 5).requires_grad_(True)
    gamma = (torch.rand(c, generator=g, dtype=F64) + 0.5).requires_grad_(True)
    if gate:
        u_t = F.conv2d(t.mean((2, 3), keepdim=True), wfc.view(c, c, 1, 1), bfc)
        want = t * (F.relu6(u_t + 3) / 6) * gamma.view(1, c, 1, 1)
    else:
        want = t * gamma.view(1, c, 1, 1)
    dout = torch.randn(shape, generator=g, dtype=F64)
    want.backward(dout)
    nhwc = lambda v: v.detach().permute(0, 2, 3, 1).reshape(n, hw, c)
    tt, dd = nhwc(t), nhwc(dout)
    s, s_abs = R.image_channel_dot(tt, None, 1.0 / hw)
    _close(s, t.detach().mean((2, 3)), "mean")
    _close(s_abs, t.detach().abs().mean((2, 3)), "mean |terms|")
    A, _ = R.image_channel_dot(dd, tt)
    if gate:
        u, gt, u_abs = R.ese_gate(s, wfc.detach(), bfc.detach())
        _close(u, u_t.detach().view(n, c), "u")
        assert (u < -3).any() and (u > 3).any() and (u.abs() < 3).any() and (u_abs >= u.abs() * (1 - 1e-12)).all()
        _close(R.scale_nc(tt, gt, gamma.detach()), nhwc(want), "out")
        r = R.ese_bwd(A, gamma.detach(), hw, gt, u, s, wfc.detach())
        _close(r["db_fc"], bfc.grad, "db_fc")
        _close(r["dW_fc"], wfc.grad, "dW_fc")
        _close(R.scale_nc(dd, gt, gamma.detach(), r["add"]), nhwc(t.grad), "dt")
        for k in ("dgamma", "db_fc", "dW_fc", "add"):
            assert (r[k + "_abs"] >= r[k].abs() * (1 - 1e-12)).all()
    else:
        _close(R.scale_nc(tt, None, gamma.detach()), nhwc(want), "out")
        r = R.ese_bwd(A, gamma.detach(), hw)
        _close(R.scale_nc(dd, None, gamma.detach()), nhwc(t.grad), "dt")
    _close(r["dgamma"], gamma.grad, "dgamma")
