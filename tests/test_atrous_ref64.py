"""Pins the float64 references of tests/_atrous_ref64.py against torch on the CPU (no GPU, no project imports)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _atrous_ref64 as R

F64 = torch.float64
U32 = 2.0 ** -24
DILS = [1, 2, 3, 6, 7, 9, 31]            # on 6 x 7: below, at and past each side (only the centre tap survives from 7 on)
RESIZES = [((7, 7), (7, 7)), ((1, 1), (8, 15)), ((1, 3), (15, 25)), ((3, 2), (13, 9)), ((6, 4), (13, 9)), ((5, 7), (6, 8)), ((2, 3), (16, 24))]


def _gen(*seed):
    return torch.Generator().manual_seed(sum(int(s) * (i + 3) for i, s in enumerate(seed)) + 99)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


# ---- im2col_dil / col2im_dil -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dil", DILS)
def test_im2col_dil_is_unfold(dil):
    n, h, w, c = 2, 6, 7, 5
    g = _gen(dil)
    x = torch.randn(n, h, w, c, generator=g, dtype=F64)
    col = R.im2col_dil(x, dil)
    assert col.shape == (n, h, w, 9, c)
    want = F.unfold(_nchw(x), 3, dilation=dil, padding=dil).view(n, c, 9, h, w)
    assert torch.equal(col.permute(0, 4, 3, 1, 2), want)
    if dil >= max(h, w):
        assert (col[:, :, :, [0, 1, 2, 3, 5, 6, 7, 8]] == 0).all() and torch.equal(col[:, :, :, 4], x)
    # tap order, stated once by hand: tap 0 is (dy, dx) = (-1, -1), tap 5 is (0, +1)
    if dil < min(h, w):
        assert torch.equal(col[:, dil:, dil:, 0], x[:, :h - dil, :w - dil]) and torch.equal(col[:, :, :w - dil, 5], x[:, :, dil:])
    # prologue: relu(x * scale + shift), rounded to the storage type
    scale, shift = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    for dt in (None, torch.bfloat16, torch.float16):
        a = torch.relu(x * scale.double() + shift.double())
        a = a if dt is None else a.to(dt).double()
        want = F.unfold(_nchw(a), 3, dilation=dil, padding=dil).view(n, c, 9, h, w)
        assert torch.equal(R.im2col_dil(x, dil, scale, shift, dt).permute(0, 4, 3, 1, 2), want)


@pytest.mark.parametrize("dil", DILS)
def test_col2im_dil_is_fold_and_the_conv_gradient(dil):
    n, h, w, c, co = 2, 6, 7, 5, 4
    g = _gen(dil, 1)
    dcol = torch.randn(n, h, w, 9, c, generator=g, dtype=F64)
    want = F.fold(dcol.permute(0, 4, 3, 1, 2).reshape(n, c * 9, h * w), (h, w), 3, dilation=dil, padding=dil)
    torch.testing.assert_close(_nchw(R.col2im_dil(dcol, dil)), want, rtol=0, atol=1e-13)
    # adjoint: <im2col x, dcol> == <x, col2im dcol>
    x = torch.randn(n, h, w, c, generator=g, dtype=F64)
    lhs, rhs = (R.im2col_dil(x, dil) * dcol).sum(), (x * R.col2im_dil(dcol, dil)).sum()
    assert abs(lhs - rhs) <= 1e-12 * (R.im2col_dil(x, dil) * dcol).abs().sum()
    # a dilated conv is a 1x1 conv over the nine copies; its input gradient is the fold of the 1x1 gradient
    wt = torch.randn(co, c, 3, 3, generator=g, dtype=F64)
    xr = _nchw(x).clone().requires_grad_(True)
    y = F.conv2d(xr, wt, padding=dil, dilation=dil)
    w9 = wt.permute(0, 2, 3, 1).reshape(co, 9, c)                              # [co, t, ci]
    torch.testing.assert_close(torch.einsum("nhwtc,otc->nhwo", R.im2col_dil(x, dil), w9), _nhwc(y), rtol=0, atol=1e-12)
    dy = torch.randn(n, h, w, co, generator=g, dtype=F64)
    y.backward(_nchw(dy))
    torch.testing.assert_close(R.col2im_dil(torch.einsum("nhwo,otc->nhwtc", dy, w9), dil), _nhwc(xr.grad), rtol=0, atol=1e-12)


def test_pointwise_and_statistics():
    g = _gen(5)
    x = torch.randn(3, 4, 5, 6, generator=g, dtype=F64)
    sc, sh = torch.rand(6, generator=g, dtype=F64) + 0.5, torch.randn(6, generator=g, dtype=F64)
    assert torch.equal(R.affine_relu(x, sc, sh), torch.relu(x * sc + sh)) and torch.equal(R.preact_mask(x, sc, sh), x * sc + sh > 0)
    assert torch.equal(R.sum_list([x, x * 2, -x], True), torch.relu(x + x * 2 - x)) and torch.equal(R.sum_list([x], False), x)
    assert torch.equal(R.relu_mask(x, sh.expand_as(x)), torch.where(sh > 0, x, torch.zeros_like(x)))
    s1, s2 = R.channel_stats(x)
    torch.testing.assert_close(s1, x.sum((0, 1, 2)), rtol=1e-14, atol=0)
    torch.testing.assert_close(s2, (x ** 2).sum((0, 1, 2)), rtol=1e-14, atol=0)
    # BatchNorm backward: d(beta) and d(gamma) of gamma * (y - mean) * invstd + beta with mean / invstd held fixed
    gam, bet = torch.ones(6, dtype=F64, requires_grad=True), torch.zeros(6, dtype=F64, requires_grad=True)
    dz = torch.randn(3, 4, 5, 6, generator=g, dtype=F64)
    (gam * (x - sh) * sc + bet).backward(dz)
    b1, b2 = R.bn_bwd_stats(dz, x, sh, sc)
    torch.testing.assert_close(b1, bet.grad, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(b2, gam.grad, rtol=1e-13, atol=1e-13)
    xin = torch.rand(2, 3, 4, 5, generator=g) * 255
    out = R.input_plain(xin, 8, 1 / 255, -0.5)
    assert torch.equal(out[..., :3], _nhwc(xin.double() * (1 / 255) - 0.5)) and (out[..., 3:] == 0).all()


# ---- max pooling -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("hw", [(8, 8), (13, 9), (10, 14), (15, 25), (16, 24)])
def test_maxpool_k_and_its_gradient(k, hw):
    (h, w), n, c = hw, 2, 3
    g = _gen(k, h, w)
    x = torch.randint(-3, 4, (n, h, w, c), generator=g).double() * 0.5          # many exact ties
    x[0, :k, :k, 0] = float("-inf")
    x[1, 0, 0, 1] = float("inf")
    xr = _nchw(x).clone().requires_grad_(True)
    y = F.max_pool2d(xr, k)
    assert torch.equal(R.maxpool_k(x, k), _nhwc(y))
    dp = torch.randn(n, h // k, w // k, c, generator=g, dtype=F64)
    y.backward(_nchw(dp))
    got = R.maxpool_k_bwd(x, dp, k)
    assert torch.equal(got, _nhwc(xr.grad))
    assert (got[:, (h // k) * k:] == 0).all() and (got[:, :, (w // k) * k:] == 0).all()
    assert got[0, 0, 0, 0] == dp[0, 0, 0, 0] and (got != 0).sum() == (dp != 0).sum()         # the -inf window: its first pixel


# ---- bilinear resize ---------------------------------------------------------------------------------------------------------------
def _weights64(in_size, out_size):
    """The [out, in] weight matrix with float64 coordinates (torch's float64 path)."""
    src = np.maximum((np.arange(out_size) + 0.5) * (in_size / out_size) - 0.5, 0.0)
    i0 = np.minimum(src.astype(np.int64), in_size - 1)
    i1 = np.minimum(i0 + 1, in_size - 1)
    a = np.zeros((out_size, in_size))
    np.add.at(a, (np.arange(out_size), i0), 1.0 - (src - i0))
    np.add.at(a, (np.arange(out_size), i1), src - i0)
    return torch.from_numpy(a)


@pytest.mark.parametrize("src,dst", RESIZES)
def test_bilinear_taps_and_up(src, dst):
    (hs, ws), (h, w) = src, dst
    for a, b in ((hs, h), (ws, w)):
        i0, i1, l1 = R.bilinear_taps(a, b)
        assert l1.dtype == np.float32 and (0 <= l1).all() and (l1 < 1).all() and (i0 >= 0).all() and (i1 <= a - 1).all() and (i1 - i0 <= 1).all()
        wm = R.bilinear_weights(a, b)
        torch.testing.assert_close(wm.sum(1), torch.ones(b, dtype=F64), rtol=0, atol=1e-15)
    x = torch.randn(2, hs, ws, 3, generator=_gen(hs, ws, h, w))
    want = _nhwc(F.interpolate(_nchw(x), size=(h, w), mode="bilinear", align_corners=False)).double()
    got = R.bilinear_up(x, h, w)
    err, bound = (got - want).abs().max().item(), 4 * U32 * x.abs().max().item()
    print(f"bilinear_up {src}->{dst}: max err {err:.3g}, bound {bound:.3g}")
    assert err <= bound
    torch.testing.assert_close(got, torch.einsum("yq,nqpc,xp->nyxc", R.bilinear_weights(hs, h), x.double(), R.bilinear_weights(ws, w)),
                               rtol=0, atol=1e-14)


def test_bilinear_coordinates_are_fused_where_torch_fuses_them():
    """At 161 -> 323 the product rounded on its own moves a coordinate by up to 2^-17: torch's vectorised CPU kernels (AVX2 / AVX512
    builds, which have FMA) fuse it, and so do the reference and the kernel.  Checked where this torch runs such a kernel."""
    if "AVX" not in torch.backends.cpu.get_cpu_capability().upper():
        return
    (hs, ws), (h, w) = (161, 162), (323, 325)
    x = torch.randn(1, hs, ws, 2, generator=_gen(161))
    want = _nhwc(F.interpolate(_nchw(x), size=(h, w), mode="bilinear", align_corners=False)).double()
    err, bound = (R.bilinear_up(x, h, w) - want).abs().max().item(), 4 * U32 * x.abs().max().item()
    print(f"bilinear_up 161x162 -> 323x325: max err {err:.3g}, bound {bound:.3g}")
    assert err <= bound


@pytest.mark.parametrize("src,dst", RESIZES + [((39, 37), (40, 41))])
def test_bilinear_up_bwd(src, dst):
    """Against autograd of F.interpolate in float64, whose coordinates are float64.  The weight of source index q at destination y is
    hat(src_y - q) (with both clamps folded in), 1-Lipschitz in src_y, and the float32 src_y carries roundings of values up to
    `in` (the scale, the fused product and difference, one to spare): |d weight| <= |d l1| <= 4 in 2^-24 per axis.  A product of two weights <= 1 moves
    by at most the sum, so |d din[q]| <= 4 2^-24 (hs + ws) sum |dout| over the destination pixels that reach q in either version."""
    (hs, ws), (h, w) = src, dst
    n, c = 2, 3
    dout = torch.randn(n, h, w, c, generator=_gen(hs, ws, h, w, 2), dtype=F64)
    din, count, abs_sum = R.bilinear_up_bwd(dout, hs, ws)
    xr = torch.zeros(n, c, hs, ws, dtype=F64, requires_grad=True)
    F.interpolate(xr, size=(h, w), mode="bilinear", align_corners=False).backward(_nchw(dout))
    reach = []
    for a, b in ((hs, h), (ws, w)):
        w32, w64 = R.bilinear_weights(a, b), _weights64(a, b)
        tap_err, tap_bound = (w32 - w64).abs().max().item(), 4 * a * U32
        print(f"taps {a}->{b}: max |f32 - f64 weight| {tap_err:.3g}, bound {tap_bound:.3g}")
        assert tap_err <= tap_bound
        reach.append(((w32 != 0) | (w64 != 0)).double())
    bound = 4 * U32 * (hs + ws) * torch.einsum("yq,nyxc,xp->nqpc", reach[0], dout.abs(), reach[1])
    err = (din - _nhwc(xr.grad)).abs()
    print(f"bilinear_up_bwd {src}->{dst}: max err {err.max().item():.3g}, max err / bound {(err / bound).max().item():.3g}")
    assert (err <= bound).all()
    # exact adjoint of the reference's own forward, and the two by-products
    x = torch.randn(n, hs, ws, c, generator=_gen(7), dtype=F64)
    lhs, rhs = (R.bilinear_up(x, h, w) * dout).sum(), (x * din).sum()
    assert abs(lhs - rhs) <= 1e-13 * (R.bilinear_up(x.abs(), h, w) * dout.abs()).sum()
    wy, wx = R.bilinear_weights(hs, h), R.bilinear_weights(ws, w)
    assert torch.equal(count, (wy != 0).sum(0)[:, None] * (wx != 0).sum(0)[None, :]) and count.sum() >= h * w
    torch.testing.assert_close(abs_sum, torch.einsum("yq,nyxc,xp->nqpc", wy, dout.abs(), wx), rtol=1e-13, atol=0)
    assert (abs_sum >= din.abs() * (1 - 1e-12)).all()
