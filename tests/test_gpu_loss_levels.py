"""The SSIM / MS-SSIM loss kernels of csrc/loss.hip one by one, per level, against the f64 reference of tests/_loss_ref64.py.

Every kernel is driven through its ops.* wrapper on buffers the test owns, at the smallest shapes that reach its edges: one valid
position, a second tile of one column, a tile of L1 pixels without a valid SSIM position, windows 3 .. 33 of the generic pair.
A level has 3 planes of different content with upstream weights (+a, 0, -b); each case runs with the coarser level's gradient and
the L1 term present, and with both absent (which also shrinks the forward grid to the valid region).

Tolerances are measured, not chosen: the same reference runs in f32 on the CPU, E32 is its max-norm error against the f64 run, and a
kernel may be off by FACTOR = 16 times max(E32, 2^-23 max|ref|) -- it rounds in another order than torch's f32 convolution (FMA
chains, f32 partial sums of up to 1024 terms in front of the f64 atomics, a tile-wise tree), so its error is of E32's size without
being E32.  Comparisons that are exact by construction (in-kernel division, the striped fold, the pair entry of the pooling) are
asserted bit for bit; pooling to 2 ulp (three f32 additions and an exact * 0.25), the weights kernel to 4 ulp of its f32 outputs
(f64 arithmetic, rounded once).

Run with -s to see the worst err / max(E32, floor) of each group; on an MI355X they were (allowed: 16):
    a fwd_k<11>, fwd_adj_k<11>   1.47   (ssim sums at (11, 11); L1 sum 0.81)        a bwd_k<11>, bwd_adj_k<11>   3.65   (dx at (11, 11))
    a bwd routes, each other     0.80                                               b in_div                     0.96
    c fwd_kernel                 1.99   (L1 sum, k = 33; sums 0.68)                 c bwd_kernel                 1.15   (k = 21)
    c asymmetric                 0.65                                               f SSIMLoss                   3.84   (gradient, (1,1,161,161))
    f degenerate                 1.16                                               f ssim() / f routes          0.06 / 0.44
The file runs in 4 s.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from _loss_ref64 import bound, compose, level, pool, weights
from oracle import loss_ref as Lr

pytestmark = pytest.mark.gpu

P = 3
C1, C2 = float(np.float32(0.01 ** 2)), float(np.float32(0.03 ** 2))      # the kernels take the constants as f32
WTS = (0.75, 0.0, -1.25)
L1C = 0.375
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    yield
    for group in sorted(WORST):
        print(f"\nworst err / max(E32, floor) [{group}]: {WORST[group]:.3f}", end="")
    print()


def _check(group, got, ref64, ref32, what=""):
    """max-norm error of `got` against ref64 within FACTOR * max(E32, floor); records the ratio of the group."""
    ref64 = torch.as_tensor(ref64, dtype=torch.float64)
    got = torch.as_tensor(got).detach().cpu().double().reshape(ref64.shape)
    assert torch.isfinite(got).all(), f"{group} {what}: non-finite values"
    tol, den = bound(ref64, ref32)
    err = (got - ref64).abs().max().item()
    ratio = err / den if den > 0 else (0.0 if err == 0 else float("inf"))
    WORST[group] = max(WORST.get(group, 0.0), ratio)
    print(f"  [{group}] {what}: err {err:.3e}  E32-or-floor {den:.3e}  ratio {ratio:.3f}")
    assert err <= tol, f"{group} {what}: error {err:.3e} is {ratio:.1f} x max(E32, floor) = {den:.3e} (allowed {tol / den:.0f} x)"


def _planes(h, w, seed, planes=P):
    """planes of different content in [0, 1]: noise, low-contrast noise, a ramp with noise; x = 0.7 y + 0.3 noise, so x != y"""
    g = torch.Generator().manual_seed(seed)
    y = torch.rand(planes, h, w, generator=g)
    if planes >= 3:
        y[1] = 0.25 + 0.5 * y[1]
        ramp = (torch.arange(h)[:, None] / max(h - 1, 1) + torch.arange(w)[None, :] / max(w - 1, 1)) / 2
        y[2] = 0.5 * ramp + 0.5 * y[2]
    x = 0.7 * y + 0.3 * torch.rand(planes, h, w, generator=g)
    return x, y


def _pooled(n):
    return (n + 2 * (n & 1) - 2) // 2 + 1


def _window(k, sigma):
    if sigma is None:                                   # normalised, asymmetric
        w = torch.arange(1, k + 1, dtype=torch.float32)
        return w / w.sum()
    return Lr.gauss_1d(k, sigma)


@functools.lru_cache(maxsize=None)
def _case(h, w, k, sigma, use_ssim, extras):
    """inputs and the f64 / f32 references of one level; extras: 'all' (coarse gradient + L1), 'pool' (coarse gradient), 'none'"""
    c = SimpleNamespace(h=h, w=w, k=k, use_ssim=use_ssim, hc=_pooled(h), wc=_pooled(w))
    c.win = _window(k, sigma)
    c.win_list = [float(v) for v in c.win]
    c.x, c.y = _planes(h, w, 1000 * h + w)
    c.wts = torch.tensor(WTS)
    g = torch.Generator().manual_seed(h * w + k)
    c.dc = torch.randn(P, c.hc, c.wc, generator=g) if extras in ("all", "pool") else None
    c.l1c = L1C if extras == "all" else 0.0
    c.with_l1 = extras == "all"
    c.r64 = level(c.x.double(), c.y.double(), c.win, C1, C2, c.wts.double(), use_ssim, c.dc, c.l1c)
    c.r32 = level(c.x, c.y, c.win, C1, C2, c.wts, use_ssim, c.dc, c.l1c)
    c.xg, c.yg, c.wg = c.x.cuda(), c.y.cuda(), c.wts.cuda()
    c.dcg = c.dc.cuda() if c.dc is not None else None
    c.l1cg = torch.tensor([c.l1c], device="cuda") if c.with_l1 else None
    return c


def _check_sums(group, c, sums, l1, what):
    sums = sums.cpu().view(P, 2)
    _check(group, sums[:, 0], c.r64[0][:, 0], c.r32[0][:, 0], f"{what} cs sums")
    _check(group, sums[:, 1], c.r64[0][:, 1], c.r32[0][:, 1], f"{what} ssim sums")
    if c.with_l1:
        _check(group, l1.cpu().reshape(()), c.r64[1], c.r32[1], f"{what} L1 sum")


def _run_fwd(c):
    from pssr2_amd import ops
    sums = torch.zeros(P * 2, dtype=torch.float64, device="cuda")
    l1 = torch.zeros(1, dtype=torch.float64, device="cuda") if c.with_l1 else None
    ops.ssim_level_fwd(c.xg, c.yg, P, c.h, c.w, c.win_list, C1, C2, sums, l1)
    return sums, l1


def _run_fwd_adj(c, stripes, x=None, y=None, in_div=1.0):
    """-> (raw striped buffer [2 stripes][P * 2 + 2], adjoint maps); adj starts as NaN: the kernel writes the valid region only"""
    from pssr2_amd import ops
    stride = P * 2 + 2
    buf = torch.zeros(2 * stripes * stride, dtype=torch.float64, device="cuda")
    adj = torch.full((P * 3 * c.h * c.w,), float("nan"), device="cuda")
    ops.ssim_level_fwd_adj(c.xg if x is None else x, c.yg if y is None else y, P, c.h, c.w, c.win_list, C1, C2, c.use_ssim, buf,
                           buf[P * 2:P * 2 + 1] if c.with_l1 else None, stripes, stride, adj, in_div)
    return buf, adj


def _fold(buf, stripes):
    rows = buf.cpu().view(2 * stripes, P * 2 + 2).sum(0)
    return rows[:P * 2], rows[P * 2]


def _run_bwd(c):
    from pssr2_amd import ops
    dx = torch.full((P, c.h, c.w), float("nan"), device="cuda")
    ops.ssim_level_bwd(c.xg, c.yg, P, c.h, c.w, c.win_list, C1, C2, c.wg, c.use_ssim, c.dcg, c.hc, c.wc, c.l1cg, dx)
    return dx


def _run_bwd_adj(c, adj, x=None, y=None, in_div=1.0):
    from pssr2_amd import ops
    dx = torch.full((P, c.h, c.w), float("nan"), device="cuda")
    ops.ssim_level_bwd_adj(c.xg if x is None else x, c.yg if y is None else y, adj, P, c.h, c.w, c.win_list, c.wg, c.dcg, c.hc, c.wc,
                           c.l1cg, dx, in_div)
    return dx


# ---------------------------------------------------------------------------------------------------------------------
# a. level kernels, 11-tap window
SHAPES11 = [(11, 11), (12, 43), (42, 33), (43, 75)]
EXTRAS = ["all", "none"]


@pytest.mark.parametrize("extras", EXTRAS)
@pytest.mark.parametrize("use_ssim", [0, 1])
@pytest.mark.parametrize("shape", SHAPES11)
def test_level_forward_k11(shape, use_ssim, extras):
    """ssim_fwd_k<11> (ops.ssim_level_fwd) and ssim_fwd_adj_k<11> with 16, 5 and 1 stripes: sums and L1 sum"""
    c = _case(*shape, 11, 1.5, use_ssim, extras)
    sums, l1 = _run_fwd(c)
    _check_sums("a fwd_k<11>", c, sums, l1, f"{shape}")
    for stripes in (16, 5, 1):
        buf, adj = _run_fwd_adj(c, stripes)
        fs, fl1 = _fold(buf, stripes)
        _check_sums("a fwd_adj_k<11>", c, fs, fl1, f"{shape} stripes={stripes}")
        a = adj.view(P, 3, c.h, c.w)
        assert torch.isfinite(a[:, :, :c.h - 10, :c.w - 10]).all()
        if not c.with_l1:
            assert buf.view(2 * stripes, -1)[:, P * 2:].abs().max().item() == 0.0          # no L1 sum asked for: none written


@pytest.mark.parametrize("extras", EXTRAS)
@pytest.mark.parametrize("use_ssim", [0, 1])
@pytest.mark.parametrize("shape", SHAPES11)
def test_level_backward_k11(shape, use_ssim, extras):
    """ssim_bwd_k<11> (ops.ssim_level_bwd) and the ssim_fwd_adj_k / ssim_bwd_adj_k pair: dx against f64 and against each other.
    The adjoint buffer is NaN outside the valid region, so a finite dx proves that the backward kernel reads nothing there."""
    c = _case(*shape, 11, 1.5, use_ssim, extras)
    dx_k = _run_bwd(c)
    _check("a bwd_k<11>", dx_k, c.r64[2], c.r32[2], f"{shape} dx")
    _, adj = _run_fwd_adj(c, 16)
    dx_adj = _run_bwd_adj(c, adj)
    assert torch.isfinite(dx_adj).all()
    _check("a bwd_adj_k<11>", dx_adj, c.r64[2], c.r32[2], f"{shape} dx")
    # the two routes differ by the rounding of one reassociated product per adjoint value (wt * (..) against (wt * ..)): the same
    # kind of error as either has against f64, so the same bound
    tol, den = bound(c.r64[2], c.r32[2])
    diff = (dx_k - dx_adj).abs().max().item()
    WORST["a bwd routes"] = max(WORST.get("a bwd routes", 0.0), diff / den)
    assert diff <= tol, f"bwd_k and bwd_adj differ by {diff:.3e} = {diff / den:.1f} x max(E32, floor)"


# ---------------------------------------------------------------------------------------------------------------------
# b. in-kernel division
@pytest.mark.parametrize("use_ssim", [0, 1])
def test_level_in_div_is_the_level_of_the_quotients(use_ssim):
    """fwd_adj / bwd_adj with in_div = 255 on [0, 255] inputs: the sums of the pair on x / 255, y / 255 bit for bit (the two exact
    pieces per sum make the f64 atomics order-independent), and that run's dx / 255 bit for bit."""
    c = _case(43, 75, 11, 1.5, use_ssim, "all")
    x255, y255 = c.xg * 255, c.yg * 255
    xq, yq = x255 / 255, y255 / 255
    buf_a, adj_a = _run_fwd_adj(c, 16, x255, y255, 255.0)
    buf_b, adj_b = _run_fwd_adj(c, 16, xq, yq)
    assert torch.equal(buf_a, buf_b)
    assert torch.equal(torch.nan_to_num(adj_a, nan=-7.0), torch.nan_to_num(adj_b, nan=-7.0))
    dx_a = _run_bwd_adj(c, adj_a, x255, y255, 255.0)
    dx_b = _run_bwd_adj(c, adj_b, xq, yq)
    assert torch.isfinite(dx_a).all() and torch.equal(dx_a, dx_b / 255)
    # and the quotient run is an ordinary level: against f64 of the same quotients
    r64 = level(xq.cpu().double(), yq.cpu().double(), c.win, C1, C2, c.wts.double(), use_ssim, c.dc, c.l1c)
    r32 = level(xq.cpu(), yq.cpu(), c.win, C1, C2, c.wts, use_ssim, c.dc, c.l1c)
    _check("b in_div", dx_b, r64[2], r32[2], "dx of the quotients")


@pytest.mark.parametrize("shape", [(43, 75), (1, 7)])
def test_pool_in_div_is_the_pool_of_the_quotients(shape):
    from pssr2_amd import ops
    h, w = shape
    x, y = _planes(h, w, 77)
    x255, y255 = x.cuda() * 255, y.cuda() * 255
    outs = [torch.full((P, _pooled(h), _pooled(w)), float("nan"), device="cuda") for _ in range(4)]
    ops.avgpool2_pair(x255, y255, outs[0], outs[1], P, h, w, 255.0)
    ops.avgpool2_pair(x255 / 255, y255 / 255, outs[2], outs[3], P, h, w)
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3])


# ---------------------------------------------------------------------------------------------------------------------
# c. generic kernels
GENERIC = [(3, 0.8, (5, 9)), (7, 1.0, (40, 39)), (21, 3.0, (53, 85)), (33, 5.0, (33, 70))]


@pytest.mark.parametrize("extras", EXTRAS)
@pytest.mark.parametrize("k,sigma,shape", GENERIC)
def test_generic_forward(k, sigma, shape, extras):
    c = _case(*shape, k, sigma, 0, extras)
    sums, l1 = _run_fwd(c)
    _check_sums("c fwd_kernel", c, sums, l1, f"k={k} {shape}")


@pytest.mark.parametrize("extras", EXTRAS)
@pytest.mark.parametrize("use_ssim", [0, 1])
@pytest.mark.parametrize("k,sigma,shape", GENERIC[:3])
def test_generic_backward(k, sigma, shape, use_ssim, extras):
    c = _case(*shape, k, sigma, use_ssim, extras)
    _check("c bwd_kernel", _run_bwd(c), c.r64[2], c.r32[2], f"k={k} {shape} dx")


@pytest.mark.parametrize("use_ssim", [0, 1])
def test_generic_asymmetric_window(use_ssim):
    """A normalised window with win[t] != win[k-1-t]: tells a correlation from a convolution in the forward pass and a transposed
    filter from the filter itself in the backward pass, which no Gaussian can.  Without the L1 term, whose border mass is defined
    for symmetric windows only."""
    c = _case(40, 39, 7, None, use_ssim, "pool")
    sums, l1 = _run_fwd(c)
    _check_sums("c asymmetric", c, sums, l1, "k=7 fwd")
    _check("c asymmetric", _run_bwd(c), c.r64[2], c.r32[2], "k=7 dx")


def test_window_limits():
    """The forward takes windows up to 33 taps and refuses 35; the backward's LDS check passes 21 (test_generic_backward) and
    refuses 23 before any launch, after which a valid call works as before."""
    from pssr2_amd import ops
    c = _case(40, 39, 7, 1.0, 1, "all")
    x, y = c.xg, c.yg
    sums = torch.zeros(P * 2, dtype=torch.float64, device="cuda")
    dx = torch.zeros(P, c.h, c.w, device="cuda")
    with pytest.raises(RuntimeError, match="pssr_ssim_level_fwd failed"):
        ops.ssim_level_fwd(x, y, P, c.h, c.w, [1 / 35] * 35, C1, C2, sums)
    with pytest.raises(RuntimeError, match=r"window 23 needs \d+ bytes of LDS"):
        ops.ssim_level_bwd(x, y, P, c.h, c.w, [float(v) for v in Lr.gauss_1d(23, 3.0)], C1, C2, c.wg, 1, None, 0, 0, None, dx)
    torch.cuda.synchronize()
    assert sums.abs().max().item() == 0.0 and dx.abs().max().item() == 0.0          # refused before any launch
    _check("c bwd_kernel", _run_bwd(c), c.r64[2], c.r32[2], "k=7 dx after the refused call")


# ---------------------------------------------------------------------------------------------------------------------
# d. pooling
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (6, 8), (43, 75), (161, 161)])
def test_pooling(shape):
    from pssr2_amd import ops
    h, w = shape
    ho, wo = _pooled(h), _pooled(w)
    x, y = _planes(h, w, 5 * h + w)
    xg, yg = x.cuda(), y.cuda()
    single = [torch.full((P, ho, wo), float("nan"), device="cuda") for _ in range(2)]
    pair = [torch.full((P, ho, wo), float("nan"), device="cuda") for _ in range(2)]
    ops.avgpool2_planes(xg, single[0], P, h, w)
    ops.avgpool2_planes(yg, single[1], P, h, w)
    ops.avgpool2_pair(xg, yg, pair[0], pair[1], P, h, w)
    for src, out, both in zip((x, y), single, pair):
        ref = pool(src.double())
        assert ref.shape == out.shape
        ulp = torch.from_numpy(np.spacing(ref.abs().numpy().astype(np.float32))).double()
        err = (out.cpu().double() - ref).abs()
        assert (err <= 2 * ulp).all(), f"pooling {shape}: {(err / ulp).max().item():.2f} ulp"
        assert torch.equal(out, both)


# ---------------------------------------------------------------------------------------------------------------------
# e. weights kernel
NVALID = [24613.0, 5893.0, 1333.0, 253.0, 33.0, 7.0, 3.0, 1.0]
L1_SUM = 12345.6789


def _synthetic_sums(planes, levels, seed):
    """[levels][planes][2] sums, multiples of 2^-10, whose level means lie in +-[0.3, 0.95]: plane p has, by p % 4, no negative
    level, one, two, or only negative levels"""
    g = torch.Generator().manual_seed(seed)
    mean = 0.3 + 0.65 * torch.rand(levels, planes, 2, generator=g, dtype=torch.float64)
    for p in range(planes):
        pat, first = p % 4, (p // 4) % levels
        neg = [] if pat == 0 else [first] if pat == 1 else [first, (first + 1) % levels] if pat == 2 else range(levels)
        for l in neg:
            mean[l, p] *= -1
    nv = torch.tensor(NVALID[:levels], dtype=torch.float64)
    sums = torch.round(mean * nv[:, None, None] * 1024) / 1024
    used = torch.stack([sums[l, :, 1 if l == levels - 1 else 0] / nv[l] for l in range(levels)])
    assert used.abs().min().item() >= 0.05 and (sums[0, :, 1] / nv[0]).abs().min().item() >= 0.05     # no clamp decision near 0
    return sums


def _level_weights(levels):
    if levels == 5:
        return torch.tensor(Lr.MS_WEIGHTS)
    w = torch.arange(1, levels + 1, dtype=torch.float32) ** 0.5
    return w / w.sum()


def _run_weights(sums_dev, levels, planes, lw, ms, mix, l1_dev, numel, go, striped=None):
    from pssr2_amd import ops
    nv = torch.tensor(NVALID[:levels], dtype=torch.float64, device="cuda")
    loss = torch.full((1,), float("nan"), device="cuda")
    wts = torch.full((levels * planes,), float("nan"), device="cuda")
    l1c = torch.full((1,), float("nan"), device="cuda")
    go_dev = None if go is None else torch.tensor([go], device="cuda")
    if striped is None:
        ops.msssim_weights(sums_dev, levels, planes, nv, lw.cuda(), ms, mix, l1_dev, numel, go_dev, loss, wts, l1c)
    else:
        stripes, stride, folded = striped
        ops.msssim_weights_striped(sums_dev, stripes, stride, folded, levels, planes, nv, lw.cuda(), ms, mix, l1_dev, numel, go_dev, loss, wts, l1c)
    return loss.cpu(), wts.cpu().view(levels, planes), l1c.cpu()


def _assert_ulps(got, ref, n, what):
    ref = torch.as_tensor(ref, dtype=torch.float64).reshape(got.shape)
    ulp = torch.from_numpy(np.spacing(ref.abs().numpy().astype(np.float32))).double()
    zero = ref == 0
    assert (got[zero] == 0).all(), f"{what}: non-zero where the reference is exactly 0"
    err = (got.double() - ref).abs()
    assert torch.isfinite(got).all() and (err[~zero] <= n * ulp[~zero]).all(), f"{what}: {(err[~zero] / ulp[~zero]).max().item():.2f} ulp"


@pytest.mark.parametrize("levels", [1, 3, 5, 8])
@pytest.mark.parametrize("planes", [1, 256, 300])
def test_weights_kernel(planes, levels):
    sums = _synthetic_sums(planes, levels, 10 * planes + levels)
    sums_dev = sums.flatten().cuda()
    lw = _level_weights(levels)
    numel = float(planes * 1000)
    l1_dev = torch.tensor([L1_SUM], dtype=torch.float64, device="cuda")
    for ms in (0, 1):
        for mix in (0.0, 0.8, 1.0):
            for go in (None, 1.5):
                with_l1 = mix < 1
                loss, wts, l1c = _run_weights(sums_dev, levels, planes, lw, ms, mix, l1_dev if with_l1 else None, numel, go)
                mix32 = float(np.float32(mix))                         # what the kernel receives
                rl, rw, rc = weights(sums, NVALID[:levels], lw.double(), ms, mix32, L1_SUM if with_l1 else None, numel, go)
                what = f"planes={planes} levels={levels} ms={ms} mix={mix} go={go}"
                _assert_ulps(loss, [rl], 4, what + " loss")
                _assert_ulps(l1c, [rc], 4, what + " l1_coef")
                if ms:
                    _assert_ulps(wts, rw, 4, what + " wts")
                    if planes >= 4 and mix > 0:
                        assert (wts[:, 3] == 0).all() and (wts[:, 1] == 0).all() and (wts[:, 0] != 0).all()
                else:
                    _assert_ulps(wts[0], rw[0], 4, what + " wts")      # plain SSIM: level 0 only


@pytest.mark.parametrize("stripes", [16, 5, 1])
@pytest.mark.parametrize("planes,levels", [(1, 1), (1, 5), (300, 1), (300, 5)])
def test_weights_kernel_striped_fold(planes, levels, stripes):
    """msssim_weights_striped == msssim_weights on the host-folded sums, bit for bit -- for ONE stripe too: ssim_fwd_adj_k writes two
    pieces per sum whatever the stripe count, so the striped entry folds whenever it is used.  The pieces are multiples of 2^-10,
    so every order of adding them is exact."""
    nvals = levels * planes * 2
    stride, rows = nvals + 2, 2 * stripes
    target = torch.cat([_synthetic_sums(planes, levels, 10 * planes + levels).flatten(), torch.tensor([round(L1_SUM * 1024) / 1024], dtype=torch.float64)])
    g = torch.Generator().manual_seed(stripes)
    buf = torch.zeros(rows, stride, dtype=torch.float64)
    buf[:rows - 1, :nvals + 1] = torch.randint(-4096, 4097, (rows - 1, nvals + 1), generator=g).double() / 1024
    buf[rows - 1, :nvals + 1] = target - buf[:rows - 1, :nvals + 1].sum(0)
    assert torch.equal(buf[:, :nvals + 1].sum(0), target) and buf[rows // 2:].abs().max().item() > 1
    lw = _level_weights(levels)
    numel = float(planes * 1000)
    for mix, go in ((0.8, None), (0.8, 1.5), (1.0, None)):
        with_l1 = mix < 1
        dev = torch.cat([buf.flatten(), torch.full((nvals + 1,), float("nan"), dtype=torch.float64)]).cuda()
        folded = dev[rows * stride:]
        got = _run_weights(dev, levels, planes, lw, 1, mix, dev[nvals:nvals + 1] if with_l1 else None, numel, go, (stripes, stride, folded))
        host = target.cuda()
        want = _run_weights(host, levels, planes, lw, 1, mix, host[nvals:nvals + 1] if with_l1 else None, numel, go)
        assert torch.equal(folded[:nvals].cpu(), target[:nvals])
        for a, b in zip(got, want):
            assert torch.isfinite(a).all() and torch.equal(a, b)


def test_one_stripe_level_feeds_the_striped_weights():
    """fwd_adj with stripes = 1 and a stride, at one valid position per plane, then the striped weights entry: the low pieces
    (everything below 2^-20 of each sum) must arrive, i.e. the result is that of the host-folded sums."""
    c = _case(11, 11, 11, 1.5, 1, "all")
    buf, _ = _run_fwd_adj(c, 1)
    stride = P * 2 + 2
    assert buf.view(2, stride)[1].abs().max().item() > 0                         # there are low pieces
    lw = torch.tensor([1.0])
    dev = torch.cat([buf, torch.full((P * 2 + 1,), float("nan"), dtype=torch.float64, device="cuda")])
    got = _run_weights(dev, 1, P, lw, 1, 0.8, dev[P * 2:P * 2 + 1], float(P * 121), None, (1, stride, dev[2 * stride:]))
    host = buf.view(2, stride).sum(0)
    want = _run_weights(host, 1, P, lw, 1, 0.8, host[P * 2:P * 2 + 1], float(P * 121), None)
    assert torch.equal(dev[2 * stride:2 * stride + P * 2 + 1], host[:P * 2 + 1])
    for a, b in zip(got, want):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# f. SSIMLoss end to end at the edges
GO = 1.5


def _oracle(x, y, **kw):
    """value and gradient (times GO) of oracle.loss_ref.ssim_loss in the dtype of x"""
    xr = x.clone().requires_grad_(True)
    loss = Lr.ssim_loss(xr, y, **kw)
    (g,) = torch.autograd.grad(loss, xr)
    return loss.detach(), g * GO


def _e2e(group, x, y, cfg, what, **oracle_kw):
    from pssr2_amd.util import SSIMLoss
    v64, g64 = _oracle(x.double(), y.double(), **oracle_kw)
    v32, g32 = _oracle(x, y, **oracle_kw)
    xg = x.cuda().requires_grad_(True)
    loss = SSIMLoss(channels=x.shape[1], **cfg)(xg, y.cuda())
    (loss * GO).backward()
    _check(group, loss, v64, v32, f"{what} value")
    _check(group, xg.grad, g64, g32, f"{what} gradient")
    return xg.grad.cpu(), g64, g32


def _images(shape, seed):
    x, y = _planes(shape[-2], shape[-1], seed, planes=shape[0] * shape[1])
    return x.view(shape), y.view(shape)


@pytest.mark.parametrize("mix", [0.8, 1.0])
@pytest.mark.parametrize("shape", [(1, 1, 161, 161), (2, 3, 161, 173)])
def test_ssim_loss_smallest_pyramid(shape, mix):
    """161: every level is odd (161, 81, 41, 21, 11), pooling pads at each, and level 4 has one valid position"""
    x, y = _images(shape, 21)
    _e2e("f SSIMLoss", x, y, dict(mix=mix), f"{shape} mix={mix}", mix=mix)


def test_ssim_loss_level_count_and_constants():
    x, y = _images((2, 3, 161, 173), 22)
    opts = {"weights": (0.3, 0.3, 0.4), "K": (0.02, 0.05)}
    _e2e("f SSIMLoss", x, y, dict(mix=0.8, kwargs=opts), "3 levels, K=(0.02, 0.05)", mix=0.8, **opts)


def test_ssim_loss_more_than_256_planes():
    x, y = _images((300, 1, 12, 13), 23)
    _e2e("f SSIMLoss", x, y, dict(ms=False), "300 planes", ms=False)


def test_ssim_loss_degenerate_planes():
    """a degraded copy, an identical pair, a constant pair and an anti-correlated pair in one batch"""
    from pssr2_amd.util import SSIMLoss
    g = torch.Generator().manual_seed(24)
    y = torch.rand(4, 1, 161, 161, generator=g)
    x = 0.7 * y + 0.3 * torch.rand(4, 1, 161, 161, generator=g)
    x[1] = y[1]
    x[2], y[2] = 0.5, 0.25
    x[3] = 1 - y[3]
    grad, g64, g32 = _e2e("f degenerate", x, y, dict(mix=0.8), "4 planes", mix=0.8)
    assert torch.isfinite(grad).all()
    tol, den = bound(g64, g32)
    for p in range(4):
        err = (grad[p].double() - g64[p]).abs().max().item()
        print(f"  [f degenerate] plane {p}: err {err:.3e} ratio {err / den:.3f}")
        assert err <= tol, f"plane {p}: {err / den:.1f} x max(E32, floor)"
    # plane 3: negative cs means, so the relu zeroes every SSIM weight of the plane and its gradient is the L1 term alone
    _, _, means = compose(x[:, 0].double(), y[:, 0].double(), Lr.gauss_1d(11, 1.5), 1e-4, 9e-4, Lr.MS_WEIGHTS, True, 0.8)
    assert (means[:4, 3] < -0.05).all() and (means[:, :3] > 0.05).all()

    def l1_only(xx, yy):
        xr = xx.clone().requires_grad_(True)
        (gl,) = torch.autograd.grad(0.2 * Lr.gaussian_l1(xr, yy), xr)
        return gl[3] * GO
    _check("f degenerate", grad[3], l1_only(x.double(), y.double()), l1_only(x, y), "plane 3 = L1 term")
    # plane 0 in a batch of its own: weights, L1 coefficient and the coarse gradients are 4 times larger, nothing else changes,
    # and a power of two scales every product and sum of the kernels exactly
    x0 = x[:1].cuda().requires_grad_(True)
    (SSIMLoss(mix=0.8)(x0, y[:1].cuda()) * GO).backward()
    assert torch.equal(x0.grad.cpu()[0], grad[0] * 4)


def test_ssim_metric_data_range_255():
    """util.ssim(data_range=255), the in-loop training metric: no gradient, so ssim_fwd_k<11>"""
    from pssr2_amd.util import ssim
    g = torch.Generator().manual_seed(25)
    Y = torch.floor(torch.rand(2, 1, 43, 75, generator=g) * 256).clamp(max=255)
    X = torch.round(0.7 * Y + 0.3 * 255 * torch.rand(2, 1, 43, 75, generator=g))
    got = ssim(X.cuda(), Y.cuda(), data_range=255)
    _check("f ssim()", got, Lr.ssim(X.double(), Y.double(), data_range=255.0), Lr.ssim(X, Y, data_range=255.0), "(2,1,43,75)")


def test_ssim_loss_grad_and_no_grad_routes_agree():
    """SSIMLoss(ms=False) without a gradient runs ssim_fwd_k<11>, with one ssim_fwd_adj_k<11>: one value"""
    from pssr2_amd.util import SSIMLoss
    x, y = _images((2, 1, 43, 75), 26)
    v64 = Lr.ssim_loss(x.double(), y.double(), ms=False)
    v32 = Lr.ssim_loss(x, y, ms=False)
    lf = SSIMLoss(ms=False)
    with torch.no_grad():
        a = lf(x.cuda(), y.cuda())
    b = lf(x.cuda().requires_grad_(True), y.cuda())
    assert b.requires_grad and not a.requires_grad
    _check("f routes", a, v64, v32, "no-grad route")
    _check("f routes", b, v64, v32, "grad route")
    tol, den = bound(v64, v32)
    assert abs(a.item() - b.item()) <= tol
