"""Every BatchNorm / input-stage / pooling / layout entry point of csrc/elementwise.hip against its plain f64 reference
(tests/_elementwise_ref64.py, pinned against torch autograd by tests/test_elementwise_ref64.py), at the smallest shapes that take each
path of each kernel.  The case ids name the path.

Outputs are written into buffers pre-filled with NaN (bytes: two different fills) and wider than the slice written: PAD spare
elements / channels on each side must stay as they were and no element of the slice may keep the fill.  Inputs that are channel
slices have NaN neighbours too, so a read outside the slice poisons the result.

Tolerances.  Data movement (pooling, masks, layout, clip, stripe folds) is bit-exact.  A reduced statistic is a sum of f32 partial
sums that the striped f64 buffer then adds exactly, so its error is bounded by 2 k 2^-24 sum|terms| with k the longest chain of f32
additions a term passes through in that kernel at that shape (k and its derivation stand next to each case; the factor 2 pays for the
f32 products inside a term, and the first addition of a chain, 0 + v, is exact).  Per-channel f32 results computed from f64 sums are
allowed the roundings the kernel's expression contains, counted in the test that uses them.  Nothing here is derived from kernel
output."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _elementwise_ref64 as R

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(F16, id="fp16"), pytest.param(F32, id="f32")]
PREC = {BF16: 8, F16: 11, F32: 24}                 # significand bits
EMIN = {BF16: -126, F16: -14, F32: -126}           # exponent of the smallest normal number
U32 = 2.0 ** -24                                   # unit roundoff of f32
SLACK = 2.0 ** -40                                 # f64 evaluation order (contraction, cancellation in var) relative to an f32 result
ROWS, STRIPES, TPB = 64, 32, 256                   # PSSR_STAT_ROWS, PSSR_STAT_STRIPES, workgroup size of elementwise.hip
PAD = 8
NAN = float("nan")


def _mods():
    from pssr2_amd import _lib as L
    from pssr2_amd import ops
    return ops, L


def _gen(*seed):
    return torch.Generator().manual_seed(sum(int(s) * (i + 1) for i, s in enumerate(seed)) + 12345)


def _f32(v):
    return float(np.float32(v))


# ---- guarded buffers -----------------------------------------------------------------------------------------------------------
def _guard(numel, dtype=F32, value=None):
    """(flat, view): flat = [PAD | numel | PAD] on the device, NaN everywhere; view = the middle, set to `value` if given."""
    flat = torch.full((numel + 2 * PAD,), NAN, dtype=dtype, device="cuda")
    view = flat[PAD:PAD + numel]
    if value is not None:
        view.copy_(torch.as_tensor(value, dtype=dtype).reshape(-1))
    return flat, view


def _guard_ok(flat, written=True):
    """The guards of a _guard buffer are untouched and (written) no element in between kept the NaN fill."""
    assert torch.isnan(flat[:PAD]).all() and torch.isnan(flat[-PAD:]).all(), "wrote outside the buffer"
    if written:
        assert not torch.isnan(flat[PAD:-PAD]).any(), "left elements unwritten"


def _stats_buf(row_len):
    """Caller-zeroed statistic buffer [ROWS][row_len] between NaN guards."""
    flat, view = _guard(ROWS * row_len, torch.float64)
    view.zero_()
    return flat, view


def _wide(lead, c, dt, data=None, left=PAD, right=PAD):
    """NHWC buffer [*lead, left + c + right] on the device, NaN everywhere except the slice [left, left + c), which holds `data`."""
    buf = torch.full((*lead, left + c + right), NAN, dtype=dt, device="cuda")
    if data is not None:
        buf[..., left:left + c] = data.to(dt).cuda()
    return buf


def _wide_ok(buf, c, left=PAD):
    assert torch.isnan(buf[..., :left]).all() and torch.isnan(buf[..., left + c:]).all(), "wrote outside the channel slice"
    assert not torch.isnan(buf[..., left:left + c]).any(), "left elements of the slice unwritten"
    return buf[..., left:left + c].cpu()


def _ref(L, t, co=0):
    return L.ptr(t), t.shape[-1], co


# ---- bounds --------------------------------------------------------------------------------------------------------------------
def _ulp(ref, dt):
    """Spacing of the storage type at |ref| (f64 tensor), the subnormal spacing below the smallest normal number."""
    _, e = torch.frexp(ref.abs().clamp_min(2.0 ** EMIN[dt]))          # |ref| = m 2^e, m in [0.5, 1)
    return torch.exp2((e - PREC[dt]).double())


def _assert_sum(got, ref, abs_terms, k, what):
    """|got - ref| <= 2 k 2^-24 sum|terms| per channel."""
    got, ref, abs_terms = (torch.as_tensor(t).double().cpu() for t in (got, ref, abs_terms))
    tol = 2.0 * k * U32 * abs_terms
    err = (got - ref).abs()
    worst = (err / tol.clamp_min(1e-300)).max().item()
    print(f"{what}: k={k} max err/bound {worst:.3g} (max err {err.max().item():.3g})")
    assert (err <= tol).all(), (what, worst)


def _assert_tol(got, ref, tol, what):
    got, ref, tol = (torch.as_tensor(t).double().cpu() for t in (got, ref, tol))
    err = (got - ref).abs()
    print(f"{what}: max err/bound {(err / tol.clamp_min(1e-300)).max().item():.3g}")
    assert (err <= tol).all(), (what, (err / tol.clamp_min(1e-300)).max().item())


def _fold(stats_view, row_len):
    """Sum of the rows of a statistic buffer (exact pieces: any order gives the same f64 sum up to one rounding of hi + lo)."""
    return stats_view.view(ROWS, row_len).sum(0).cpu()


def _assert_stat_rows(stats_view, row_len, workgroups, adds_each=1):
    """The structure documented at PSSR_STAT_ROWS: rows 0..31 hold multiples of 2^-20, an element of row 32 + s the remainders of the
    workgroups that add to stripe s (index mod 32, `adds_each` such grids), each at most half of 2^-20."""
    rows = stats_view.view(ROWS, row_len).cpu()
    hi = rows[:STRIPES] * 2.0 ** 20
    assert torch.equal(hi, torch.round(hi))
    per_stripe = torch.tensor([len(range(s, workgroups, STRIPES)) for s in range(STRIPES)], dtype=torch.float64)
    assert (rows[STRIPES:].abs() <= per_stripe[:, None] * adds_each * 2.0 ** -21).all()
    assert (rows[:STRIPES][per_stripe == 0] == 0).all() and rows[:STRIPES].abs().sum() > 0


def _spread_rows(total, g):
    """[ROWS, L] f64 whose column sums are `total` (multiples of 2^-20) exactly, spread unevenly and with both signs over all rows;
    every piece is a multiple of 2^-20 below 2^20, so the f64 sum of a column is exact in any order."""
    t = torch.round(total.double() * 2.0 ** 20).to(torch.int64)
    wts = torch.rand(ROWS, t.numel(), generator=g, dtype=torch.float64) ** 4 * 6.0 - 1.0
    pieces = torch.round(wts * t.abs().clamp_min(1 << 20).double()).to(torch.int64)
    pieces[ROWS - 1] = t - pieces[:ROWS - 1].sum(0)
    assert torch.equal(pieces.sum(0), t) and (pieces != 0).float().mean() > 0.99
    return pieces.double() * 2.0 ** -20


def _image(n, c, h, w, g):
    """Integer-valued pixels with a gradient across rows, columns and channels: asymmetric, no constant rows."""
    ramp = torch.arange(h).view(1, 1, h, 1) * 7 + torch.arange(w).view(1, 1, 1, w) * 3 + torch.arange(c).view(1, c, 1, 1) * 29
    x = (torch.randint(0, 160, (n, c, h, w), generator=g) + ramp) % 256
    assert (x.diff(dim=-1) != 0).any(-1).all() and (x.diff(dim=-2) != 0).any(-2).all()
    return x.float()


def _channel_params(c, g):
    """Distinct per-channel f32 (gamma in [0.5, 1.5], beta, mean, invstd in [0.5, 1.5])."""
    idx = torch.arange(c, dtype=torch.float32)
    gamma = 0.5 + (torch.rand(c, generator=g) + idx) / c
    beta = torch.randn(c, generator=g) + 0.01 * idx
    mean = torch.randn(c, generator=g) - 0.01 * idx
    invstd = 1.5 - (torch.rand(c, generator=g) + idx) / c
    return gamma, beta, mean, invstd


# ---- channel_stats_nchw --------------------------------------------------------------------------------------------------------
# k = trips of the per-thread loop + the 8 levels of the 256-wide LDS tree.  chunks = min(ceil(hw / 2048), 64) workgroups share a
# plane, a thread strides by chunks * 256: trips = ceil(hw / (chunks * 256)).  Planes and chunks meet in the exact f64 rows.
NCHW_STATS = [
    pytest.param((2, 1, 7, 9), (1 / 128, -1.0), 1 + 8, id="hw63-below-one-workgroup"),                  # 1 chunk, 63 of 256 threads: 1 trip
    pytest.param((2, 3, 40, 60), (1 / 128, -1.0), 5 + 8, id="hw2400-two-chunks"),                        # stride 512: ceil(2400 / 512) = 5
    pytest.param((2, 3, 40, 60), (0.0173, 0.31), 5 + 8, id="hw2400-two-chunks-general-affine"),
    pytest.param((1, 1, 384, 384), (1 / 128, -1.0), 9 + 8, id="hw147456-64-chunk-cap-thread-loop"),      # 72 -> 64 chunks, stride 16384: 9
]


@pytest.mark.parametrize("shape,pre,k", NCHW_STATS)
def test_channel_stats_nchw(shape, pre, k):
    ops, _ = _mods()
    n, c, h, w = shape
    ps, pb = _f32(pre[0]), _f32(pre[1])
    x = _image(n, c, h, w, _gen(*shape))
    flat, stats = _stats_buf(2 * c)
    ops.channel_stats_nchw(x.cuda(), stats, ps, pb)
    _guard_ok(flat)
    got = _fold(stats, 2 * c)
    s1, s2 = R.nchw_stats(x, ps, pb)
    a1, _ = R.nchw_stats((x.double() * ps + pb).abs())
    _assert_sum(got[:c], s1, a1, k, "sum")
    _assert_sum(got[c:], s2, s2, k, "sum of squares")
    chunks = min(-(-h * w // (TPB * 8)), 64)
    _assert_stat_rows(stats, 2 * c, chunks, adds_each=n)               # n planes per channel, `chunks` workgroups each


# ---- bn_finalize / bn_bwd_coefs / bn_eval_affine -------------------------------------------------------------------------------
def _bn_sums(c, count, g):
    """(s1, s2) as multiples of 2^-20 for per-channel means and variances of order one; the last channel's variance comes out
    slightly negative (-2^-20), which the finaliser clamps."""
    mu = torch.randn(c, generator=g, dtype=torch.float64) * 2.0
    var = torch.rand(c, generator=g, dtype=torch.float64) * 2.0 + 0.25
    s1 = torch.round(mu * count * 2.0 ** 20) * 2.0 ** -20
    s2 = torch.round((var + (s1 / count) ** 2) * count * 2.0 ** 20) * 2.0 ** -20
    m = torch.round(mu[-1] * 16) / 16                                     # exactly representable mean
    s1[-1], s2[-1] = m * count, m * m * count - count * 2.0 ** -20
    return s1, s2


@pytest.mark.parametrize("variant", ["affine-running-meaninvstd", "no-gamma-beta", "no-running", "no-mean-invstd", "count1"])
@pytest.mark.parametrize("c", [1, 3, 32, 33, 100])
def test_bn_finalize(c, variant):
    """From hand-built [64][2c] rows: every output within the f32 roundings of its expression, running statistics blended with
    non-zero old values, the negative variance of the last channel clamped, absent outputs not required."""
    ops, _ = _mods()
    g = _gen(c, len(variant))
    count = 1.0 if variant == "count1" else 977.0
    eps, mom = _f32(1e-5), _f32(0.1)
    s1, s2 = _bn_sums(c, count, g)
    rows = torch.cat([_spread_rows(s1, g), _spread_rows(s2, g)], 1)           # [64][2c]
    gamma, beta, old_m, old_v = _channel_params(c, g)
    if variant == "no-gamma-beta":
        gamma = beta = None
    running = variant != "no-running"
    side = variant != "no-mean-invstd"
    ref = R.bn_finalize(s1, s2, count, gamma, beta, eps, mom, running=(old_m, old_v) if running else None)
    assert ref["var"][-1] == 0.0 and (s2[-1] / count - (s1[-1] / count) ** 2) < 0          # the clamp runs
    fs, stats = _guard(ROWS * 2 * c, torch.float64, rows)
    bufs = {k: _guard(c) for k in ("scale", "shift", "mean", "invstd")}
    frm, rm = _guard(c, value=old_m)
    frv, rv = _guard(c, value=old_v)
    ops.bn_finalize(stats, count, None if gamma is None else gamma.cuda(), None if beta is None else beta.cuda(), eps, mom,
                    rm if running else None, rv if running else None, bufs["scale"][1], bufs["shift"][1],
                    bufs["mean"][1] if side else None, bufs["invstd"][1] if side else None)
    assert torch.equal(stats.cpu(), rows.reshape(-1))
    for k in ("scale", "shift") + (("mean", "invstd") if side else ()):
        _guard_ok(bufs[k][0])
    mu, inv = ref["mean"], ref["invstd"]
    gm = torch.ones(c, dtype=torch.float64) if gamma is None else gamma.double()
    bt = torch.zeros(c, dtype=torch.float64) if beta is None else beta.double()
    u = U32 + SLACK
    if side:
        _assert_tol(bufs["mean"][1], mu, u * mu.abs(), "mean")                                   # one rounding of the f64 mean
        _assert_tol(bufs["invstd"][1], inv, u * inv, "invstd")                                  # one rounding
    _assert_tol(bufs["scale"][1], ref["scale"], 2 * u * ref["scale"].abs(), "scale")            # invstd rounded, one product
    # shift = b - ((float)mu * g) * is: mu, two products and the rounded invstd = 4 roundings of the product, 1 of the difference
    _assert_tol(bufs["shift"][1], ref["shift"], 4 * u * (mu * gm * inv).abs() + u * ref["shift"].abs(), "shift")
    if running:
        # (1.f - m) * old + m * (float)new: 1 - m and its product, the f32 new value and its product, the sum
        unbiased = ref["var"] if count == 1 else ref["var"] * count / (count - 1)
        for got, key, new, old in ((rm, "running_mean", mu, old_m), (rv, "running_var", unbiased, old_v)):
            tol = 2 * u * ((1 - mom) * old.double()).abs() + 2 * u * (mom * new).abs() + u * ref[key].abs()
            _assert_tol(got, ref[key], tol, key)
        _guard_ok(frm), _guard_ok(frv)
        assert (rm.cpu() != old_m).any() and (rv.cpu() != old_v).any()


@pytest.mark.parametrize("variant", ["dgamma-dbeta", "no-dgamma-dbeta", "count1"])
@pytest.mark.parametrize("c", [1, 3, 32, 33, 100])
def test_bn_bwd_coefs(c, variant):
    """A, B, C are one f32 rounding of f64 expressions of the folded sums; dgamma / dbeta are the folded sums rounded."""
    ops, _ = _mods()
    g = _gen(c, len(variant), 7)
    count = 1.0 if variant == "count1" else 1234.0
    s1 = torch.round(torch.randn(c, generator=g, dtype=torch.float64) * 300 * 2.0 ** 20) * 2.0 ** -20
    s2 = torch.round(torch.randn(c, generator=g, dtype=torch.float64) * 200 * 2.0 ** 20) * 2.0 ** -20
    rows = torch.cat([_spread_rows(s1, g), _spread_rows(s2, g)], 1)
    gamma, _, mean, invstd = _channel_params(c, g)
    ref = R.bn_bwd_coefs(s1, s2, count, gamma, mean, invstd)
    fs, stats = _guard(ROWS * 2 * c, torch.float64, rows)
    bufs = {k: _guard(c) for k in ("A", "B", "C", "dgamma", "dbeta")}
    both = variant != "no-dgamma-dbeta"
    ops.bn_bwd_coefs(stats, count, gamma.cuda(), mean.cuda(), invstd.cuda(), bufs["A"][1], bufs["B"][1], bufs["C"][1],
                     bufs["dgamma"][1] if both else None, bufs["dbeta"][1] if both else None)
    for k in ("A", "B", "C") + (("dgamma", "dbeta") if both else ()):
        _guard_ok(bufs[k][0])
    u = U32 + SLACK
    gi = (gamma.double() * invstd.double()).abs()
    _assert_tol(bufs["A"][1], ref["A"], u * ref["A"].abs(), "A")
    _assert_tol(bufs["B"][1], ref["B"], u * ref["B"].abs(), "B")
    # C = g is (mu is c2 - c1): the f64 difference may cancel, its own rounding is relative to the two operands
    cancel = 2.0 ** -48 * gi * ((mean.double() * invstd.double() * s2 / count).abs() + (s1 / count).abs())
    _assert_tol(bufs["C"][1], ref["C"], u * ref["C"].abs() + cancel, "C")
    if both:
        assert torch.equal(bufs["dgamma"][1].cpu(), s2.float()) and torch.equal(bufs["dbeta"][1].cpu(), s1.float())


@pytest.mark.parametrize("c", [pytest.param(1, id="c1"), pytest.param(257, id="c257-two-workgroups")])
def test_bn_eval_affine(c):
    """All f32: rvar + eps (1/2 ulp), sqrt (<= 1 ulp, halving what came before), 1 / x (<= 2.5 ulp) leave invstd within 4 ulp;
    scale adds a product (5 ulp of 2^-23), shift two products and a difference (6 ulp of |beta| + |rmean gamma invstd|)."""
    ops, _ = _mods()
    g = _gen(c, 3)
    gamma, beta, rmean, rvar = _channel_params(c, g)
    eps = _f32(1e-5)
    fs, scale = _guard(c)
    fh, shift = _guard(c)
    ops.bn_eval_affine(gamma.cuda(), beta.cuda(), rmean.cuda(), rvar.cuda(), eps, scale, shift)
    _guard_ok(fs), _guard_ok(fh)
    rs, rh = R.bn_eval_affine(gamma, beta, rmean, rvar, eps)
    _assert_tol(scale, rs, 5 * 2.0 ** -23 * rs.abs(), "scale")
    _assert_tol(shift, rh, 6 * 2.0 ** -23 * (beta.double().abs() + (rmean.double() * rs).abs()), "shift")


# ---- input_im2col --------------------------------------------------------------------------------------------------------------
def _im2col_tol(x, scale, shift, xc, ref, dt, d_scale=0.0, d_shift=0.0):
    """|xcol - ref|: two f32 FMAs (the first, x / 128 - 1 on integer pixels, is exact) and the rounding to the storage type, plus what
    an error (d_scale, d_shift) of the per-channel coefficients moves; half the subnormal spacing where fp16 underflows."""
    prod = R.input_im2col(x, scale, torch.zeros_like(shift), xc).abs()                        # |xtilde * scale|, zero at padding taps
    xt = R.input_im2col(x, torch.ones_like(scale), torch.zeros_like(shift), xc).abs()         # |xtilde|
    valid = R.input_im2col(torch.full_like(x, 256.0), torch.ones_like(scale), torch.zeros_like(shift), xc) != 0
    d_scale = R.input_im2col(torch.full_like(x, 256.0), torch.as_tensor(d_scale).expand_as(scale), torch.zeros_like(shift), xc)
    d_shift = R.input_im2col(torch.full_like(x, 256.0), torch.as_tensor(d_shift).expand_as(scale), torch.zeros_like(shift), xc)
    tol = 2.0 ** -PREC[dt] * ref.abs() + 2 * U32 * (prod + ref.abs()) + xt * d_scale + d_shift + 2.0 ** (EMIN[dt] - PREC[dt])
    return torch.where(valid, tol, torch.zeros_like(tol)), valid


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", [pytest.param((2, 1, 5, 7, 16), id="c1-xc16"), pytest.param((1, 3, 6, 5, 32), id="c3-xc32"),
                                   pytest.param((1, 1, 4, 4, 48), id="c1-xc48-mostly-zero-channels")])
def test_input_im2col(shape, dt):
    ops, _ = _mods()
    n, c, h, w, xc = shape
    g = _gen(*shape)
    x = _image(n, c, h, w, g)
    scale, shift, _, _ = _channel_params(c, g)
    flat, view = _guard(n * h * w * xc, dt)
    xcol = view.view(n, h, w, xc)
    ops.input_im2col(x.cuda(), xcol, scale.cuda(), shift.cuda(), ops.dtype_code(dt))
    _guard_ok(flat)
    ref = R.input_im2col(x, scale, shift, xc)
    tol, valid = _im2col_tol(x, scale, shift, xc, ref, dt)
    got = xcol.cpu().double()
    assert (got[~valid] == 0).all() and (~valid[..., 9 * c:]).all() and (~valid[:, 0, :, 1]).all()      # borders and channels >= 9c
    assert valid.sum() == n * c * (9 * h * w - 6 * (h + w) + 4)
    _assert_tol(got, ref, tol, "xcol")


@pytest.mark.parametrize("dt", DTYPES)
def test_forward_chain_stats_finalize_im2col(dt):
    """channel_stats_nchw -> bn_finalize -> input_im2col on the device against the reference chain.  The statistic bounds
    (k = 1 trip + 8 tree levels at hw = 30) give bounds on mean and variance, those on scale and shift, those on xcol."""
    ops, _ = _mods()
    n, c, h, w, xc = 2, 3, 6, 5, 32
    g = _gen(n, c, h, w, xc)
    x = _image(n, c, h, w, g)
    gamma, beta, _, _ = _channel_params(c, g)
    ps, pb, eps, count, k = 1 / 128, -1.0, _f32(1e-5), float(n * h * w), 1 + 8
    fst, stats = _stats_buf(2 * c)
    fsc, scale = _guard(c)
    fsh, shift = _guard(c)
    fx, view = _guard(n * h * w * xc, dt)
    xcol = view.view(n, h, w, xc)
    xd = x.cuda()
    ops.channel_stats_nchw(xd, stats, ps, pb)
    ops.bn_finalize(stats, count, gamma.cuda(), beta.cuda(), eps, _f32(0.1), None, None, scale, shift, None, None)
    ops.input_im2col(xd, xcol, scale, shift, ops.dtype_code(dt))
    for f in (fst, fsc, fsh, fx):
        _guard_ok(f)
    s1, s2 = R.nchw_stats(x, ps, pb)
    a1, _ = R.nchw_stats((x.double() * ps + pb).abs())
    fin = R.bn_finalize(s1, s2, count, gamma, beta, eps)
    d_mu = 2 * k * U32 * a1 / count
    d_var = 2 * k * U32 * s2 / count + 2 * fin["mean"].abs() * d_mu + d_mu ** 2
    d_is = 1.0 / torch.sqrt((fin["var"] - d_var).clamp_min(0) + eps) - fin["invstd"]
    gm, mu, inv = gamma.double(), fin["mean"], fin["invstd"]
    d_scale = gm * d_is + 3 * U32 * fin["scale"].abs()
    d_shift = gm * (mu.abs() * d_is + (inv + d_is) * d_mu) + 5 * U32 * (beta.double().abs() + (mu * gm * inv).abs())
    _assert_tol(scale, fin["scale"], d_scale, "scale")
    _assert_tol(shift, fin["shift"], d_shift, "shift")
    ref = R.input_im2col(x, fin["scale"], fin["shift"], xc)
    tol, valid = _im2col_tol(x, fin["scale"], fin["shift"], xc, ref, dt, d_scale, d_shift)
    got = xcol.cpu().double()
    assert (got[~valid] == 0).all()
    _assert_tol(got, ref, tol, "xcol")


# ---- input_norm_bwd / input_norm_bwd2 ------------------------------------------------------------------------------------------
# k = additions that form g (9 taps per im2col source, 1 for the patch gradient) + trips of the per-thread loop + 8 tree levels.
# gx = min(ceil(n h w / 1024), 512) workgroups per channel, a thread strides by gx * 256: trips = ceil(n h w / (gx * 256)).
INPUT_NORM_BWD = [
    pytest.param((2, 1, 5, 7, 16), 1, 0, 9 + 1 + 8, id="a-only-70px-one-workgroup"),
    pytest.param((2, 1, 5, 7, 16), 2, 0, 18 + 1 + 8, id="a+b-70px-one-workgroup"),
    pytest.param((2, 3, 24, 28, 32), 1, 0, 9 + 3 + 8, id="a-only-1344px-two-workgroups"),           # gx = 2: ceil(1344 / 512) = 3
    pytest.param((2, 3, 24, 28, 32), 2, 0, 18 + 3 + 8, id="a+b-1344px-two-workgroups"),
    pytest.param((2, 3, 8, 12, 32), 0, 2, 1 + 1 + 8, id="patch2-alone"),
    pytest.param((2, 3, 8, 12, 32), 1, 2, 10 + 1 + 8, id="patch2+a"),
    pytest.param((2, 3, 8, 12, 32), 0, 4, 1 + 1 + 8, id="patch4-alone"),
    pytest.param((2, 3, 8, 12, 32), 1, 4, 10 + 1 + 8, id="patch4+a"),
]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,ncol,pk,k", INPUT_NORM_BWD)
def test_input_norm_bwd(shape, ncol, pk, k, dt):
    """sum g and sum g * xhat per channel, then bn_bwd_coefs on the device result: dgamma / dbeta are those sums rounded to f32.  The
    channels of dxcol / dpatch beyond 9 c / c pk^2 hold NaN: they are not read."""
    ops, _ = _mods()
    n, c, h, w, xc = shape
    g = _gen(*shape, ncol, pk)
    x = _image(n, c, h, w, g)
    gamma, _, mean, invstd = _channel_params(c, g)
    cols = []
    for _ in range(ncol):
        d = torch.full((n, h, w, xc), NAN)
        d[..., :9 * c] = torch.randn(n, h, w, 9 * c, generator=g)
        cols.append(d.to(dt))
    dpatch = None
    if pk:
        pc = c * pk * pk + 4
        dpatch = torch.full((n, h // pk, w // pk, pc), NAN)
        dpatch[..., :c * pk * pk] = torch.randn(n, h // pk, w // pk, c * pk * pk, generator=g)
        dpatch = dpatch.to(dt)
    flat, stats = _stats_buf(2 * c)
    dev = [d.cuda() for d in cols] + [None, None]
    code = ops.dtype_code(dt)
    if pk:
        ops.input_norm_bwd2(dev[0], dev[1], dpatch.cuda(), pk, x.cuda(), mean.cuda(), invstd.cuda(), stats, code)
    else:
        ops.input_norm_bwd(dev[0], dev[1], x.cuda(), mean.cuda(), invstd.cuda(), stats, code)
    _guard_ok(flat)
    got = _fold(stats, 2 * c)
    c64 = [d[..., :9 * c].double() for d in cols]
    p64 = None if dpatch is None else dpatch[..., :c * pk * pk].double()
    _, s1, s2 = R.input_norm_bwd(c64, p64, pk, x, mean, invstd)
    g_abs = R.input_norm_fold([d.abs() for d in c64], None if p64 is None else p64.abs(), pk, n, c, h, w)      # sum of |leaf terms|
    xhat = (x.double() / 128 - 1 - mean.double()[None, :, None, None]) * invstd.double()[None, :, None, None]
    a1, a2 = g_abs.sum((0, 2, 3)), (g_abs * xhat.abs()).sum((0, 2, 3))
    _assert_sum(got[:c], s1, a1, k, "sum g")
    _assert_sum(got[c:], s2, a2, k, "sum g xhat")
    bufs = {kk: _guard(c) for kk in ("A", "B", "C", "dgamma", "dbeta")}
    ops.bn_bwd_coefs(stats, float(n * h * w), gamma.cuda(), mean.cuda(), invstd.cuda(), *(bufs[kk][1] for kk in ("A", "B", "C", "dgamma", "dbeta")))
    for kk in bufs:
        _guard_ok(bufs[kk][0])
    assert torch.equal(bufs["dbeta"][1].cpu(), got[:c].float()) and torch.equal(bufs["dgamma"][1].cpu(), got[c:].float())
    _assert_tol(bufs["dbeta"][1], s1, 2 * k * U32 * a1 + U32 * s1.abs(), "dbeta")
    _assert_tol(bufs["dgamma"][1], s2, 2 * k * U32 * a2 + U32 * s2.abs(), "dgamma")


# ---- max_pool 2x2 --------------------------------------------------------------------------------------------------------------
def _post_relu(shape, g):
    """About a third exact zeros, so windows tie (whole windows of zeros included)."""
    a = torch.relu(torch.randn(*shape, generator=g) + 0.43)
    assert 0.2 < (a == 0).float().mean() < 0.45
    return a


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", [pytest.param((2, 6, 10, 4), id="even-c4"), pytest.param((1, 5, 7, 12), id="odd-h-odd-w-c12"),
                                   pytest.param((1, 4, 4, 64), id="c64-into-channel-slice")])
def test_maxpool2(shape, dt):
    ops, _ = _mods()
    n, h, w, c = shape
    x = torch.randn(n, h, w, c, generator=_gen(*shape)).to(dt)
    src = _wide((n, h, w), c, dt, x)
    out = _wide((n, h // 2, w // 2), c, dt)
    ops.maxpool2(src, out, n, h, w, c, ops.dtype_code(dt), in_coff=PAD, out_coff=PAD)
    got = _wide_ok(out, c)
    assert torch.equal(got, F.max_pool2d(x.float().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).to(dt))
    assert torch.equal(got.double(), R.maxpool2(x))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("skip", [pytest.param(True, id="dskip"), pytest.param(False, id="dskip-null")])
@pytest.mark.parametrize("hw", [pytest.param((5, 6), id="odd-h"), pytest.param((6, 5), id="odd-w"), pytest.param((5, 7), id="odd-h-odd-w"),
                                pytest.param((4, 4), id="even")])
def test_maxpool2_bwd(hw, skip, dt):
    """Bit-exact against the reference rounded to the storage type; every tensor is a channel slice at offset PAD; the NaN fill
    proves that the odd trailing row / column was written (dskip, or 0)."""
    ops, L = _mods()
    (h, w), n, c = hw, 2, 12
    g = _gen(h, w, skip)
    act = _post_relu((n, h, w, c), g).to(dt)
    act[0, :2, :2] = 0                                                     # a window of four equal values
    dpool = torch.randn(n, h // 2, w // 2, c, generator=g).to(dt)
    dskip = torch.randn(n, h, w, c, generator=g).to(dt) if skip else None
    d_act, d_dpool = _wide((n, h, w), c, dt, act), _wide((n, h // 2, w // 2), c, dt, dpool)
    d_dskip = _wide((n, h, w), c, dt, dskip) if skip else None
    dout = _wide((n, h, w), c, dt)
    ds = _ref(L, d_dskip, PAD) if skip else (None, 0, 0)
    L.check(L.lib().pssr_maxpool2_bwd(*_ref(L, d_act, PAD), *_ref(L, d_dpool, PAD), *ds, *_ref(L, dout, PAD), n, h, w, c, ops.dtype_code(dt),
                                      L.stream_ptr()), "pssr_maxpool2_bwd")
    got = _wide_ok(dout, c)
    want = R.maxpool2_bwd(act, dpool, dskip).to(dt)
    assert torch.equal(got, want)
    if h % 2:
        assert torch.equal(got[:, -1], dskip[:, -1] if skip else torch.zeros(n, w, c, dtype=dt))
    if w % 2:
        assert torch.equal(got[:, :, -1], dskip[:, :, -1] if skip else torch.zeros(n, h, c, dtype=dt))


# ---- relu_bwd_stats / bn_bwd_apply ---------------------------------------------------------------------------------------------
# (dtype, c, pixels of relu_bwd_stats, pixels of bn_bwd_apply, channel offset of `out`, k, workgroups of relu_bwd_stats)
# Generic kernels (f32, c not a power of two in [8, 2048], or a slice that is not 16-byte aligned): cg = c / 4 channel groups;
#   cg <= 256: ppb = 256 / cg pixels per workgroup, grid = min(ceil(npix / ppb), 2048), k = trips + ppb additions of the LDS combine;
#   cg > 256: one pixel per workgroup and trip, no LDS combine, k = trips.  With one trip (k = 1) every term reaches the f64 rows alone and
#   the bound is spent on the term's own roundings, y - mean and two products: 3 against the 2 allowed, each at most 2^-24 and
#   of either sign, over the ~12 unmasked pixels of a channel.
# 8-channel kernels (16-bit): cg = c / 8, grid = min(ceil(npix cg / 256), 2048), k = trips + 256 / cg additions of the combine.
BN_BWD = [
    pytest.param(F32, 8, 301, 301, PAD, 1 + 128, 3, id="f32-c8-generic"),                                   # cg 2, ppb 128
    pytest.param(F32, 1024, 37, 37, PAD, 1 + 1, 37, id="f32-c1024-cg-equals-workgroup"),                    # cg 256, ppb 1
    pytest.param(F32, 1028, 37, 37, PAD, 1, 37, id="f32-c1028-cg-above-workgroup"),                         # cg 257
    pytest.param(BF16, 4096, 19, 19, PAD, 1, 19, id="bf16-c4096-past-8ch-limit-generic"),                   # cg 1024
    pytest.param(BF16, 2048, 41, 41, PAD, 1 + 1, 41, id="bf16-c2048-widest-8ch"),                           # cg 256 of 8
    pytest.param(BF16, 64, 101, 101, 4, 1 + 16, 7, id="bf16-c64-out-offset-4-misaligned-generic"),          # cg 16, ppb 16
    pytest.param(F16, 64, 66000, 132000, PAD, 2 + 32, 2048, id="fp16-c64-8ch-grid-stride-past-caps"),       # 2063 -> 2048 workgroups
]


def _grid16(shape, g, lo=-127):
    """Multiples of 1/16 in (-8, 8): exact in every storage type, products and sums of three of them exact in f32."""
    return torch.randint(lo, 128, shape, generator=g).float() / 16


@pytest.mark.parametrize("dt,c,npix_s,npix_a,out_co,k,wgs", BN_BWD)
def test_relu_bwd_stats_and_bn_bwd_apply(dt, c, npix_s, npix_a, out_co, k, wgs):
    """dz bit-exact; statistics within 2 k 2^-24 sum|terms| and with the documented row structure; dy within one unit in the last
    place of the storage type of the f64 value.  Tensors and coefficients are multiples of 1/16 below 8, so both FMAs of
    a * g + (b * y + c) are exact in f32 and the store is the kernel's only rounding: the bound holds whatever cancels."""
    ops, L = _mods()
    code = ops.dtype_code(dt)
    g = _gen(c, npix_s, out_co)
    npix = max(npix_s, npix_a)
    dout, y = _grid16((npix, c), g), _grid16((npix, c), g)
    out = torch.relu(_grid16((npix, c), g, lo=-64))                          # 65 of 192 values are zero
    _, _, mean, invstd = _channel_params(c, g)
    d_dout, d_y = _wide((npix,), c, dt, dout), _wide((npix,), c, dt, y)
    d_out = _wide((npix,), c, dt, out, left=out_co, right=2 * PAD - out_co)
    dz = _wide((npix,), c, dt)
    flat, stats = _stats_buf(2 * c)
    d_mean, d_invstd = mean.cuda(), invstd.cuda()
    L.check(L.lib().pssr_relu_bwd_stats(*_ref(L, d_dout, PAD), *_ref(L, d_out, out_co), *_ref(L, d_y, PAD), L.ptr(d_mean), L.ptr(d_invstd),
                                        *_ref(L, dz, PAD), L.ptr(stats), C.c_int64(npix_s), c, code, L.stream_ptr()), "pssr_relu_bwd_stats")
    _guard_ok(flat)
    assert torch.isnan(dz[npix_s:]).all()                                   # pixels beyond npix are not touched
    got_dz = _wide_ok(dz[:npix_s], c)
    ref_dz, s1, s2 = R.relu_bwd_stats(dout[:npix_s], out[:npix_s], y[:npix_s], mean, invstd)
    assert torch.equal(got_dz, ref_dz.to(dt))
    got = _fold(stats, 2 * c)
    _assert_sum(got[:c], s1, ref_dz.abs().sum(0), k, "sum dz")
    _assert_sum(got[c:], s2, (ref_dz * (y[:npix_s].double() - mean.double()) * invstd.double()).abs().sum(0), k, "sum dz xhat")
    _assert_stat_rows(stats, 2 * c, wgs)
    # a g + b y + c with g = the dz just written (re-filled beyond npix_s where the apply covers more pixels)
    if npix_a > npix_s:
        dz[npix_s:, PAD:PAD + c] = dout[npix_s:].to(dt).cuda()
    gv = dz[:npix_a, PAD:PAD + c].cpu().double()
    a, b, cc = (_grid16((c,), g) for _ in range(3))
    dy = _wide((npix_a,), c, dt)
    ops.bn_bwd_apply(dz, d_y, a.cuda(), b.cuda(), cc.cuda(), dy, npix_a, c, code, g_coff=PAD, y_coff=PAD, dy_coff=PAD)
    got_dy = _wide_ok(dy, c).double()
    ref_dy = R.bn_bwd_apply(gv, y[:npix_a], a, b, cc)
    _assert_tol(got_dy, ref_dy, _ulp(ref_dy, dt), "dy")


# ---- channel_sum_nhwc ----------------------------------------------------------------------------------------------------------
# 300 pixels.  cg = c / 4; cg <= 256: ppb = 256 / cg, grid = min(ceil(300 / ppb), max(128, 131072 / c)), k = trips + ppb;
# cg > 256: grid = min(300, max(128, 131072 / c)), k = trips.
CHANNEL_SUM = [
    pytest.param(4, 1 + 256, 2, id="c4-one-group-256-pixel-lanes"),                       # ppb 256, 2 workgroups
    pytest.param(24, 1 + 42, 8, id="c24-252-active-threads"),                             # cg 6, ppb 42, 8 workgroups
    pytest.param(600, 2 + 1, 218, id="c600-past-atomics-cap"),                            # ppb 1, 300 -> 218 workgroups: 2 trips
    pytest.param(1028, 3, 128, id="c1028-cg-above-workgroup"),                            # 300 -> 128 workgroups: 3 trips
]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("c,k,wgs", CHANNEL_SUM)
def test_channel_sum_nhwc(c, k, wgs, dt):
    """A slice at channel offset PAD of a buffer 16 channels wider, NaN around it."""
    ops, _ = _mods()
    npix = 300
    x = torch.randn(npix, c, generator=_gen(c)).to(dt)
    buf = _wide((npix,), c, dt, x)
    flat, out = _stats_buf(c)
    ops.channel_sum_nhwc(buf, npix, c, out, ops.dtype_code(dt), coff=PAD)
    _guard_ok(flat)
    _assert_sum(_fold(out, c), R.channel_sum(x), x.double().abs().sum(0), k, "channel sum")
    _assert_stat_rows(out, c, wgs)


# ---- nchw_to_nhwc / clip_u8 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", [pytest.param((2, 1, 5, 7, 16), id="c1-cs16"), pytest.param((1, 3, 4, 6, 8), id="c3-cs8")])
def test_nchw_to_nhwc(shape, dt):
    ops, _ = _mods()
    n, c, h, w, cs = shape
    x = torch.randn(n, c, h, w, generator=_gen(*shape)) * 40
    flat, view = _guard(n * h * w * cs, dt)
    out = view.view(n, h, w, cs)
    scale = _f32(1 / 3)
    ops.nchw_to_nhwc(x.cuda(), out, scale, ops.dtype_code(dt))
    _guard_ok(flat)
    got = out.cpu()
    assert torch.equal(got[..., :c], (x * torch.tensor(scale)).to(dt).permute(0, 2, 3, 1)) and (got[..., c:] == 0).all()
    assert torch.equal(got, R.nchw_to_nhwc(x, cs, scale).to(dt))


def _clip_u8_check(v):
    ops, _ = _mods()
    n, pad = v.numel(), 16
    want = torch.from_numpy(R.clip_u8(v.numpy()))
    for fill in (0x55, 0xAA):                                              # an unwritten element shows under one fill or the other
        flat = torch.full((n + 2 * pad,), fill, dtype=torch.uint8, device="cuda")
        ops.clip_u8(v.cuda(), flat[pad:pad + n])
        assert (flat[:pad] == fill).all() and (flat[-pad:] == fill).all()
        assert torch.equal(flat[pad:pad + n].cpu(), want)


def test_clip_u8_edges():
    v = torch.tensor([-1e10, -0.0, 0.49, 0.5, 0.999, 254.999, 255, 255.5, 256, 1e10, float("inf"), float("-inf")])
    assert R.clip_u8(v.numpy()).tolist() == [0, 0, 0, 0, 0, 254, 255, 255, 255, 255, 255, 0]
    _clip_u8_check(v)


def test_clip_u8_past_grid_cap():
    """2.2 M values: 8594 workgroups' worth, past the 8192-workgroup grid, so the grid-stride loop runs."""
    _clip_u8_check(torch.rand(2_200_000, generator=_gen(9)) * 300 - 20)


# ---- f64_to_f32 / f64_to_f32_batch ---------------------------------------------------------------------------------------------
def _exact_rows(stripes, n, g):
    """Integer multiples of 2^-20 below 2^20: every f64 sum of them is exact in any order."""
    return torch.randint(-(2 ** 40) + 1, 2 ** 40, (stripes, n), generator=g).double() * 2.0 ** -20


FOLD_STRIPES = [pytest.param(1, id="1-stripe-masked"), pytest.param(7, id="7-stripes-masked-tail"), pytest.param(64, id="64-stripes-one-full-trip"),
                pytest.param(65, id="65-stripes-second-trip"), pytest.param(130, id="130-stripes-third-trip-masked-tail")]


@pytest.mark.parametrize("accumulate", [pytest.param(False, id="store"), pytest.param(True, id="accumulate")])
@pytest.mark.parametrize("stripes", FOLD_STRIPES)
def test_f64_to_f32(stripes, accumulate):
    ops, _ = _mods()
    for n in (1, 31, 32, 33, 100):                                          # below, at and past one 32-channel workgroup
        g = _gen(stripes, n, accumulate)
        src = _exact_rows(stripes, n, g)
        old = torch.randn(n, generator=g) * 1e5
        fs, dsrc = _guard(stripes * n, torch.float64, src)
        fd, dst = _guard(n, value=old if accumulate else None)
        ops.f64_to_f32(dsrc, dst, accumulate=accumulate, stripes=stripes)
        _guard_ok(fd)
        want = R.stripe_fold(src.numpy(), old.numpy() if accumulate else None)
        assert np.array_equal(dst.cpu().numpy(), want), (n, stripes)


@pytest.mark.parametrize("stripes", [pytest.param(64, id="64-stripes"), pytest.param(130, id="130-stripes")])
def test_f64_to_f32_batch(stripes):
    """17 items = two launches; 1 and 100 elements side by side, so the workgroups past a short item return early."""
    ops, _ = _mods()
    g = _gen(stripes, 17)
    sizes = [1, 100, 31, 32, 33, 100, 1, 7, 64, 65, 2, 100, 1, 33, 5, 96, 100]
    items, keep = [], []
    for i, n in enumerate(sizes):
        acc = i % 3 != 0
        src, old = _exact_rows(stripes, n, g), torch.randn(n, generator=g) * 1e5
        _, dsrc = _guard(stripes * n, torch.float64, src)
        fd, dst = _guard(n, value=old if acc else None)
        items.append((dsrc, dst, acc))
        keep.append((fd, dst, R.stripe_fold(src.numpy(), old.numpy() if acc else None)))
    ops.f64_to_f32_batch(items, stripes=stripes)
    for i, (fd, dst, want) in enumerate(keep):
        _guard_ok(fd)
        assert np.array_equal(dst.cpu().numpy(), want), (i, sizes[i])
