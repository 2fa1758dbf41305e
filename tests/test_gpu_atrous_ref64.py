"""Every entry point of csrc/atrous.hip through ops.* in bf16, fp16 and f32 against its plain f64 reference
(tests/_atrous_ref64.py, pinned against torch by tests/test_atrous_ref64.py), at the smallest shapes that take each path.  The case
ids name the path.  The torch-f32 comparisons of tests/test_gpu_atrous_ops.py stay as they are.

Outputs go into NaN-filled buffers wider than the slice written (guard elements / channels on both sides must stay NaN, no element
of the slice may keep the fill); input slices have NaN neighbours, at channel offsets that are no multiple of 4.

Bounds, none taken from kernel output.  U = 2^-24; ulp_T = spacing of the storage type at the reference, zero for f32.
  bit-exact      im2col_dil without prologue (zero padding and the zero channels c..cp included), maxpool_k, maxpool_k_bwd,
                 relu_mask, the zero tail of input_plain, every masked / padded zero.
  one fmaf       input_plain, affine_relu, the im2col_dil prologue: U |ref| + ulp_T / 2, the reference with the f32 scale and
                 shift.  A pre-activation that is exactly zero gives exactly 0 and a false mask (channel 0: scale = shift = 0;
                 channel 1: 1.5 * 2 - 3).  fmaf is correctly rounded, so the sign of the f32 pre-activation is the sign of the f64 one.
  sum_relu       m inputs: (m - 1) U sum|terms| + ulp_T / 2 (0 + x is exact).
  col2im_dil     values: 8 U sum|taps| + ulp_T / 2 (nine taps, eight inexact additions); the mask exact.
  statistics     _assert_sum, 2 k U sum|terms|, k = additions of the per-thread pixel loop + the 256 / cw additions of flush.  A term of
                 the second col2im_dil statistic carries three roundings (y - mean and two products) and the first addition of each
                 chain is exact, so the error is (k - 2 + 3) U sum|terms| <= 2 k U sum|terms| for the k >= 2 of every case here.  The
                 col2im_dil sums are compared with the f64 sums of the tensor the kernel wrote, read back: "statistics of the stored
                 gradient"; that gradient is checked against the reference separately.
  bilinear_up    8 U sum|w v| + ulp_T / 2 with the float32 coordinates of R.bilinear_taps (part of the definition).
  bilinear_up_bwd  (count + 2) U sum|terms| + ulp_T / 2, count and the sum from the reference.

Not asserted: NaN through the fmaxf ReLU or max pooling.  fmaxf(NaN, 0) is 0 and fmaxf(m, NaN) is m, so a NaN activation comes
out of sum_relu / affine_relu as 0 and is ignored by maxpool_k; csrc/elementwise.hip uses the same idiom."""
import ctypes as C

import pytest
import torch

import _atrous_ref64 as R
from test_gpu_elementwise_ops import (BF16, DTYPES, F32, NAN, U32, _assert_sum, _assert_tol, _f32, _fold, _guard, _guard_ok, _stats_buf,
                                      _ulp, _wide, _wide_ok)

pytestmark = pytest.mark.gpu

PSSR_ERR_ARG = -1
WRAP_DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(F32, id="f32")]
INF = float("inf")


def _mods():
    from pssr2_amd import _lib as L
    from pssr2_amd import ops
    return ops, L


def _gen(*seed):
    return torch.Generator().manual_seed(sum(int(s) * (i + 1) for i, s in enumerate(seed)) + 4242)


def _rand(shape, dt, g):
    return torch.randn(*shape, generator=g).to(dt)


def _half_ulp(ref, dt):
    return torch.zeros_like(ref) if dt == F32 else _ulp(ref, dt) / 2


def _vec(v):
    """f32 per-channel vector on the device between NaN guards."""
    return _guard(v.numel(), F32, v)[1]


def _affine(c, g):
    """(scale, shift) f32 [c]; channel 0 has scale = shift = 0 and (c >= 3) channel 1 has 2, -3: with an input of 1.5 there the
    pre-activation is exactly zero."""
    scale, shift = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    if c >= 2:
        scale[0], shift[0] = 0.0, 0.0
    if c >= 3:
        scale[1], shift[1] = 2.0, -3.0
    return scale, shift


def _preact_input(shape, dt, g):
    x = _rand(shape, dt, g)
    if shape[-1] >= 3:
        x[..., 1] = 1.5
    return x


# ---- input_plain ---------------------------------------------------------------------------------------------------------------
def _input_plain(shape, out_cs, dt):
    ops, _ = _mods()
    n, c, h, w = shape
    x = torch.rand(n, c, h, w, generator=_gen(*shape, out_cs)) * 255
    a, b = _f32(1 / 255), _f32(-0.5)
    flat, view = _guard(n * h * w * out_cs, dt)
    ops.input_plain(x.cuda(), view.view(n, h, w, out_cs), ops.dtype_code(dt), pre_scale=a, pre_shift=b)
    _guard_ok(flat)
    got = view.view(n, h, w, out_cs).cpu().double()
    ref = R.input_plain(x, out_cs, a, b)
    assert (got[..., c:] == 0).all()
    _assert_tol(got[..., :c], ref[..., :c], U32 * ref[..., :c].abs() + _half_ulp(ref[..., :c], dt), "input_plain")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("c,out_cs", [pytest.param(1, 1, id="c1-cs1-no-tail"), pytest.param(1, 16, id="c1-cs16"), pytest.param(3, 3, id="c3-cs3-no-tail"),
                                      pytest.param(3, 16, id="c3-cs16")])
def test_input_plain(c, out_cs, dt):
    _input_plain((2, c, 7, 9), out_cs, dt)


@pytest.mark.parametrize("dt", WRAP_DTYPES)
def test_input_plain_grid_wrap(dt):
    """513 * 512 * 16 = 4 202 496 elements > 16384 * 256: the last 8192 elements are a second trip."""
    _input_plain((1, 3, 513, 512), 16, dt)


# ---- affine_relu / relu_mask / sum_relu ----------------------------------------------------------------------------------------
POINTWISE = [pytest.param(198, 20, id="198px-c20"), pytest.param(198, 1, id="198px-c1")]
WRAP_PX, WRAP_C = 323 * 325, 40                           # 4 199 000 elements: 4696 past the 16384 * 256 of one trip


def _affine_relu(npix, c, dt):
    ops, _ = _mods()
    g = _gen(npix, c, 1)
    x = _preact_input((npix, c), dt, g)
    scale, shift = _affine(c, g)
    src, out = _wide((npix,), c, dt, x, left=3, right=6), _wide((npix,), c, dt, left=5, right=2)
    ops.affine_relu(src, _vec(scale), _vec(shift), out, npix, c, ops.dtype_code(dt), coff=3, out_coff=5)
    got = _wide_ok(out, c, left=5).double()
    ref = R.affine_relu(x, scale, shift)
    zero = R.preact(x, scale, shift) <= 0
    assert (got[zero] == 0).all() and (c < 3 or zero[:, :2].all())
    _assert_tol(got, ref, torch.where(zero, 0.0, U32 * ref.abs() + _half_ulp(ref, dt)), "affine_relu")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("npix,c", POINTWISE)
def test_affine_relu(npix, c, dt):
    _affine_relu(npix, c, dt)


@pytest.mark.parametrize("dt", WRAP_DTYPES)
def test_affine_relu_grid_wrap(dt):
    _affine_relu(WRAP_PX, WRAP_C, dt)


def _relu_mask(npix, c, dt):
    ops, _ = _mods()
    g = _gen(npix, c, 2)
    dout = _rand((npix, c), dt, g)
    out = torch.relu(_rand((npix, c), dt, g))                  # half exact zeros
    out[::7] = -out[::7]                                       # and negative values, -0 among them
    d_dout, d_out = _wide((npix,), c, dt, dout, left=1, right=7), _wide((npix,), c, dt, out, left=6, right=1)
    dz = _wide((npix,), c, dt, left=2, right=3)
    ops.relu_mask(d_dout, d_out, dz, npix, c, ops.dtype_code(dt), do_coff=1, o_coff=6, dz_coff=2)
    got = _wide_ok(dz, c, left=2)
    assert torch.equal(got.double(), R.relu_mask(dout, out)) and 0.3 < (got == 0).float().mean() < 0.7
    print("relu_mask: bit-exact")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("npix,c", POINTWISE)
def test_relu_mask(npix, c, dt):
    _relu_mask(npix, c, dt)


@pytest.mark.parametrize("dt", WRAP_DTYPES)
def test_relu_mask_grid_wrap(dt):
    _relu_mask(WRAP_PX, WRAP_C, dt)


def _sum_relu(npix, c, m, relu, alias, dt):
    """Input k sits at channel offset 1 + k of a buffer 10 + c wide for even k, 13 + c wide for odd k: distinct strides and offsets."""
    ops, _ = _mods()
    g = _gen(npix, c, m, relu, alias)
    xs = [_rand((npix, c), dt, g) for _ in range(m)]
    bufs = [_wide((npix,), c, dt, x, left=1 + k, right=9 - k + 3 * (k % 2)) for k, x in enumerate(xs)]
    out, left = (bufs[0], 1) if alias else (_wide((npix,), c, dt, left=5, right=4), 5)
    ops.sum_relu([(b, 1 + k) for k, b in enumerate(bufs)], out, npix, c, ops.dtype_code(dt), relu=relu, out_coff=left)
    got = _wide_ok(out, c, left=left).double()
    ref = R.sum_list(xs, relu)
    terms = R.sum_list([x.abs() for x in xs], False)
    if relu:
        assert (got >= 0).all() and (got == 0).any()
    _assert_tol(got, ref, (m - 1) * U32 * terms + _half_ulp(ref, dt), f"sum_relu m={m}")
    if m == 1:
        assert torch.equal(got, ref)                           # the copy


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("relu", [pytest.param(False, id="plain"), pytest.param(True, id="relu")])
@pytest.mark.parametrize("m", [1, 2, 3, 8])
def test_sum_relu(m, relu, dt):
    _sum_relu(198, 20, m, relu, False, dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("m,relu", [pytest.param(2, False, id="acc-plus-t-as-the-engines"), pytest.param(3, True, id="3-inputs-relu")])
def test_sum_relu_output_aliases_input0(m, relu, dt):
    _sum_relu(198, 20, m, relu, True, dt)


@pytest.mark.parametrize("dt", WRAP_DTYPES)
def test_sum_relu_grid_wrap(dt):
    _sum_relu(WRAP_PX, WRAP_C, 2, True, False, dt)


# ---- the channel walk: channel_stats_nhwc and col2im_dil -----------------------------------------------------------------------
# make_walk(c): cw = the power of two >= c, at most 256; rows = 256 / cw pixels per workgroup and trip; the workgroups are
# min(ceil(npix / rows), 2048), so a thread's pixel loop runs ceil(npix / (workgroups * rows)) times: k = trips + rows.
# (n, h, w, c, k)
WALK = [
    pytest.param(2, 9, 11, 1, 1 + 256, id="c1-cw1-256-rows"),                      # 1 workgroup
    pytest.param(2, 9, 11, 3, 1 + 64, id="c3-cw4-idle-lane"),                      # 4 workgroups, lane 3 of every 4 idle
    pytest.param(2, 9, 11, 16, 1 + 16, id="c16-exact-power-of-two"),               # 13 workgroups
    pytest.param(2, 9, 11, 20, 1 + 8, id="c20-cw32"),                              # 25 workgroups
    pytest.param(2, 9, 11, 256, 1 + 1, id="c256-one-pixel-per-workgroup"),         # 198 workgroups
    pytest.param(2, 9, 11, 257, 1 + 1, id="c257-second-cbase-pass"),               # second pass: 1 of 256 lanes busy, flush twice
]
CAP = [
    pytest.param(1, 46, 45, 260, 2 + 1, id="c260-2070px-past-2048-workgroups-two-passes"),       # rows 1: 22 pixels on a second trip
    pytest.param(1, 65, 64, 128, 2 + 2, id="c128-4160px-past-2048-workgroups"),                  # rows 2: 2080 -> 2048, 64 pixels wrap
]


def _channel_stats(npix, c, k, dt):
    ops, _ = _mods()
    x = _rand((npix, c), dt, _gen(npix, c, 3))
    buf = _wide((npix,), c, dt, x, left=3, right=2)
    flat, stats = _stats_buf(2 * c)
    ops.channel_stats_nhwc(buf, c, npix, stats, ops.dtype_code(dt), coff=3)
    _guard_ok(flat)
    got = _fold(stats, 2 * c)
    s1, s2 = R.channel_stats(x)
    a1, _ = R.channel_stats(x.abs())
    _assert_sum(got[:c], s1, a1, k, "sum")
    _assert_sum(got[c:], s2, s2, k, "sum of squares")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n,h,w,c,k", WALK + CAP)
def test_channel_stats_nhwc(n, h, w, c, k, dt):
    _channel_stats(n * h * w, c, k, dt)


@pytest.mark.parametrize("dt", DTYPES)
def test_channel_stats_nhwc_c1_past_workgroup_cap(dt):
    """c = 1: 256 pixels per workgroup, 524 800 pixels = 2050 -> 2048 workgroups, 512 pixels on a second trip: k = 2 + 256."""
    _channel_stats(524_800, 1, 2 + 256, dt)


def _col2im(n, h, w, c, dil, mode, k, dt):
    """mode: "fold" (no y), "mask" (y, no statistics), "mask-stats"."""
    ops, _ = _mods()
    g = _gen(n, h, w, c, dil, len(mode))
    cp = -(-c // 16) * 16 + (16 if c % 16 == 0 else 0)                       # always spare channels: they hold NaN and are not read
    dcol = torch.full((n, h, w, 9, cp), NAN, dtype=dt)
    dcol[..., :c] = _rand((n, h, w, 9, c), dt, g)
    y = _preact_input((n, h, w, c), dt, g)
    scale, shift = _affine(c, g)
    mean, invstd = torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) + 0.5
    out = _wide((n, h, w), c, dt, left=5, right=2)
    kw, flat = {}, None
    if mode != "fold":
        kw = dict(y=_wide((n, h, w), c, dt, y, left=3, right=6), y_coff=3, scale=_vec(scale), shift=_vec(shift))
    if mode == "mask-stats":
        flat, stats = _stats_buf(2 * c)
        kw.update(mean=_vec(mean), invstd=_vec(invstd), stats=stats)
    ops.col2im_dil(dcol.view(n, h, w, 9 * cp).cuda(), cp, out, c, n, h, w, dil, ops.dtype_code(dt), out_coff=5, **kw)
    got = _wide_ok(out, c, left=5).double()
    ref = R.col2im_dil(dcol[..., :c], dil)
    tol = 8 * U32 * R.col2im_dil(dcol[..., :c].abs(), dil)
    if mode != "fold":
        mask = R.preact_mask(y, scale, shift)
        assert (got[~mask] == 0).all() and (c < 3 or not mask[..., :2].any()) and mask[..., -1].any() and not mask[..., -1].all()
        ref = torch.where(mask, ref, 0.0)
        tol = torch.where(mask, tol + _half_ulp(ref, dt), 0.0)
    else:
        tol = tol + _half_ulp(ref, dt)
    _assert_tol(got, ref, tol, f"col2im_dil {mode} dil={dil}")
    if mode == "mask-stats":
        _guard_ok(flat)
        s = _fold(stats, 2 * c)
        s1, s2 = R.bn_bwd_stats(got, y, mean, invstd)
        a1, a2 = R.bn_bwd_stats(got.abs(), y, mean, invstd)[0], (got * (y.double() - mean.double()) * invstd.double()).abs().reshape(-1, c).sum(0)
        _assert_sum(s[:c], s1, a1, k, "sum g")
        _assert_sum(s[c:], s2, a2, k, "sum g xhat")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("mode", ["fold", "mask", "mask-stats"])
@pytest.mark.parametrize("n,h,w,c,k", WALK)
def test_col2im_dil_channel_walk(n, h, w, c, k, mode, dt):
    _col2im(n, h, w, c, 2, mode, k, dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n,h,w,c,k", CAP)
def test_col2im_dil_past_workgroup_cap(n, h, w, c, k, dt):
    _col2im(n, h, w, c, 3, "mask-stats", k, dt)


# ---- dilation ------------------------------------------------------------------------------------------------------------------
# on 15 x 18: 14 leaves one row of off-centre taps, 15 none vertically, 17 one column, 18 and 31 the centre tap alone
DILS = [pytest.param(1, id="dil1"), pytest.param(3, id="dil3"), pytest.param(14, id="dil14-h-1"), pytest.param(15, id="dil15-h"),
        pytest.param(17, id="dil17-w-1"), pytest.param(18, id="dil18-w-centre-tap-only"), pytest.param(31, id="dil31-centre-tap-only")]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("dil", DILS)
def test_col2im_dil_dilations(dil, dt):
    _col2im(2, 15, 18, 20, dil, "mask-stats", 1 + 8, dt)               # 540 pixels, rows 8: 68 workgroups, one trip


def _im2col(n, h, w, c, cp, dil, prologue, dt):
    ops, _ = _mods()
    g = _gen(n, h, w, c, dil, prologue)
    x = _preact_input((n, h, w, c), dt, g)
    src = _wide((n, h, w), c, dt, x, left=3, right=6)
    flat, view = _guard(n * h * w * 9 * cp, dt)
    scale, shift = _affine(c, g)
    kw = dict(scale=_vec(scale), shift=_vec(shift)) if prologue else {}
    ops.im2col_dil(src, c, view.view(n, h, w, 9 * cp), cp, n, h, w, dil, ops.dtype_code(dt), in_coff=3, **kw)
    _guard_ok(flat)
    got = view.view(n, h, w, 9, cp).cpu().double()
    assert (got[..., c:] == 0).all()
    got = got[..., :c]
    if not prologue:
        assert torch.equal(got, R.im2col_dil(x, dil))
        print("im2col_dil: bit-exact")
        return
    ref = R.im2col_dil(x, dil, scale, shift)
    live = R.im2col_dil(R.preact_mask(x, scale, shift).double(), dil) != 0               # inside the image and a positive pre-activation
    assert (got[~live] == 0).all() and (c < 3 or not live[..., :2].any())
    _assert_tol(got, ref, torch.where(live, U32 * ref.abs() + _half_ulp(ref, dt), 0.0), f"im2col_dil prologue dil={dil}")
    # the storage rounding of the reference differs from the kernel's only where the f32 value sits within U |ref| of a tie
    rounded = R.im2col_dil(x, dil, scale, shift, round_to=dt)
    assert ((got != rounded).float().mean() < 1e-3) if dt != F32 else True


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("prologue", [pytest.param(False, id="plain"), pytest.param(True, id="bn-relu-prologue")])
@pytest.mark.parametrize("dil", DILS)
def test_im2col_dil_dilations(dil, prologue, dt):
    _im2col(2, 15, 18, 20, 32, dil, prologue, dt)


@pytest.mark.parametrize("dt", WRAP_DTYPES)
@pytest.mark.parametrize("prologue", [pytest.param(False, id="plain"), pytest.param(True, id="bn-relu-prologue")])
def test_im2col_dil_grid_wrap(prologue, dt):
    """171 * 171 * 9 * 16 = 4 210 704 elements: 16 400 on a second trip."""
    _im2col(1, 171, 171, 5, 16, 2, prologue, dt)


# ---- max pooling ---------------------------------------------------------------------------------------------------------------
POOL_K = [pytest.param(1, id="k1"), pytest.param(2, id="k2"), pytest.param(3, id="k3"), pytest.param(4, id="k4"), pytest.param(8, id="k8")]
POOL_HW = [pytest.param(8, 8, id="8x8"), pytest.param(13, 9, id="13x9"), pytest.param(10, 14, id="10x14"), pytest.param(15, 25, id="15x25"),
           pytest.param(16, 24, id="16x24")]


def _pool(n, h, w, c, k, dt, infs=True):
    """Forward and gradient, bit-exact.  Quantised inputs (multiples of 1/2 in [-1.5, 1.5]): most windows tie; one window of
    all -inf (its gradient goes to its first pixel) and one holding +inf."""
    ops, _ = _mods()
    g = _gen(n, h, w, c, k)
    x = (torch.randint(-3, 4, (n, h, w, c), generator=g).float() * 0.5).to(dt)
    if infs:
        x[0, :k, :k, 0] = -INF
        x[n - 1, 0, 0, 1] = INF
    ho, wo = h // k, w // k
    src = _wide((n, h, w), c, dt, x, left=3, right=2)
    out = _wide((n, ho, wo), c, dt, left=1, right=6)
    ops.maxpool_k(src, out, n, h, w, c, k, ops.dtype_code(dt), in_coff=3, out_coff=1)
    assert torch.equal(_wide_ok(out, c, left=1).double(), R.maxpool_k(x, k))
    dp = _rand((n, ho, wo, c), dt, g)
    dx = _wide((n, h, w), c, dt, left=6, right=1)
    ops.maxpool_k_bwd(src, _wide((n, ho, wo), c, dt, dp, left=2, right=3), dx, n, h, w, c, k, ops.dtype_code(dt), act_coff=3, dp_coff=2, dx_coff=6)
    got = _wide_ok(dx, c, left=6).double()
    assert torch.equal(got, R.maxpool_k_bwd(x, dp, k))
    assert (got[:, ho * k:] == 0).all() and (got[:, :, wo * k:] == 0).all() and (got != 0).sum() == (dp != 0).sum()
    print("maxpool_k, maxpool_k_bwd: bit-exact")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("h,w", POOL_HW)
@pytest.mark.parametrize("k", POOL_K)
def test_maxpool_k_and_bwd(k, h, w, dt):
    _pool(2, h, w, 12, k, dt)


@pytest.mark.parametrize("dt", WRAP_DTYPES)
def test_maxpool_k_grid_wrap(dt):
    """k = 2 on 646 x 650, c = 40: 323 * 325 * 40 outputs."""
    ops, _ = _mods()
    n, h, w, c, k = 1, 646, 650, 40, 2
    x = (torch.randint(-3, 4, (n, h, w, c), generator=_gen(646)).float() * 0.5).to(dt)
    out = _wide((n, h // k, w // k), c, dt, left=1, right=2)
    ops.maxpool_k(_wide((n, h, w), c, dt, x, left=3, right=1), out, n, h, w, c, k, ops.dtype_code(dt), in_coff=3, out_coff=1)
    assert torch.equal(_wide_ok(out, c, left=1).double(), R.maxpool_k(x, k))


@pytest.mark.parametrize("dt", WRAP_DTYPES)
def test_maxpool_k_bwd_grid_wrap(dt):
    """k = 2 on 323 x 325, c = 40: the last row and column lie outside every window."""
    _pool(1, 323, 325, WRAP_C, 2, dt, infs=False)


# ---- bilinear resize -----------------------------------------------------------------------------------------------------------
RESIZE = [pytest.param(7, 7, 7, 7, id="7x7-identity"), pytest.param(1, 1, 8, 15, id="1x1-to-8x15-one-source-pixel"),
          pytest.param(1, 3, 15, 25, id="1x3-to-15x25-hs1"), pytest.param(3, 2, 13, 9, id="3x2-to-13x9"),
          pytest.param(6, 4, 13, 9, id="6x4-to-13x9-k2-remainder"), pytest.param(5, 7, 6, 8, id="5x7-to-6x8-ratio-just-above-1"),
          pytest.param(2, 3, 16, 24, id="2x3-to-16x24-k8")]


def _up(n, hs, ws, h, w, c, dt):
    ops, _ = _mods()
    x = _rand((n, hs, ws, c), dt, _gen(hs, ws, h, w, c))
    out = _wide((n, h, w), c, dt, left=5, right=2)
    ops.bilinear_up(_wide((n, hs, ws), c, dt, x, left=3, right=6), out, n, hs, ws, h, w, c, ops.dtype_code(dt), in_coff=3, out_coff=5)
    got = _wide_ok(out, c, left=5).double()
    ref = R.bilinear_up(x, h, w)
    _assert_tol(got, ref, 8 * U32 * R.bilinear_up(x.abs(), h, w) + _half_ulp(ref, dt), "bilinear_up")
    if (hs, ws) == (h, w):
        assert torch.equal(got, x.double())


def _up_bwd(n, hs, ws, h, w, c, dt):
    ops, _ = _mods()
    dout = _rand((n, h, w, c), dt, _gen(hs, ws, h, w, c, 1))
    din = _wide((n, hs, ws), c, dt, left=1, right=4)
    ops.bilinear_up_bwd(_wide((n, h, w), c, dt, dout, left=6, right=3), din, n, hs, ws, h, w, c, ops.dtype_code(dt), do_coff=6, di_coff=1)
    got = _wide_ok(din, c, left=1).double()
    ref, count, abs_sum = R.bilinear_up_bwd(dout, hs, ws)
    _assert_tol(got, ref, (count[None, :, :, None] + 2) * U32 * abs_sum + _half_ulp(ref, dt), "bilinear_up_bwd")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("hs,ws,h,w", RESIZE)
def test_bilinear_up(hs, ws, h, w, dt):
    _up(2, hs, ws, h, w, 12, dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("hs,ws,h,w", RESIZE)
def test_bilinear_up_bwd(hs, ws, h, w, dt):
    _up_bwd(2, hs, ws, h, w, 12, dt)


@pytest.mark.parametrize("dt", WRAP_DTYPES)
def test_bilinear_up_grid_wrap(dt):
    """To 323 x 325 from its k = 2 pooling, 161 x 162: coordinates up to 161, where a product rounded on its own would show."""
    _up(1, 161, 162, 323, 325, WRAP_C, dt)


@pytest.mark.parametrize("dt", WRAP_DTYPES)
def test_bilinear_up_bwd_grid_wrap(dt):
    """324 x 324 x 40 = 4 199 040 source elements, ratio 325 / 324."""
    _up_bwd(1, 324, 324, 325, 325, WRAP_C, dt)


# ---- argument checks -----------------------------------------------------------------------------------------------------------
# name: parameters in ABI order; p pointer, i int, l int64, f float, P / I the pointer / int arrays of sum_relu
SIGS = {
    "input_plain": "x:p out:p n:i c:i h:i w:i out_cs:i pre_scale:f pre_shift:f dtype:i",
    "im2col_dil": "in:p in_cs:i in_co:i c:i scale:p shift:p col:p cp:i n:i h:i w:i dil:i dtype:i",
    "col2im_dil": "dcol:p cp:i out:p out_cs:i out_co:i c:i n:i h:i w:i dil:i y:p y_cs:i y_co:i scale:p shift:p mean:p invstd:p stats:p dtype:i",
    "channel_stats_nhwc": "x:p cs:i co:i c:i npix:l stats:p dtype:i",
    "sum_relu": "ins:P in_cs:I in_co:I n_in:i out:p out_cs:i out_co:i npix:l c:i relu:i dtype:i",
    "relu_mask": "dout:p do_cs:i do_co:i out:p o_cs:i o_co:i dz:p dz_cs:i dz_co:i npix:l c:i dtype:i",
    "affine_relu": "x:p cs:i co:i scale:p shift:p out:p out_cs:i out_co:i npix:l c:i dtype:i",
    "maxpool_k": "in:p in_cs:i in_co:i out:p out_cs:i out_co:i n:i h:i w:i c:i k:i dtype:i",
    "maxpool_k_bwd": "act:p act_cs:i act_co:i dpool:p dp_cs:i dp_co:i dx:p dx_cs:i dx_co:i n:i h:i w:i c:i k:i dtype:i",
    "bilinear_up": "in:p in_cs:i in_co:i out:p out_cs:i out_co:i n:i hs:i ws:i h:i w:i c:i dtype:i",
    "bilinear_up_bwd": "dout:p do_cs:i do_co:i din:p di_cs:i di_co:i n:i hs:i ws:i h:i w:i c:i dtype:i",
}
GOOD = dict(n=1, c=8, h=4, w=4, hs=2, ws=2, k=2, dil=1, cp=16, npix=16, relu=1, n_in=2, dtype=0, pre_scale=1.0, pre_shift=0.0)
OPTIONAL = {"im2col_dil": {"scale", "shift"}, "col2im_dil": {"y", "scale", "shift", "mean", "invstd", "stats"}}


def _params(name):
    return [p.split(":") for p in SIGS[name].split()]


def _call(name, buf, **over):
    """Status of pssr_<name> with valid small arguments (every pointer the same 256 KiB device buffer, slices (cs, co, c) =
    (16, 4, 8)) except those overridden."""
    _, L = _mods()
    args = []
    for pname, kind in _params(name):
        v = GOOD.get(pname, 16 if pname.endswith("cs") else 4 if pname.endswith("co") else buf.data_ptr())
        v = over.get(pname, v)
        if kind == "p":
            args.append(None if v is None else C.c_void_p(v))
        elif kind == "P":
            args.append(None if v is None else (C.c_void_p * 8)(*(v if isinstance(v, list) else [buf.data_ptr()] * 8)))
        elif kind == "I":
            args.append(None if v is None else (C.c_int * 8)(*(v if isinstance(v, list) else [v] * 8)))
        elif kind == "l":
            args.append(C.c_int64(v))
        elif kind == "f":
            args.append(C.c_float(v))
        else:
            args.append(C.c_int(v))
    return getattr(L.lib(), "pssr_" + name)(*args, L.stream_ptr())


@pytest.mark.parametrize("name", list(SIGS))
def test_argument_errors(name):
    """PSSR_ERR_ARG with a message that names the entry point; the valid call the refusals are varied from returns 0."""
    _, L = _mods()
    buf = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
    assert _call(name, buf) == 0, L.lib().pssr_last_error()
    torch.cuda.synchronize()

    def refused(**over):
        status = _call(name, buf, **over)
        msg = L.lib().pssr_last_error()
        assert status == PSSR_ERR_ARG and name.encode() in msg, (name, over, status, msg)

    names = [p for p, _ in _params(name)]
    for pname, kind in _params(name):
        if kind in "pPI" and pname not in OPTIONAL.get(name, ()):
            refused(**{pname: None})
    refused(dtype=3), refused(dtype=-1)
    for pname in ("c", "n", "npix", "h", "w", "hs", "ws"):
        if pname in names and not (name.startswith("bilinear") and pname in ("h", "w")):
            refused(**{pname: 0}), refused(**{pname: -1})
    for pname in names:                                            # every slice: co + c > cs, co < 0
        if pname.endswith("co"):
            cs = pname[:-1] + "s"
            refused(**{pname: 9}), refused(**{pname: -1}), refused(**{pname: -8}), refused(**{cs: 11}), refused(**{cs: 0})
    if name == "sum_relu":
        refused(n_in=0), refused(n_in=9), refused(n_in=-1)
        refused(in_co=[4, 9, 4, 4, 4, 4, 4, 4]), refused(in_co=[4, -1, 4, 4, 4, 4, 4, 4]), refused(in_cs=[16, 11, 16, 16, 16, 16, 16, 16])
        refused(ins=[buf.data_ptr(), None, 0, 0, 0, 0, 0, 0])
        assert _call(name, buf, in_co=[4, 4, 9, -1, 9, 9, 9, 9]) == 0              # inputs beyond n_in are not looked at
    if name == "input_plain":
        refused(out_cs=7)
    if "dil" in names:
        refused(dil=0), refused(dil=-1), refused(cp=7)
    if "k" in names:
        refused(k=0), refused(k=-1), refused(k=5), refused(k=4, w=3), refused(k=4, h=3)
        assert _call(name, buf, k=4) == 0 and _call(name, buf, k=3) == 0
    if name.startswith("bilinear"):
        refused(h=1), refused(w=1), refused(h=0), refused(w=-1)
        assert _call(name, buf, h=2, w=2) == 0
    if name == "im2col_dil":
        refused(shift=None), refused(scale=None)
        assert _call(name, buf, scale=None, shift=None) == 0
    if name == "col2im_dil":
        refused(scale=None), refused(shift=None)                  # the mask needs both
        refused(y=None), refused(mean=None), refused(invstd=None)            # statistics need the pre-activation, mean and invstd
        assert _call(name, buf, y=None, stats=None, y_co=99) == 0          # the slice of an absent y is not looked at
        assert _call(name, buf, stats=None, mean=None, invstd=None) == 0
    torch.cuda.synchronize()
