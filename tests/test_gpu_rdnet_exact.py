"""Every entry point of csrc/rdnet.hip against its plain f64 reference (tests/_rdnet_ref64.py, pinned against torch autograd by
tests/test_rdnet_ref64.py), at the smallest shapes that take each path of each launcher.  The case ids name the path.

Conventions of tests/test_gpu_elementwise_ops.py, whose helpers are imported: inputs are rounded to the storage type before the
reference sees them; outputs are written into NaN-filled buffers wider than the slice written by PAD channels / elements on each
side, which must stay NaN while no written element may keep the fill; inputs that are channel slices have NaN neighbours; channel
offsets are non-zero wherever the entry point takes them.

Tolerances, all derived.  Data movement (the weight packs, the zero fill of pad channels, the space-to-depth placement) and repeated
runs of every kernel without atomics are bit-exact, and so is the tile kernel of dwconv7 against the row-segment kernel.  An f32 sum
is within 2 k 2^-24 sum|terms| of the reference, k the longest chain of f32 additions a term passes through on that path at that shape
(derived beside each case; the factor 2 pays for the roundings inside a term, and `x += sum` counts one more addition); with f32 atomics
the order is free and k = terms - 1.  A result stored in a 16-bit type gets one spacing of that type at |ref| on top.  LayerNorm's
mean / rstd / out / dx propagate the bounds of the two wave sums through the kernel's expression (_ln_fwd_bounds, _ln_bwd_bounds).
Nothing here is derived from kernel output."""
import ctypes as C
from contextlib import contextmanager

import pytest
import torch

import _rdnet_ref64 as R
import test_gpu_elementwise_ops as E
from test_gpu_elementwise_ops import (DTYPES, F32, NAN, PAD, U32, _assert_sum, _assert_tol, _f32, _fold, _guard, _guard_ok,
                                      _image, _mods, _ref, _stats_buf, _ulp, _wide, _wide_ok)

pytestmark = pytest.mark.gpu

F64 = torch.float64


def _gen(*seed):
    return torch.Generator().manual_seed(sum(int(s) * (i + 1) for i, s in enumerate(seed)) + 777)


def _cdiv(a, b):
    return -(-a // b)


def _q(x, dt):
    """Rounded to the storage type, as f64."""
    return x.to(dt).double()


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _store(ref, dt):
    """What storing into `dt` adds to a bound: one spacing of the type at |ref|; nothing for f32, whose last rounding the bound counts."""
    return torch.zeros_like(ref) if dt == F32 else _ulp(ref, dt)


@contextmanager
def _option(name, value):
    """Sets a library option (None: leaves it) and restores the old value."""
    _, L = _mods()
    if value is None:
        yield
        return
    old = L.lib().pssr_set_option(name, value)
    assert old >= 0
    try:
        yield
    finally:
        L.lib().pssr_set_option(name, old)


def _wide_px(lead, c, dt, data):
    """_wide with a spare NaN pixel before the first pixel and after the last: a read one pixel outside the tensor stays inside the
    buffer and poisons the result."""
    npix = 1
    for d in lead:
        npix *= d
    flat = torch.full((npix + 2, c + 2 * PAD), NAN, dtype=dt, device="cuda")
    buf = flat[1:npix + 1].view(*lead, c + 2 * PAD)
    buf[..., PAD:PAD + c] = data.to(dt).cuda()
    return buf


def _sum_tol(k, mag, extra=0.0):
    return 2.0 * k * U32 * mag + extra


# ---- input_patchify ------------------------------------------------------------------------------------------------------------
PATCHIFY = [
    pytest.param((2, 3, 8, 12), 2, 16, id="ps2-c3-12-of-16"),
    pytest.param((1, 1, 4, 6), 2, 64, id="ps2-c1-wide-zero-tail-4-of-64"),
    pytest.param((1, 1, 8, 8), 4, 16, id="ps4-c1-no-tail"),
    pytest.param((2, 3, 8, 12), 4, 48, id="ps4-c3-no-tail"),
    pytest.param((1, 2, 8, 4), 4, 48, id="ps4-c2-32-of-48"),
]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,ps,pc", PATCHIFY)
def test_input_patchify(shape, ps, pc, dt):
    """Integer pixels: x / 128 - 1 is exact, so the second FMA's rounding is the only one before the store: 2^-24 |ref|, plus the
    storage spacing.  The zero tail is bit-exact."""
    ops, _ = _mods()
    n, c, h, w = shape
    g = _gen(*shape, ps, pc)
    x = _image(n, c, h, w, g)
    scale, shift, _, _ = E._channel_params(c, g)
    flat, view = _guard(n * (h // ps) * (w // ps) * pc, dt)
    xp = view.view(n, h // ps, w // ps, pc)
    ops.input_patchify(x.cuda(), xp, scale.cuda(), shift.cuda(), ps, ops.dtype_code(dt))
    _guard_ok(flat)
    ref = R.patchify(x, ps, pc, scale, shift)
    got = xp.cpu().double()
    assert (got[..., c * ps * ps:] == 0).all() and (ref[..., c * ps * ps:] == 0).all()
    _assert_tol(got, ref, U32 * ref.abs() + _store(ref, dt), "xpatch")


# ---- dwconv7_pack / dwconv7_pack_batch -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [pytest.param(False, id="forward"), pytest.param(True, id="flipped")])
@pytest.mark.parametrize("c", [4, 12, 68, 1028])
def test_dw_pack(c, flip):
    ops, _ = _mods()
    w = torch.randn(c, 1, 7, 7, generator=_gen(c, flip))
    flat, out = _guard(49 * c)
    _, wd = _guard(49 * c, value=w)                                        # NaN before and after the weight
    ops.dwconv7_pack(wd.view(c, 1, 7, 7), out, flip=flip)
    _guard_ok(flat)
    assert torch.equal(out.cpu().view(49, c), R.dw_pack(w, flip))


def test_dw_pack_batch():
    """48 items = one full launch, both orientations, channel counts from 4 to 1028 side by side (the workgroups past a small item's
    end do nothing)."""
    ops, L = _mods()
    g = _gen(48)
    cs = [4, 1028, 12, 68, 8, 264] * 8
    assert len(cs) == L.DWPACK_BATCH_MAX
    items, keep = [], []
    for i, c in enumerate(cs):
        w = torch.randn(c, 1, 7, 7, generator=g)
        flat, out = _guard(49 * c)
        flip = bool((i // 6) & 1) ^ bool(i & 1)
        items.append((_guard(49 * c, value=w)[1].view(c, 1, 7, 7), out, flip))
        keep.append((flat, out, R.dw_pack(w, flip), c))
    ops.dwconv7_pack_batch(items)
    for i, (flat, out, want, c) in enumerate(keep):
        _guard_ok(flat)
        assert torch.equal(out.cpu().view(49, c), want), (i, c)


# ---- dwconv7 -------------------------------------------------------------------------------------------------------------------
# k: the accumulator starts from the bias (or 0) and takes one FMA per tap; taps outside the image are skipped (plain kernel) or add an
# exact zero (row-segment and tile kernels), so a term passes through at most min(7, h) * min(7, w) additions, one more with accumulate.
DWCONV = [
    pytest.param((2, 8, 3, 5), None, id="plain-w5-every-tap-row-clipped"),
    pytest.param((1, 12, 9, 13), None, id="plain-w13"),
    pytest.param((2, 68, 5, 8), 1, id="tile8-partial-channel-tile-w8-h5"),                     # 2 images x 2 channel tiles = 4 workgroups
    pytest.param((1, 64, 8, 24), 1, id="tile8-half-filled-last-column-tile"),
    pytest.param((1, 132, 9, 16), 1, id="tile16-one-row-tile-rows-9-15-idle"),
    pytest.param((3, 72, 17, 40), 1, id="tile16-36-workgroups-xcd-remap-32-of-36"),           # 3 x 2 row x 3 column x 2 channel tiles
    pytest.param((2, 12, 4, 8), 0, id="seg-one-segment-left-and-right-edge"),
    pytest.param((1, 8, 9, 24), 0, id="seg-three-segments"),
]


def _dw_inputs(shape, dt, g):
    n, c, h, w = shape
    x = _q(torch.randn(shape, generator=g), dt)
    wt = torch.randn(c, 1, 7, 7, generator=g) / 7
    bias = torch.randn(c, generator=g)
    prev = _q(torch.randn(shape, generator=g), dt)
    return x, wt, bias, prev


def _run_dwconv(ops, xin, wp, bias, prev, shape, dt, accumulate):
    n, c, h, w = shape
    out = _wide((n, h, w), c, dt, _nhwc(prev) if accumulate else None)
    ops.dwconv7(xin, wp, bias, out, n, h, w, c, ops.dtype_code(dt), in_coff=PAD, out_coff=PAD, accumulate=accumulate)
    return _nchw(_wide_ok(out, c))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,tile", DWCONV)
def test_dwconv7(shape, tile, dt):
    """Forward (R.dw_pack) and input gradient (the flipped pack), with and without bias, storing and accumulating; the storing runs
    are repeated and must give the same bits."""
    ops, _ = _mods()
    n, c, h, w = shape
    g = _gen(*shape, 1)
    x, wt, bias, prev = _dw_inputs(shape, dt, g)
    xin = _wide_px((n, h, w), c, dt, _nhwc(x))
    taps = min(7, h) * min(7, w)
    with _option(b"DWCONV_TILE", tile):
        for direction, flip, (ref0, mag0) in (("fwd", False, R.dwconv7(x, wt)), ("dgrad", True, R.dwconv7_dgrad(x, wt))):
            wp = R.dw_pack(wt, flip).cuda()
            for use_bias in (True, False):
                for acc in (False, True):
                    ref, mag = ref0.clone(), mag0.clone()
                    if use_bias:
                        ref += bias.double()[None, :, None, None]
                        mag += bias.double().abs()[None, :, None, None]
                    if acc:
                        ref += prev
                        mag += prev.abs()
                    got = _run_dwconv(ops, xin, wp, bias.cuda() if use_bias else None, prev, shape, dt, acc)
                    _assert_tol(got, ref, _sum_tol(taps + acc, mag) + _store(ref, dt), f"{direction} bias={use_bias} accumulate={acc}")
                    if not acc:
                        again = _run_dwconv(ops, xin, wp, bias.cuda() if use_bias else None, prev, shape, dt, acc)
                        assert torch.equal(got, again)


@pytest.mark.parametrize("shape", [pytest.param((2, 12, 4, 8), id="one-segment"), pytest.param((1, 8, 9, 24), id="three-segments"),
                                   pytest.param((2, 68, 5, 8), id="tile8"), pytest.param((3, 72, 17, 40), id="tile16-xcd-remap")])
def test_dwconv7_tile_equals_seg(shape):
    """DWCONV_TILE=1 against DWCONV_TILE=0 on the same finite f32 inputs: both add the same 49 FMAs in the same order onto the bias, so
    the bits agree.  A cross-check: each kernel meets the reference in test_dwconv7."""
    ops, _ = _mods()
    n, c, h, w = shape
    x, wt, bias, prev = _dw_inputs(shape, F32, _gen(*shape, 2))
    xin = _wide_px((n, h, w), c, F32, _nhwc(x))
    wp = R.dw_pack(wt).cuda()
    for use_bias in (True, False):
        for acc in (False, True):
            res = []
            for tile in (1, 0):
                with _option(b"DWCONV_TILE", tile):
                    res.append(_run_dwconv(ops, xin, wp, bias.cuda() if use_bias else None, prev, shape, F32, acc))
            assert torch.equal(res[0], res[1]), (use_bias, acc)


# ---- dwconv7_wgrad (f32 atomics) -----------------------------------------------------------------------------------------------
# The workgroups meet in dw through f32 atomics in any order: k = terms - 1, at most n h w - 1 per tap, + 1 for dw += onto the non-zero
# prior contents.
WGRAD = [
    pytest.param((2, 8, 3, 5), id="plain-c8-128-pixel-lanes"),
    pytest.param((1, 12, 9, 13), id="plain-c12-thread-255-idle"),
    pytest.param((1, 1028, 3, 5), id="plain-c1028-second-channel-pass-one-live-lane"),
    pytest.param((2, 132, 5, 8), id="rows-atomics-w8-second-channel-block-one-live-lane"),
]


def _wgrad_inputs(shape, dt, g):
    n, c, h, w = shape
    x, dy = _q(torch.randn(shape, generator=g), dt), _q(torch.randn(shape, generator=g), dt)
    prev = torch.randn(c, 49, generator=g)
    return x, dy, prev, _wide_px((n, h, w), c, dt, _nhwc(x)), _wide_px((n, h, w), c, dt, _nhwc(dy))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", WGRAD)
def test_dwconv7_wgrad_atomics(shape, dt):
    ops, L = _mods()
    n, c, h, w = shape
    x, dy, prev, xin, dyin = _wgrad_inputs(shape, dt, _gen(*shape, 3))
    flat, dw = _guard(c * 49, value=prev)
    L.check(L.lib().pssr_dwconv7_wgrad(*_ref(L, dyin, PAD), *_ref(L, xin, PAD), L.ptr(dw), n, h, w, c, ops.dtype_code(dt), L.stream_ptr()),
            "pssr_dwconv7_wgrad")
    _guard_ok(flat)
    ref, mag = R.dwconv7_wgrad(dy, x)
    _assert_sum(dw.cpu().view(c, 49), ref + prev.double(), mag + prev.double().abs(), n * h * w, "dw")


# ---- dwconv7_wgrad_ws (slabs, fixed order) -------------------------------------------------------------------------------------
# A workgroup of the rows kernel walks per_block row segments of 8 pixels: 8 per_block FMAs into an accumulator (zero padding adds exact
# zeros).  The reduce kernel gives every 16th slab to one of 16 lanes (at most ceil(slabs / 16) additions, + 2 where the four partial
# sums of the unrolled loop meet), adds the 16 lane sums in order (16) and then dw += (1).
# (shape, DWWG_BLOCKS, slabs, per_block)
WGRAD_WS = [
    pytest.param((1, 8, 1, 8), None, 1, 1, id="1-slab"),
    pytest.param((1, 8, 17, 32), None, 17, 4, id="17-slabs-second-tail-trip"),
    pytest.param((1, 8, 33, 64), None, 66, 4, id="66-slabs-unrolled-reduce-xcd-remap"),
    pytest.param((2, 132, 9, 16), None, 9, 4, id="9-slabs-second-channel-block"),
    pytest.param((1, 8, 33, 64), 3, 3, 88, id="DWWG_BLOCKS-3-88-segments-per-slab"),
]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,blocks,slabs,per_block", WGRAD_WS)
def test_dwconv7_wgrad_ws(shape, blocks, slabs, per_block, dt):
    ops, L = _mods()
    lib = L.lib()
    lib.pssr_dwconv7_wgrad_workspace_bytes.restype = C.c_int64
    n, c, h, w = shape
    x, dy, prev, xin, dyin = _wgrad_inputs(shape, dt, _gen(*shape, 4))
    ref, mag = R.dwconv7_wgrad(dy, x)
    gy = _cdiv(c // 4, 32)
    k = 8 * per_block + _cdiv(slabs, 16) + 2 + 16 + 1
    runs = []
    with _option(b"DWWG_BLOCKS", blocks):
        need = lib.pssr_dwconv7_wgrad_workspace_bytes(n, h, w, c)
        assert need == slabs * gy * 128 * 49 * 4
        for _ in range(2):
            fws, ws = _guard(need // 4)                                    # NaN: a slab element read before it is written poisons dw
            flat, dw = _guard(c * 49, value=prev)
            L.check(lib.pssr_dwconv7_wgrad_ws(*_ref(L, dyin, PAD), *_ref(L, xin, PAD), L.ptr(dw), n, h, w, c, ops.dtype_code(dt), L.ptr(ws),
                                              C.c_int64(need), L.stream_ptr()), "pssr_dwconv7_wgrad_ws")
            _guard_ok(flat)
            _guard_ok(fws, written=False)
            runs.append(dw.cpu().view(c, 49))
    assert torch.equal(runs[0], runs[1])
    _assert_sum(runs[0], ref + prev.double(), mag + prev.double().abs(), k, "dw")


# ---- layernorm2d_fwd / layernorm2d_bwd -----------------------------------------------------------------------------------------
EPS = _f32(1e-6)


def _ln_fwd_bounds(x, gamma, beta, c):
    """(out, mean, rstd) of the reference and their bounds (tol_out, d_mu, d_rs), for f32 results before any 16-bit store.

    Forward kernel, per pixel, nit = ceil(c / 256) channel slices per lane:
      S = wave_sum(s), s += (v0 + v1) + (v2 + v3) per slice: 2 + nit additions in the lane, 6 butterfly levels: k1 = 2 + nit + 6 and
          |S^ - S| <= 2 k1 u sum|x|.  mu^ = S^ * fl(1 / c): two more roundings, d_mu = 2 k1 u sum|x| / c + 2 u |mu|.
      Q = wave_sum(q), q = fma(d, d, q) with d = fl(v - mu^): sum (x - mu^)^2 = sum (x - mu)^2 + c (mu - mu^)^2 exactly, 4 nit FMAs in
          the lane and 6 levels: k2 = 4 nit + 6, and 2 k2 u covers the two roundings of d inside d^2.  var^ + eps = Q^ * fl(1 / c) + eps:
          the rounding of 1 / c, of the product and of the sum, all relative to at most var + eps, with the factor 2 again:
          d_var = (2 k2 + 4) u (var + eps) + d_mu^2.
      rstd^ = rsqrtf(var^ + eps): 1 / sqrt is decreasing and convex, so its change is at most 1 / sqrt(var + eps - d_var) - rstd; the
          function itself is allowed 2 ulp = 4 u rstd.  That is d_rs.
      out = fma(fl(fl(v - mu^) * rstd^), gamma, beta): first order in d_mu and d_rs,
          |gamma| (|x - mu| d_rs + d_mu (rstd + d_rs)), plus the three roundings: 2 u |xhat gamma| + u |out|."""
    out, mean, rstd = R.layernorm2d_fwd(x, gamma, beta, EPS)
    nit = _cdiv(c, 256)
    k1, k2 = 2 + nit + 6, 4 * nit + 6
    d_mu = 2 * k1 * U32 * x.abs().sum(1) / c + 2 * U32 * mean.abs()
    var_eps = 1.0 / rstd ** 2
    d_var = (2 * k2 + 4) * U32 * var_eps + d_mu ** 2
    assert (d_var < 0.5 * var_eps).all()
    d_rs = 1.0 / torch.sqrt(var_eps - d_var) - rstd + 4 * U32 * rstd
    xc = x - mean[:, None]
    gm = gamma.double().abs()[None, :, None, None]
    tol = gm * (xc.abs() * d_rs[:, None] + d_mu[:, None] * (rstd + d_rs)[:, None]) + 2 * U32 * (xc * rstd[:, None]).abs() * gm + U32 * out.abs()
    return out, mean, rstd, tol, d_mu, d_rs


def _ln_bwd_bounds(g, x, gamma, mean, rstd, c):
    """dx of the reference and its bound, from the saved f32 mean / rstd (inputs: exact).  Backward kernel, per pixel:
      xh = fl(fl(x - mu) * rs): 2 roundings; gg = fl(g * gamma): 1.
      m1 = wave_sum(s1) * fl(1 / c), s1 += gg: 4 nit additions in the lane, 6 levels, k = 4 nit + 6; 2 k u pays for gg's rounding too:
          d_m1 = 2 k u sum|gg| / c + 2 u |m1|.   m2 the same over fma(gg, xh, s2): a term carries 3 roundings and k >= 10 additions,
          within 2 k u: d_m2 = 2 k u sum|gg xh| / c + 2 u |m2|.
      o = fl(rs * fl(fl(gg - m1) - fl(xh * m2))):
          rs (u |gg| + d_m1 + |xh| d_m2 + 3 u |xh m2| + u |gg - m1| + u |gg - m1 - xh m2|) + u |dx|
          (gg's rounding; the two means; xh's two roundings and the product's; the two differences; the last product)."""
    dx, dgamma, dbeta, a_dgamma, a_dbeta = R.layernorm2d_bwd(g, x, gamma, mean, rstd)
    nit = _cdiv(c, 256)
    k = 4 * nit + 6
    xh = (x - mean[:, None]) * rstd[:, None]
    gg = g * gamma.double()[None, :, None, None]
    m1, m2 = gg.sum(1, keepdim=True) / c, (gg * xh).sum(1, keepdim=True) / c
    d_m1 = 2 * k * U32 * gg.abs().sum(1, keepdim=True) / c + 2 * U32 * m1.abs()
    d_m2 = 2 * k * U32 * (gg * xh).abs().sum(1, keepdim=True) / c + 2 * U32 * m2.abs()
    e = U32 * gg.abs() + d_m1 + xh.abs() * d_m2 + 3 * U32 * (xh * m2).abs() + U32 * (gg - m1).abs() + U32 * (gg - m1 - xh * m2).abs()
    return dx, rstd[:, None] * e + U32 * dx.abs(), dgamma, dbeta, a_dgamma, a_dbeta


def _ln_bwd_k(npix, c, cap=256):
    """dgamma / dbeta: a wave adds one term per pixel it visits (trips), the first wave adds the NT / 64 waves' sums in order, the f64
    rows are exact.  NT and the workgroup count as pssr_layernorm2d_bwd picks them; `cap` = LN_BWD_BLOCKS."""
    waves = (1024 if c <= 512 else 512 if c <= 1024 else 256) // 64
    blocks = max(1, min(_cdiv(npix, waves) // 4, cap))
    return _cdiv(npix, blocks * waves) + waves, blocks


# (shape, c_pad, s2d, LN_BWD_BLOCKS, forward only)
LN = [
    pytest.param((1, 8, 3, 5), 16, False, None, False, id="c8-NIT1-PP4-15px-tail-repeats-last-pixel"),
    pytest.param((1, 16, 3, 3), 16, False, None, False, id="c16-c_pad-equals-c"),
    pytest.param((1, 260, 3, 3), 272, False, None, False, id="c260-NIT2-PP2-odd-pixel-count-one-lane-in-second-slice"),
    pytest.param((1, 256, 2, 2), 272, False, None, False, id="c256-c_pad272-crosses-slice-fwd-NIT2-bwd-NIT1"),
    pytest.param((2, 516, 2, 4), 528, False, None, False, id="c516-NIT4-bwd-NT512"),
    pytest.param((1, 1028, 2, 2), 1040, False, None, False, id="c1028-NIT8"),
    pytest.param((1, 2048, 2, 2), 2048, False, None, False, id="c2048-NIT8-widest-c_pad-equals-c"),
    pytest.param((1, 8, 258, 256), 16, False, None, True, id="c8-66048px-fwd-4096-workgroup-cap-grid-stride"),
    pytest.param((1, 8, 48, 48), 16, False, None, False, id="c8-2304px-bwd-36-workgroups-stripes-wrap"),
    pytest.param((1, 8, 48, 48), 16, False, 1, False, id="c8-2304px-LN_BWD_BLOCKS-1-cap"),
    pytest.param((1, 8, 4, 6), 16, True, None, False, id="s2d-c8-NIT1-PP4"),
    pytest.param((1, 260, 2, 4), 272, True, None, False, id="s2d-c260-NIT2-PP2"),
    pytest.param((1, 256, 2, 2), 272, True, None, False, id="s2d-c256-c_pad272-crosses-slice"),
    pytest.param((2, 516, 2, 4), 528, True, None, False, id="s2d-c516-NIT4-bwd-NT512"),
    pytest.param((1, 1028, 2, 2), 1040, True, None, False, id="s2d-c1028-NIT8"),
    pytest.param((1, 8, 48, 48), 8, True, None, False, id="s2d-c8-c_pad-equals-c-bwd-36-workgroups"),
]


def _ln_layout(v, c_pad, s2d, fill):
    """NCHW f64 -> the layout the kernel writes / reads: [n, h, w, c_pad] or the space-to-depth one, `fill` in the pad channels."""
    if s2d:
        return R.s2d_fold(v, c_pad, fill)
    n, c, h, w = v.shape
    out = torch.full((n, h, w, c_pad), fill, dtype=v.dtype)
    out[..., :c] = _nhwc(v)
    return out


def _ln_inputs(shape, dt, g):
    n, c, h, w = shape
    x = _q(torch.randn(shape, generator=g) * 2 + 0.5, dt)
    gamma = 0.5 + torch.rand(c, generator=g)
    beta = torch.rand(c, generator=g) - 0.5
    return x, gamma, beta


def _ln_fwd(ops, x, gamma, beta, shape, c_pad, s2d, dt, stats=True):
    n, c, h, w = shape
    xin = _wide_px((n, h, w), c, dt, _nhwc(x))
    lead, cw = ((n, h // 2, w // 2), 4 * c_pad) if s2d else ((n, h, w), c_pad)
    out = _wide(lead, cw, dt)
    fm, mean = _guard(n * h * w)
    fr, rstd = _guard(n * h * w)
    ops.layernorm2d_fwd(xin, gamma.cuda(), beta.cuda(), EPS, out, n, h, w, c, ops.dtype_code(dt), in_coff=PAD, out_coff=PAD, s2d=s2d, c_pad=c_pad,
                        mean=mean if stats else None, rstd=rstd if stats else None)
    _guard_ok(fm, written=stats), _guard_ok(fr, written=stats)
    if not stats:
        assert torch.isnan(mean).all() and torch.isnan(rstd).all()
    return _wide_ok(out, cw), mean.cpu().view(n, h, w), rstd.cpu().view(n, h, w), xin


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,c_pad,s2d,cap,fwd_only", LN)
def test_layernorm2d(shape, c_pad, s2d, cap, fwd_only, dt):
    """Forward: out in the kernel's layout, so that a pixel in the wrong place or a non-zero pad channel fails with tolerance 0 there;
    mean and rstd; two runs give the same bits.  Backward from the reference's mean / rstd rounded to f32, g in the same layout with
    NaN in its pad channels, storing and accumulating; dgamma / dbeta from the folded statistic rows."""
    ops, _ = _mods()
    n, c, h, w = shape
    npix = n * h * w
    g = _gen(*shape, c_pad, s2d)
    x, gamma, beta = _ln_inputs(shape, dt, g)
    ref, mean, rstd, tol, d_mu, d_rs = _ln_fwd_bounds(x, gamma, beta, c)
    got, got_mean, got_rstd, xin = _ln_fwd(ops, x, gamma, beta, shape, c_pad, s2d, dt)
    ref_l, tol_l = _ln_layout(ref, c_pad, s2d, 0.0), _ln_layout(tol + _store(ref, dt), c_pad, s2d, 0.0)
    pad = _ln_layout(torch.zeros_like(ref), c_pad, s2d, 1.0) == 1.0
    assert (got[pad] == 0).all() and pad.sum() == npix * (c_pad - c)
    _assert_tol(got, ref_l, tol_l, "out")
    _assert_tol(got_mean, mean, d_mu, "mean")
    _assert_tol(got_rstd, rstd, d_rs, "rstd")
    again = _ln_fwd(ops, x, gamma, beta, shape, c_pad, s2d, dt)
    assert torch.equal(got, again[0]) and torch.equal(got_mean, again[1]) and torch.equal(got_rstd, again[2])
    if fwd_only:
        return
    gr = _q(torch.randn(shape, generator=g), dt)
    prev = _q(torch.randn(shape, generator=g), dt)
    mean32, rstd32 = mean.float(), rstd.float()
    lead, cw = ((n, h // 2, w // 2), 4 * c_pad) if s2d else ((n, h, w), c_pad)
    gin = _wide_px(lead, cw, dt, _ln_layout(gr, c_pad, s2d, NAN))
    dx_ref, dx_tol, dgamma, dbeta, a_dgamma, a_dbeta = _ln_bwd_bounds(gr, x, gamma, mean32, rstd32, c)
    k, blocks = _ln_bwd_k(npix, c, 256 if cap is None else cap)
    with _option(b"LN_BWD_BLOCKS", cap):
        for acc in (False, True):
            dx = _wide((n, h, w), c, dt, _nhwc(prev) if acc else None)
            fs, stats = _stats_buf(2 * c)
            ops.layernorm2d_bwd(gin, xin, gamma.cuda(), mean32.cuda().view(-1), rstd32.cuda().view(-1), dx, stats, n, h, w, c, ops.dtype_code(dt),
                                g_coff=PAD, x_coff=PAD, dx_coff=PAD, s2d=s2d, c_pad=c_pad, accumulate=acc)
            _guard_ok(fs)
            total = dx_ref + prev if acc else dx_ref
            t = dx_tol + U32 * total.abs() if acc else dx_tol
            _assert_tol(_nchw(_wide_ok(dx, c)), total, t + _store(total, dt), f"dx accumulate={acc}")
            sums = _fold(stats, 2 * c)
            _assert_sum(sums[:c], dgamma, a_dgamma, k, f"dgamma ({blocks} workgroups)")
            _assert_sum(sums[c:], dbeta, a_dbeta, k, "dbeta")
            rows = stats.view(E.ROWS, 2 * c).cpu()
            used = torch.tensor([s < blocks for s in range(E.STRIPES)])
            assert (rows[:E.STRIPES][~used] == 0).all() and (rows[:E.STRIPES][used].abs().sum(1) > 0).all()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,c_pad,s2d", [pytest.param((1, 8, 3, 5), 16, False, id="mean-rstd-null-c8-plain"), pytest.param((1, 260, 2, 4), 272, True, id="mean-rstd-null-c260-s2d")])
def test_layernorm2d_fwd_without_mean_rstd(shape, c_pad, s2d, dt):
    """mean = rstd = NULL (inference): the same bits in `out` as with them, nothing written to the buffers that were not passed."""
    ops, _ = _mods()
    x, gamma, beta = _ln_inputs(shape, dt, _gen(*shape, 9))
    with_stats = _ln_fwd(ops, x, gamma, beta, shape, c_pad, s2d, dt)
    without = _ln_fwd(ops, x, gamma, beta, shape, c_pad, s2d, dt, stats=False)
    assert torch.equal(with_stats[0], without[0])
    ref, _, _, tol, _, _ = _ln_fwd_bounds(x, gamma, beta, shape[1])
    _assert_tol(without[0], _ln_layout(ref, c_pad, s2d, 0.0), _ln_layout(tol + _store(ref, dt), c_pad, s2d, 0.0), "out")


# ---- image_channel_dot ---------------------------------------------------------------------------------------------------------
# A thread of the 128 pixel lanes takes ceil(hw / 128) FMAs (four per trip of the 4-pixels-in-flight loop while p + 384 < hw, then one
# per trip), the LDS tree has 7 levels, and out += sum * scale is one more addition: k = ceil(hw / 128) + 7 + 1.  The rounding of
# sum * scale is inside the factor 2.
ICD = [
    pytest.param(35, 4, id="hw35-c4-below-32-channels-below-one-trip"),
    pytest.param(512, 36, id="hw512-c36-one-full-4-pixel-trip-second-workgroup-one-lane"),
    pytest.param(513, 4, id="hw513-c4-4-pixel-trip-then-tail"),
    pytest.param(900, 36, id="hw900-c36-two-4-pixel-trips-4-lanes-in-the-second"),
]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("with_b", [pytest.param(True, id="a*b"), pytest.param(False, id="a-alone")])
@pytest.mark.parametrize("hw,c", ICD)
def test_image_channel_dot(hw, c, with_b, dt):
    """Two images; a spare NaN pixel follows the last one, so a read past an image's end poisons the sum or meets the wrong image."""
    ops, _ = _mods()
    n = 2
    g = _gen(hw, c, with_b)
    a = _q(torch.randn(n, hw, c, generator=g), dt)
    b = _q(torch.randn(n, hw, c, generator=g), dt) if with_b else None
    prev = torch.randn(n, c, generator=g)
    scale = _f32(0.37 if with_b else 1.0 / hw)

    def wide(v):
        buf = torch.full((n * hw + 1, c + 2 * PAD), NAN, dtype=dt, device="cuda")
        buf[:n * hw, PAD:PAD + c] = v.reshape(n * hw, c).to(dt).cuda()
        return buf
    ain, bin_ = wide(a), wide(b) if with_b else None
    runs = []
    for _ in range(2):
        flat, out = _guard(n * c, value=prev)
        ops.image_channel_dot(ain, bin_, n, hw, c, scale, out, ops.dtype_code(dt), a_coff=PAD, b_coff=PAD)
        _guard_ok(flat)
        runs.append(out.cpu().view(n, c))
    assert torch.equal(runs[0], runs[1])
    ref, mag = R.image_channel_dot(a, b, scale)
    _assert_sum(runs[0], ref + prev.double(), mag + prev.double().abs(), _cdiv(hw, 128) + 7 + 1, "out")


# ---- ese_gate ------------------------------------------------------------------------------------------------------------------
# One wave per output: a lane takes ceil(c / 64) FMAs, 6 shuffle levels, + b: k = ceil(c / 64) + 6 + 1.
ESE_GATE = [pytest.param(3, 5, id="n3-c5-below-one-wave-15-outputs-last-workgroup-partial"), pytest.param(2, 68, id="n2-c68-lane-loop-second-trip"),
            pytest.param(3, 328, id="n3-c328-six-trips")]


def _u_k(c):
    return _cdiv(c, 64) + 6 + 1


@pytest.mark.parametrize("n,c", ESE_GATE)
def test_ese_gate(n, c):
    """u within its sum bound; gate = min(max(u + 3, 0), 6) * fl(1 / 6) within that bound / 6 plus 2 f32 ulp (the sum, the constant, the
    product).  Two runs give the same bits."""
    ops, _ = _mods()
    g = _gen(n, c, 5)
    s, w, b = torch.randn(n, c, generator=g), torch.randn(c, c, generator=g) * 3 / c ** 0.5, torch.randn(c, generator=g) * 2
    (_, sd), (_, wd), (_, bd) = _guard(n * c, value=s), _guard(c * c, value=w), _guard(c, value=b)
    runs = []
    for _ in range(2):
        fu, u = _guard(n * c)
        fg, gate = _guard(n * c)
        ops.ese_gate(sd.view(n, c), wd, bd, u, gate)
        _guard_ok(fu), _guard_ok(fg)
        runs.append((u.cpu().view(n, c), gate.cpu().view(n, c)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    u_ref, gate_ref, mag = R.ese_gate(s, w, b)
    assert (u_ref < -3).any() and (u_ref > 3).any() and (u_ref.abs() < 3).any()
    tol_u = _sum_tol(_u_k(c), mag)
    _assert_tol(runs[0][0], u_ref, tol_u, "u")
    _assert_tol(runs[0][1], gate_ref, tol_u / 6 + 2 * _ulp(gate_ref, F32), "gate")


# ---- scale_nc ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("with_gate", [pytest.param(True, id="gate"), pytest.param(False, id="no-gate")])
@pytest.mark.parametrize("with_add", [pytest.param(True, id="add"), pytest.param(False, id="no-add")])
@pytest.mark.parametrize("hw", [pytest.param(1, id="hw1"), pytest.param(35, id="hw35")])
def test_scale_nc(hw, with_add, with_gate, dt):
    """fma(t, fl(gate * gamma), add): the product's rounding acts on |t gate gamma|, the FMA's on |out|; then the store."""
    ops, _ = _mods()
    n, c = 3, 12
    g = _gen(hw, with_add, with_gate)
    t = _q(torch.randn(n, hw, c, generator=g), dt)
    gate, gamma, add = torch.rand(n, c, generator=g), 0.5 + torch.rand(c, generator=g), torch.randn(n, c, generator=g)
    tin = _wide((n * hw,), c, dt, t.reshape(n * hw, c))
    out = _wide((n * hw,), c, dt)
    (_, gd), (_, gmd), (_, ad) = _guard(n * c, value=gate), _guard(c, value=gamma), _guard(n * c, value=add)
    ops.scale_nc(tin, gd if with_gate else None, gmd, ad if with_add else None, out, n, hw, c, ops.dtype_code(dt), t_coff=PAD, out_coff=PAD)
    got = _wide_ok(out, c).view(n, hw, c)
    ref = R.scale_nc(t, gate if with_gate else None, gamma, add if with_add else None)
    prod = R.scale_nc(t, gate if with_gate else None, gamma, None).abs()
    _assert_tol(got, ref, U32 * prod + U32 * ref.abs() + _store(ref, dt), "out")
    again = _wide((n * hw,), c, dt)
    ops.scale_nc(tin, gd if with_gate else None, gmd, ad if with_add else None, again, n, hw, c, ops.dtype_code(dt), t_coff=PAD, out_coff=PAD)
    assert torch.equal(_wide_ok(again, c).view(n, hw, c), got)


# ---- ese_bwd -------------------------------------------------------------------------------------------------------------------
def _ese_inputs(n, c, g):
    """s, W, b with u = b + W s clear of +-3: b takes one of four levels (two outside, two inside (-3, 3)) plus a quarter of noise and
    W s has a standard deviation of 0.15, so every region is populated and no |u| comes near 3.  Returns f32 tensors and the reference
    (u, gate, bound of u)."""
    s = torch.randn(n, c, generator=g)
    w = torch.randn(c, c, generator=g) * 0.15 / c ** 0.5
    levels = torch.tensor([-4.5, -1.25, 0.75, 4.25])
    b = levels[torch.arange(c) % 4] + 0.25 * torch.rand(c, generator=g)
    u, gate, mag = R.ese_gate(s, w, b)
    return s, w, b, u, gate, _sum_tol(_u_k(c), mag)


# k per output and path.  du = fl(fl(A gamma) * fl(1 / 6)): 3 u |du|, which every sum of du terms carries on top (`extra`).
#   fused (c <= 2048): dgamma, db_fc: 4 image groups of ceil(n / 4) additions, then (r0 + r1) + (r2 + r3): ceil(n / 4) + 2.
#                      dW_fc cached (n * rows <= 2048): two accumulators of ceil(n / 2), then a0 + a1: ceil(n / 2) + 1; uncached: n.
#                      add: 4 thread groups x 4 accumulators of at most ceil(c / 16) + 3 FMAs, (a0 + a1) + (a2 + a3), the same over the
#                      groups, then * fl(1 / hw) with its two roundings: ceil(c / 16) + 3 + 2 + 2 + 2.
#   staged (c > 2048): one thread per output, plain loops: n for dgamma, db_fc, dW_fc; c + 2 for add.
ESE_BWD = [
    pytest.param(3, 4, "fused", id="n3-c4-fused-c-below-64"),
    pytest.param(3, 68, "fused", id="n3-c68-fused-second-channel-chunk"),
    pytest.param(2, 328, "fused", id="n2-c328-fused"),
    pytest.param(516, 4, "uncached", id="n516-c4-fused-uncached-dW-role"),
    pytest.param(2, 2052, "staged", id="n2-c2052-staged-fallback"),
]


@pytest.mark.parametrize("n,c,path", ESE_BWD)
def test_ese_bwd_gate(n, c, path):
    ops, _ = _mods()
    hw = 35
    g = _gen(n, c, 6)
    s, w, b, u_ref, gate_ref, u_tol = _ese_inputs(n, c, g)
    # the indicator |u| < 3 must not depend on rounding: every u is 100 bounds away from +-3, and all three regions occur
    assert ((u_ref.abs() - 3).abs() > 100 * u_tol).all()
    assert (u_ref < -3).any() and (u_ref > 3).any() and (u_ref.abs() < 3).any()
    u, gate = u_ref.float(), gate_ref.float()
    A, gamma = torch.randn(n, c, generator=g) * 3, 0.5 + torch.rand(c, generator=g)
    ins = {k: _guard(v.numel(), value=v)[1] for k, v in dict(A=A, gate=gate, u=u, gamma=gamma, s=s, w=w).items()}
    outs = {k: _guard(m) for k, m in dict(du=n * c, dgamma=c, db_fc=c, dW_fc=c * c, add=n * c).items()}
    ops.ese_bwd(ins["A"].view(n, c), ins["gate"], ins["u"], ins["gamma"], ins["s"], ins["w"], hw, *(outs[k][1] for k in ("du", "dgamma", "db_fc", "dW_fc", "add")))
    for k in outs:
        _guard_ok(outs[k][0])
    r = R.ese_bwd(A, gamma, hw, gate, u, s, w)
    assert (r["du"] == 0).any() and (r["du"] != 0).any()
    _assert_tol(outs["du"][1].view(n, c), r["du"], 3 * U32 * r["du"].abs(), "du")
    fused = path != "staged"
    ks = {"dgamma": _cdiv(n, 4) + 2 if fused else n, "db_fc": _cdiv(n, 4) + 2 if fused else n,
          "dW_fc": _cdiv(n, 2) + 1 if path == "fused" else n, "add": _cdiv(c, 16) + 9 if fused else c + 2}
    for k, shape in (("dgamma", (c,)), ("db_fc", (c,)), ("dW_fc", (c, c)), ("add", (n, c))):
        extra = 0.0 if k == "dgamma" else 3 * U32 * r[k + "_abs"]
        _assert_tol(outs[k][1].view(shape), r[k], _sum_tol(ks[k], r[k + "_abs"], extra), f"{k} k={ks[k]}")


def test_ese_bwd_no_gate():
    """Plain layer scale, (n, c) = (3, 24): dgamma = sum_n A by one thread per channel, k = n; no other output is touched."""
    ops, _ = _mods()
    n, c = 3, 24
    g = _gen(n, c, 7)
    A, gamma = torch.randn(n, c, generator=g), 0.5 + torch.rand(c, generator=g)
    (_, Ad), (_, gd) = _guard(n * c, value=A), _guard(c, value=gamma)
    flat, dgamma = _guard(c)
    ops.ese_bwd(Ad.view(n, c), None, None, gd, None, None, 35, None, dgamma, None, None, None)
    _guard_ok(flat)
    r = R.ese_bwd(A, gamma, 35)
    _assert_sum(dgamma, r["dgamma"], r["dgamma_abs"], n, "dgamma")


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _refused(L, rc, name, *untouched):
    assert rc == -1, (name, rc)
    msg = L.lib().pssr_last_error().decode()
    assert name in msg, (name, msg)
    torch.cuda.synchronize()
    for t in untouched:
        assert torch.isnan(t).all(), name


def test_refusals_dwconv7():
    ops, L = _mods()
    lib, st = L.lib(), L.stream_ptr()
    lib.pssr_dwconv7_wgrad_workspace_bytes.restype = C.c_int64
    n, h, w, c = 1, 4, 8, 8
    x = torch.zeros(n, h, w, 16, device="cuda")
    wp, out, dw = torch.zeros(49, 8, device="cuda"), torch.full((n, h, w, 16), NAN, device="cuda"), torch.full((8, 49), NAN, device="cuda")
    _refused(L, lib.pssr_dwconv7(L.ptr(x), 16, 0, L.ptr(wp), None, L.ptr(out), 16, 0, n, h, w, 6, 0, L.F32, st), "dwconv7", out)
    _refused(L, lib.pssr_dwconv7(L.ptr(x), 16, 12, L.ptr(wp), None, L.ptr(out), 16, 0, n, h, w, c, 0, L.F32, st), "dwconv7 in", out)
    _refused(L, lib.pssr_dwconv7(L.ptr(x), 16, 0, L.ptr(wp), None, L.ptr(out), 16, 12, n, h, w, c, 0, L.F32, st), "dwconv7 out", out)
    _refused(L, lib.pssr_dwconv7(L.ptr(x), 16, 0, L.ptr(wp), None, L.ptr(out), 16, 0, n, h, w, c, 0, 7, st), "bad dtype", out)
    _refused(L, lib.pssr_dwconv7_wgrad(L.ptr(x), 16, 0, L.ptr(x), 16, 0, L.ptr(dw), n, h, w, 6, L.F32, st), "dwconv7_wgrad", dw)
    _refused(L, lib.pssr_dwconv7_wgrad(L.ptr(x), 16, 12, L.ptr(x), 16, 0, L.ptr(dw), n, h, w, c, L.F32, st), "dwconv7_wgrad dy", dw)
    _refused(L, lib.pssr_dwconv7_wgrad(L.ptr(x), 16, 0, L.ptr(x), 16, 12, L.ptr(dw), n, h, w, c, L.F32, st), "dwconv7_wgrad x", dw)
    need = lib.pssr_dwconv7_wgrad_workspace_bytes(n, h, w, c)
    assert need > 0 and lib.pssr_dwconv7_wgrad_workspace_bytes(n, h, 9, c) == 0 and lib.pssr_dwconv7_wgrad_workspace_bytes(n, h, w, 6) == 0
    ws = torch.full((need // 4,), NAN, device="cuda")
    args = (L.ptr(x), 16, 0, L.ptr(x), 16, 0, L.ptr(dw), n, h)
    _refused(L, lib.pssr_dwconv7_wgrad_ws(*args, w, c, L.F32, L.ptr(ws), C.c_int64(need - 1), st), "dwconv7_wgrad_ws", dw, ws)
    _refused(L, lib.pssr_dwconv7_wgrad_ws(*args, 9, c, L.F32, L.ptr(ws), C.c_int64(need), st), "dwconv7_wgrad_ws", dw, ws)
    _refused(L, lib.pssr_dwconv7_wgrad_ws(*args, w, 6, L.F32, L.ptr(ws), C.c_int64(need), st), "dwconv7_wgrad_ws", dw, ws)
    _refused(L, lib.pssr_dwconv7_wgrad_ws(*args, w, c, L.F32, None, C.c_int64(need), st), "dwconv7_wgrad_ws", dw, ws)


def test_refusals_pack_and_patchify():
    ops, L = _mods()
    lib, st = L.lib(), L.stream_ptr()
    w = torch.zeros(8, 1, 7, 7, device="cuda")
    out = torch.full((49, 8), NAN, device="cuda")
    b = L.DwPackBatch()
    for i in range(L.DWPACK_BATCH_MAX):
        b.w[i], b.packed[i], b.c[i], b.flip[i] = w.data_ptr(), out.data_ptr(), 8, 0
    _refused(L, lib.pssr_dwconv7_pack_batch(C.byref(b), 0, st), "dwconv7_pack_batch", out)
    _refused(L, lib.pssr_dwconv7_pack_batch(C.byref(b), L.DWPACK_BATCH_MAX + 1, st), "dwconv7_pack_batch", out)
    b.c[3] = 0
    _refused(L, lib.pssr_dwconv7_pack_batch(C.byref(b), 5, st), "dwconv7_pack_batch: item 3", out)
    _refused(L, lib.pssr_dwconv7_pack(L.ptr(w), L.ptr(out), 0, 0, st), "dwconv7_pack", out)
    x = torch.zeros(1, 3, 4, 4, device="cuda")
    sc = torch.ones(3, device="cuda")
    xp = torch.full((1, 2, 2, 16), NAN, device="cuda")
    f = C.c_float
    _refused(L, lib.pssr_input_patchify(L.ptr(x), L.ptr(xp), 1, 3, 4, 4, 2, 12, f(1), f(0), L.ptr(sc), L.ptr(sc), L.F32, st), "input_patchify", xp)
    _refused(L, lib.pssr_input_patchify(L.ptr(x), L.ptr(xp), 1, 3, 4, 4, 3, 32, f(1), f(0), L.ptr(sc), L.ptr(sc), L.F32, st), "input_patchify", xp)


def test_refusals_layernorm2d():
    ops, L = _mods()
    lib, st = L.lib(), L.stream_ptr()
    n, h, w, c = 1, 2, 4, 8
    x = torch.zeros(n, h, w, 16, device="cuda")
    gm = torch.ones(2052, device="cuda")
    out = torch.full((n, h, w, 64), NAN, device="cuda")
    mean, rstd = torch.full((n * h * w,), NAN, device="cuda"), torch.full((n * h * w,), NAN, device="cuda")
    eps = C.c_float(1e-6)

    def fwd(in_cs=16, in_co=0, out_cs=64, out_co=0, s2d=0, c_pad=16, hh=h, cc=c, m=mean, r=rstd):
        return lib.pssr_layernorm2d_fwd(L.ptr(x), in_cs, in_co, L.ptr(gm), L.ptr(gm), eps, L.ptr(out), out_cs, out_co, s2d, c_pad, n, hh, w, cc,
                                        L.ptr(m), L.ptr(r), L.F32, st)
    keep = (out, mean, rstd)
    _refused(L, fwd(cc=2052, in_cs=2052, c_pad=2064, out_cs=2064), "layernorm2d_fwd", *keep)
    _refused(L, fwd(cc=6), "layernorm2d_fwd", *keep)
    _refused(L, fwd(s2d=1, hh=1), "layernorm2d_fwd: c_pad / s2d", *keep)
    _refused(L, fwd(c_pad=4), "layernorm2d_fwd: c_pad / s2d", *keep)
    _refused(L, fwd(m=None), "layernorm2d_fwd: mean/rstd", *keep)
    _refused(L, fwd(r=None), "layernorm2d_fwd: mean/rstd", *keep)
    _refused(L, fwd(in_co=12), "layernorm2d_fwd in", *keep)
    _refused(L, fwd(out_cs=16, out_co=4), "layernorm2d_fwd out", *keep)
    _refused(L, fwd(s2d=1, out_cs=48), "layernorm2d_fwd out", *keep)                  # s2d needs 4 * c_pad channels
    stats = torch.full((64 * 2 * c,), NAN, dtype=F64, device="cuda")
    dx = torch.full((n, h, w, 16), NAN, device="cuda")
    zm = torch.zeros(n * h * w, device="cuda")

    def bwd(g_cs=64, g_co=0, s2d=0, c_pad=16, x_co=0, dx_co=0, hh=h, cc=c):
        return lib.pssr_layernorm2d_bwd(L.ptr(out), g_cs, g_co, s2d, c_pad, L.ptr(x), 16, x_co, L.ptr(gm), L.ptr(zm), L.ptr(zm), L.ptr(dx), 16, dx_co, 0,
                                        n, hh, w, cc, L.ptr(stats), L.F32, st)
    keep = (dx, stats)
    _refused(L, bwd(cc=2052), "layernorm2d_bwd", *keep)
    _refused(L, bwd(s2d=1, hh=1), "layernorm2d_bwd: c_pad / s2d", *keep)
    _refused(L, bwd(c_pad=4), "layernorm2d_bwd: c_pad / s2d", *keep)
    _refused(L, bwd(s2d=1, g_cs=48), "layernorm2d_bwd g", *keep)
    _refused(L, bwd(x_co=12), "layernorm2d_bwd x", *keep)
    _refused(L, bwd(dx_co=12), "layernorm2d_bwd dx", *keep)


def test_refusals_ese():
    ops, L = _mods()
    lib, st = L.lib(), L.stream_ptr()
    n, hw, c = 2, 4, 8
    t = torch.zeros(n * hw, 16, device="cuda")
    v = torch.zeros(c * c, device="cuda")
    out = torch.full((n * hw, 16), NAN, device="cuda")
    nc = torch.full((n * c,), NAN, device="cuda")
    f = C.c_float
    _refused(L, lib.pssr_image_channel_dot(L.ptr(t), 16, 0, None, 0, 0, n, hw, 6, f(1), L.ptr(nc), L.F32, st), "image_channel_dot", nc)
    _refused(L, lib.pssr_image_channel_dot(L.ptr(t), 16, 12, None, 0, 0, n, hw, c, f(1), L.ptr(nc), L.F32, st), "image_channel_dot a", nc)
    _refused(L, lib.pssr_image_channel_dot(L.ptr(t), 16, 0, L.ptr(t), 16, 12, n, hw, c, f(1), L.ptr(nc), L.F32, st), "image_channel_dot b", nc)
    _refused(L, lib.pssr_ese_gate(L.ptr(v), L.ptr(v), L.ptr(v), 0, c, L.ptr(nc), L.ptr(nc), st), "ese_gate", nc)
    _refused(L, lib.pssr_scale_nc(L.ptr(t), 16, 0, None, L.ptr(v), None, L.ptr(out), 16, 0, n, hw, 6, L.F32, st), "scale_nc", out)
    _refused(L, lib.pssr_scale_nc(L.ptr(t), 16, 12, None, L.ptr(v), None, L.ptr(out), 16, 0, n, hw, c, L.F32, st), "scale_nc t", out)
    _refused(L, lib.pssr_scale_nc(L.ptr(t), 16, 0, None, L.ptr(v), None, L.ptr(out), 16, 12, n, hw, c, L.F32, st), "scale_nc out", out)
    _refused(L, lib.pssr_ese_bwd(L.ptr(v), None, None, L.ptr(v), None, None, n, c, 0, None, L.ptr(nc), None, None, None, st), "ese_bwd", nc)
    _refused(L, lib.pssr_ese_bwd(L.ptr(v), L.ptr(v), None, L.ptr(v), L.ptr(v), L.ptr(v), n, c, hw, L.ptr(nc), L.ptr(nc), L.ptr(nc), L.ptr(nc), L.ptr(nc), st),
             "ese_bwd: gate path", nc)
