"""Bit-exact tests of the implicit-GEMM convolutions on every tiling the default dispatch takes.

Operands are dyadic with few significant bits (tests/_conv_exact.py): every kernel's f32 accumulator holds the exact result whatever
its summation order, so a 16-bit store must equal the float64 reference rounded once to nearest even, and an f32 result must equal
it outright.  Outputs are compared with torch.equal, and every case first asserts which kernels production dispatch launched for it
(conv_igemm_impl.h: launch_bn / launch_geo / launch / use_v3 at the table defaults of the tunables)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from _conv_exact import (B_GRID, SCALE_GRID, SHIFT_GRID, X_GRID, W_GRID, Grid, assert_equal, assert_exact_premise, assert_guards, dev,
                         dyadic, expected, from_blocked, launched_kernels, nchw, nhwc, per_channel, production_tunables, shuf2_perm,
                         tunables)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("production_tunables")]
_ = production_tunables      # (the fixture is used through the mark above)

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DT16 = (BF16, F16)
RELU, STATS, AFFINE, SHUF2, SOLO = 1, 2, 4, 16, 32     # PSSR_FLAG_*

IG, V3, FLAT, FIN = "conv_igemm_kernel", "conv_v3_kernel", "conv_flat_kernel", "conv_splitk_finish_kernel"

# id: ((n, cin, cout, h, w, ks), flags, kernels production launches, 16-bit only)
ROWS = {
    "v3_128": ((6, 16, 128, 120, 120, 3), 0, [(V3, (128,))], True),              # 8 * 8 * 6 = 384 workgroups, partial tiles
    "v3_64": ((12, 16, 48, 128, 120, 3), 0, [(V3, (64,))], True),                # 4 * 8 * 12 = 384, ragged channel tile
    "v3_64s": ((12, 16, 64, 128, 120, 3), 0, [(V3, (64,))], True),               # the same tiles, cout % 32 == 0 (FLAG_SHUF2)
    "n64_192": ((12, 32, 256, 32, 32, 3), SOLO, [(IG, (64, 0, 9))], True),       # 128 x 128 tiles: 192 workgroups -> 128 x 64
    "n64_216": ((12, 32, 256, 24, 40, 3), SOLO, [(IG, (64, 0, 9))], True),       # 216, partial tiles
    "n128_192": ((12, 32, 256, 32, 32, 3), 0, [(IG, (128, 0, 9))], True),        # the same launches without FLAG_SOLO
    "n128_216": ((12, 32, 256, 24, 40, 3), 0, [(IG, (128, 0, 9))], True),
    "big_64": ((2, 32, 64, 16, 48, 3), 0, [(IG, (64, 5, 9))], True),             # 256 x 64 tiles (IGEMM_BIG)
    "flat_kc4": ((2, 64, 96, 12, 20, 1), 0, [(FLAT, (128, 0, 4))], False),       # 1x1, 4-chunk stages
    "flat_kc9": ((2, 144, 48, 12, 20, 1), 0, [(FLAT, (64, 0, 9))], False),       # 1x1, 9-chunk stages
    "splitk_9tap": ((2, 256, 128, 16, 16, 3), 0, [(IG, (128, 0, 9)), (FIN, (128, 0))], False),
    "splitk_1x1": ((1, 1040, 64, 16, 16, 1), 0, [(FLAT, (64, 0, 9)), (FIN, (64, 0))], False),
}
for _geo, (_n, _hw) in enumerate([(2, 12), (3, 8), (9, 4), (33, 2), (130, 1)]):        # GEO 0-4: tiles of 1, 2, 8, 32, 128 images
    for _bn, _cout in [(128, 96), (64, 48), (32, 24)]:
        ROWS[f"geo{_geo}_bn{_bn}"] = ((_n, 32, _cout, _hw, _hw, 3), 0, [(IG, (_bn, _geo, 9))], False)


def _params(ids, dts=(BF16, F16, F32)):
    return [pytest.param(r, dt, id=f"{r}-{str(dt)[6:]}") for r in ids for dt in dts if dt != F32 or not ROWS[r][3]]


def _seed(*key):
    return abs(hash(key)) % (1 << 31)


@functools.lru_cache(maxsize=32)
def operands(shape):
    """exact operands of one forward case and their float64 accumulator (no bias), shared by every dtype and epilogue"""
    n, cin, cout, h, w, ks = shape
    g = torch.Generator().manual_seed(_seed(*shape))
    x = dyadic(g, (n, cin, h, w), X_GRID)
    wt = dyadic(g, (cout, cin, ks, ks), W_GRID)
    b = dyadic(g, (cout,), B_GRID)
    return x, wt, b, F.conv2d(x, wt, padding=ks // 2)


def conv(dt, x, wt, *, bias=None, flags=0, out_coff=8, blk=0, pro=None, x1=None, w1=None, tail=None, affine=None, stats=False,
         shuf=False, mode=0, mask=None):
    """One pssr_conv2d launch on NHWC copies of the float64 operands, input at channel offset 16 of a wider buffer, output at
    `out_coff` of a buffer with guard channels on both sides (FLAG_SHUF2: the [n, 2h, 2w, cout / 4 + 16] buffer, offset 8).
    Returns (output buffer, kernels launched, striped statistics).  tail = (aux, scale, shift): EPI_TAIL; affine = (scale, shift):
    FLAG_AFFINE; mask = (aux, scale, shift, mean, invstd): EPI_DGRAD_MASK; mode 1: `wt` is the layer weight of a data gradient."""
    from pssr2_amd import ops, _lib as L
    code = ops.dtype_code(dt)
    n, cin, h, w = x.shape
    cout = wt.shape[1] if mode == 1 else wt.shape[0]
    kw = dict(n=n, h=h, w=w, in0_coff=16, flags=flags, in0_blk=blk, out_blk=blk, aux_blk=blk)
    xd = nhwc(x, dt, coff=16, cstride=cin + 32, blk=blk)
    pw = ops.pack_conv_weight(dev(wt), code, mode=mode)
    if bias is not None:
        kw["bias"] = dev(bias)
    if pro is not None:
        kw.update(pro_scale=dev(pro[0]), pro_shift=dev(pro[1]))
    if x1 is not None:
        kw.update(x1=nhwc(x1, dt), cin1=x1.shape[1], w1=ops.pack_conv_weight(dev(w1), code))
    aux = tail if tail is not None else mask
    if aux is not None:
        kw.update(epilogue=L.EPI_TAIL if tail is not None else L.EPI_DGRAD_MASK, aux=nhwc(aux[0], dt, coff=8, cstride=cout + 16, blk=blk),
                  aux_coff=8, aux_scale=dev(aux[1]), aux_shift=dev(aux[2]))
    if mask is not None:
        kw.update(aux_mean=dev(mask[3]), aux_invstd=dev(mask[4]))
    if affine is not None:
        kw.update(flags=kw["flags"] | AFFINE, aux_scale=dev(affine[0]), aux_shift=dev(affine[1]))
    st = None
    if stats:
        st = torch.zeros(ops.STAT_STRIPES, 2 * cout, dtype=torch.float64, device="cuda")
        kw.update(stats=st, flags=kw["flags"] | STATS)
    if shuf:
        out = torch.full((n, 2 * h, 2 * w, cout // 4 + 16), -7.0, dtype=dt, device="cuda")
    else:
        out = torch.full((n, h, w, out_coff + cout + 8), -7.0, dtype=dt, device="cuda")
    _, ks = launched_kernels(lambda: ops.conv2d(xd, cin, pw, out, cout, out_coff=out_coff, **kw))
    return out, ks, st


def result(out, coff, c, blk=0):
    """the NHWC output window of a conv() buffer in plain pixel order, after checking its guard channels"""
    assert_guards(out, coff, c)
    return from_blocked(out.cpu(), blk)[..., coff:coff + c]


def nhwc_ref(ref, dt):
    return expected(ref, dt).permute(0, 2, 3, 1)


def assert_stats(st, c, s1, s2):
    """striped f32 partial sums against float64 sums of the stored values (the bound of tests/test_gpu_conv.py)"""
    s = st.sum(0).cpu()
    torch.testing.assert_close(s[:c], s1, rtol=1e-6, atol=1e-4)
    torch.testing.assert_close(s[c:], s2, rtol=1e-6, atol=1e-4)


# ---------------------------------------------------------------------------------------------------------------------
# a. forward dispatch table
@pytest.mark.parametrize("row,dt", _params(ROWS))
def test_forward_dispatch_store_bias_relu(row, dt):
    """each row launches the kernels its comment names; the store + bias (+ FLAG_RELU) is bit-exact, the 8-channel epilogue (aligned
    output) and the generic one (out_coff % 8 != 0) alike"""
    shape, flags, kernels, _ = ROWS[row]
    n, cin, cout, h, w, ks = shape
    assert_exact_premise(cin * ks * ks, dt=dt, bias=B_GRID)
    x, wt, b, acc = operands(shape)
    ref = acc + nchw(b)
    out, launched, _ = conv(dt, x, wt, bias=b, flags=flags)
    assert launched == sorted(kernels), f"{row}: launched {launched}"
    assert_equal(result(out, 8, cout), nhwc_ref(ref, dt), f"{row} store")
    want = nhwc_ref(ref.clamp_min(0), dt)
    out, launched, _ = conv(dt, x, wt, bias=b, flags=flags | RELU)
    assert launched == sorted(kernels)
    assert_equal(result(out, 8, cout), want, f"{row} store + relu")
    if dt != F32:
        out, _, _ = conv(dt, x, wt, bias=b, flags=flags | RELU, out_coff=4)
        assert_equal(result(out, 4, cout), want, f"{row} generic epilogue")


# ---------------------------------------------------------------------------------------------------------------------
# b. epilogues on the paths production uses them on
@pytest.mark.parametrize("row,dt", _params(["v3_128", "geo0_bn128", "n64_192", "n64_216", "splitk_9tap"]))
def test_forward_bn_prologue_and_stats(row, dt):
    """training forward: BatchNorm + ReLU of the producing layer in the loader, FLAG_STATS in the epilogue"""
    shape, flags, kernels, _ = ROWS[row]
    n, cin, cout, h, w, ks = shape
    assert_exact_premise(cin * ks * ks, dt=dt, pro=(SCALE_GRID, SHIFT_GRID), bias=B_GRID)
    x, wt, b, _ = operands(shape)
    scale, shift, _, _ = per_channel(row, cin)
    ref = F.conv2d((x * nchw(scale) + nchw(shift)).clamp_min(0), wt, b, padding=ks // 2)
    out, launched, st = conv(dt, x, wt, bias=b, flags=flags, pro=(scale, shift), stats=True)
    assert launched == sorted(kernels), f"{row}: launched {launched}"
    got = result(out, 8, cout)
    assert_equal(got, nhwc_ref(ref, dt), f"{row} prologue")
    g = got.double()
    assert_stats(st, cout, g.sum((0, 1, 2)), (g * g).sum((0, 1, 2)))


EVAL_ROWS = ["v3_128", "v3_64s", "n64_192", "n64_216", "big_64"]


@pytest.mark.parametrize("row,dt", _params(EVAL_ROWS, DT16))
def test_forward_affine_relu(row, dt):
    """eval forward: BatchNorm folded into the producing convolution's epilogue (FLAG_AFFINE | FLAG_RELU)"""
    shape, flags, kernels, _ = ROWS[row]
    n, cin, cout, h, w, ks = shape
    assert_exact_premise(cin * ks * ks, dt=dt, bias=B_GRID, affine=(SCALE_GRID, SHIFT_GRID))
    x, wt, b, acc = operands(shape)
    scale, shift, _, _ = per_channel(row + "affine", cout)
    ref = ((acc + nchw(b)) * nchw(scale) + nchw(shift)).clamp_min(0)
    out, launched, _ = conv(dt, x, wt, bias=b, flags=flags | RELU, affine=(scale, shift))
    assert launched == sorted(kernels), f"{row}: launched {launched}"
    assert_equal(result(out, 8, cout), nhwc_ref(ref, dt), f"{row} affine")


@pytest.mark.parametrize("row,dt", _params(EVAL_ROWS, DT16))
def test_forward_pixel_shuffle_relu(row, dt):
    """eval forward: F.pixel_shuffle(relu(conv), 2) done by the store (FLAG_SHUF2) into an 8-aligned channel window of a wider
    high-resolution buffer; the weights and bias arrive in sub-pixel-major order"""
    shape, flags, kernels, _ = ROWS[row]
    n, cin, cout, h, w, ks = shape
    assert_exact_premise(cin * ks * ks, dt=dt, bias=B_GRID)
    x, wt, b, acc = operands(shape)
    perm = shuf2_perm(cout)
    ref = F.pixel_shuffle((acc + nchw(b)).clamp_min(0), 2)
    out, launched, _ = conv(dt, x, wt[perm], bias=b[perm], flags=flags | RELU | SHUF2, shuf=True)
    assert launched == sorted(kernels), f"{row}: launched {launched}"
    assert_equal(result(out, 8, cout // 4), nhwc_ref(ref, dt), f"{row} shuffle")


@pytest.mark.parametrize("row,dt", _params(["v3_128", "geo0_bn128", "big_64", "flat_kc4"]))
def test_forward_tail_two_sources(row, dt):
    """residual tail: relu(conv(x0) + conv1x1(x1) + bias + aux * scale + shift), the second source a 1x1 one"""
    shape, flags, kernels, _ = ROWS[row]
    n, cin, cout, h, w, ks = shape
    cin1 = 16
    assert_exact_premise(cin * ks * ks + cin1, dt=dt, bias=B_GRID, tail=(X_GRID, SCALE_GRID, SHIFT_GRID))
    x, wt, b, acc = operands(shape)
    g = torch.Generator().manual_seed(_seed(row, "tail"))
    x1, w1, aux = dyadic(g, (n, cin1, h, w), X_GRID), dyadic(g, (cout, cin1, 1, 1), W_GRID), dyadic(g, (n, cout, h, w), X_GRID)
    scale, shift, _, _ = per_channel(row + "tail", cout)
    ref = (acc + F.conv2d(x1, w1) + nchw(b) + aux * nchw(scale) + nchw(shift)).clamp_min(0)
    out, launched, _ = conv(dt, x, wt, bias=b, flags=flags, x1=x1, w1=w1, tail=(aux, scale, shift))
    if ks == 1:      # a second source takes a 1x1 launch to the 9-tap loop's 1-tap instance; in f32 its 8 chunks split K
        kernels = [(IG, (128, 0, 1))] + ([(FIN, (128, 0))] if dt == F32 else [])
    assert launched == sorted(kernels), f"{row}: launched {launched}"
    assert_equal(result(out, 8, cout), nhwc_ref(ref, dt), f"{row} tail")


@pytest.mark.parametrize("dt", [BF16, F16, F32])
def test_forward_final(dt):
    """EPI_FINAL: f32 NCHW output (acc + bias) * 128 + 128"""
    from pssr2_amd import ops, _lib as L
    for shape in [(2, 32, 4, 24, 40, 3), (3, 16, 1, 16, 16, 3)]:
        n, cin, cout, h, w, ks = shape
        assert_exact_premise(cin * ks * ks, dt=dt, bias=B_GRID, final=(Grid(0, 128.0), Grid(0, 128.0)))
        x, wt, b, acc = operands(shape)
        want = expected((acc + nchw(b)) * 128 + 128, F32)
        out = torch.full((n, cout, h, w), -7.0, device="cuda")
        xd = nhwc(x, dt, coff=16, cstride=cin + 32)
        pw = ops.pack_conv_weight(dev(wt), ops.dtype_code(dt))
        _, launched = launched_kernels(lambda: ops.conv2d(xd, cin, pw, out, cout, n=n, h=h, w=w, in0_coff=16, bias=dev(b),
                                                          epilogue=L.EPI_FINAL, out_scale=128.0, out_shift=128.0))
        assert launched == [(IG, (32, 0, 9))], launched
        assert_equal(out, want, f"{shape} final")


@pytest.mark.parametrize("blk", [1, 2])
@pytest.mark.parametrize("row,dt", _params(["v3_128", "geo0_bn128", "flat_kc4"]))
def test_forward_blocked_orders(row, dt, blk):
    """input, output and residual in the blocked pixel order (r = 2, 4) with the tail epilogue"""
    shape, flags, kernels, _ = ROWS[row]
    n, cin, cout, h, w, ks = shape
    assert_exact_premise(cin * ks * ks, dt=dt, bias=B_GRID, tail=(X_GRID, SCALE_GRID, SHIFT_GRID))
    x, wt, b, acc = operands(shape)
    g = torch.Generator().manual_seed(_seed(row, "blk"))
    aux = dyadic(g, (n, cout, h, w), X_GRID)
    scale, shift, _, _ = per_channel(row + "blk", cout)
    ref = (acc + nchw(b) + aux * nchw(scale) + nchw(shift)).clamp_min(0)
    out, launched, _ = conv(dt, x, wt, bias=b, flags=flags, blk=blk, tail=(aux, scale, shift))
    assert launched == sorted(kernels), f"{row}: launched {launched}"
    assert_equal(result(out, 8, cout, blk), nhwc_ref(ref, dt), f"{row} blocked {blk}")


# ---------------------------------------------------------------------------------------------------------------------
# c. data gradient
@pytest.mark.parametrize("mask", [False, True], ids=["store", "mask_stats"])
@pytest.mark.parametrize("row,dt", _params(["v3_128", "geo0_bn128", "v3_64", "flat_kc4", "splitk_9tap"]))
def test_dgrad(row, dt, mask):
    """input gradient through mode-1 packed weights (no FLAG_SOLO): plain store, and the ReLU mask aux * scale + shift > 0 with the
    BatchNorm-backward statistics [sum g, sum g * xhat].  The layer weight is wt.transpose(0, 1).flip(2, 3), so the reference is the
    forward accumulator of the row (tests/test_conv_exact_helpers.py::test_dgrad_reference_identity)."""
    shape, _, kernels, _ = ROWS[row]
    n, cdy, cdx, h, w, ks = shape
    assert_exact_premise(cdy * ks * ks, dt=dt)
    dy, wt, _, ref = operands(shape)
    layer_w = wt.transpose(0, 1).flip(2, 3).contiguous()          # [cdy, cdx, ks, ks]
    m = None
    if mask:
        g = torch.Generator().manual_seed(_seed(row, "mask"))
        y = dyadic(g, (n, cdx, h, w), X_GRID)                     # the pre-activation of the layer's input
        scale, shift, mean, invstd = per_channel(row + "mask", cdx)
        ref = torch.where(y * nchw(scale) + nchw(shift) > 0, ref, torch.zeros_like(ref))
        m = (y, scale, shift, mean, invstd)
    out, launched, st = conv(dt, dy, layer_w, mode=1, mask=m, stats=mask)
    assert launched == sorted(kernels), f"{row}: launched {launched}"
    got = result(out, 8, cdx)
    assert_equal(got, nhwc_ref(ref, dt), f"{row} dgrad")
    if mask:
        xhat = ((y - nchw(mean)) * nchw(invstd)).permute(0, 2, 3, 1)
        gd = got.double()
        assert_stats(st, cdx, gd.sum((0, 1, 2)), (gd * xhat).sum((0, 1, 2)))


# ---------------------------------------------------------------------------------------------------------------------
# d. tilings agree bit for bit
TILINGS = {
    # row: [(tunables, extra flags, kernels)]
    "n128_216": [({}, 0, [(IG, (128, 0, 9))]), ({}, SOLO, [(IG, (64, 0, 9))]), ({"IGEMM_N64": 0}, SOLO, [(IG, (128, 0, 9))]),
                 ({"IGEMM_V3": 0}, SOLO, [(IG, (64, 0, 9))]), ({"IGEMM_V3": 2}, 0, [(V3, (128,))]), ({"IGEMM_V3": 2}, SOLO, [(V3, (128,))]),
                 ({"IGEMM_BIG": 0}, 0, [(IG, (128, 0, 9))]), ({"IGEMM_BIG": 2}, 0, [(IG, (64, 5, 9))]),
                 ({"CONV_EPI8": 0}, 0, [(IG, (128, 0, 9))]), ({"CONV_EPI8": 0}, SOLO, [(IG, (64, 0, 9))])],
    "v3_64": [({}, 0, [(V3, (64,))]), ({"IGEMM_V3": 2}, 0, [(V3, (64,))]), ({"IGEMM_V3_64": 0}, 0, [(IG, (64, 5, 9))]),
              ({"IGEMM_V3": 0}, 0, [(IG, (64, 5, 9))]), ({"IGEMM_V3": 0, "IGEMM_BIG": 0}, 0, [(IG, (64, 0, 9))]),
              ({"CONV_EPI8": 0}, 0, [(IG, (64, 5, 9))])],
    "splitk_9tap": [({}, 0, [(IG, (128, 0, 9)), (FIN, (128, 0))]), ({"IGEMM_KSPLIT": 1}, 0, [(IG, (128, 0, 9))]),
                    ({"CONV_EPI8": 0}, 0, [(IG, (128, 0, 9)), (FIN, (128, 0))])],
    "flat_kc9": [({}, 0, [(FLAT, (64, 0, 9))]), ({"IGEMM_FLAT": 0}, 0, [(IG, (64, 0, 1)), (FIN, (64, 0))]), ({"CONV_EPI8": 0}, 0, [(FLAT, (64, 0, 9))])],
}


@pytest.mark.parametrize("row,dt", [pytest.param(r, dt, id=f"{r}-{str(dt)[6:]}") for r in TILINGS for dt in DT16])
def test_tilings_agree(row, dt):
    """every tiling of one launch stores the same bits: FLAG_SOLO on and off, IGEMM_V3 0/1/2, IGEMM_V3_64, IGEMM_BIG 0/1/2,
    IGEMM_N64, CONV_EPI8 0/1, split-K off (IGEMM_KSPLIT=1), IGEMM_FLAT 0/1"""
    shape = ROWS[row][0]
    cout = shape[2]
    x, wt, b, acc = operands(shape)
    want = nhwc_ref((acc + nchw(b)).clamp_min(0), dt)
    for tun, flags, kernels in TILINGS[row]:
        with tunables(**tun):
            out, launched, _ = conv(dt, x, wt, bias=b, flags=flags | RELU)
        assert launched == sorted(kernels), f"{row} {tun} flags {flags}: launched {launched}"
        assert_equal(result(out, 8, cout), want, f"{row} {tun} flags {flags}")


# ---------------------------------------------------------------------------------------------------------------------
# e. weight gradient: four production-sized rows, each in atomic and in partial-slab mode on four layouts.  The table with one row per
# (family, template integers) of csrc/conv_wgrad.hip, the walk of the tile loop and the GELU prologue are in
# tests/test_gpu_wgrad_exact.py; the unpack pass on its own (windows, permuted and padded rows, part lanes, modes 2 and 4) is in
# tests/test_gpu_unpack_exact.py
WG = "conv_wgrad_kernel"
WG_ROWS = {
    # id: ((n, cin, cout, h, w, ks), prologue, 16-bit kernels, f32 kernels)
    "lean_pro": ((4, 64, 64, 32, 32, 3), True, [("conv_wgrad16_kernel", (64, 64, 0, 9))], [(WG, (64, 64, 0, 9))]),
    "dma": ((4, 64, 64, 32, 32, 3), False, [("conv_wgrad16d_kernel", (64, 64, 0, 9))], [(WG, (64, 64, 0, 9))]),
    "1x1": ((4, 208, 72, 16, 32, 1), True, [("conv_wgrad16_1x1_kernel", (0,))], [(WG, (64, 64, 0, 1))]),
    "generic": ((2, 80, 24, 12, 20, 3), True, [(WG, (32, 128, 0, 9))], [(WG, (32, 128, 0, 9))]),      # partial tiles: no lean kernel
}


@functools.lru_cache(maxsize=8)
def wgrad_case(row):
    shape, pro, _, _ = WG_ROWS[row]
    n, cin, cout, h, w, ks = shape
    g = torch.Generator().manual_seed(_seed(row, "wgrad"))
    x, dy = dyadic(g, (n, cin, h, w), X_GRID), dyadic(g, (n, cout, h, w), X_GRID)
    scale, shift, _, _ = per_channel(row + "wgrad", cin)
    act = (x * nchw(scale) + nchw(shift)).clamp_min(0) if pro else x
    ref = torch.nn.grad.conv2d_weight(act, (cout, cin, ks, ks), dy, padding=ks // 2)
    return x, dy, scale, shift, expected(ref, F32)


@pytest.mark.parametrize("parts", [False, True], ids=["atomic", "parts"])
@pytest.mark.parametrize("row,dt", [pytest.param(r, dt, id=f"{r}-{str(dt)[6:]}") for r in WG_ROWS for dt in (BF16, F16, F32)])
def test_wgrad_exact(row, dt, parts):
    """dw in f32 equals the float64 reference exactly, in atomic and in partial-slab mode, with channel offsets and in the blocked
    pixel orders (blk 1 and 2); the BatchNorm + ReLU prologue where the row has one.  At these shapes every workgroup takes one pixel
    tile and the unpack pass runs its contiguous path only: see tests/test_gpu_wgrad_exact.py and tests/test_gpu_unpack_exact.py"""
    from pssr2_amd import ops
    shape, pro, k16, k32 = WG_ROWS[row]
    n, cin, cout, h, w, ks = shape
    assert_exact_premise(n * h * w, X_GRID, X_GRID, dt=dt, pro=(SCALE_GRID, SHIFT_GRID) if pro else None)
    x, dy, scale, shift, want = wgrad_case(row)
    kw = dict(n=n, h=h, w=w, dtype=ops.dtype_code(dt))
    if pro:
        kw.update(pro_scale=dev(scale), pro_shift=dev(shift))
    for dy_coff, in_coff, blk in [(0, 0, 0), (8, 16, 0), (8, 16, 1), (0, 0, 2)]:
        dyd = nhwc(dy, dt, coff=dy_coff, cstride=dy_coff + cout + 8, blk=blk)
        xd = nhwc(x, dt, coff=in_coff, cstride=in_coff + cin + 16, blk=blk)
        args = dict(kw, dy_coff=dy_coff, in_coff=in_coff, dy_blk=blk, in_blk=blk)
        if parts:
            dwp, launched = launched_kernels(lambda: ops.conv2d_wgrad_parts(dyd, cout, xd, cin, ks * ks, **args))
        else:
            dwp = torch.zeros(cout, ks * ks, cin, device="cuda")
            _, launched = launched_kernels(lambda: ops.conv2d_wgrad(dyd, cout, xd, cin, ks * ks, dwp, **args))
        assert launched == sorted(k32 if dt == F32 else k16), f"{row} blk {blk}: launched {launched}"
        dw = torch.full((cout, cin, ks, ks), 9.0, device="cuda")
        ops.unpack_conv_wgrad(dwp, dw, k_pad=cin)
        assert_equal(dw, want, f"{row} dw (offsets {dy_coff}/{in_coff}, blk {blk})")
