"""Bit-exact tests of every weight-gradient kernel the library holds (csrc/conv_wgrad.hip).

Operands are dyadic with few significant bits (tests/_conv_exact.py), so the f32 weight gradient must equal the float64 reference
outright, whatever the order in which pixel tiles, partial slabs and atomics are summed.  Every case first asserts which kernel
the dispatch (launch_shape / launch_geo / launch_t at the table defaults of the tunables) launched for it.

a. one row per (family, template integers): the row table declares the kernel each row launches in 16 bits and in f32, and
   test_every_wgrad_instantiation_has_a_row compares the union of these declarations with the kernels in the built library
b. the tile loop: WGRAD_BLOCKS / WGRAD_BLOCKS_1X1 force the number of partial slabs, so that workgroups walk 1, an even number, an
   odd number and unequal numbers of pixel tiles (prefetch of tile i + 1, the LDS double buffer of the DMA kernel, the remainder)
c. the GELU prologue on the kernels production runs it on, against an oracle whose staged operand is known exactly

The two-group kernel (conv_wgrad16x2_kernel, WGRAD_X2=1) has tests of its own, named *_x2_*."""
import functools
from typing import NamedTuple

import pytest
import torch

from _conv_exact import (SCALE_GRID, SHIFT_GRID, X_GRID, assert_equal, assert_exact_premise, dev, dyadic, expected, gelu64,
                         gelu_exact_inputs, launched_kernels, library_kernel_table, nchw, nhwc, per_channel, pick, production_tunables,
                         stable_seed, tiles_per_workgroup, tunables)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("production_tunables")]
_ = production_tunables      # (the fixture is used through the mark above)

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DT16 = (BF16, F16)
WG, WG16, WG16D, WG1X1, WGX2 = ("conv_wgrad_kernel", "conv_wgrad16_kernel", "conv_wgrad16d_kernel", "conv_wgrad16_1x1_kernel",
                                "conv_wgrad16x2_kernel")


class Row(NamedTuple):
    shape: tuple        # n, cin, cout, h, w, ks
    pro: bool           # BatchNorm + ReLU prologue
    k16: tuple          # the kernel a 16-bit launch takes
    k32: tuple          # the kernel an f32 launch takes (None: the row is 16-bit only)


# (n, h, w) -> GEO and whether every tile is a full one
PIXELS = {
    "g0": ((3, 16, 32), 0, True),       # 16x8 tiles, 2x2 per image: interior halos in both directions and all four image borders
    "g1": ((4, 16, 8), 1, True),        # 8x8 tiles of two images, two tile rows
    "g2": ((9, 8, 4), 2, True),         # 4x4 tiles of eight images: two image groups, the second with one image
    "p0": ((2, 12, 20), 0, False),      # partial 16x8 tiles: the generic kernel in 16 bits too
    "p1": ((3, 10, 6), 1, False),       # partial 8x8 tiles, a half-filled image pair
}
# (CO_T, CI_T) -> {taps: (cin, cout)}: channel tails of 16 and 8 where the tiling allows, cout * elemsize % 16 == 0 in every type
CHANNELS = {
    (64, 64): {9: (80, 72), 1: (32, 40)},       # 1 tap: cin_pad <= 32 keeps the row off the 1x1 slab kernel
    (128, 32): {9: (32, 136), 1: (16, 136)},
    (32, 128): {9: (144, 24), 1: (144, 24)},
}
ROWS = {}
for (_co, _ci), _chans in CHANNELS.items():
    for _taps, (_cin, _cout) in _chans.items():
        for _pix, ((_n, _h, _w), _geo, _full) in PIXELS.items():
            _lean = _full and _geo < 2
            ROWS[f"t{_co}x{_ci}_k{_taps}_{_pix}"] = Row((_n, _cin, _cout, _h, _w, 3 if _taps == 9 else 1), True,
                                                        (WG16 if _lean else WG, (_co, _ci, _geo, _taps)), (WG, (_co, _ci, _geo, _taps)))
for _pix in ("g0", "g1"):
    (_n, _h, _w), _geo, _ = PIXELS[_pix]
    # no prologue: both operands go to LDS by DMA
    ROWS[f"dma_{_pix}"] = Row((_n, 80, 72, _h, _w, 3), False, (WG16D, (64, 64, _geo, 9)), (WG, (64, 64, _geo, 9)))
    # 1x1 with both channel counts beyond one 32-wide sub-tile: 128 x 128 slabs, tails of 16 and 8
    ROWS[f"slab_{_pix}"] = Row((_n, 144, 136, _h, _w, 1), True, (WG1X1, (_geo,)), (WG, (64, 64, _geo, 1)))
# WGRAD_X2=1: 16x8 tiles, 9 taps, full tiles
X2_ROWS = {f"x2_{_co}x{_ci}": Row((3, *_chans[9], 16, 32, 3), True, (WGX2, (_co, _ci)), None) for (_co, _ci), _chans in CHANNELS.items()}
ALL_ROWS = {**ROWS, **X2_ROWS}

LAYOUTS = [(0, 0, 0), (8, 16, 0), (8, 16, 1)]       # dy_coff, in_coff, log2 block size of the pixel order


def _params(rows, dts):
    return [pytest.param(r, dt, id=f"{r}-{str(dt)[6:]}") for r in rows for dt in dts]


@functools.lru_cache(maxsize=None)
def wgrad_case(row):
    """exact operands of a row and the float64 reference of its weight gradient, shared by every dtype, layout and mode"""
    (n, cin, cout, h, w, ks), pro, _, _ = ALL_ROWS[row]
    g = torch.Generator().manual_seed(stable_seed(row, "wgrad"))
    x, dy = dyadic(g, (n, cin, h, w), X_GRID), dyadic(g, (n, cout, h, w), X_GRID)
    scale, shift, _, _ = per_channel(row + "wgrad", cin)
    act = (x * nchw(scale) + nchw(shift)).clamp_min(0) if pro else x
    ref = torch.nn.grad.conv2d_weight(act, (cout, cin, ks, ks), dy, padding=ks // 2)
    return x, dy, scale, shift, expected(ref, F32)


def wgrad(row, dt, layout, *, parts=True, profile=False):
    """one weight-gradient launch of a row on NHWC copies with guard channels; returns (packed gradient, kernels launched or None)"""
    from pssr2_amd import ops
    (n, cin, cout, h, w, ks), pro, _, _ = ALL_ROWS[row]
    x, dy, scale, shift, _ = wgrad_case(row)
    dy_coff, in_coff, blk = layout
    dyd = nhwc(dy, dt, coff=dy_coff, cstride=dy_coff + cout + 8, blk=blk)
    xd = nhwc(x, dt, coff=in_coff, cstride=in_coff + cin + 16, blk=blk)
    kw = dict(n=n, h=h, w=w, dtype=ops.dtype_code(dt), dy_coff=dy_coff, in_coff=in_coff, dy_blk=blk, in_blk=blk)
    if pro:
        kw.update(pro_scale=dev(scale), pro_shift=dev(shift))
    if parts:
        def fn():
            return ops.conv2d_wgrad_parts(dyd, cout, xd, cin, ks * ks, **kw)
    else:
        def fn():
            return ops.conv2d_wgrad(dyd, cout, xd, cin, ks * ks, torch.zeros(cout, ks * ks, cin, device="cuda"), **kw)
    if profile:
        return launched_kernels(fn)
    return fn(), None


def unpacked(row, dwp):
    from pssr2_amd import ops
    (_, cin, cout, _, _, ks), _, _, _ = ALL_ROWS[row]
    dw = torch.full((cout, cin, ks, ks), 9.0, device="cuda")
    return ops.unpack_conv_wgrad(dwp, dw, k_pad=cin)


def check_row(row, dt):
    r = ALL_ROWS[row]
    n, _, _, h, w, _ = r.shape
    assert_exact_premise(n * h * w, X_GRID, X_GRID, dt=dt, pro=(SCALE_GRID, SHIFT_GRID) if r.pro else None)
    want = wgrad_case(row)[4]
    for i, layout in enumerate(LAYOUTS):
        dwp, launched = wgrad(row, dt, layout, profile=i == 0)       # partial slabs; the first launch under the profiler
        if i == 0:
            assert launched == [r.k32 if dt == F32 else r.k16], f"{row}: launched {launched}"
        assert_equal(unpacked(row, dwp), want, f"{row} partial slabs, layout {layout}")
    dwp, _ = wgrad(row, dt, LAYOUTS[1], parts=False)
    assert_equal(unpacked(row, dwp), want, f"{row} atomics, layout {LAYOUTS[1]}")


# ---------------------------------------------------------------------------------------------------------------------
# a. one row per instantiation
@pytest.mark.parametrize("row,dt", _params(ROWS, (BF16, F16, F32)))
def test_wgrad_rows(row, dt):
    """dw equals the float64 reference exactly in partial-slab mode on three layouts (channel offsets with guard channels, the blocked
    pixel order) and in atomic mode on one, with the BatchNorm + ReLU prologue wherever the kernel takes one (shifts of both signs: a
    positive shift on a zero-filled halo pixel must still stage 0)"""
    check_row(row, dt)


@pytest.mark.parametrize("row,dt", _params(X2_ROWS, DT16))
def test_wgrad_x2_rows(row, dt):
    """the same for the three tilings of the two-group kernel (opt-in: WGRAD_X2=1)"""
    with tunables(WGRAD_X2=1):
        check_row(row, dt)


def test_every_wgrad_instantiation_has_a_row():
    """the weight-gradient kernels in the built library are exactly those the row tables declare: a new instantiation fails here
    until it gets a row (this only reads the library)"""
    built = {p for p in library_kernel_table().values() if p is not None and p[0].startswith("conv_wgrad")}
    declared = {k for r in ALL_ROWS.values() for k in (r.k16, r.k32) if k is not None}
    assert built == declared, f"without a row: {sorted(built - declared)}; declared but not built: {sorted(declared - built)}"


# ---------------------------------------------------------------------------------------------------------------------
# b. the tile loop
N_TILES = 12                    # (3, 16, 32) in 16x8 tiles
SPLITS = (1, 5, 7, 12)          # tiles per workgroup: 12 | 3 3 2 2 2 | 2 2 2 2 2 1 1 | 1 each
# family: (row, types, tunables, the tunable that sets the workgroup count, slabs, kernel)
WALKS = {
    "generic16": ("t64x64_k9_g0", DT16, {"WGRAD_LEAN": 0}, "WGRAD_BLOCKS", 4, (WG, (64, 64, 0, 9))),        # prefetch in registers
    "generic32": ("t64x64_k9_g0", (F32,), {}, "WGRAD_BLOCKS", 4, (WG, (64, 64, 0, 9))),                     # synchronous loads
    "lean": ("t64x64_k9_g0", DT16, {}, "WGRAD_BLOCKS", 4, (WG16, (64, 64, 0, 9))),
    "dma": ("dma_g0", DT16, {}, "WGRAD_BLOCKS", 4, (WG16D, (64, 64, 0, 9))),                                # LDS double buffer
    "slab": ("slab_g0", DT16, {}, "WGRAD_BLOCKS_1X1", 4, (WG1X1, (0,))),
}
X2_WALK = ("x2_64x64", DT16, {"WGRAD_X2": 1}, "WGRAD_BLOCKS", 4, (WGX2, (64, 64)))


def test_splits_cover_the_tile_counts():
    counts = [tiles_per_workgroup(N_TILES, s) for s in SPLITS]
    flat = {c for cs in counts for c in cs}
    assert 1 in flat and any(c > 1 and c % 2 == 0 for c in flat) and any(c > 1 and c % 2 == 1 for c in flat)
    assert any(len(set(cs)) > 1 for cs in counts), "no launch with unequal tile counts"
    assert any(N_TILES % s != 0 for s in SPLITS), "no remainder"


def check_walk(walk, dt):
    row, _, tun, blocks, slabs, kernel = walk
    want = wgrad_case(row)[4]
    for split in SPLITS:
        with tunables(**tun, **{blocks: slabs * split}):
            dwp, launched = wgrad(row, dt, LAYOUTS[0], profile=True)
            assert dwp.shape[0] == split, f"{row}: {dwp.shape[0]} partial slabs for split {split}"
            assert launched == [kernel], f"{row} split {split}: launched {launched}"
            assert_equal(unpacked(row, dwp), want, f"{row} split {split}")
            if kernel[0] == WG16D:      # same tiles in the same order, same MFMA sequence as the register-staged kernel
                with tunables(WGRAD_DMA=0):
                    staged, launched = wgrad(row, dt, LAYOUTS[0], profile=True)
                assert launched == [(WG16, kernel[1])], f"{row} split {split}, WGRAD_DMA=0: launched {launched}"
                assert torch.equal(dwp, staged), f"{row} split {split}: the DMA kernel's partial slabs differ from WGRAD_DMA=0"


@pytest.mark.parametrize("family,dt", [pytest.param(f, dt, id=f"{f}-{str(dt)[6:]}") for f, wk in WALKS.items() for dt in wk[1]])
def test_wgrad_tile_walk(family, dt):
    """workgroups that walk 12, 3 or 2, 2 or 1 and 1 pixel tiles give the same exact gradient, in as many partial slabs as asked for"""
    check_walk(WALKS[family], dt)


@pytest.mark.parametrize("dt", DT16, ids=["bfloat16", "float16"])
def test_wgrad_x2_tile_walk(dt):
    """the two groups of the two-group kernel take alternate tiles: 6 + 6, 2 + 1 or 1 + 1, 1 + 1 or 1 + 0, 1 + 0"""
    check_walk(X2_WALK, dt)


# ---------------------------------------------------------------------------------------------------------------------
# c. GELU prologue (RDNet's second 1x1 convolution)
GELU_ROWS = [("t128x32_k1_g0", DT16), ("t64x64_k1_g0", DT16), ("slab_g0", DT16), ("slab_g1", DT16), ("t64x64_k1_g0", (F32,))]


@pytest.mark.parametrize("row,dt", [pytest.param(r, dt, id=f"{r}-{str(dt)[6:]}") for r, dts in GELU_ROWS for dt in dts])
def test_wgrad_gelu_prologue(row, dt):
    """dw = dy^T gelu(z) on the lean kernels production runs it on (and the generic one in f32).  The polynomial GELU of the 16-bit
    builds is not exact, so z only takes values whose gelu(z), give or take twice the error bound of csrc/common.h, rounds to one
    number of the storage type: the staged operand g = round(gelu64(z)) is then known, dy * g is exact in f32, and what remains is
    the f32 summation: |dw - ref| <= 2 * npix * 2^-24 * sum |dy * g| per element (the bound for any order, doubled).  f32 (erff, no
    rounding of g): every z, and 4 * 2^-24 * |g| more per term for the function.  A dropped or misplaced pixel moves an element by
    at least min |dy * g| ~ 0.25 * 0.045."""
    from pssr2_amd import ops
    (n, cin, cout, h, w, ks), _, k16, k32 = ROWS[row]
    assert ks == 1
    zs = torch.arange(-32, 33, dtype=torch.float64) / 8 if dt == F32 else gelu_exact_inputs(dt)
    assert len(zs) >= 32, f"only {len(zs)} of 65 GELU inputs survive the screening for {dt}"
    gen = torch.Generator().manual_seed(stable_seed(row, "gelu"))
    z, dy = pick(gen, (n, cin, h, w), zs.tolist()), dyadic(gen, (n, cout, h, w), X_GRID)
    g = gelu64(z) if dt == F32 else gelu64(z).float().to(dt).double()
    ref = torch.nn.grad.conv2d_weight(g, (cout, cin, 1, 1), dy)
    mag = torch.nn.grad.conv2d_weight(g.abs(), (cout, cin, 1, 1), dy.abs())
    bound = 2 * n * h * w * 2.0 ** -24 * mag + (4 * 2.0 ** -24 * mag if dt == F32 else 0)
    dy_coff, in_coff, blk = LAYOUTS[1]
    dyd = nhwc(dy, dt, coff=dy_coff, cstride=dy_coff + cout + 8)
    zd = nhwc(z, dt, coff=in_coff, cstride=in_coff + cin + 16)
    dwp, launched = launched_kernels(lambda: ops.conv2d_wgrad_parts(dyd, cout, zd, cin, 1, n=n, h=h, w=w, dtype=ops.dtype_code(dt),
                                                                    dy_coff=dy_coff, in_coff=in_coff, gelu_in=True))
    assert launched == [k32 if dt == F32 else k16], f"{row}: launched {launched}"
    err = (unpacked(row, dwp).cpu().double() - ref).abs()
    assert bool((mag > 0).all())
    ratio = float((err / bound).max())
    print(f"gelu prologue {row} {dt}: {len(zs)} inputs, worst error / bound = {ratio:.3g} (worst error {float(err.max()):.3g})")
    assert ratio <= 1.0, f"{row}: error / bound = {ratio} at {tuple((err / bound).flatten().argmax().unsqueeze(0).tolist())}"
