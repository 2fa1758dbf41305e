"""Bit-exact and float64 tests of the Reconstruction head kernels (csrc/head_conv.hip) and of the fused head of `pre`
(conv_headq_epilogue in csrc/conv_igemm_impl.h + pssr_head_q_gather).

1. Dyadic operands (tests/_conv_exact.py): activations and gradient on X_GRID, weights on a per-dtype grid with (storage bits - 1)
   fractional bits, so every in-kernel conversion is exact, every f32 partial sum is exact whatever its order, and a 16-bit store must
   equal the float64 reference rounded once.  Everything is compared with torch.equal; every case asserts the template arguments of
   the kernel that ran; activations and data gradients sit at a channel offset inside wider buffers whose guard channels are checked.
2. The tap planes of PSSR_EPI_HEADQ / PSSR_FLAG_HEADQ against the float64 reference, and the gather on them.
3. One case per entry point on normal random data, where the conversions of the weights and of g * g_scale to 16 bits do round:
   against a float64 reference that restates those roundings, within 2 k 2^-24 sum|terms| (+ half a storage ulp for 16-bit results).

Known divergence: for a NaN activation head_dgrad_kernel writes 0 while head_bwd_kernel's packed integer test passes the
gradient of a +NaN.  The tests use finite activations."""
import functools
import itertools
import zlib
from typing import NamedTuple

import pytest
import torch
import torch.nn.functional as F

from _conv_exact import (B_GRID, HEAD_BWD_GRID, HEAD_WGRAD_GRID, SENTINEL, STAT_ROWS, X_GRID, Grid, assert_guards, assert_head_premise,
                         assert_headq_premise, dyadic, expected, fold_stat_rows, from_blocked, head_refs, head_tiles, head_weight_grid,
                         is_head_kernel, later_trip_mask, launched_kernels, mask_edge_values, needs_rounding, nhwc, production_tunables,
                         stored_grid, storage_ulp, sum_fits)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("production_tunables")]
_ = production_tunables      # (the fixture is used through the mark above)

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DT16 = (BF16, F16)
NAN = float("nan")
ACT_OFF, ACT_PAD, D_OFF, D_PAD = 16, 32, 8, 16        # activation at channel 16 of [.., cin + 32], dact at channel 8 of [.., cin + 16]
GUARD = 4                                            # guard elements on both sides of an f32 / f64 output (16-byte aligned)
FWD, DGRAD, WGRAD, BWD = "head_fwd_kernel", "head_dgrad_kernel", "head_wgrad_kernel", "head_bwd_kernel"


class Case(NamedTuple):
    n: int
    cin: int
    cout: int
    h: int
    w: int
    blk: int
    gs: float       # g_scale: 128 (production) or 1.5


def _gs(i):
    return (128.0, 1.5)[i % 2]


# every cin x cout on two partial tiles per image; the block order and g_scale cycle independently of cout
MATRIX = [Case(2, cin, cout, 24, 40, (i + i // 3) % 3, _gs(i))
          for i, (cin, cout) in enumerate(itertools.product((32, 64, 96, 128), (1, 2, 3)))]
# one full tile / halos between images / smaller than a tile / one-pixel ragged tiles / full multi-tile (FULL = true) / blk = 3
GEOMETRY = [Case(n, cin, cout, h, w, blk, _gs(i + j))
            for j, (cin, cout) in enumerate([(32, 1), (128, 3)])
            for i, (n, h, w, blk) in enumerate([(1, 16, 16, 0), (3, 16, 16, 2), (1, 4, 8, 2), (1, 17, 33, 0), (2, 48, 80, 2), (1, 8, 8, 3)])]
# bias sums, f32-atomic and striped: six ragged tiles, few enough pixels per (sub-pixel, channel) for the f32 sums to be exact
BIAS = [Case(1, cin, 1, 20, 36, blk, 128.0 if blk == 0 else 1.5) for cin in (32, 64, 128) for blk in (0, 1, 2)]
# more tiles than workgroups: 529 full / 529 ragged tiles over the 512 of head_bwd_kernel, 1056 over the 1024 of head_wgrad_kernel
PERSIST_BWD = [Case(1, 32, 1, 368, 368, 0, 128.0), Case(1, 32, 3, 362, 354, 1, 128.0)]
PERSIST_WGRAD = [Case(1, 32, 1, 528, 512, 2, 128.0)]
EDGES = [Case(2, 64, 2, 24, 40, 1, 1.5), Case(1, 32, 1, 17, 33, 0, 128.0), Case(1, 128, 3, 16, 16, 2, 1.5)]
ROUNDING = Case(2, 64, 3, 24, 40, 1, 1.5)


# ---------------------------------------------------------------------------------------------------------------------
# which kernel a case takes (the launch code of csrc/head_conv.hip restated), and where the bias sums are provably exact
def bias_modes(c: Case, dt):
    """(f32-atomic bias_sum, striped bias_rows): whether the premise walk proves the f32 sums of the stored dact exact -- over all the
    pixels of a (sub-pixel, channel) for the atomics, over those of one workgroup's tiles for the rows (f64 from there on)"""
    if c.cin not in (32, 64, 128) or c.blk > 2:
        return False, False
    stored = stored_grid(assert_head_premise(c.cin, c.cout, c.n * c.h * c.w, c.gs, dt=dt).dP, dt)
    tiles = head_tiles(c.n, c.h, c.w)[0]
    per_wg = -(-tiles // HEAD_BWD_GRID) * (256 >> (2 * c.blk))
    return sum_fits(stored, c.n * c.h * c.w >> (2 * c.blk)), sum_fits(stored, per_wg)


def kernels(entry, c: Case, dt):
    if entry == "fwd":
        return [(FWD, (-(-c.cout * 9 // 16), c.cin // 32))]
    if entry == "dgrad":
        return [(DGRAD, (c.cin // 16,))]
    if entry == "wgrad":
        return [(WGRAD, (c.cout,))]
    bs = bias_modes(c, dt)[0 if entry == "bwd" else 1]
    return [(BWD, (c.cin // 16, int(bs), int(c.h % 16 == 0 and c.w % 16 == 0)))]


def _id(entry, c: Case, dt):
    if entry in ("bwd", "bwd_rows") and c.blk == 3:
        path = "refused"
    else:
        fam, ints = kernels(entry, c, dt)[0]
        names = {FWD: ("NT", "KS"), DGRAD: ("NT",), WGRAD: ("COUT",), BWD: ("NT", "BS", "FULL")}[fam]
        path = "_".join(f"{k}{v}" for k, v in zip(names, ints))
    tiles = head_tiles(c.n, c.h, c.w)[0]
    return f"{entry}_{path}-n{c.n}c{c.cin}o{c.cout}_{c.h}x{c.w}_b{c.blk}_g{c.gs:g}_t{tiles}-{str(dt)[6:]}"


def _params(entry, cases):
    return [pytest.param(c, dt, id=_id(entry, c, dt)) for c in cases for dt in DT16]


# ---------------------------------------------------------------------------------------------------------------------
# operands and float64 references, kept in compact form (16-bit / small tensors) and shared by the tests of all entry points
class Ops(NamedTuple):
    act: torch.Tensor           # [n, cin, h, w] in dt
    wt: torch.Tensor            # f32 OIHW
    bias: torch.Tensor          # f32 [cout]
    g: torch.Tensor             # f32 NCHW, unscaled
    out: torch.Tensor           # f32 NCHW: (conv + bias) * 128 + 128
    out_nobias: torch.Tensor
    dact: torch.Tensor          # dt [n, h, w, cin], plain pixel order
    share: float                # share of the dP values that the 16-bit store has to round
    base: torch.Tensor          # f32 OIHW: the gradient that is already there
    dw: torch.Tensor            # f32 OIHW: base + dW
    dw_only: torch.Tensor       # f64 OIHW
    bsum: torch.Tensor          # f64 [4^blk * cin]: sums of the expected dact per (sub-pixel, channel)


def _seed(*key):
    return zlib.crc32(repr(tuple(key)).encode()) & 0x7fffffff


def bias_sums(dact_nhwc, blk):
    """float64 sums per (sub-pixel = (y % r) * r + x % r, channel) of a [n, h, w, c] tensor in plain pixel order"""
    n, h, w, c = dact_nhwc.shape
    r = 1 << blk
    return dact_nhwc.double().reshape(n, h // r, r, w // r, r, c).sum(dim=(0, 1, 3)).reshape(-1)


@functools.lru_cache(maxsize=None)
def operands(c: Case, dt, later=0, edges=False) -> Ops:
    """later > 0: the gradient is zero except in the tiles of index >= later (the later trips of a persistent kernel of `later`
    workgroups); edges: activations around the mask's decision instead of X_GRID (only `dact` is meaningful then)"""
    n, cin, cout, h, w, blk, gs = c
    grids = assert_head_premise(cin, cout, n * h * w, gs, dt=dt)
    gen = torch.Generator().manual_seed(_seed(*c, str(dt), later, edges))
    if edges:
        vals = mask_edge_values(dt)
        act16 = vals[torch.randint(0, len(vals), (n, cin, h, w), generator=gen)]
        act = torch.where(act16.double().abs() == 1.0, act16.double(), torch.zeros((), dtype=torch.float64))    # forward / dW unused
    else:
        act = dyadic(gen, (n, cin, h, w), X_GRID)
        act = torch.where(torch.rand(act.shape, generator=gen) < 0.5, act.clamp_min(0), act)     # half ReLU-like, half keep negatives
        act16 = act.to(dt)
        assert torch.equal(act16.double(), act)
    wt = dyadic(gen, (cout, cin, 3, 3), head_weight_grid(dt))
    bias = dyadic(gen, (cout,), B_GRID)
    g = dyadic(gen, (n, cout, h, w), X_GRID)
    if later:
        g = g * later_trip_mask(n, h, w, later)
        assert bool((g != 0).any()), "no tile beyond the grid"
    conv, dP, dW = head_refs(act, wt, g * gs)
    out = expected((conv + bias.view(1, -1, 1, 1)) * 128 + 128, F32)
    out_nobias = expected(conv * 128 + 128, F32)
    dP16 = expected(dP, dt)
    dact = torch.where(act16.double() > 0, dP16, torch.zeros((), dtype=dt)).permute(0, 2, 3, 1).contiguous()
    base = torch.randint(-8, 9, dW.shape, generator=gen).double() / 2.0 ** grids.dW.e
    return Ops(act16, wt.float(), bias.float(), g.float(), out, out_nobias, dact, needs_rounding(dP, dt), base.float(),
               expected(base + dW, F32), dW, bias_sums(dact, blk) if blk <= 2 else None)


class Dev:
    """device buffers of one run: activation with NaN guard channels, sentinel-filled outputs between guards"""

    def __init__(self, c: Case, dt, o: Ops):
        self.c, self.dt = c, dt
        self.act = nhwc(o.act, dt, coff=ACT_OFF, cstride=c.cin + ACT_PAD, blk=c.blk, sentinel=NAN)
        self.wt, self.bias, self.g = o.wt.cuda().contiguous(), o.bias.cuda(), o.g.cuda().contiguous()
        self.dact = torch.full((c.n, c.h, c.w, c.cin + D_PAD), SENTINEL, dtype=dt, device="cuda")
        self.guarded = []

    def buf(self, shape, dtype=F32, init=None):
        """an output of `shape` between GUARD sentinel elements; init: a tensor to start from (default: the sentinel)"""
        numel = 1
        for s in shape:
            numel *= s
        whole = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
        view = whole[GUARD:GUARD + numel].view(shape)
        if init is not None:
            view.copy_(init)
        self.guarded.append(whole)
        return view

    def check_guards(self):
        for whole in self.guarded:
            assert bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all()), "a store went outside an output"

    def got_dact(self):
        assert_guards(self.dact, D_OFF, self.c.cin)
        return from_blocked(self.dact.cpu(), self.c.blk)[..., D_OFF:D_OFF + self.c.cin]


def assert_equal(got, want, what=""):
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {want.numel()} values differ; first at {i}: got {got[i].item()!r}, want {want[i].item()!r}")


def run(entry, d: Dev, **out):
    """one launch of `entry` on the buffers of d through the ops wrappers; returns the kernels that ran"""
    from pssr2_amd import ops
    c, code = d.c, ops.dtype_code(d.dt)
    dims = (c.n, c.h, c.w, c.cin, c.cout)
    off = dict(act_coff=ACT_OFF, dact_coff=D_OFF)
    fn = {
        "fwd": lambda: ops.head_conv_fwd(d.act, c.blk, d.wt, out.get("bias"), out["out"], *dims, 128.0, 128.0, code, act_coff=ACT_OFF),
        "dgrad": lambda: ops.head_conv_dgrad(d.g, c.gs, d.wt, d.act, d.dact, c.blk, *dims, code, **off),
        "wgrad": lambda: ops.head_conv_wgrad(d.g, c.gs, d.act, c.blk, out.get("dw"), *dims, code, act_coff=ACT_OFF),
        "bwd": lambda: ops.head_conv_bwd(d.g, c.gs, d.wt, d.act, d.dact, c.blk, out.get("dw"), out.get("bias_sum"), *dims, code, **off),
        "bwd_rows": lambda: ops.head_conv_bwd_rows(d.g, c.gs, d.wt, d.act, d.dact, c.blk, out.get("dw_rows"), out.get("bias_rows"), *dims, code, **off),
    }[entry]
    return launched_kernels(fn, is_head_kernel)[1]


def trips(c: Case, grid):
    """the gradients a case runs with: dense, and -- when the kernel loops -- nonzero only in the tiles of its later trips"""
    return (0, grid) if head_tiles(c.n, c.h, c.w)[0] > grid else (0,)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the five entry points on dyadic operands
@pytest.mark.parametrize("c,dt", _params("fwd", MATRIX + GEOMETRY))
def test_head_conv_fwd(c, dt):
    o = operands(c, dt)
    for bias, want in ((True, o.out), (False, o.out_nobias)):
        d = Dev(c, dt, o)
        out = d.buf((c.n, c.cout, c.h, c.w))
        ks = run("fwd", d, out=out, bias=d.bias if bias else None)
        assert ks == kernels("fwd", c, dt), ks
        assert_equal(out, want, f"out (bias={bias})")
        d.check_guards()


@pytest.mark.parametrize("c,dt", _params("dgrad", MATRIX + GEOMETRY))
def test_head_conv_dgrad(c, dt):
    o = operands(c, dt)
    print(f"share of dP values that need rounding in {dt}: {o.share:.3f}")
    assert o.share >= 0.05, o.share
    d = Dev(c, dt, o)
    ks = run("dgrad", d)
    assert ks == kernels("dgrad", c, dt), ks
    assert_equal(d.got_dact(), o.dact, "dact")


@pytest.mark.parametrize("c,dt", _params("wgrad", MATRIX + GEOMETRY + PERSIST_WGRAD))
def test_head_conv_wgrad(c, dt):
    for later in trips(c, HEAD_WGRAD_GRID):
        o = operands(c, dt, later)
        d = Dev(c, dt, o)
        dw = d.buf(o.base.shape, init=o.base)
        ks = run("wgrad", d, dw=dw)
        assert ks == kernels("wgrad", c, dt), ks
        assert_equal(dw, o.dw, f"dw (gradient in tiles >= {later})")
        d.check_guards()


def _refused(entry, c, dt):
    """blk = 3: the fused backward refuses on the host and touches nothing"""
    o = operands(c, dt)
    d = Dev(c, dt, o)
    outs = dict(dw=d.buf(o.base.shape), dw_rows=d.buf((STAT_ROWS,) + o.base.shape, torch.float64))
    with pytest.raises(RuntimeError, match="blocked order"):
        run(entry, d, **outs)
    torch.cuda.synchronize()
    for t in (d.dact, *d.guarded):
        assert bool((t == SENTINEL).all()), "a refused call wrote something"


@pytest.mark.parametrize("c,dt", _params("bwd", MATRIX + GEOMETRY + BIAS + PERSIST_BWD))
def test_head_conv_bwd(c, dt):
    if c.blk == 3:
        return _refused("bwd", c, dt)
    with_bias = bias_modes(c, dt)[0]
    assert with_bias or c not in BIAS, "the bias-sum cases must pass the premise walk"
    for later in trips(c, HEAD_BWD_GRID):
        o = operands(c, dt, later)
        d = Dev(c, dt, o)
        dw = d.buf(o.base.shape, init=o.base)
        bsum = d.buf(o.bsum.shape, init=torch.zeros_like(o.bsum)) if with_bias else None
        ks = run("bwd", d, dw=dw, bias_sum=bsum)
        assert ks == kernels("bwd", c, dt), ks
        assert_equal(d.got_dact(), o.dact, f"dact (gradient in tiles >= {later})")
        assert_equal(dw, o.dw, f"dw (gradient in tiles >= {later})")
        if with_bias:
            assert_equal(bsum, expected(o.bsum, F32), "bias_sum")
        d.check_guards()


def _rows_run(c, dt, o, with_bias):
    d = Dev(c, dt, o)
    dw_rows = d.buf((STAT_ROWS,) + o.base.shape, torch.float64, init=torch.zeros(()))
    bias_rows = d.buf((STAT_ROWS,) + o.bsum.shape, torch.float64, init=torch.zeros(())) if with_bias else None
    ks = run("bwd_rows", d, dw_rows=dw_rows, bias_rows=bias_rows)
    d.check_guards()
    return d, ks, dw_rows, bias_rows


@pytest.mark.parametrize("c,dt", _params("bwd_rows", MATRIX + GEOMETRY + BIAS + PERSIST_BWD))
def test_head_conv_bwd_rows(c, dt):
    from pssr2_amd import ops
    if c.blk == 3:
        return _refused("bwd_rows", c, dt)
    with_bias = bias_modes(c, dt)[1]
    assert with_bias or c not in BIAS + PERSIST_BWD, "the bias-sum and persistent cases must pass the premise walk"
    tiles = head_tiles(c.n, c.h, c.w)[0]
    wgs = -(-min(tiles, HEAD_BWD_GRID) // 32)          # workgroups per stripe; a weight receives one value per wave, a bias sum one
    for later in trips(c, HEAD_BWD_GRID):
        o = operands(c, dt, later)
        d, ks, dw_rows, bias_rows = _rows_run(c, dt, o, with_bias)
        assert ks == kernels("bwd_rows", c, dt), ks
        assert_equal(d.got_dact(), o.dact, f"dact (gradient in tiles >= {later})")
        assert_equal(fold_stat_rows(dw_rows, 4 * wgs), o.dw_only, "dw_rows summed in float64")
        dw = torch.empty_like(o.base, device="cuda")
        ops.f64_to_f32(dw_rows, dw)
        assert_equal(dw, expected(o.dw_only, F32), "f64_to_f32(dw_rows)")
        if with_bias:
            assert_equal(fold_stat_rows(bias_rows, wgs), o.bsum, "bias_rows summed in float64")
            bs = torch.empty(o.bsum.shape, device="cuda")
            ops.f64_to_f32(bias_rows, bs)
            assert_equal(bs, expected(o.bsum, F32), "f64_to_f32(bias_rows)")
        if later or tiles > HEAD_BWD_GRID:
            continue
        # a second run: bit-identical dact and rows; without bias_rows: the rest unchanged
        d2, _, dw_rows2, bias_rows2 = _rows_run(c, dt, o, with_bias)
        assert torch.equal(d2.dact, d.dact) and torch.equal(dw_rows2, dw_rows), "the second run differs"
        if with_bias:
            assert torch.equal(bias_rows2, bias_rows), "the second run's bias rows differ"
            d3, ks3, dw_rows3, _ = _rows_run(c, dt, o, False)
            assert ks3 == [(BWD, (c.cin // 16, 0, kernels("bwd_rows", c, dt)[0][1][2]))], ks3
            assert torch.equal(d3.dact, d.dact) and torch.equal(dw_rows3, dw_rows), "bias_rows=None changes dact or dw_rows"


@pytest.mark.parametrize("entry", ["dgrad", "bwd", "bwd_rows"])
@pytest.mark.parametrize("c,dt", [pytest.param(c, dt, id=f"n{c.n}c{c.cin}o{c.cout}_{c.h}x{c.w}_b{c.blk}-{str(dt)[6:]}") for c in EDGES for dt in DT16])
def test_mask_edges(c, dt, entry):
    """+0, -0, negative values and nothing else are masked: subnormals, the smallest normal number and the largest finite one pass"""
    o = operands(c, dt, 0, True)
    d = Dev(c, dt, o)
    outs = dict(dw=d.buf(o.base.shape, init=o.base), dw_rows=d.buf((STAT_ROWS,) + o.base.shape, torch.float64, init=torch.zeros(())))
    run(entry, d, **outs)
    assert_equal(d.got_dact(), o.dact, "dact")
    d.check_guards()


# ---------------------------------------------------------------------------------------------------------------------
# refusals: every one is decided on the host before any launch (check_common, head_conv_bwd_impl, pssr_head_conv_bwd_rows)
REFUSALS = {
    "cout4": dict(cout=4), "cin48": dict(cin=48), "cin160": dict(cin=160), "f32": dict(dtype="f32"), "cs_not_8": dict(cs_pad=28),
    "co_cin_over_cs": dict(cs_pad=8), "h_not_blocked": dict(h=18, blk=2), "bias_cin96": dict(cin=96, bias=True), "null_dw_rows": dict(null_rows=True),
}
REFUSAL_ENTRIES = {"bias_cin96": ("bwd", "bwd_rows"), "null_dw_rows": ("bwd_rows",)}
ENTRIES = ("fwd", "dgrad", "wgrad", "bwd", "bwd_rows")


@pytest.mark.parametrize("name,entry", [pytest.param(r, e, id=f"{r}-{e}") for r in REFUSALS for e in REFUSAL_ENTRIES.get(r, ENTRIES)])
def test_refusals(name, entry):
    import ctypes as C
    from pssr2_amd import _lib as L
    r = dict(n=1, cin=32, cout=1, h=16, w=16, blk=0, dtype="bf16", cs_pad=ACT_PAD, bias=False, null_rows=False)
    r.update(REFUSALS[name])
    n, cin, cout, h, w, blk = (r[k] for k in ("n", "cin", "cout", "h", "w", "blk"))
    code = {"bf16": L.BF16, "f32": L.F32}[r["dtype"]]
    big = 1 << 20           # every buffer holds whatever a launch of these sizes could touch
    act = torch.zeros(big, dtype=BF16, device="cuda")
    wt, bias, g = torch.zeros(big, device="cuda"), torch.zeros(8, device="cuda"), torch.zeros(big, device="cuda")
    outs = {k: torch.full((big,), SENTINEL, dtype=dt, device="cuda")
            for k, dt in (("out", F32), ("dact", BF16), ("dw", F32), ("bsum", F32), ("dw_rows", torch.float64), ("bias_rows", torch.float64))}
    p = {k: L.ptr(v) for k, v in outs.items()}
    a = (L.ptr(act), cin + r["cs_pad"], ACT_OFF)
    dd = (p["dact"], cin + D_PAD, D_OFF)
    dims = (n, h, w, cin, cout, code, L.stream_ptr())
    gsc = C.c_float(128.0)
    lib = L.lib()
    rc = {
        "fwd": lambda: lib.pssr_head_conv_fwd(*a, blk, L.ptr(wt), L.ptr(bias), p["out"], n, h, w, cin, cout, gsc, gsc, code, L.stream_ptr()),
        "dgrad": lambda: lib.pssr_head_conv_dgrad(L.ptr(g), gsc, L.ptr(wt), *a, *dd, blk, *dims),
        "wgrad": lambda: lib.pssr_head_conv_wgrad(L.ptr(g), gsc, *a, blk, p["dw"], *dims),
        "bwd": lambda: lib.pssr_head_conv_bwd(L.ptr(g), gsc, L.ptr(wt), *a, *dd, blk, p["dw"], p["bsum"] if r["bias"] else None, *dims),
        "bwd_rows": lambda: lib.pssr_head_conv_bwd_rows(L.ptr(g), gsc, L.ptr(wt), *a, *dd, blk, None if r["null_rows"] else p["dw_rows"],
                                                        p["bias_rows"] if r["bias"] else None, *dims),
    }[entry]()
    assert rc != 0
    with pytest.raises(RuntimeError, match="failed"):
        L.check(rc, entry)
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert bool((v == SENTINEL).all()), f"the refused call wrote to {k}"


# ---------------------------------------------------------------------------------------------------------------------
# 2. the fused head of `pre`: tap planes out of the accumulators (EPI_HEADQ / FLAG_HEADQ), then the gather
V3 = "conv_v3_kernel"
CIN0 = 32
# coarser activations than X_GRID so that the nine-tap sum of 64-channel products fits 24 bits, and a large bias so that the 16-bit
# rounding of relu(acc + bias) happens often: (x, w, bias of pre, head weight, head bias)
HEADQ_GRIDS = {BF16: (Grid(1, 1.0), Grid(2, 0.5), Grid(3, 64.0), Grid(5, 0.5), B_GRID),
               F16: (Grid(2, 1.0), Grid(2, 0.5), Grid(4, 512.0), Grid(2, 0.5), B_GRID)}


class HeadQ(NamedTuple):
    x: torch.Tensor             # f64 NCHW
    wt: torch.Tensor            # f64 [1024, CIN0, 3, 3]: stored channel sub * 64 + c
    b: torch.Tensor
    hw: torch.Tensor            # f64 [1, 64, 3, 3]
    hb: torch.Tensor
    act: torch.Tensor           # dt [n, 1024, h, w]: expected(relu(acc + bias))
    planes: torch.Tensor        # f32 [9, 16, n, h, w]
    out: torch.Tensor           # f32 [n, 1, 4h, 4w]


@functools.lru_cache(maxsize=None)
def headq_case(shape, dt) -> HeadQ:
    n, h, w = shape
    gx, gw, gb, ghw, ghb = HEADQ_GRIDS[dt]
    assert_headq_premise(9 * CIN0, gx, gw, gb, ghw, ghb, dt=dt)
    gen = torch.Generator().manual_seed(_seed(*shape, str(dt)))
    x, wt, b = dyadic(gen, (n, CIN0, h, w), gx), dyadic(gen, (1024, CIN0, 3, 3), gw), dyadic(gen, (1024,), gb)
    hw, hb = dyadic(gen, (1, 64, 3, 3), ghw), dyadic(gen, (1,), ghb)
    pre = F.relu(F.conv2d(x, wt, b, padding=1))
    share = needs_rounding(pre, dt)
    print(f"share of pre's activations that need rounding in {dt}: {share:.3f}")
    assert share >= 0.05, share
    act = expected(pre, dt)
    a64 = act.double()
    planes = torch.einsum("nschw,ct->tsnhw", a64.view(n, 16, 64, h, w), hw.view(64, 9))
    hr = a64.view(n, 4, 4, 64, h, w).permute(0, 3, 4, 1, 5, 2).reshape(n, 64, 4 * h, 4 * w)         # sub-pixel (i, j) = (sub >> 2, sub & 3)
    out = (F.conv2d(hr, hw, hb, padding=1)) * 128 + 128
    return HeadQ(x, wt, b, hw, hb, act, expected(planes.contiguous(), F32), expected(out, F32))


def _gather(planes_dev, q: HeadQ, shape):
    from pssr2_amd import ops
    n, h, w = shape
    whole = torch.full((n * 16 * h * w + 2 * GUARD,), SENTINEL, device="cuda")
    out = whole[GUARD:-GUARD].view(n, 1, 4 * h, 4 * w)
    ops.head_q_gather(planes_dev, q.hb.float().cuda(), out, n, h, w, 128.0, 128.0)
    assert_equal(out, q.out, "head_q_gather")
    assert bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())


@pytest.mark.parametrize("dt", DT16, ids=["bfloat16", "float16"])
@pytest.mark.parametrize("shape", [(2, 32, 32), (1, 36, 52)], ids=["2x32x32", "ragged_1x36x52"])
@pytest.mark.parametrize("mode", ["EPI_HEADQ", "FLAG_HEADQ"])
def test_pre_tap_planes(mode, shape, dt):
    """one conv2d launch as Engine._head_forward issues it: 16 * 64 stored channels on the conv_v3 tiling.  The tap planes equal, bit for
    bit, the float64 sums over the 64 channels of one sub-pixel of (the activation as the store rounds it) x (head weight); with
    FLAG_HEADQ the stored activation is that rounded value too; the gather of the planes is the head convolution * 128 + 128."""
    from pssr2_amd import ops, _lib as L
    n, h, w = shape
    q = headq_case(shape, dt)
    code = ops.dtype_code(dt)
    xd = nhwc(q.x, dt, coff=16, cstride=CIN0 + 32, sentinel=NAN)
    pw = ops.pack_conv_weight(q.wt.float().contiguous().cuda(), code)
    whole = torch.full((9 * 16 * n * h * w + 2 * GUARD,), SENTINEL, device="cuda")
    planes = whole[GUARD:-GUARD].view(9, 16, n, h, w)
    kw = dict(n=n, h=h, w=w, in0_coff=16, bias=q.b.float().cuda(), head_w=q.hw.float().contiguous().cuda(), head_q=planes)
    if mode == "EPI_HEADQ":
        _, ks = launched_kernels(lambda: ops.conv2d(xd, CIN0, pw, planes, 1024, epilogue=L.EPI_HEADQ, **kw))
    else:
        store = torch.full((n, h, w, 1024 + 16), SENTINEL, dtype=dt, device="cuda")
        _, ks = launched_kernels(lambda: ops.conv2d(xd, CIN0, pw, store, 1024, out_coff=8, flags=L.FLAG_RELU | L.FLAG_HEADQ, **kw))
        assert_guards(store, 8, 1024)
        assert_equal(store[..., 8:8 + 1024], q.act.permute(0, 2, 3, 1).contiguous(), "stored activation")
    assert ks == [(V3, (128,))], ks
    assert_equal(planes, q.planes, "tap planes")
    assert bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all()), "a store went outside the tap planes"
    _gather(planes, q, shape)


@pytest.mark.parametrize("shape", [(2, 32, 32), (1, 17, 18), (2, 16, 21)], ids=["w32_gather4", "w18_gather", "w21_gather"])
def test_head_q_gather_exact(shape):
    """pssr_head_q_gather on the reference's tap planes, both kernels (widths that are / are not multiples of 4)"""
    q = headq_case(shape, BF16)
    _gather(q.planes.cuda(), q, shape)


# ---------------------------------------------------------------------------------------------------------------------
# 3. normal random data: the conversions of w and of g * g_scale to 16 bits round.  The float64 reference restates those two roundings
# (w.to(dt); the f32 product g * g_scale, then .to(dt) -- the separate wgrad keeps the f32 product).  Bound: 2 k 2^-24 sum|terms|, plus half
# a storage ulp for a 16-bit result, k = the longest chain of f32 additions a term passes through, an MFMA counted as its K additions.
# At ROUNDING = (2, 64, 3, 24, 40, blk 1): 2 * 2 * 3 = 12 tiles, one per workgroup (no persistent trips).
#   fwd       64 (two 16x16x32 MFMAs over cin = 64) + 9 (bias + nine taps, one after the other) + 1 (the fma of * 128 + 128)      = 74
#   dP        32 (one 16x16x32 MFMA over the 27 (co, tap) slots), then the 16-bit store                                           = 32
#   wgrad     16 (a thread's fma chain: 256 pixels / 16 pixel lanes at cin = 64) + 16 (the lanes' sum) + 12 (atomics, base first)   = 44
#   bwd dW    64 (a wave's four 32x32x16 MFMAs: its four tile rows) + 48 (atomics of 4 waves x 12 workgroups onto the base)         = 112
#   bwd rows  64 (as above; the f64 atomics are exact) + 1 (the fold's rounding to f32)                                             = 65
#   bias_sum  4 (a thread's pieces of one sub-pixel row set: 8 pieces / NS = 2) + 16 (LDS atomics: 64 pixels per (sub-pixel,
#             channel) and tile in groups of 4) + 12 (global atomics)                                                              = 32
#   bias_rows 4 + 16 (the ordered sum over 32 pixel slots x NS = 2, a quarter of them on one sub-pixel) + 1 (the fold)              = 21
#   every bias sum adds the kernel's own 16-bit dact values, which differ from the reference's by up to the dP bound each: that sum of
#   bounds is added.
K_FWD, K_DP, K_WGRAD, K_BWD_DW, K_ROWS_DW, K_BSUM, K_BROWS = 74, 32, 44, 112, 65, 32, 21
U32 = 2.0 ** -24


class Rnd(NamedTuple):
    o: Ops
    out_abs: torch.Tensor       # sum|terms| of out
    dP: torch.Tensor            # f64 NHWC masked reference, unrounded
    dP_tol: torch.Tensor
    dW16: torch.Tensor          # with the gradient rounded to dt (fused backward)
    dW16_abs: torch.Tensor
    dW32: torch.Tensor          # with the f32 product (separate wgrad)
    dW32_abs: torch.Tensor


@functools.lru_cache(maxsize=None)
def rounding_case(dt) -> Rnd:
    c = ROUNDING
    gen = torch.Generator().manual_seed(_seed(*c, str(dt), "normal"))
    act16 = torch.randn(c.n, c.cin, c.h, c.w, generator=gen).to(dt)
    wt = (torch.randn(c.cout, c.cin, 3, 3, generator=gen) / (9 * c.cin) ** 0.5)
    bias, g, base = torch.randn(c.cout, generator=gen), torch.randn(c.n, c.cout, c.h, c.w, generator=gen), torch.randn(c.cout, c.cin, 3, 3, generator=gen)
    act, w16 = act16.double(), wt.to(dt).double()
    g32 = g * torch.tensor(c.gs, dtype=F32)                  # the f32 product, as the kernels form it
    g16 = g32.to(dt).double()
    conv, dP, dW16 = head_refs(act, w16, g16)
    conv_abs, dP_abs, dW16_abs = head_refs(act.abs(), w16.abs(), g16.abs())
    _, _, dW32 = head_refs(act, w16, g32.double())
    _, _, dW32_abs = head_refs(act.abs(), w16.abs(), g32.double().abs())
    b = bias.double().view(1, -1, 1, 1)
    out = (conv + b) * 128 + 128
    out_abs = (conv_abs + b.abs()) * 128 + 128
    mask = (act > 0).permute(0, 2, 3, 1)
    dPm = torch.where(mask, dP.permute(0, 2, 3, 1), torch.zeros((), dtype=torch.float64)).contiguous()
    dP_tol = torch.where(mask, 2 * K_DP * U32 * dP_abs.permute(0, 2, 3, 1) + 0.5 * storage_ulp(dP.permute(0, 2, 3, 1), dt), torch.zeros((), dtype=torch.float64))
    o = Ops(act16, wt, bias, g, out, None, None, 0.0, base, None, None, None)
    return Rnd(o, out_abs, dPm, dP_tol, dW16, dW16_abs + base.double().abs(), dW32, dW32_abs + base.double().abs())


def assert_within(got, ref, tol, what):
    got, ref, tol = (torch.as_tensor(t).double().cpu() for t in (got, ref, tol))
    assert got.shape == ref.shape == tol.shape, (what, got.shape, ref.shape, tol.shape)
    err = (got - ref).abs()
    ratio = (err / tol.clamp_min(1e-300))[tol > 0].max().item()
    print(f"{what}: max err/bound {ratio:.3g} (max err {err.max().item():.3g})")
    assert bool((err <= tol).all()), (what, ratio)


@pytest.mark.parametrize("dt", DT16, ids=["bfloat16", "float16"])
@pytest.mark.parametrize("entry", ["fwd", "dgrad", "wgrad", "bwd", "bwd_rows"])
def test_rounding_of_the_operand_conversions(entry, dt):
    from pssr2_amd import ops
    c, r = ROUNDING, rounding_case(dt)
    o = r.o
    d = Dev(c, dt, o)
    base = o.base.double()
    bs_ref, bs_abs, bs_tols = bias_sums(r.dP, c.blk), bias_sums(r.dP.abs(), c.blk), bias_sums(r.dP_tol, c.blk)
    if entry == "fwd":
        out = d.buf(o.out.shape)
        run("fwd", d, out=out, bias=d.bias)
        assert_within(out, o.out, 2 * K_FWD * U32 * r.out_abs, f"fwd {dt} k={K_FWD}")
    elif entry == "dgrad":
        run("dgrad", d)
        assert_within(d.got_dact(), r.dP, r.dP_tol, f"dgrad dact {dt} k={K_DP}")
    elif entry == "wgrad":
        dw = d.buf(base.shape, init=o.base)
        run("wgrad", d, dw=dw)
        assert_within(dw, base + r.dW32, 2 * K_WGRAD * U32 * r.dW32_abs, f"wgrad dw {dt} k={K_WGRAD}")
    elif entry == "bwd":
        dw, bsum = d.buf(base.shape, init=o.base), d.buf(bs_ref.shape, init=torch.zeros(()))
        ks = run("bwd", d, dw=dw, bias_sum=bsum)
        assert ks == [(BWD, (4, 1, 0))], ks
        assert_within(d.got_dact(), r.dP, r.dP_tol, f"bwd dact {dt} k={K_DP}")
        assert_within(dw, base + r.dW16, 2 * K_BWD_DW * U32 * r.dW16_abs, f"bwd dw {dt} k={K_BWD_DW}")
        assert_within(bsum, bs_ref, bs_tols + 2 * K_BSUM * U32 * bs_abs, f"bwd bias_sum {dt} k={K_BSUM}")
    else:
        dw_rows = d.buf((STAT_ROWS,) + base.shape, torch.float64, init=torch.zeros(()))
        bias_rows = d.buf((STAT_ROWS,) + bs_ref.shape, torch.float64, init=torch.zeros(()))
        ks = run("bwd_rows", d, dw_rows=dw_rows, bias_rows=bias_rows)
        assert ks == [(BWD, (4, 1, 0))], ks
        assert_within(d.got_dact(), r.dP, r.dP_tol, f"bwd_rows dact {dt} k={K_DP}")
        dw_abs = r.dW16_abs - base.abs()
        assert_within(fold_stat_rows(dw_rows, 4), r.dW16, 2 * (K_ROWS_DW - 1) * U32 * dw_abs, f"bwd_rows dw_rows in f64 {dt} k={K_ROWS_DW - 1}")
        assert_within(fold_stat_rows(bias_rows, 1), bs_ref, bs_tols + 2 * (K_BROWS - 1) * U32 * bs_abs, f"bwd_rows bias_rows in f64 {dt} k={K_BROWS - 1}")
        dw, bs = torch.empty(base.shape, device="cuda"), torch.empty(bs_ref.shape, device="cuda")
        ops.f64_to_f32(dw_rows, dw)
        ops.f64_to_f32(bias_rows, bs)
        assert_within(dw, r.dW16, 2 * K_ROWS_DW * U32 * dw_abs, f"bwd_rows f64_to_f32(dw_rows) {dt} k={K_ROWS_DW}")
        assert_within(bs, bs_ref, bs_tols + 2 * K_BROWS * U32 * bs_abs, f"bwd_rows f64_to_f32(bias_rows) {dt} k={K_BROWS}")
    d.check_guards()
