"""Helpers for the bit-exact convolution tests (tests/test_gpu_conv_exact.py, tests/test_conv_exact_helpers.py).

The idea: operands are dyadic numbers with few significant bits, so that every product and every partial sum of the GEMM is exact
in f32 whatever the summation order (MFMA, split-K, atomics).  The f32 accumulator then holds the exact value, and a 16-bit store
must hold exactly the float64 reference rounded once, to nearest even.  No tolerances: any difference is a bug.

`Grid(e, m)` describes a set of values: multiples of 2**-e with magnitude at most m.  `assert_exact_premise` walks a convolution's
arithmetic on such grids and fails when an intermediate value could need more than 24 significant bits.
"""
from __future__ import annotations

import contextlib
import functools
import math
import re
import zlib
from pathlib import Path
from typing import NamedTuple

import pytest
import torch

F32_BITS = 24
STORAGE_BITS = {torch.float32: 24, torch.bfloat16: 8, torch.float16: 11}
F16_MAX, F16_MIN_NORMAL_E = 65504.0, 14

# the conv tunables at their table defaults (pssr2_amd/csrc/api_common.cpp)
PRODUCTION_TUNABLES = {
    "IGEMM_FLAT": 1, "IGEMM_BIG": 1, "IGEMM_V3": 1, "IGEMM_V3_64": 1, "IGEMM_N64": 1, "IGEMM_KSPLIT": 384, "CONV_EPI8": 1,
    "WGRAD_LEAN": 1, "WGRAD_X2": 0, "WGRAD_DMA": 1, "WGRAD_BLOCKS": 256, "WGRAD_BLOCKS_1X1": 384,
}


# ---------------------------------------------------------------------------------------------------------------------
# value grids and the premise check
class Grid(NamedTuple):
    e: int          # values are multiples of 2**-e
    m: float        # ... with magnitude at most m

    def __mul__(self, o):
        return Grid(self.e + o.e, self.m * o.m)

    def __add__(self, o):
        return Grid(max(self.e, o.e), self.m + o.m)

    def sum(self, k):
        return Grid(self.e, k * self.m)

    def units(self):
        """largest magnitude in units of the grid step: the value set fits p significant bits if this is <= 2**p"""
        return self.m * 2.0 ** self.e


X_GRID = Grid(2, 1.0)           # activations, residuals, data gradients: multiples of 1/4 in [-1, 1]
W_GRID = Grid(4, 0.5)           # weights: multiples of 1/16 in [-1/2, 1/2]
B_GRID = Grid(6, 1.0)           # bias: multiples of 1/64 in [-1, 1]
SCALE_GRID = Grid(1, 2.0)       # BatchNorm scales from {1/2, 1, 3/2, 2}
SHIFT_GRID = Grid(2, 1.0)       # shifts: multiples of 1/4 in [-1, 1]
SCALES = (0.5, 1.0, 1.5, 2.0)


def _fits(g: Grid, bits: int, what: str):
    assert g.units() <= 2.0 ** bits, f"exactness premise broken: {what} {g} needs more than {bits} significant bits"


def _storable(g: Grid, dt, what: str):
    _fits(g, STORAGE_BITS[dt], f"{what} in {dt}")
    if dt == torch.float16:
        assert g.m <= F16_MAX and g.e <= F16_MIN_NORMAL_E, f"{what} {g} leaves the normal float16 range"


def assert_exact_premise(k, x=X_GRID, w=W_GRID, *, dt=torch.bfloat16, pro=None, bias=None, affine=None, tail=None, final=None):
    """Check that a convolution whose dot products have length `k`, over operands on grids `x` and `w`, is computed exactly in f32.
    pro=(scale, shift): relu(x * scale + shift), rounded to `dt` before the multiply (so it must be storable); bias: grid of the bias;
    affine=(scale, shift): (acc + bias) * scale + shift; tail=(aux, scale, shift): acc + aux * scale + shift; final=(out_scale,
    out_shift): the f32 output transform.  A 16-bit result is rounded by the store: only its float16 range is checked.  Returns the
    grid of the f32 result."""
    _storable(x, dt, "input")
    _storable(w, dt, "weight")
    if pro is not None:
        x = x * pro[0] + pro[1]
        _fits(x, F32_BITS, "prologue")
        _storable(x, dt, "prologue output")
    acc = (x * w).sum(k)
    _fits(acc, F32_BITS, f"accumulator (K = {k})")
    if bias is not None:
        acc = acc + bias
        _fits(acc, F32_BITS, "accumulator + bias")
    if affine is not None:
        acc = acc * affine[0] + affine[1]
        _fits(acc, F32_BITS, "affine epilogue")
    if tail is not None:
        acc = acc + (tail[0] * tail[1] + tail[2])
        _fits(acc, F32_BITS, "tail epilogue")
    if final is not None:
        acc = acc * final[0] + final[1]
        _fits(acc, F32_BITS, "final epilogue")
    if dt == torch.float16:
        assert acc.m <= F16_MAX, f"output {acc} overflows float16"
    return acc


# ---------------------------------------------------------------------------------------------------------------------
# operands and the reference
def dyadic(gen, shape, g: Grid):
    """float64 values on grid g, uniform over its integers"""
    q = int(g.m * 2 ** g.e)
    return torch.randint(-q, q + 1, shape, generator=gen, dtype=torch.int64).double() / 2.0 ** g.e


def pick(gen, shape, values):
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), shape, generator=gen)]


def expected(ref: torch.Tensor, dt) -> torch.Tensor:
    """What a kernel must store for the float64 reference `ref`: asserts that ref is exact in f32 (the premise on the actual data),
    then rounds once, to nearest even, into the storage type."""
    assert ref.dtype == torch.float64
    r32 = ref.float()
    assert torch.equal(r32.double(), ref), "reference is not exact in f32: the operands break the exactness premise"
    return r32.to(dt)


def stable_seed(*key):
    """a generator seed that depends on the key alone (hash() of a string changes from process to process)"""
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


MEAN_GRID = Grid(2, 0.5)


def per_channel(key, c):
    """BatchNorm-like per-channel constants on the exact grids: scale, shift (both signs), mean, invstd"""
    g = torch.Generator().manual_seed(stable_seed(key, c))
    return pick(g, (c,), SCALES), dyadic(g, (c,), SHIFT_GRID), dyadic(g, (c,), MEAN_GRID), pick(g, (c,), (0.5, 1.0, 2.0))


def nchw(t):
    return t.view(1, -1, 1, 1)


def dev(t):
    return t.float().contiguous().cuda()


def assert_equal(got, want, what=""):
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {want.numel()} values differ; first at {i}: got {got[i].item()!r}, "
                             f"want {want[i].item()!r}")


# ---------------------------------------------------------------------------------------------------------------------
# layouts
SENTINEL = -7.0


def nhwc(x: torch.Tensor, dt, *, coff=0, cstride=None, blk=0, sentinel=SENTINEL, device="cuda"):
    """NCHW tensor -> [n, h, w, cstride] buffer of dtype dt holding x at channels coff.., the guard channels on both sides filled with
    `sentinel`; blk > 0: the pixels in the blocked order of that log2 block size."""
    n, c, h, w = x.shape
    cstride = coff + c if cstride is None else cstride
    buf = torch.full((n, h, w, cstride), sentinel, dtype=dt)
    buf[..., coff:coff + c] = x.permute(0, 2, 3, 1).to(dt)
    return to_blocked(buf, blk).to(device)


def assert_guards(buf: torch.Tensor, coff, c, sentinel=SENTINEL):
    """the channels of buf outside [coff, coff + c) still hold the sentinel"""
    b = buf.cpu()
    assert bool((b[..., :coff] == sentinel).all()), "a store went below the channel window"
    assert bool((b[..., coff + c:] == sentinel).all()), "a store went past the channel window"


def pix_index(gi, gy, gx, H, W, blk):
    """position of pixel (gi, gy, gx) in the blocked order of log2 block size blk (pix_index, pssr2_amd/csrc/common.h)"""
    if blk == 0:
        return (gi * H + gy) * W + gx
    R = 1 << blk
    return (((gi * (H >> blk) + (gy >> blk)) * (W >> blk) + (gx >> blk)) << (2 * blk)) + ((gy & (R - 1)) << blk) + (gx & (R - 1))


def to_blocked(t: torch.Tensor, blk):
    """[n, h, w, c] in plain order -> the same shape with the pixels in blocked order"""
    if blk == 0:
        return t
    n, h, w, c = t.shape
    R = 1 << blk
    return t.reshape(n, h // R, R, w // R, R, c).permute(0, 1, 3, 2, 4, 5).reshape(n, h, w, c).contiguous()


def from_blocked(t: torch.Tensor, blk):
    if blk == 0:
        return t
    n, h, w, c = t.shape
    R = 1 << blk
    return t.reshape(n, h // R, w // R, R, R, c).permute(0, 1, 3, 2, 4, 5).reshape(n, h, w, c).contiguous()


def shuf2_perm(cout):
    """FLAG_SHUF2 row order: packed row s * cout / 4 + c holds torch channel 4 c + s"""
    q = cout // 4
    return torch.tensor([4 * c + s for s in range(4) for c in range(q)], dtype=torch.int64)


# ---------------------------------------------------------------------------------------------------------------------
# which kernels ran
_MANGLED = re.compile(r"^_ZN(?:\d+_GLOBAL__N_1)?(\d+)")
_MANGLED_INT = re.compile(r"L[ijlmsb](n?\d+)E")
_DEMANGLED = re.compile(r"([A-Za-z_]\w*)<([^<>]*)>")


def parse_kernel_name(name: str):
    """kernel name (Itanium-mangled or demangled) -> (family, integer template arguments), or None for a non-template name"""
    m = _MANGLED.match(name)
    if m:
        ln = int(m.group(1))
        fam, rest = name[m.end():m.end() + ln], name[m.end() + ln:]
        if not rest.startswith("I"):
            return None
        targs = rest.split("EEv", 1)[0] + "E"
        return fam, tuple(int(v.replace("n", "-")) for v in _MANGLED_INT.findall(targs))
    m = _DEMANGLED.search(name)
    if not m:
        return None
    ints = []
    for a in m.group(2).split(","):
        a = a.strip()
        if re.fullmatch(r"-?\d+[uUlL]*", a):
            ints.append(int(a.rstrip("uUlL")))
        elif a in ("true", "false"):
            ints.append(int(a == "true"))
    return m.group(1), tuple(ints)


def is_conv_kernel(parsed):
    return parsed is not None and parsed[0].startswith("conv_") and parsed[0].endswith("_kernel")


def is_head_kernel(parsed):
    """the templated kernels of csrc/head_conv.hip (the two head_q_gather kernels have no template arguments: see plain_kernel_names)"""
    return parsed is not None and parsed[0].startswith("head_") and parsed[0].endswith("_kernel")


_SYMBOL = re.compile(rb"_ZN[0-9A-Za-z_]*?_kernelI[0-9A-Za-z_]+")


def kernel_name_table(symbols, demangle):
    """{name as a profiler may report it: (family, ints)} for mangled kernel symbols.  A profiler reports a kernel under its mangled
    name or under what its demangler makes of it, and an old demangler garbles some names beyond parsing: it reads the `DF16b` of
    __bf16 followed by a small integer literal as a fixed-point type (head_fwd_kernel<__bf16, 1, 1> comes out as
    head_fwd_kernel<bool _Accum, int, E, 1>).  So every symbol is passed through the same demangler and looked up by the result; a
    name that two different kernels share maps to None."""
    table = {}
    for s in symbols:
        p = parse_kernel_name(s)
        if p is None:
            continue
        for name in {s, demangle(s)}:
            if table.setdefault(name, p) != p:
                table[name] = None
    return table


@functools.lru_cache(maxsize=None)
def library_kernel_table():
    """kernel_name_table of the template kernels in the built library, through this process's demangler"""
    from pssr2_amd import _lib as L
    data = Path(L._LIB_PATH).read_bytes()
    return kernel_name_table(sorted({m.group(0).decode() for m in _SYMBOL.finditer(data)}), torch._C._demangle)


def launched_kernels(fn, select=is_conv_kernel):
    """Run fn() under torch.profiler; returns (its result, the sorted (family, ints) of this library's kernels that ran and that the
    predicate `select` accepts: the convolution kernels unless told otherwise).  Fails -- never skips -- when the profiler reports none."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        res = fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    table = library_kernel_table()
    parsed = []
    for n in names:
        assert table.get(n, ()) is not None, f"the profiler's name {n!r} stands for more than one kernel of the library"
        parsed.append(table[n] if n in table else parse_kernel_name(n))
    ks = sorted(p for p in parsed if select(p))
    assert ks, f"the profiler reported no selected kernel of this library (events: {sorted(set(names))[:20]})"
    return res, ks


# ---------------------------------------------------------------------------------------------------------------------
# the Reconstruction head (csrc/head_conv.hip): grids, premise, references
HEAD_TS = 16                    # tile edge of every head kernel
HEAD_BWD_GRID, HEAD_WGRAD_GRID = 512, 1024      # workgroup caps of the persistent kernels (head_conv_bwd_impl, pssr_head_conv_wgrad)
STAT_ROWS, STAT_HI_ROWS = 64, 32                # PSSR_STAT_ROWS; rows [0, 32) hold the multiple-of-2^-20 pieces, [32, 64) the remainders


def scaled(g: Grid, s: float) -> Grid:
    """The grid of g's values times the exact scalar s = k * 2**j (k an odd integer).  The significant bits are counted, not
    magnitude / step: a power of two shifts the exponent (k = 1, units() unchanged), any other scale costs the bits of k."""
    assert s != 0 and s == float(s)
    k, j = abs(float(s)), 0
    while k != int(k):
        k, j = k * 2, j - 1
    while int(k) % 2 == 0:
        k, j = k / 2, j + 1
    return Grid(g.e - j, g.m * abs(s))


def head_weight_grid(dt) -> Grid:
    """head weights: (storage bits - 1) fractional bits in [-1/2, 1/2] -- exactly representable, and the products need rounding often"""
    return Grid(STORAGE_BITS[dt] - 1, 0.5)


class HeadGrids(NamedTuple):
    out: Grid       # forward output (conv + bias) * 128 + 128
    dP: Grid        # data gradient before the 16-bit store
    dW: Grid        # weight gradient (without the pre-existing gradient)


def assert_head_premise(cin, cout, pixels, g_scale, *, dt, x=X_GRID, g=X_GRID, bias=B_GRID) -> HeadGrids:
    """Walk the arithmetic of the head kernels on the grids of the tests: activations x, weights head_weight_grid(dt), gradient g times
    g_scale (an f32 product, then -- dgrad, fused backward -- converted to dt), `pixels` = n * h * w terms per weight-gradient sum."""
    w = head_weight_grid(dt)
    out = assert_exact_premise(9 * cin, x, w, dt=torch.float32, bias=bias, final=(Grid(-7, 128.0), Grid(-7, 128.0)))
    _storable(x, dt, "activation")
    _storable(w, dt, "weight")
    gs = scaled(g, g_scale)
    _fits(gs, F32_BITS, "g * g_scale")
    _storable(gs, dt, "g * g_scale")
    dP = (gs * w).sum(9 * cout)
    _fits(dP, F32_BITS, "dP accumulator")
    if dt == torch.float16:
        assert dP.m <= F16_MAX, f"dP {dP} overflows float16"
    dW = (gs * x).sum(pixels)
    _fits(dW, F32_BITS, f"dW accumulator ({pixels} pixels)")
    return HeadGrids(out, dP, dW)


def stored_grid(g: Grid, dt) -> Grid:
    """the grid of g's values after the 16-bit store: still multiples of g's step, the largest magnitude rounded like any other"""
    return Grid(g.e, float(torch.tensor(g.m, dtype=torch.float64).to(dt)))


def assert_headq_premise(k, x: Grid, w: Grid, b: Grid, hw: Grid, hb: Grid, *, dt):
    """The fused head of `pre` (conv_headq_epilogue + pssr_head_q_gather): relu(acc + b) of a convolution with dot products of length
    k, rounded to dt; times the head weights hw (converted to dt), summed over the 64 channels of a sub-pixel in f32 (a tap plane);
    nine planes and the head bias hb summed, * 128 + 128.  Returns the grids (activation, tap plane, output)."""
    acc = assert_exact_premise(k, x, w, dt=dt, bias=b)
    act = stored_grid(acc, dt)
    _storable(hw, dt, "head weight")
    plane = (act * hw).sum(64)
    _fits(plane, F32_BITS, "tap plane")
    out = plane.sum(9) + hb
    _fits(out, F32_BITS, "gathered sum + bias")
    out = out * Grid(-7, 128.0) + Grid(-7, 128.0)
    _fits(out, F32_BITS, "output")
    return act, plane, out


def sum_fits(g: Grid, count) -> bool:
    """an f32 sum of `count` values of grid g is exact whatever its order"""
    return g.sum(count).units() <= 2.0 ** F32_BITS


def needs_rounding(ref: torch.Tensor, dt) -> float:
    """share of the float64 values that the storage type cannot hold (the 16-bit store has to round them)"""
    return float((ref.to(dt).double() != ref).double().mean())


def storage_ulp(ref: torch.Tensor, dt) -> torch.Tensor:
    """spacing of the storage type at |ref| (float64), the subnormal spacing below the smallest normal number"""
    emin = {torch.bfloat16: -126, torch.float16: -14, torch.float32: -126}[dt]
    _, e = torch.frexp(ref.abs().clamp_min(2.0 ** emin))          # |ref| = m 2^e, m in [0.5, 1)
    return torch.exp2((e - STORAGE_BITS[dt]).double())


def head_refs(act, wt, g):
    """float64 references of the three head operations on NCHW / OIHW float64 operands (g already scaled): the 3x3 convolution of
    act, the data gradient (no mask) and the weight gradient"""
    import torch.nn.functional as F
    conv = F.conv2d(act, wt, padding=1)
    dP = F.conv_transpose2d(g, wt, padding=1)
    dW = torch.nn.grad.conv2d_weight(act, wt.shape, g, padding=1)
    return conv, dP, dW


def head_tiles(n, h, w):
    tx, ty = -(-w // HEAD_TS), -(-h // HEAD_TS)
    return n * ty * tx, ty, tx


def later_trip_mask(n, h, w, grid):
    """[n, 1, h, w] mask of the pixels in tiles whose index (img, tile row, tile column) is >= grid: the tiles a persistent kernel of
    `grid` workgroups reaches on its second and later trips"""
    _, ty, tx = head_tiles(n, h, w)
    img = torch.arange(n).view(n, 1, 1)
    yy = (torch.arange(h) // HEAD_TS).view(1, h, 1)
    xx = (torch.arange(w) // HEAD_TS).view(1, 1, w)
    return (((img * ty + yy) * tx + xx) >= grid).view(n, 1, h, w)


def fold_stat_rows(rows: torch.Tensor, addends: int) -> torch.Tensor:
    """rows: float64 [STAT_ROWS, ...] as stat_add (csrc/common.h) leaves them, every slot having received at most `addends` values.
    Checks the two pieces -- rows [0, 32) multiples of 2^-20, rows [32, 64) multiples of 2^-64 of magnitude below 2^-21 per addend --
    and returns the float64 sum over the rows."""
    r = rows.detach().cpu().reshape(STAT_ROWS, -1)
    hi, lo = r[:STAT_HI_ROWS], r[STAT_HI_ROWS:]
    assert torch.equal(hi * 2.0 ** 20, (hi * 2.0 ** 20).round()), "a stripe row holds something finer than 2^-20"
    assert torch.equal(lo * 2.0 ** 64, (lo * 2.0 ** 64).round()), "a remainder row holds something finer than 2^-64"
    assert float(lo.abs().max()) <= addends * 2.0 ** -21, "a remainder row holds more than its addends can bring"
    return r.sum(0).reshape(rows.shape[1:])


def mask_edge_values(dt):
    """activations around the ReLU mask's decision, built from their bit patterns: +0, -0, +-smallest subnormal, +-smallest normal,
    -1, +1, largest finite"""
    bits = {torch.bfloat16: [0x0000, 0x8000, 0x0001, 0x8001, 0x0080, 0x8080, 0xBF80, 0x3F80, 0x7F7F],
            torch.float16: [0x0000, 0x8000, 0x0001, 0x8001, 0x0400, 0x8400, 0xBC00, 0x3C00, 0x7BFF]}[dt]
    return torch.tensor([b - 65536 if b >= 32768 else b for b in bits], dtype=torch.int16).view(dt)


# ---------------------------------------------------------------------------------------------------------------------
# the weight gradient (csrc/conv_wgrad.hip) and its unpack pass (csrc/pack.hip)
def tiles_per_workgroup(n_tiles, split):
    """pixel tiles each of the `split` workgroups of one slab walks: workgroup b takes tiles b, b + split, ..."""
    return [len(range(b, n_tiles, split)) for b in range(split)]


def unpack_map(mode, cout, cin, ks, k_pad, *, ci_begin=0, ci_count=None, n_perm=None):
    """Where pssr_unpack_conv_wgrad_parts puts element [n][tap][k] of a packed gradient f32 [rows][taps][k_pad] (taps = ks * ks in mode
    0, else 1): int64 [cout, taps, k_pad] of flat indices into the OIHW gradient [cout, cin, ks, ks], -1 where the element is
    discarded.  Written from the layouts in include/pssr_mi355.h:
      mode 0  K = input channel - ci_begin, one slice per tap; row n is output channel n_perm[n]
      mode 2  K = (input channel - ci_begin) * ks * ks + tap; row n is output channel n_perm[n]
      mode 4  K = tap * cpad + input channel, cpad = cin rounded up to 16 (no channel window, no permutation)"""
    kk = ks * ks
    taps = kk if mode == 0 else 1
    ci_count = cin - ci_begin if ci_count is None else ci_count
    n = torch.arange(cout).view(cout, 1, 1)
    tap = torch.arange(taps).view(1, taps, 1)
    k = torch.arange(k_pad).view(1, 1, k_pad)
    co = n if n_perm is None else n_perm.long().view(cout, 1, 1)
    if mode == 0:
        ci, tp, ok = ci_begin + k, tap, k < ci_count
    elif mode == 2:
        ci, tp, ok = ci_begin + k // kk, k % kk, k < ci_count * kk
    elif mode == 4:
        assert ci_begin == 0 and ci_count == cin and n_perm is None
        cpad = (cin + 15) // 16 * 16
        ci, tp = k % cpad, k // cpad
        ok = (tp < kk) & (ci < cin)
    else:
        raise ValueError(mode)
    idx = (co * cin + ci) * kk + tp
    return torch.where(ok.expand_as(idx), idx, torch.full_like(idx, -1))


def unpack_reference(parts, dest, umap, accumulate):
    """float64 result of the unpack pass: parts [parts, rows, taps, k_pad] summed over the parts and scattered by `umap` into a copy of
    the OIHW tensor `dest` (added to it when `accumulate`); what the map does not address keeps its value"""
    cout = umap.shape[0]
    sel = umap >= 0
    idx = umap[sel]
    assert idx.unique().numel() == idx.numel(), "the map addresses a destination element twice"
    s = parts[:, :cout].sum(0)[sel]
    out = dest.clone().reshape(-1)
    out[idx] = (out[idx] + s) if accumulate else s
    return out.view_as(dest)


# ---------------------------------------------------------------------------------------------------------------------
# the weight pack (csrc/pack.hip: pssr_pack_conv_weight, pssr_pack_conv_weight_batch)
def pack_eps(dtype):
    """(EPS, KCH) of a storage type (include/pssr_mi355.h): elements per 16-byte slot, K indices per chunk"""
    eps = 16 // torch.empty(0, dtype=dtype).element_size()
    return eps, 2 * eps


def pack_dims(mode, cout, cin, ks, ci_count):
    """(taps, GEMM-K, GEMM-N) of a packing mode"""
    kk = ks * ks
    s2d = kk * ((cin + 15) // 16 * 16)
    gk = {0: ci_count, 1: cout, 2: ci_count * kk, 3: cout, 4: s2d, 5: cout}[mode]
    gn = {0: cout, 1: ci_count, 2: cout, 3: ci_count * kk, 4: cout, 5: s2d}[mode]
    return (kk if mode < 2 else 1), gk, gn


def pack_map(mode, cout, cin, ks, k_pad, n_pad, dtype, *, ci_begin=0, ci_count=None, n_perm=None, center=False):
    """Which source element every element of a packed weight holds: int64 [taps * k_pad * n_pad] in packed order
    packed[chunk][tap][n][slot][e] of flat indices into the OIHW tensor [cout, cin, ks, ks]; -1 is padding (stored as +0).  Written
    from the layouts in include/pssr_mi355.h:
      position -> (k, tap, n): the slot at byte offset 16 s of column n holds half h = s ^ ((n >> 3) & 1) of the chunk, so
                  k = chunk * KCH + h * EPS + e
      mode 0  K = input channel - ci_begin, N = output channel n_perm[n], one slice per tap
      mode 1  K = output channel n_perm[k], N = input channel - ci_begin, slice `tap` holds kernel tap ks * ks - 1 - tap
      mode 2  one slice; K = (input channel - ci_begin) * ks * ks + tap, N = output channel n_perm[n]
      mode 3  its transpose: K = output channel n_perm[k], N = the flat index
      mode 4  one slice; K = tap * cpad + input channel, cpad = cin rounded up to 16, N = output channel (no window, no permutation)
      mode 5  its transpose
    center (modes 2 / 3, ks = 3): the source is a 1x1 weight [cout, cin, 1, 1] standing for the centre tap of a 3x3 kernel."""
    eps, kch = pack_eps(dtype)
    kk = ks * ks
    ci_count = cin - ci_begin if ci_count is None else ci_count
    taps = kk if mode < 2 else 1
    assert k_pad % kch == 0 and n_pad % 128 == 0
    assert not center or (mode in (2, 3) and ks == 3)
    chunk = torch.arange(k_pad // kch).view(-1, 1, 1, 1, 1)
    tap = torch.arange(taps).view(1, -1, 1, 1, 1)
    n = torch.arange(n_pad).view(1, 1, -1, 1, 1)
    s = torch.arange(2).view(1, 1, 1, 2, 1)
    e = torch.arange(eps).view(1, 1, 1, 1, -1)
    k = chunk * kch + (s ^ ((n >> 3) & 1)) * eps + e
    k, tap, n = torch.broadcast_tensors(k, tap, n)
    if mode in (1, 3, 5):       # the transposed forms: the output channel runs along K
        o, i = k, n
    else:
        o, i = n, k
    if mode in (0, 1):
        ci, tp, ok = ci_begin + i, (tap if mode == 0 else kk - 1 - tap), i < ci_count
    elif mode in (2, 3):
        ci, tp, ok = ci_begin + i // kk, i % kk, i < ci_count * kk
    elif mode in (4, 5):
        assert ci_begin == 0 and ci_count == cin and n_perm is None
        cpad = (cin + 15) // 16 * 16
        ci, tp = i % cpad, i // cpad
        ok = (tp < kk) & (ci < cin)
    else:
        raise ValueError(mode)
    ok = ok & (o < cout)
    co = o if n_perm is None else n_perm.long()[o.clamp(max=cout - 1)]
    if center:
        idx, ok = co * cin + ci, ok & (tp == 4)
    else:
        idx = (co * cin + ci) * kk + tp
    return torch.where(ok, idx, torch.full_like(idx, -1)).reshape(-1)


def pack_reference(w, pmap, dtype):
    """what the pack must store: the source elements gathered by `pmap` and converted with torch (round to nearest even), +0 where
    the map says padding"""
    out = torch.zeros(pmap.numel(), dtype=dtype)
    sel = pmap >= 0
    out[sel] = w.reshape(-1)[pmap[sel]].to(dtype)
    return out


def packed_matrices(packed, taps, k_pad, n_pad, dtype):
    """de-swizzle a packed weight (flat, packed order) to the per-tap GEMM matrices B[tap][k][n]; `dtype` gives EPS and KCH (the
    tensor itself may hold anything, float64 values or indices)"""
    eps, kch = pack_eps(dtype)
    p = packed.view(k_pad // kch, taps, n_pad, 2, eps)
    flip = ((torch.arange(n_pad) >> 3) & 1).bool()
    halves = torch.where(flip.view(1, 1, -1, 1, 1), p.flip(3), p)          # [chunk][tap][n][half][e]
    return halves.permute(1, 0, 3, 4, 2).reshape(taps, k_pad, n_pad)


def pack_position(i, taps, n_pad, dtype):
    """flat packed index -> (chunk, tap, n, slot, e)"""
    eps, _ = pack_eps(dtype)
    i, e = divmod(int(i), eps)
    i, s = divmod(i, 2)
    i, n = divmod(i, n_pad)
    chunk, tap = divmod(i, taps)
    return chunk, tap, n, s, e


def assert_packed_equal(got_bytes, want, taps, n_pad, what=""):
    """got_bytes: the uint8 buffer of a packed weight; want: pack_reference's tensor.  Bytewise: padding must be +0, not -0, and every
    byte of the buffer must have been written."""
    got = got_bytes.cpu().view(want.dtype)
    assert got.numel() == want.numel(), f"{what}: {got.numel()} packed elements, want {want.numel()}"
    ibits = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[want.element_size()]
    gb, wb = got.view(ibits), want.view(ibits)
    if not torch.equal(gb, wb):
        bad = (gb != wb).nonzero().view(-1)
        i = int(bad[0])
        mask = (1 << (8 * want.element_size())) - 1
        raise AssertionError(f"{what}: {len(bad)} of {want.numel()} packed elements differ; first at (chunk, tap, n, slot, e) = "
                             f"{pack_position(i, taps, n_pad, want.dtype)}: got {got[i].item()!r} (bits {int(gb[i]) & mask:#x}), "
                             f"want {want[i].item()!r} (bits {int(wb[i]) & mask:#x})")


# f32 bit patterns the pack has to convert or carry right, for every storage type
PACK_EDGE_BITS = (
    0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,     # bf16 ties: +-(1 + 2^-8) -> 1 (even), +-(1 + 3 2^-8) -> 1 + 2^-6
    0x3F801000, 0x3F803000, 0xBF801000, 0xBF803000,     # f16 ties: +-(1 + 2^-11) -> 1, +-(1 + 3 2^-11) -> 1 + 2^-9
    0x3F808001, 0x3F807FFF, 0x3F801001, 0x3F800FFF,     # one f32 ulp above / below a tie
    0x80000000, 0x00000000,                             # -0.0, +0.0
    0x00010000, 0x80010000, 0x7F7F0000, 0xFF7F0000,     # bf16: smallest subnormal 2^-133, largest finite
    0x00008000, 0x00018000, 0x0000C000,                 # bf16 subnormal ties (-> 0, -> 2 steps) and 3/4 of a step (-> 1 step)
    0x33800000, 0xB3800000, 0x477FE000, 0xC77FE000,     # f16: smallest subnormal 2^-24, largest finite 65504
    0x33000000, 0x33C00000, 0x33000001,                 # f16 subnormal ties 2^-25 (-> 0), 3 2^-25 (-> 2^-23), just above the first
    0x477FF000, 0x477FEFFF, 0xC77FF000,                 # 65520 -> f16 inf, 65519.996 -> 65504, -65520 -> -inf
    0x00000001, 0x80000001, 0x00400000, 0x007FFFFF,     # f32 subnormals
    0x7F7FFFFF, 0xFF7FFFFF, 0x00800000,                 # f32 largest finite, smallest normal
)


def pack_source(key, shape, pmap, *, nan_outside=False):
    """f32 OIHW source of a pack test: seeded normal values, PACK_EDGE_BITS at evenly spread elements that `pmap` addresses, and
    (nan_outside) NaN in every element it does not address"""
    g = torch.Generator().manual_seed(stable_seed("pack", key))
    w = torch.randn(shape, generator=g, dtype=torch.float32)
    flat = w.view(-1)
    addressed = pmap[pmap >= 0].unique()
    edge = torch.tensor([b - (1 << 32) if b >= 1 << 31 else b for b in PACK_EDGE_BITS], dtype=torch.int64).to(torch.int32).view(torch.float32)
    assert addressed.numel() >= edge.numel()
    flat[addressed[torch.arange(edge.numel()) * (addressed.numel() // edge.numel())]] = edge
    if nan_outside:
        outside = torch.ones(flat.numel(), dtype=torch.bool)
        outside[addressed] = False
        flat[outside] = float("nan")
    return w


def gelu64(z):
    return 0.5 * z * (1.0 + torch.special.erf(z / math.sqrt(2.0)))


GELU16_ERR = 7e-6       # the error bound csrc/common.h states for the polynomial GELU of the 16-bit builds


def gelu_exact_inputs(dt):
    """The z = k / 8, |k| <= 32, for which the 16-bit GELU prologue stages a known value: gelu(z) +- 2 * GELU16_ERR (the factor 2 for
    the f32 evaluation) rounds to one number of the storage type.  z = 0 is kept too: the kernel maps it to exactly 0."""
    z = torch.arange(-32, 33, dtype=torch.float64) / 8
    g = gelu64(z)
    keep = ((g - 2 * GELU16_ERR).float().to(dt) == (g + 2 * GELU16_ERR).float().to(dt)) | (z == 0)
    return z[keep]


# ---------------------------------------------------------------------------------------------------------------------
# tunables
@contextlib.contextmanager
def tunables(**values):
    """set library tunables for the duration of the block, restoring the previous values"""
    from pssr2_amd import _lib as L
    old = {}
    try:
        for k, v in values.items():
            r = L.lib().pssr_set_option(k.encode(), int(v))
            assert r >= 0, f"pssr_set_option({k}, {v}) failed: {L.lib().pssr_last_error().decode()}"
            old[k] = r
        yield
    finally:
        for k, v in old.items():
            L.lib().pssr_set_option(k.encode(), v)


@pytest.fixture
def production_tunables():
    """every conv tunable at its table default, so that no PSSR_* variable in the environment changes what is tested"""
    from pssr2_amd import ops
    solo, ops.SOLO[0] = ops.SOLO[0], False
    try:
        with tunables(**PRODUCTION_TUNABLES):
            yield PRODUCTION_TUNABLES
    finally:
        ops.SOLO[0] = solo
