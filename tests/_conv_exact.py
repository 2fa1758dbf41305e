"""Helpers for the bit-exact convolution tests (tests/test_gpu_conv_exact.py, tests/test_conv_exact_helpers.py).

The idea: operands are dyadic numbers with few significant bits, so that every product and every partial sum of the GEMM is exact
in f32 whatever the summation order (MFMA, split-K, atomics).  The f32 accumulator then holds the exact value, and a 16-bit store
must hold exactly the float64 reference rounded once, to nearest even.  No tolerances: any difference is a bug.

`Grid(e, m)` describes a set of values: multiples of 2**-e with magnitude at most m.  `assert_exact_premise` walks a convolution's
arithmetic on such grids and fails when an intermediate value could need more than 24 significant bits.
"""
from __future__ import annotations

import contextlib
import re
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


def launched_kernels(fn):
    """Run fn() under torch.profiler; returns (its result, the sorted (family, ints) of this library's convolution kernels that ran).
    Fails -- never skips -- when the profiler reports none."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        res = fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    ks = sorted(p for p in (parse_kernel_name(n) for n in names) if is_conv_kernel(p))
    assert ks, f"the profiler reported no convolution kernel of this library (events: {sorted(set(names))[:20]})"
    return res, ks


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
