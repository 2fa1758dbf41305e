"""Every extern "C" entry point of csrc/hist.hip called directly, against the f64 reference and the error measures of
tests/_hist_ref64.py (checked without a GPU by tests/test_hist_ref64.py).

GradHist forward and backward: kernel q <= 4 * max(q_f32, 1), where q is q_h / q_dx of _hist_ref64 (error over one f32 rounding unit
of what each output sums, plus the skip loss the kernel's header documents) and q_f32 is the same measure of the same reference code
run in f32 on the device for the same case.  4 is the allowance of tests/test_gpu_window_attn.py for two f32 evaluations that differ
in summation order and in their exp / reciprocal; the floor 1 is one rounding unit.  Every bin and every pixel is compared.
Configurations and shapes (_hist_ref64.CASES) reach a ragged last wave and chunk, bins = 1 and 8192, N < 256 and workgroups that
take two tiles; the inputs carry pixels on the ends of the kernels' skip windows, computed the way the kernels compute them.  The
backward is measured twice per case: with every planted pixel ("edges") and without those above the last centre ("inner"), where any
f32 evaluation of s (1 - s) is dominated by the rounding of 1 - s and would set the yardstick for all pixels
(_hist_ref64.edge_values).

Inputs given as a pair (a, b) are built so that a - b is exact in f32 (b integer, a - b on a 2^-10 grid): the f64 reference then sees
the x the kernel sees, and the bound stays as sharp as for a single input.

The small kernels of the crappifier loss are exact (profiles, subsample, backward scalars, clamp) or exact up to the final rounding
(loss combine: an f64 tree rounded once).  _crappifier_loss end to end is compared with an f64 composition of _hist_ref64 and
_loss_ref64.compose.

Run with -s for the figures.  On an MI355X they were (kernel q / yardstick q_f32):
    forward (allowed 4 * max(q_f32, 1))
      one pair      def-1320 1.99 / 0.56   def-67tiles 0.26 / 0.26   def-3ch 0.20 / 0.20    wide-63 0.50 / 0.63    wide-3ch 0.36 / 0.38
                    ragged-300 0.78 / 0.78 bins-65 1.01 / 0.96       bins-257 0.48 / 0.48   bins-1 0.10 / 0.10     bins-1000 0.50 / 0.50
                    bins-max 0.22 / 0.22
      two pairs     def-1320 1.99 / 0.56   def-67tiles 0.49 / 0.18   ragged-300 1.47 / 1.47 bins-65 1.01 / 0.96
      clamp_first   def-1320 1.14 / 1.14   wide-63 0.44 / 0.54       non-finite: def-1320 0.24 / 0.20, ragged-300 0.47 / 0.47,
                    bins-65 0.47 / 0.47, bins-1 0.11 / 0.23
    backward, "inner" pixels
      plain         def-1320 198.6 / 198.6 def-67tiles 222.3 / 222.0 def-3ch 193.4 / 194.7  wide-63 2.77 / 2.78    wide-3ch 3.34 / 3.99
                    ragged-300 11.2 / 11.3 bins-65 74.9 / 75.1       bins-257 27.6 / 27.8   bins-1 4.37 / 4.37     bins-1000 28.3 / 28.1
                    bins-max 5.21 / 5.41
      one option    (def-1320, bins-65)    xb 73.7 / 73.8, 45.4 / 45.4        g_ref 54.8 / 54.8, 30.6 / 30.6     dev_scale 75.7 / 74.9, 47.4 / 47.2
                    g_scale 73.2 / 73.5, 46.2 / 42.7       accumulate 66.0 / 66.0, 17.5 / 17.5    clamp 165.2 / 165.2, 1196.6 / 1196.4
                    clamp+xb 73.7 / 73.8, 45.4 / 45.4      production 43.0 / 43.6, 15.2 / 15.2    non-finite 66.0 / 66.0, 45.4 / 45.4
    backward, "edges" pixels: kernel and yardstick agree to the digits shown, 144.6 (bins-max) .. 88226.6 (bins-257); the pixel
      above the last centre sets both (s (1 - s) evaluates to 0 in f32, the error is the f64 value itself)
    q_dx is well above 1 in every f32 evaluation because 1 - s_k carries a 2^-24 absolute error into each of the many bins below a
    pixel, where s_k (1 - s_k) is small; the kernel tracks the yardstick within 8 %.
    Before the fixes of this file's pull request the forward read 1188.9 at bins-1000 (the centres' multiply-add was fused: one
    rounding instead of two) and 5.66 at clamp_first def-1320 (f32 accumulation over 226 pixels clamped to 255), the backward 229.9
    at bins-1000; h[b, 0] was one short per -inf pixel and dx was 0 for a NaN pixel.
The file runs in 4 s.
"""
import ctypes as C
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _hist_ref64 as R
from _loss_ref64 import bound as loss_bound, compose
from oracle import loss_ref as Lr

pytestmark = pytest.mark.gpu

FACTOR = 4.0
PSSR_ERR_ARG = -1
PAST_GRID_CAP = 4096 * 256 + 513            # grid_1d caps the grid at 4096 workgroups of 256: the stride loop runs
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def report_figures():
    yield
    for key in sorted(WORST):
        q, q32 = WORST[key]
        print(f"\n{key:28s} kernel q {q:10.3f}   f32 yardstick {q32:10.3f}   allowed {FACTOR * max(q32, 1.0):10.3f}", end="")
    print()


def _assert_q(key, q, q32):
    old = WORST.get(key)
    if old is None or q / max(q32, 1.0) > old[0] / max(old[1], 1.0):
        WORST[key] = (q, q32)
    print(f"  [{key}] kernel q {q:.3f}  f32 yardstick {q32:.3f}")
    assert q <= FACTOR * max(q32, 1.0), f"{key}: kernel q {q:.3f} above {FACTOR:.0f} * max(q_f32 = {q32:.3f}, 1)"


def _args(cfg):
    bins, (lo, hi), sigma = cfg
    return bins, lo, hi, sigma


def _fwd_check(key, x_eff, args, h):
    """h against the f64 histogram of x_eff (what the kernel forms on load, exact in f32 by construction)."""
    h64, S = R.hist_fwd(x_eff, *args, with_s=True)
    h32 = R.hist_fwd(x_eff, *args, dtype=torch.float32)
    n = x_eff[0].numel()
    b, j = R.worst_bin(h, h64, S, n)
    print(f"  [{key}] worst bin ({b}, {j}): kernel {h[b, j].item():.9g} f64 {h64[b, j].item():.12g} f32 {h32[b, j].item():.9g} S {S[b, j].item():.6g}")
    _assert_q(key, R.q_h(h, h64, S, n), R.q_h(h32, h64, S, n))


def _bwd_check(key, args, dx, xa, g, **kw):
    dx64, W, T = R.hist_bwd(xa, g, *args, with_w=True, **kw)
    dx32 = R.hist_bwd(xa, g, *args, dtype=torch.float32, **kw)
    _assert_q(key, R.q_dx(dx, dx64, W, T), R.q_dx(dx32, dx64, W, T))
    return dx64


@functools.lru_cache(maxsize=None)
def _case(name, above_range=True):
    _, cfg, shape = R.CASES[R.CASE_IDS.index(name)]
    c = SimpleNamespace(cfg=cfg, shape=shape, args=_args(cfg))
    c.x = R.case_inputs(shape, cfg, 11, above_range=above_range).cuda()
    c.g = torch.randn(shape[0], cfg[0], generator=torch.Generator().manual_seed(12)).cuda()
    return c


def _pair(x, seed, lo_int=0, hi_int=256):
    """(a, b) with b integer-valued and a - b == x on a 2^-10 grid: the subtraction is exact in f32 (asserted)."""
    xq = torch.round(x.cpu() * 1024) / 1024
    xq = torch.where(torch.isfinite(x.cpu()), xq, x.cpu())
    b = torch.randint(lo_int, hi_int, x.shape, generator=torch.Generator().manual_seed(seed)).float()
    a = xq + b
    fin = torch.isfinite(xq)
    assert torch.equal((a.double() - b.double())[fin], xq.double()[fin]) and torch.equal((a - b)[fin], xq[fin])
    return a.cuda(), b.cuda(), xq.cuda()


# ---------------------------------------------------------------------------------------------------------------------
# pssr_gradhist_fwd
@pytest.mark.parametrize("name", R.CASE_IDS)
def test_forward_one_pair(name):
    from pssr2_amd import ops
    c = _case(name)
    (h,) = ops.gradhist_fwd([(c.x, None)], *c.args)
    _fwd_check(f"fwd {name}", c.x, c.args, h)
    (again,) = ops.gradhist_fwd([(c.x, None)], *c.args)
    assert torch.equal(h, again)


@pytest.mark.parametrize("second_b", [False, True], ids=["b1-none", "b1-given"])
@pytest.mark.parametrize("name", ["def-1320", "ragged-300", "bins-65", "def-67tiles"])
def test_forward_two_pairs(name, second_b):
    """The second pair goes through the same launch (blockIdx.z = pair * chunks + chunk) into its own rows of the workspace."""
    from pssr2_amd import ops
    c = _case(name)
    a0, b0, x0 = _pair(c.x, 21)
    other = R.case_inputs(c.shape, c.cfg, 13).cuda()
    a1, b1, x1 = _pair(other, 22) if second_b else (other, None, other)
    h0, h1 = ops.gradhist_fwd([(a0, b0), (a1, b1)], *c.args)
    _fwd_check(f"fwd 2 pairs {name}", x0, c.args, h0)
    _fwd_check(f"fwd 2 pairs {name}", x1, c.args, h1)
    assert torch.equal(h0, ops.gradhist_fwd([(a0, b0)], *c.args)[0])            # a pair's rows do not depend on its neighbour
    assert torch.equal(h1, ops.gradhist_fwd([(a1, b1)], *c.args)[0])


def _clamp_operand(shape, seed):
    """xa in about [-60, 320] on a 2^-10 grid with values exactly 0 and 255, just inside, just outside and far outside"""
    gen = torch.Generator().manual_seed(seed)
    xa = torch.round((torch.rand(shape, generator=gen) * 380 - 60) * 1024) / 1024
    flat = xa.view(shape[0], -1)
    special = torch.tensor([0.0, 255.0, -2.0 ** -10, 255.0 + 2.0 ** -10, 2.0 ** -10, 255.0 - 2.0 ** -10, -1e4, 1e4])
    m = min(flat.shape[1], special.numel())
    flat[:, :m] = special[:m]
    return xa


@pytest.mark.parametrize("name", ["def-1320", "wide-63"])
def test_forward_clamp_first(name):
    """PSSR_HIST_CLAMP clamps a0 (not a0 - b0, and not the second pair) to [0, 255] on load."""
    from pssr2_amd import ops
    c = _case(name)
    xa = _clamp_operand(c.shape, 31)
    b0 = torch.randint(0, 256, c.shape, generator=torch.Generator().manual_seed(32)).float()
    if name == "wide-63":
        b0 = xa.clamp(0, 255).round() + torch.randint(-20, 21, c.shape, generator=torch.Generator().manual_seed(33)).float()
    xa1 = _clamp_operand(c.shape, 34)
    x0 = xa.clamp(0, 255) - b0
    assert torch.equal(x0.double(), xa.clamp(0, 255).double() - b0.double())
    h0, h1 = ops.gradhist_fwd([(xa.cuda(), b0.cuda()), (xa1.cuda(), None)], *c.args, clamp_first=True)
    _fwd_check(f"fwd clamp {name}", x0.cuda(), c.args, h0)
    _fwd_check(f"fwd clamp {name}", xa1.cuda(), c.args, h1)
    (h_one,) = ops.gradhist_fwd([(xa.cuda(), None)], *c.args, clamp_first=True)
    _fwd_check(f"fwd clamp {name}", xa.clamp(0, 255).cuda(), c.args, h_one)


def _non_finite(x):
    """image 0: a NaN, image 1: +inf twice, image 2 (if any): -inf three times; somewhere past the planted pixels"""
    x = x.clone()
    flat = x.view(x.shape[0], -1)
    n = flat.shape[1]
    flat[0, n - 1] = float("nan")
    flat[1, n // 2], flat[1, n - 2] = float("inf"), float("inf")
    if x.shape[0] > 2:
        flat[2, n // 3], flat[2, n - 3], flat[2, 0] = -float("inf"), -float("inf"), -float("inf")
    else:
        flat[1, n // 3] = -float("inf")
    return x


@pytest.mark.parametrize("name", ["def-1320", "ragged-300", "bins-65", "bins-1"])
def test_forward_non_finite_pixels(name):
    """A NaN pixel makes its row NaN; +inf adds nothing; -inf adds s_{-1} - s_0 = 1 to bin 0 (the wave that holds bin 0 has no
    lower window)."""
    from pssr2_amd import ops
    c = _case(name)
    x = _non_finite(c.x)
    (h,) = ops.gradhist_fwd([(x, None)], *c.args)
    assert torch.isnan(h[0]).all() and torch.isfinite(h[1:]).all()
    _fwd_check(f"fwd non-finite {name}", x, c.args, h)
    # said once more without the measure: the -inf pixels are whole counts in bin 0
    b = 2 if x.shape[0] > 2 else 1
    finite_only = torch.where(torch.isinf(x), torch.full_like(x, 1e30), x)          # 1e30 adds exactly 0 everywhere
    (h_fin,) = ops.gradhist_fwd([(finite_only, None)], *c.args)
    count = float((x[b] == -float("inf")).sum())
    n = x[0].numel()                # at most n sequential f32 additions round at 2^-24 of the running sum each
    assert abs((h[b, 0] - h_fin[b, 0]).item() - count) <= n * 2.0 ** -24 * max(1.0, h[b, 0].item()), (h[b, 0].item(), h_fin[b, 0].item(), count)
    assert torch.equal(h[b, 1:], h_fin[b, 1:])


def test_forward_argument_errors():
    """PSSR_ERR_ARG, and nothing is launched: the output keeps its poison."""
    from pssr2_amd import _lib as L
    lib = L.lib()
    batch, n = 2, 300
    x = torch.randn(batch, n, device="cuda")
    ws_bytes = lib.pssr_gradhist_workspace_bytes(batch, C.c_int64(n), 512)
    assert ws_bytes == 2 * batch * 2 * 512 * 4                      # pairs * batch * tiles * bins floats
    assert lib.pssr_gradhist_workspace_bytes(batch, C.c_int64(129 * 131), 512) == 2 * batch * 64 * 512 * 4      # capped at HIST_MAX_WG
    assert lib.pssr_gradhist_workspace_bytes(0, C.c_int64(n), 512) == 0
    ws = torch.empty(2 * batch * 2 * R.MAX_BINS, device="cuda")
    h0 = torch.full((batch, R.MAX_BINS + 1), -7.0, device="cuda")
    h1 = torch.full((batch, R.MAX_BINS + 1), -7.0, device="cuda")

    def call(bins=512, lo=-256.0, hi=256.0, sigma=5.0, ws_b=ws.numel() * 4, a1=None, b1=None, out1=None):
        return lib.pssr_gradhist_fwd(L.ptr(x), None, L.ptr(a1), L.ptr(b1), L.ptr(h0), L.ptr(out1), L.ptr(ws), C.c_int64(ws_b), batch,
                                     C.c_int64(n), bins, C.c_float(lo), C.c_float(hi), C.c_float(sigma), 0, L.stream_ptr())

    assert call(bins=0) == PSSR_ERR_ARG
    assert call(bins=R.MAX_BINS + 1) == PSSR_ERR_ARG
    assert call(lo=3.0, hi=3.0) == PSSR_ERR_ARG and call(lo=3.0, hi=-3.0) == PSSR_ERR_ARG
    assert call(sigma=0.0) == PSSR_ERR_ARG and call(sigma=-1.0) == PSSR_ERR_ARG
    assert call(ws_b=ws_bytes - 4) == PSSR_ERR_ARG
    assert call(a1=x) == PSSR_ERR_ARG                               # a1 without h1
    assert call(out1=h1) == PSSR_ERR_ARG                            # h1 without a1
    assert call(b1=x) == PSSR_ERR_ARG                               # b1 without a1
    assert b"gradhist_fwd" in lib.pssr_last_error()
    torch.cuda.synchronize()
    assert (h0 == -7.0).all() and (h1 == -7.0).all()
    assert call(ws_b=ws_bytes) == 0 and call(bins=R.MAX_BINS) == 0
    torch.cuda.synchronize()
    assert (h0.view(-1)[:batch * R.MAX_BINS] != -7.0).all()


# ---------------------------------------------------------------------------------------------------------------------
# pssr_gradhist_bwd through ops.gradhist_bwd
def _run_bwd(c, xa, g, poison=float("nan"), dx=None, **kw):
    from pssr2_amd import ops
    dx = torch.full_like(xa, poison) if dx is None else dx
    return ops.gradhist_bwd(xa, kw.pop("xb", None), g, dx, *c.args, **kw)


@pytest.mark.parametrize("pixels", ["inner", "edges"])
@pytest.mark.parametrize("name", R.CASE_IDS)
def test_backward_plain(name, pixels):
    """No option: dx overwrites a poisoned buffer.  Batch > 1 in all but bins-max, with different g per image."""
    c = _case(name, above_range=pixels == "edges")
    dx = _run_bwd(c, c.x, c.g)
    _bwd_check(f"bwd {pixels} {name}", c.args, dx, c.x, c.g)
    assert torch.equal(dx, _run_bwd(c, c.x, c.g, poison=1e30))


OPTION_CASES = ["def-1320", "bins-65"]


def _option_inputs(name):
    """xa, xb with xa - xb exact; xa has values at 0 and 255 and outside; g, g_ref like two histograms"""
    c = _case(name, above_range=False)
    gen = torch.Generator().manual_seed(41)
    bins = c.cfg[0]
    xb = torch.randint(0, 256, c.shape, generator=gen).float()
    xa = torch.round(c.x.cpu() * 1024) / 1024 + xb
    flat = xa.view(c.shape[0], -1)
    flat[:, -8:] = torch.tensor([0.0, 255.0, -2.0 ** -10, 255.0 + 2.0 ** -10, 2.0 ** -10, 255.0 - 2.0 ** -10, -40.0, 300.0])
    flat[:, 7] = 100.0
    centre = (c.cfg[1][0] + c.cfg[1][1]) / 2
    xb.view(c.shape[0], -1)[:, -8:] = flat[:, -8:].clamp(0, 255).round() - centre + torch.tensor([1.0, -2.0, 3.0, -1.0, 2.0, -3.0, 1.0, -1.0])
    assert torch.equal((xa - xb).double(), xa.double() - xb.double())
    assert torch.equal((xa.clamp(0, 255) - xb).double(), xa.clamp(0, 255).double() - xb.double())
    n = flat.shape[1]
    g_ref = (torch.rand(c.shape[0], bins, generator=gen) * 2 * n / bins)
    g = g_ref + torch.randn(c.shape[0], bins, generator=gen) * (n / bins) ** 0.5
    dx_in = torch.randn(c.shape, generator=gen)              # of the histogram part's size (scaled like it under "production")
    dev = torch.tensor([-0.4321])
    return c, SimpleNamespace(xa=xa.cuda(), xb=xb.cuda(), g=g.cuda(), g_ref=g_ref.cuda(), dx_in=dx_in.cuda(), dev=dev.cuda(),
                              g_scale=2.0 / (c.shape[0] * bins * c.shape[-1] ** 2))


@pytest.mark.parametrize("option", ["xb", "g_ref", "dev_scale", "g_scale", "accumulate", "clamp", "clamp+xb", "production"])
@pytest.mark.parametrize("name", OPTION_CASES)
def test_backward_options_one_at_a_time(name, option):
    """Each input of the C ABI alone, then the combination _CrappifierLossFunction.backward uses (all of them)."""
    c, s = _option_inputs(name)
    kernel_kw, ref_kw, xa, dx = {}, {}, s.xa - s.xb, None
    if option in ("xb", "clamp+xb", "production"):
        kernel_kw["xb"] = ref_kw["xb"] = s.xb
        xa = s.xa
    if option in ("clamp", "clamp+xb", "production"):
        kernel_kw["clamp"] = ref_kw["clamp"] = True
        xa = s.xa
    if option in ("g_ref", "production"):
        kernel_kw["g_ref"] = ref_kw["g_ref"] = s.g_ref
    if option in ("dev_scale", "production"):
        kernel_kw["dev_scale"] = ref_kw["dev_scale"] = s.dev
    if option in ("g_scale", "production"):
        kernel_kw["g_scale"] = ref_kw["g_scale"] = s.g_scale
    if option in ("accumulate", "production"):
        dx_in = s.dx_in * (s.g_scale * abs(s.dev.item()) if option == "production" else 1.0)
        kernel_kw["accumulate"], ref_kw["dx_in"] = True, dx_in
        dx = dx_in.clone()
    got = _run_bwd(c, xa, s.g, dx=dx, **kernel_kw)
    dx64 = _bwd_check(f"bwd {option} {name}", c.args, got, xa, s.g, **ref_kw)
    if ref_kw.get("clamp"):
        cut = (xa < 0) | (xa > 255)
        assert cut.any() and (got[cut] == 0).all()
        edge = (xa == 0) | (xa == 255)                              # inclusive bounds: these keep their gradient
        assert (dx64[edge] != 0).any() and torch.equal(got[edge] != 0, dx64[edge] != 0)
    dx2 = ref_kw["dx_in"].clone() if dx is not None else None
    assert torch.equal(got, _run_bwd(c, xa, s.g, dx=dx2, **kernel_kw))


@pytest.mark.parametrize("clamp", [False, True], ids=["plain", "clamp"])
@pytest.mark.parametrize("name", ["def-1320", "bins-65"])
def test_backward_non_finite_pixels(name, clamp):
    """A NaN x gives dx = NaN, as torch does; under the clamp flag a NaN xa is cut and gets 0, a NaN that enters through xb stays
    NaN.  x = +-inf gives 0 (s (1 - s) = 0).  The other pixels are not disturbed."""
    c, s = _option_inputs(name)
    xa = _non_finite(s.xa.cpu()).cuda()
    xb = s.xb.clone()
    xb.view(c.shape[0], -1)[0, 7] = float("nan")                # xa finite and in range, x = NaN
    got = _run_bwd(c, xa, s.g, xb=xb, clamp=clamp)
    dx64 = _bwd_check(f"bwd non-finite {name}", c.args, got, xa, s.g, xb=xb, clamp=clamp)
    flat, n = got.view(c.shape[0], -1), xa[0].numel()
    assert torch.isnan(dx64.view(c.shape[0], -1)[0, 7]) and torch.isnan(flat[0, 7])
    assert (flat[0, n - 1] == 0) if clamp else torch.isnan(flat[0, n - 1])
    assert int(torch.isnan(got).sum()) == (1 if clamp else 2)
    assert (got[torch.isinf(xa)] == 0).all()
    acc = _run_bwd(c, xa, s.g, xb=xb, clamp=clamp, accumulate=True, dx=s.dx_in.clone())
    _bwd_check(f"bwd non-finite {name}", c.args, acc, xa, s.g, xb=xb, clamp=clamp, dx_in=s.dx_in)


# ---------------------------------------------------------------------------------------------------------------------
# the small kernels
def _with_nan(t, idx):
    t.view(-1)[idx] = float("nan")
    return t


@pytest.mark.parametrize("clamp", [False, True], ids=["plain", "clamp"])
@pytest.mark.parametrize("n", [1, 1320, PAST_GRID_CAP])
def test_crappifier_profiles(n, clamp):
    from pssr2_amd import ops
    gen = torch.Generator().manual_seed(n)
    lr_hat = torch.rand(n, generator=gen) * 400 - 70
    lr = torch.randint(0, 256, (n,), generator=gen).float()
    ds = torch.rand(n, generator=gen) * 255
    if n > 8:
        lr_hat[:8] = torch.tensor([0.0, 255.0, -1e-3, 255.001, float("nan"), float("inf"), -float("inf"), 128.0])
        lr[n - 1] = float("nan")
        ds[n - 2] = float("nan")
    else:
        lr_hat[0] = 300.0
    lr_hat, lr, ds = lr_hat.cuda(), lr.cuda(), ds.cuda()
    pred, target = torch.full_like(lr, 9e9), torch.full_like(lr, 9e9)
    ops.crappifier_profiles(lr_hat, lr, ds, pred, target, clamp)
    want_p = (lr_hat.clamp(0, 255) if clamp else lr_hat) - ds
    want_t = lr - ds
    for got, want in ((pred, want_p), (target, want_t)):
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got[~torch.isnan(want)], want[~torch.isnan(want)])
    if n > 8:
        assert torch.isnan(pred[4]) and torch.isnan(pred[n - 2]) and torch.isnan(target[n - 1]) and torch.isnan(target[n - 2])
        assert pred[5] == (255 - ds[5] if clamp else float("inf"))


@pytest.mark.parametrize("shape,stride", [((2, 3, 7, 9), 1), ((2, 3, 7, 9), 2), ((2, 3, 7, 9), 3), ((2, 3, 7, 9), 4), ((2, 3, 7, 9), 8),
                                          ((2, 3, 7, 9), 11), ((5, 13, 11), 2), ((1, 1, 1031, 1023), 1), ((3, 1, 1031, 1023), 2)])
def test_subsample(shape, stride):
    """src[..., ::s, ::s]: odd sizes, several planes, a stride above H (8) and above both (11), more outputs than the grid holds"""
    from pssr2_amd import ops
    src = torch.randn(shape, generator=torch.Generator().manual_seed(stride)).cuda()
    got = ops.subsample(src, stride)
    want = src[..., ::stride, ::stride]
    assert got.shape == want.shape and got.is_contiguous() and torch.equal(got, want)


def _ulp_apart(a, b):
    """distance of two f32 values in units in the last place (same sign)"""
    ia, ib = np.float32(a).view(np.int32), np.float32(b).view(np.int32)
    return abs(int(ia) - int(ib))


@pytest.mark.parametrize("m", [1, 63, 256, 1320])
def test_crappifier_loss_combine(m):
    """D: the f64 sum rounded once (the kernel's f64 tree differs from it in the 16th digit, so only the last rounding can flip);
    out = [D * P, D, P] with the product formed in f32 from the rounded D."""
    from pssr2_amd import ops
    gen = torch.Generator().manual_seed(m)
    t = torch.rand(m, generator=gen) * 40
    p = t + torch.randn(m, generator=gen) * 3
    dist_scale = float(np.float32(1.0 / m / (40 * 40)))
    ssim = torch.tensor([0.43219876], device="cuda")
    out = torch.full((3,), float("nan"), device="cuda")
    ops.crappifier_loss_combine(p.cuda(), t.cuda(), ssim, dist_scale, out)
    L, D, P = (np.float32(v) for v in out.cpu().numpy())
    d64 = math.fsum(((p.double() - t.double()) ** 2).tolist()) * dist_scale
    assert _ulp_apart(D, np.float32(d64)) <= 1, (D, d64)
    assert abs(float(D) - d64) <= 2.0 ** -24 * d64 * (1 + 1e-6)                    # said in f64: half an ulp, plus the tree's 1e-16
    assert P == np.float32(ssim.item()) and L == np.float32(D * P)
    out2 = torch.empty_like(out)
    ops.crappifier_loss_combine(p.cuda(), t.cuda(), ssim, dist_scale, out2)
    assert torch.equal(out, out2)


@pytest.mark.parametrize("dL", [1.0, 0.37, -2.5, 0.0, 3e-7])
def test_crappifier_loss_bwd_scalars(dL):
    from pssr2_amd import ops
    parts = torch.tensor([0.0123, 0.0456789, 0.2701234], device="cuda")
    go = torch.tensor([dL], device="cuda")
    out = torch.full((2,), float("nan"), device="cuda")
    ops.crappifier_loss_bwd_scalars(parts, go, out)
    assert torch.equal(out, torch.stack([parts[1] * go[0], parts[2] * go[0]]))
    assert torch.equal(out.cpu(), torch.stack([parts.cpu()[1] * dL, parts.cpu()[2] * dL]))


def test_clamp_past_the_grid_cap_and_in_place():
    from pssr2_amd import ops
    x = torch.randn(PAST_GRID_CAP, generator=torch.Generator().manual_seed(5)) * 4
    x[::1001] = float("nan")
    x[1::1001] = float("inf")
    x[2::1001] = -float("inf")
    x[3], x[4] = 3.0, -3.0
    x = x.cuda()
    want = torch.clamp(x, -3.0, 3.0)
    got = ops.clamp_f32(x, -3.0, 3.0)
    nan = torch.isnan(x)
    assert torch.equal(torch.isnan(got), nan) and torch.equal(got[~nan], want[~nan]) and got[-1] == want[-1]
    y = x.clone()
    assert ops.clamp_f32(y, -3.0, 3.0, out=y) is y
    assert torch.equal(torch.isnan(y), nan) and torch.equal(y[~nan], want[~nan])


# ---------------------------------------------------------------------------------------------------------------------
# _crappifier_loss end to end
GO = 0.37
C1, C2 = float(np.float32(0.01 ** 2)), float(np.float32(0.03 ** 2))      # the SSIM kernels take the constants as f32
SSIM_MIX = 0.8


def _loss_composition(lr, lr_hat, ds, clamp, dtype):
    """value and d(GO * L)/d(lr_hat) of L = D * P in `dtype` (pred and target are formed in `dtype` too):
    D = mean((H(pred) - H(target))^2) / W_lr^2 with H from _hist_ref64, P and dP/dpred from _loss_ref64.compose."""
    bins, lo, hi, sigma = _args(R.DEF)
    B, W_lr = lr.shape[0], lr.shape[-1]
    a = lr_hat.to(dtype)
    pred = (a.clamp(0, 255) if clamp else a) - ds.to(dtype)
    target = lr.to(dtype) - ds.to(dtype)
    hp, ht = R.hist_fwd(pred, bins, lo, hi, sigma, dtype=dtype), R.hist_fwd(target, bins, lo, hi, sigma, dtype=dtype)
    D = ((hp - ht) ** 2).mean() / W_lr ** 2
    planes = lambda t: t.reshape(-1, *t.shape[-2:])
    win = Lr.gauss_1d(11, 1.5)
    P, _, _ = compose(planes(pred), planes(target), win, C1, C2, [1.0], False, SSIM_MIX)
    _, dP, _ = compose(planes(pred), planes(target), win, C1, C2, [1.0], False, SSIM_MIX, grad_out=GO * float(D))
    dD = R.hist_bwd(pred, 2 * (hp - ht) / (B * bins * W_lr ** 2), bins, lo, hi, sigma, dtype=dtype)
    grad = dP.reshape(lr.shape).to(dtype) + GO * P * dD
    if clamp:
        grad = torch.where((a >= 0) & (a <= 255), grad, torch.zeros_like(grad))
    parts = SimpleNamespace(ssim=(dP.reshape(lr.shape).double()).abs().max().item(), hist=(GO * P * dD.double()).abs().max().item(),
                            D=float(D), P=P, pred=pred, target=target)
    return float(D) * P, grad, parts


def _loss_inputs(shape, clamp, seed):
    gen = torch.Generator().manual_seed(seed)
    ds = torch.randint(20, 236, shape, generator=gen).float()
    lr = (ds + torch.randn(shape, generator=gen) * 13).round().clamp(0, 255)
    lr_hat = ds + torch.randn(shape, generator=gen) * 9 + 1.5
    if clamp:
        flat, dflat = lr_hat.view(-1), ds.view(-1)
        dflat[:12] = torch.tensor([3.0, 250.0] * 6)
        flat[:12] = torch.tensor([0.0, 255.0, -4.5, 259.25, 0.0, 255.0, -0.001, 255.001, 2.0, 254.0, -30.0, 300.0])
    return lr, lr_hat, ds


@pytest.mark.parametrize("clamp", [False, True], ids=["plain", "clamp"])
@pytest.mark.parametrize("shape", [(3, 1, 24, 40), (2, 1, 16, 16)])
def test_crappifier_loss_end_to_end(shape, clamp):
    """_crappifier_loss and its gradient through (0.37 * L) against the f64 composition.  W_lr != H_lr in (3, 1, 24, 40): a scaling by
    the wrong axis is off by (40 / 24)^2.

    value:    |L - L64| <= max(4 * |L32 - L64|, 2^-23 |L64|), L32 the same composition in f32 on the CPU;
    gradient: _loss_ref64.bound, 16 * max(E32, 2^-23 max|grad64|), the rule of the SSIM part.  Of the two terms the histogram one,
              P dD/dpred, dominates: its largest entry is 85 times (24 x 40) and 26 .. 30 times (16 x 16) that of D dP/dpred, and the
              measured error (1.3e-11 .. 5.2e-11, 4e-7 .. 5e-7 of the histogram term) sits in it: the SSIM term is smaller than that
              error times 3e4 and its kernels are good to 1e-6 of their own output (tests/test_gpu_loss_levels.py).
    Measured on an MI355X: value error 0.35 .. 0.93 of the f32 composition's own (allowed 4); gradient error 0.84 .. 1.13 times
    max(E32, floor) (allowed 16).  With the forward's f32 accumulation the value was off by 5.0 .. 10.3 times the f32 composition's
    error: target = lr - ds is integer-valued, many pixels share a value, and D was 3e-7 .. 6e-7 low.
    Under the clamp, pixels at exactly 0 and 255 keep their gradient and pixels outside get exactly 0."""
    from pssr2_amd.models import GradHist
    from pssr2_amd.train import _crappifier_loss
    from pssr2_amd.util import SSIMLoss
    lr, lr_hat, ds = _loss_inputs(shape, clamp, 51)
    L64, g64, parts = _loss_composition(lr, lr_hat, ds, clamp, torch.float64)
    L32, g32, _ = _loss_composition(lr, lr_hat, ds, clamp, torch.float32)
    x = lr_hat.cuda().requires_grad_(True)
    L = _crappifier_loss(lr.cuda(), x, ds.cuda(), GradHist(sigma=5), SSIMLoss(ms=False), clamp=clamp)
    (GO * L).backward()
    err_v, tol_v = abs(float(L.item()) - L64), max(FACTOR * abs(L32 - L64), 2.0 ** -23 * abs(L64))
    grad = x.grad.cpu().double()
    tol_g, den_g = loss_bound(g64, g32)
    err_g = (grad - g64).abs().max().item()
    print(f"  [loss {shape} clamp={clamp}] L {L64:.6e}: err {err_v:.3e} (f32 composition {abs(L32 - L64):.3e}, allowed {tol_v:.3e}); "
          f"gradient err {err_g:.3e} = {err_g / den_g:.3f} x max(E32, floor) (allowed 16); max|ssim part| {parts.ssim:.3e} "
          f"max|hist part| {parts.hist:.3e}")
    assert err_v <= tol_v, (L.item(), L64, L32)
    assert torch.isfinite(grad).all() and err_g <= tol_g, (err_g, den_g)
    if clamp:
        raw = lr_hat
        assert (grad[(raw < 0) | (raw > 255)] == 0).all() and ((raw < 0) | (raw > 255)).sum() >= 6
        assert (grad[(raw == 0) | (raw == 255)] != 0).all() and ((raw == 0) | (raw == 255)).sum() >= 4
