"""CPU checks of the bit-exact convolution test helpers (tests/_conv_exact.py)."""
import re
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from _conv_exact import (B_GRID, PRODUCTION_TUNABLES, SCALE_GRID, SHIFT_GRID, W_GRID, X_GRID, Grid, assert_exact_premise, dyadic,
                         expected, from_blocked, parse_kernel_name, pix_index, shuf2_perm, to_blocked)

ROOT = Path(__file__).resolve().parent.parent


def test_premise_accepts_the_budget_and_rejects_what_is_over_it():
    # 3x3 over 256 channels with bias and an affine epilogue: well inside 24 bits
    assert assert_exact_premise(9 * 256, bias=B_GRID, affine=(SCALE_GRID, SHIFT_GRID)).units() <= 2 ** 24
    # K * |x| * |w| * 2^(ex + ew) = 2^24 exactly fits; one more term does not
    assert_exact_premise(2 ** 19, dt=torch.float32)
    with pytest.raises(AssertionError, match="premise"):
        assert_exact_premise(2 ** 19 + 1, dt=torch.float32)
    # a bias on a finer grid pushes the accumulator over
    with pytest.raises(AssertionError, match="premise"):
        assert_exact_premise(9 * 256, bias=Grid(20, 1.0))
    # operands that bf16 cannot hold (511/512 needs 9 significant bits), but multiples of 1/256 it can
    assert_exact_premise(9, x=Grid(8, 1.0))
    with pytest.raises(AssertionError, match="premise"):
        assert_exact_premise(9, x=Grid(9, 1.0))
    # a prologue output that needs more bits than bf16 has, but that float16 holds
    with pytest.raises(AssertionError, match="premise"):
        assert_exact_premise(9, pro=(Grid(6, 2.0), SHIFT_GRID))
    assert_exact_premise(9, dt=torch.float16, pro=(Grid(6, 2.0), SHIFT_GRID))
    # float16 range
    with pytest.raises(AssertionError, match="float16"):
        assert_exact_premise(9, x=Grid(0, 2.0 ** 17), w=Grid(0, 1.0), dt=torch.float16)


def test_dyadic_operands_stay_on_their_grid():
    g = torch.Generator().manual_seed(0)
    for grid in (X_GRID, W_GRID, B_GRID):
        v = dyadic(g, (4096,), grid)
        assert float(v.abs().max()) == grid.m          # the bound is reached...
        q = v * 2 ** grid.e
        assert torch.equal(q, q.round())                # ...and every value is a multiple of the step


@pytest.mark.parametrize("dt,bits", [(torch.bfloat16, 8), (torch.float16, 11)])
def test_expected_rounds_once_to_nearest_even(dt, bits):
    u = 2.0 ** (1 - bits)                    # spacing of the storage type in [1, 2)
    ref = torch.tensor([1 + u / 2,           # tie, down to the even 1
                        1 + 3 * u / 2,       # tie, up to the even 1 + 2u
                        -(1 + u / 2),        # ties are symmetric
                        1 + u / 2 + u / 8,   # above the tie: up
                        1 + u / 2 - u / 8,   # below the tie: down
                        1 + u], dtype=torch.float64)
    want = torch.tensor([1, 1 + 2 * u, -1, 1 + u, 1, 1 + u], dtype=torch.float64)
    got = expected(ref, dt)
    assert got.dtype == dt and torch.equal(got.double(), want)
    with pytest.raises(AssertionError, match="not exact in f32"):
        expected(torch.tensor([1 + 2.0 ** -30], dtype=torch.float64), dt)


def test_kernel_name_parser_reads_both_forms():
    assert parse_kernel_name("_ZN12_GLOBAL__N_117conv_igemm_kernelIDF16_Li64ELi0ELi9EEEvN9pssr_conv8ConvArgsE") == \
        ("conv_igemm_kernel", (64, 0, 9))
    assert parse_kernel_name("_ZN12_GLOBAL__N_114conv_v3_kernelIDF16bLi128EEEvN9pssr_conv8ConvArgsE") == ("conv_v3_kernel", (128,))
    assert parse_kernel_name("_ZN12_GLOBAL__N_119conv_wgrad16_kernelIDF16bLi128ELi32ELi0ELi1EEEvNS_9WgradArgsE") == \
        ("conv_wgrad16_kernel", (128, 32, 0, 1))
    assert parse_kernel_name("conv_igemm_kernel<__hip_bfloat16, 64, 0, 9>") == ("conv_igemm_kernel", (64, 0, 9))
    assert parse_kernel_name("void (anonymous namespace)::conv_flat_kernel<float, 128, 0, 4>(pssr_conv::ConvArgs)") == \
        ("conv_flat_kernel", (128, 0, 4))
    assert parse_kernel_name("void (anonymous namespace)::conv_splitk_finish_kernel<_Float16, 64, 0>(pssr_conv::ConvArgs)") == \
        ("conv_splitk_finish_kernel", (64, 0))
    assert parse_kernel_name("Memset (Device)") is None


def test_blocked_order_follows_the_header_formula():
    n, h, w, c = 2, 8, 12, 3
    t = torch.arange(n * h * w * c).reshape(n, h, w, c)
    for blk in (0, 1, 2):
        b = to_blocked(t, blk).reshape(-1, c)
        for gi in range(n):
            for gy in range(h):
                for gx in range(w):
                    assert torch.equal(b[pix_index(gi, gy, gx, h, w, blk)], t[gi, gy, gx])
        assert torch.equal(from_blocked(to_blocked(t, blk), blk), t)
    # include/pssr_mi355.h: pixel (y, x) of an r-times upsampled image lives at ((y/r*W/r + x/r)*r*r + (y%r)*r + x%r)
    assert pix_index(0, 5, 7, 8, 12, 1) == ((5 // 2 * 6 + 7 // 2) * 4 + (5 % 2) * 2 + 7 % 2)


def test_shuf2_rows_are_sub_pixel_major():
    p = shuf2_perm(32)
    assert sorted(p.tolist()) == list(range(32))
    # F.pixel_shuffle puts channel 4 c + 2 i + j at sub-pixel (i, j) of output channel c
    x = torch.arange(32.).view(1, 32, 1, 1)
    hi = F.pixel_shuffle(x, 2)
    packed = x[:, p]
    for s in range(4):
        for c in range(8):
            assert hi[0, c, s >> 1, s & 1] == packed[0, s * 8 + c, 0, 0]


def test_dgrad_reference_identity():
    """the data gradient of a layer with weight wt.transpose(0, 1).flip(2, 3) is the forward convolution with wt (the GPU tests
    reuse the forward accumulators as the data-gradient reference)"""
    g = torch.Generator().manual_seed(1)
    for ks in (1, 3):
        x = dyadic(g, (2, 5, 6, 7), X_GRID)
        wt = dyadic(g, (4, 5, ks, ks), W_GRID)
        layer_w = wt.transpose(0, 1).flip(2, 3).contiguous()
        dx = torch.nn.grad.conv2d_input((2, 4, 6, 7), layer_w, x, padding=ks // 2)
        assert torch.equal(dx, F.conv2d(x, wt, padding=ks // 2))


def test_production_tunables_match_the_table_defaults():
    src = (ROOT / "pssr2_amd" / "csrc" / "api_common.cpp").read_text()
    table = {m.group(1): int(m.group(2)) for m in re.finditer(r'\{"(\w+)", &PssrTunables::\w+, (\d+),', src)}
    for k, v in PRODUCTION_TUNABLES.items():
        assert table[k] == v, (k, table[k], v)
    conv = {k for k in table if k.startswith(("IGEMM_", "CONV_", "WGRAD_")) and k != "IGEMM_DBG"}
    assert conv == set(PRODUCTION_TUNABLES), conv ^ set(PRODUCTION_TUNABLES)
