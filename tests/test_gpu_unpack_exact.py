"""Exact test of pssr_unpack_conv_wgrad_parts (csrc/pack.hip) on its own: no convolution involved.

The partial slabs dw_parts[parts][rows][taps][k_pad] hold dyadic values (multiples of 1/16 in [-1, 1]), whose sums are exact in f32
in any order for up to 2^16 parts; the OIHW destination is pre-filled with other dyadic values, and the rows past cout and the
columns the layout discards hold NaN.  Then
  * every destination element the layout addresses equals (its old value if `accumulate`, else 0) + the float64 sum of the parts,
  * every other destination element keeps the bits it had,
  * no NaN arrives anywhere.
The reference index maps (tests/_conv_exact.py: unpack_map) are written from the layouts documented in include/pssr_mi355.h and are
themselves checked against torch.nn.grad.conv2d_weight in tests/test_conv_exact_helpers.py."""
import pytest
import torch

from _conv_exact import Grid, dyadic, expected, production_tunables, shuf2_perm, stable_seed, unpack_map, unpack_reference

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("production_tunables")]
_ = production_tunables      # (the fixture is used through the mark above)

F32 = torch.float32
PART_GRID = Grid(4, 1.0)
OLD_GRID = Grid(3, 2.0)


def case(mode, cout, cin, ks, k_pad, parts, *, ci_begin=0, ci_count=None, perm=False, rows=None):
    return dict(mode=mode, cout=cout, cin=cin, ks=ks, k_pad=k_pad, parts=parts, ci_begin=ci_begin, ci_count=ci_count, perm=perm, rows=rows)


CASES = {}
for _ks in (3, 1):          # unpack9_kernel<9> and <1>
    CASES[f"m0_k{_ks}_contig"] = case(0, 16, 32, _ks, 32, 3)                                   # the `contig` fast path
    CASES[f"m0_k{_ks}_kpad"] = case(0, 16, 24, _ks, 32, 3)                                     # k_pad > cin
    CASES[f"m0_k{_ks}_window"] = case(0, 16, 40, _ks, 32, 3, ci_begin=8, ci_count=20)          # a channel window strictly inside cin
    CASES[f"m0_k{_ks}_perm"] = case(0, 16, 32, _ks, 32, 3, perm=True)                          # pixel-shuffle row order
    CASES[f"m0_k{_ks}_rows"] = case(0, 12, 32, _ks, 32, 3, rows=16)                            # rows padded past cout
    CASES[f"m0_k{_ks}_all"] = case(0, 12, 40, _ks, 32, 5, ci_begin=8, ci_count=20, perm=True, rows=16)
# part lanes: pl = 0, 1, 1 (ragged), 2 (ragged), 6, 6 (ragged), 6 (two rounds and a ragged third) at cout * k_pad = 512 <= 16384
for _parts in (1, 2, 3, 5, 64, 65, 130):
    CASES[f"m0_parts{_parts}"] = case(0, 16, 24, 3, 32, _parts)
CASES["m0_parts65_contig"] = case(0, 16, 32, 3, 32, 65)
# cout * k_pad = 1152 is no multiple of the 1024 (one part lane) or 512 (two) pairs of a workgroup iteration
CASES["m0_ragged_pl0"] = case(0, 24, 48, 3, 48, 1)
CASES["m0_ragged_pl1"] = case(0, 24, 40, 3, 48, 2)
# workgroup counts: 8 and 16 (renumbered over the XCDs), 6 (plain numbering, ragged last workgroup)
CASES["m0_grid8"] = case(0, 64, 128, 3, 128, 1)
CASES["m0_grid8_perm"] = case(0, 64, 128, 1, 128, 1, perm=True)
CASES["m0_grid16_perm"] = case(0, 64, 128, 3, 128, 2, perm=True)
CASES["m0_grid6"] = case(0, 72, 80, 3, 80, 1)
CASES["m0_grid6_kpad"] = case(0, 72, 72, 3, 80, 1)
# flat-K (mode 2): the input-image source of Reconstruction.pre, permuted rows and a channel window
CASES["m2_k3"] = case(2, 16, 20, 3, 32, 3, ci_begin=16, ci_count=3, perm=True)
CASES["m2_k1"] = case(2, 16, 40, 1, 32, 2, ci_begin=8, ci_count=20, perm=True, rows=32)
# space-to-depth (mode 4), cin no multiple of 16; the part loop of unpack_kernel is unrolled four times
for _parts in (1, 3, 4, 5, 9):
    CASES[f"m4_k2_parts{_parts}"] = case(4, 24, 20, 2, 128, _parts)
    CASES[f"m4_k3_parts{_parts}"] = case(4, 24, 10, 3, 144, _parts, rows=32)


@pytest.mark.parametrize("name", list(CASES))
def test_unpack_parts(name):
    from pssr2_amd import ops
    c = CASES[name]
    mode, cout, cin, ks, k_pad, parts = c["mode"], c["cout"], c["cin"], c["ks"], c["k_pad"], c["parts"]
    rows = c["rows"] or cout
    taps = ks * ks if mode == 0 else 1
    perm = shuf2_perm(cout) if c["perm"] else None
    umap = unpack_map(mode, cout, cin, ks, k_pad, ci_begin=c["ci_begin"], ci_count=c["ci_count"], n_perm=perm)
    assert (PART_GRID.sum(parts) + OLD_GRID).units() <= 2.0 ** 24, "the sums are not exact in f32"
    addressed = torch.zeros(cout * cin * ks * ks, dtype=torch.bool)
    addressed[umap[umap >= 0]] = True
    addressed = addressed.view(cout, cin, ks, ks)
    if name.endswith(("_window", "_all")) or mode == 2:
        assert not bool(addressed.all()), "the window leaves nothing outside"
    perm_dev = None if perm is None else perm.to(torch.int32).cuda()
    for accumulate in (False, True):
        gen = torch.Generator().manual_seed(stable_seed(name, accumulate))
        slabs = dyadic(gen, (parts, rows, taps, k_pad), PART_GRID)
        old = dyadic(gen, (cout, cin, ks, ks), OLD_GRID)
        want = expected(unpack_reference(slabs, old, umap, accumulate), F32)
        src = slabs.float()
        src[:, cout:] = float("nan")
        src[:, :cout][:, umap < 0] = float("nan")
        dw = old.float().cuda()
        ops.unpack_conv_wgrad(src.cuda(), dw, mode=mode, ci_begin=c["ci_begin"], ci_count=c["ci_count"], n_perm=perm_dev, k_pad=k_pad,
                              accumulate=accumulate)
        got = dw.cpu()
        what = f"{name} accumulate={accumulate}"
        assert not bool(got.isnan().any()), f"{what}: a NaN from a padding row or a discarded column arrived"
        bad = (got != want) & addressed
        assert not bool(bad.any()), (f"{what}: {int(bad.sum())} addressed elements differ; first at {tuple(bad.nonzero()[0].tolist())}: "
                                     f"got {got[bad][0].item()!r}, want {want[bad][0].item()!r}")
        assert torch.equal(got.view(torch.int32)[~addressed], old.float().view(torch.int32)[~addressed]), \
            f"{what}: an element outside the map changed"
