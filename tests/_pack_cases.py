"""The case table of the weight-pack tests (tests/test_gpu_pack_exact.py; tests/test_conv_exact_helpers.py perturbs the references of
the same cases on the CPU).  The shapes are the smallest at which each path of csrc/pack.hip can still go wrong."""
import functools

import torch

from _conv_exact import pack_dims, pack_map, pack_reference, pack_source, shuf2_perm, stable_seed

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
ALL = (F32, BF16, F16)
DT_NAME = {F32: "f32", BF16: "bf16", F16: "f16"}


def case(mode, cout, cin, ks, *, ci_begin=0, ci_count=None, perm=False, dtypes=ALL, center=False):
    return dict(mode=mode, cout=cout, cin=cin, ks=ks, ci_begin=ci_begin, ci_count=cin - ci_begin if ci_count is None else ci_count,
                perm=perm, dtypes=dtypes, center=center)


CASES = {}
# pack_tiles33 (ks = 3, modes 0 and 1): one LDS tile per (K chunk, 128 columns)
CASES["t33_m0"] = case(0, 16, 24, 3)
CASES["t33_m1"] = case(1, 16, 24, 3)
CASES["t33_m0_oddk"] = case(0, 16, 21, 3)                                   # odd GEMM-K: the `k + 1 < gk` guard of the k pairs
CASES["t33_m1_oddk"] = case(1, 21, 16, 3)
CASES["t33_m0_2tiles"] = case(0, 130, 24, 3)                                # two N tiles, the second ragged
CASES["t33_m1_2tiles"] = case(1, 16, 130, 3)
CASES["t33_m0_window"] = case(0, 16, 40, 3, ci_begin=8, ci_count=19)
CASES["t33_m1_window"] = case(1, 16, 40, 3, ci_begin=8, ci_count=19)
CASES["t33_m0_perm"] = case(0, 16, 24, 3, perm=True)
CASES["t33_m1_perm"] = case(1, 16, 24, 3, perm=True)
CASES["t33_m0_all"] = case(0, 132, 40, 3, ci_begin=8, ci_count=19, perm=True)
CASES["t33_m1_all"] = case(1, 21, 140, 3, ci_begin=8, ci_count=130, perm=True)
# pack_elems: one packed element per thread
CASES["el_m0_k1"] = case(0, 16, 24, 1)
CASES["el_m1_k1"] = case(1, 16, 24, 1)
CASES["el_m0_k1_all"] = case(0, 132, 40, 1, ci_begin=8, ci_count=19, perm=True)
CASES["el_m1_k1_all"] = case(1, 21, 140, 1, ci_begin=8, ci_count=130, perm=True)
for _m in (2, 3):
    CASES[f"el_m{_m}_k3_head"] = case(_m, 16, 20, 3, ci_begin=16, ci_count=3, perm=True)     # the input-image source of Reconstruction.pre
    CASES[f"el_m{_m}_k1"] = case(_m, 24, 20, 1, ci_begin=4, ci_count=13, perm=True)
    CASES[f"el_m{_m}_k2"] = case(_m, 24, 20, 2, ci_begin=4, ci_count=13, perm=True)
for _m in (4, 5):
    CASES[f"el_m{_m}_k2"] = case(_m, 24, 20, 2)                                              # cpad 32
    CASES[f"el_m{_m}_k3"] = case(_m, 24, 10, 3)
# the single launch has at most 4096 workgroups of 256 elements per trip: 1.18 M packed elements take a second one
CASES["grid_m0"] = case(0, 1100, 1024, 1, dtypes=(BF16, F32))
CASES["grid_m1"] = case(1, 1100, 1024, 1, dtypes=(BF16, F32))

# the batch launch has 384 workgroups per item: more (K chunk, N tile) pairs than that for pack_tiles33, more than 384 * 256 elements
# for pack_elems
BIG = {
    "big_bf16_m0": case(0, 2000, 392, 3, dtypes=(BF16,)),       # 25 chunks x 16 N tiles
    "big_bf16_m1": case(1, 2000, 392, 3, dtypes=(BF16,)),       # 125 x 4
    "big_f32_m0": case(0, 2000, 200, 3, dtypes=(F32,)),         # 26 x 16
    "big_f32_m1": case(1, 2000, 200, 3, dtypes=(F32,)),         # 250 x 2
    "big_el_m0": case(0, 512, 256, 1, dtypes=(BF16, F32)),      # 131 072 elements
    "big_el_m1": case(1, 512, 256, 1, dtypes=(BF16,)),
}
# centre items: the source is [cout, cin, 1, 1], packed as the centre tap of a 3x3 kernel
CENTER = {f"center_m{_m}{'_perm' if _p else ''}": case(_m, 24, 20, 3, perm=_p, center=True) for _m in (2, 3) for _p in (False, True)}
CENTER["center_m2_window"] = case(2, 24, 20, 3, ci_begin=4, ci_count=13, perm=True, center=True)
CENTER["center_m3_window"] = case(3, 24, 20, 3, ci_begin=4, ci_count=13, perm=True, center=True)

EVERY = {**CASES, **BIG, **CENTER}


def pad_to(v, m):
    return (v + m - 1) // m * m


def perm_of(name):
    """the case's n_perm (int64): the pixel-shuffle row order where cout allows it, a seeded permutation otherwise"""
    c = EVERY[name]
    if not c["perm"]:
        return None
    if c["cout"] % 4 == 0:
        return shuf2_perm(c["cout"])
    return torch.randperm(c["cout"], generator=torch.Generator().manual_seed(stable_seed("perm", name)))


def geometry(name):
    """(taps, k_pad, n_pad) as ops.pack_conv_weight sizes them: GEMM-K rounded up to 16, GEMM-N to 128"""
    c = EVERY[name]
    taps, gk, gn = pack_dims(c["mode"], c["cout"], c["cin"], c["ks"], c["ci_count"])
    return taps, pad_to(gk, 16), pad_to(gn, 128)


def case_map(name, dt):
    """pack_map of a case (kept for the small cases; the maps of the big ones have millions of entries)"""
    return _case_map(name, dt) if name in BIG or name.startswith("grid") else _kept_map(name, dt)


@functools.lru_cache(maxsize=None)
def _kept_map(name, dt):
    return _case_map(name, dt)


def _case_map(name, dt):
    c = EVERY[name]
    _, k_pad, n_pad = geometry(name)
    return pack_map(c["mode"], c["cout"], c["cin"], c["ks"], k_pad, n_pad, dt, ci_begin=c["ci_begin"], ci_count=c["ci_count"],
                    n_perm=perm_of(name), center=c["center"])


def source_shape(name):
    c = EVERY[name]
    ks = 1 if c["center"] else c["ks"]
    return c["cout"], c["cin"], ks, ks


def source(name, dt, variant=0, nan_outside=False, pmap=None):
    """the f32 source of a case (variant: another seed, for the second pack into the same buffer)"""
    pmap = case_map(name, dt) if pmap is None else pmap
    return pack_source((name, DT_NAME[dt], variant), source_shape(name), pmap, nan_outside=nan_outside)


def reference(name, dt, w, pmap=None):
    return pack_reference(w, case_map(name, dt) if pmap is None else pmap, dt)
