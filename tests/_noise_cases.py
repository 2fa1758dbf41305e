"""The inputs, seeds and parameters of tests/test_gpu_noise_streams.py, and their expected values by tests/_noise_ref.py.

One place for both, because tests/test_noise_ref.py checks the premises of the GPU comparison (Poisson margin, fragile share) on the
CPU for exactly these cases: a seed that happens to put a value next to a decision is found, and changed, there.
numpy only; `reference(case)` is cached, so tests of one process share it and must not write into what it returns.
"""
from __future__ import annotations

from collections import namedtuple
from functools import lru_cache

import numpy as np

import _noise_ref as R

Case = namedtuple("Case", "id kind x p0 gain spread seed tile_offset flags")     # p0: intensity, or the salt-and-pepper amount

SMALL = (3, 1, 37, 53)           # per_tile = 1961: no multiple of the 256-thread workgroup, so tile boundaries fall inside workgroups
# Every launcher of csrc/crappify.hip starts at most 8192 workgroups (grid1d's cap) of 256 threads: 2,097,152 elements in one sweep
# of the grid, the rest by the grid-stride loop.  9 * 3 * 300 * 260 = 2,106,000 is just over it.
GRID_CAP_BLOCKS, BLOCK_THREADS = 8192, 256
STRIDE = (9, 3, 300, 260)
SEED_G = 0x123456789ABCDEF0
SEED_P = 0x0C0FFEE7654321AB
SEED_P_STRIDE = 0x0C0FFEE7654321AC   # 2.5 million rejection rounds: the seed next to it leaves one of them 5e-11 from tipping
SEED_S = 0xFEDCBA9876543210
SEED_B = 0x00000003DEADBEEF
SEED_CHAIN = 0x5EED00020000001F
CHAIN_STEP = 7919                # DevicePairGenerator seeds stage i with seed + 7919 * i


@lru_cache(maxsize=None)
def _x(name):
    rng = np.random.default_rng({"gauss": 1, "poisson": 2, "stride_u8": 3, "stride_pois": 4, "blur": 5, "chain": 6}.get(name, 0))
    if name == "gauss":          # uint8 values, some at the ends of the range so that the clip acts on both sides
        x = rng.integers(0, 256, SMALL).astype(np.float32)
        x.reshape(3, -1)[:, 100:108] = 0.0
        x.reshape(3, -1)[:, 1900:1908] = 255.0
    elif name == "poisson":      # both samplers and their switch at 10, lambda <= 0, fractions, and values beyond the uint8 range
        x = np.where(rng.random(SMALL) < 0.5, rng.uniform(0, 20, SMALL), rng.uniform(0, 300, SMALL)).astype(np.float32)
        special = np.array([0.0, -3.5, -0.25, 0.5, 2.75, 9.999, 10.0, 255.0, 300.0], dtype=np.float32)
        x.reshape(3, -1)[:, 200:200 + 40 * special.size] = np.repeat(special, 40)
    elif name == "salt":         # a non-integer value: an untouched pixel is recognisable
        x = np.full(SMALL, 100.25, dtype=np.float32)
    elif name == "stride_u8":
        x = rng.integers(0, 256, STRIDE).astype(np.float32)
    elif name == "stride_salt":
        x = np.full(STRIDE, 100.25, dtype=np.float32)
    elif name == "stride_pois":  # lambda >= 10 everywhere: the rejection sampler alone, a few rounds per pixel
        x = rng.uniform(10, 255, STRIDE).astype(np.float32)
    elif name == "blur":
        x = rng.uniform(0, 255, (16, 2, 20, 24)).astype(np.float32)
    elif name == "chain":
        x = rng.integers(0, 256, (4, 1, 256, 256), dtype=np.uint8)
    x.setflags(write=False)
    return x


def _cases():
    out = []
    for flags in (0, R.CLIP, R.ROUND_CLIP):
        for spread in (0.0, 3.0):
            out.append(Case(f"gaussian-f{flags}-s{spread:g}", "gaussian", "gauss", 13.0, 2.0, spread, SEED_G, 5, flags))
    out.append(Case("gaussian-offset-2^40+3", "gaussian", "gauss", 13.0, 2.0, 3.0, SEED_G, (1 << 40) + 3, R.ROUND_CLIP))
    out.append(Case("gaussian-seed0-offset0", "gaussian", "gauss", 13.0, 2.0, 0.0, 0, 0, 0))
    for intensity, gain, spread in ((1.0, 0.0, 0.0), (0.5, 4.0, 0.0), (0.7, 1.5, 0.2)):
        for flags in (0, R.ROUND_CLIP):
            out.append(Case(f"poisson-i{intensity:g}-g{gain:g}-s{spread:g}-f{flags}", "poisson", "poisson", intensity, gain, spread, SEED_P, 5, flags))
    for amount in (0.05, 0.5):
        for spread in (0.0, 0.02):
            for flags in (0, R.ROUND_CLIP):
                out.append(Case(f"saltpepper-a{amount:g}-s{spread:g}-f{flags}", "saltpepper", "salt", amount, 3.0, spread, SEED_S, 5, flags))
    out.append(Case("stride-gaussian", "gaussian", "stride_u8", 13.0, 2.0, 3.0, SEED_G, 5, R.ROUND_CLIP))
    out.append(Case("stride-saltpepper", "saltpepper", "stride_salt", 0.05, 3.0, 0.02, SEED_S, 5, 0))
    out.append(Case("stride-poisson", "poisson", "stride_pois", 0.7, 1.5, 0.2, SEED_P_STRIDE, 5, R.ROUND_CLIP))
    return out


CASES = _cases()
SMALL_CASES = [c for c in CASES if not c.id.startswith("stride-")]
STRIDE_CASES = [c for c in CASES if c.id.startswith("stride-")]
BLUR_CASES = {"A": (2.0, 0.5), "B": (0.3, 1.0)}      # sigma, spread; 16 tiles, gain 1.5, offset 5, SEED_B
BLUR_GAIN, BLUR_OFFSET = 1.5, 5


def case_input(case):
    return _x(case.x)


def blur_input():
    return _x("blur")


def chain_input():
    return _x("chain")


Ref = namedtuple("Ref", "out fragile margin")        # margin: inf where the kernel takes no comparison that could tip


@lru_cache(maxsize=None)
def reference(case):
    x = case_input(case)
    res = getattr(R, case.kind)(x, case.p0, case.gain, case.spread, case.seed, case.tile_offset, case.flags)
    ref = Ref(res[0], res[1], res[2] if len(res) > 2 else np.inf)
    ref.out.setflags(write=False)
    ref.fragile.setflags(write=False)
    return ref


@lru_cache(maxsize=None)
def chain_reference():
    """MultiCrappifier(AdditiveGaussian(13, spread=2), Poisson(0.5, spread=0.1)) as DevicePairGenerator(4, ..., seed=SEED_CHAIN) runs it
    at tile_offset 0: the Pillow reduction, the Gaussian stage with the seed and the clip between stages, then the Poisson stage with
    seed + 7919 and round-and-clip.  Returns (clean LR float32, Ref of the final LR); fragile is the union of both stages'."""
    from oracle import pairs_ref as P
    hr = chain_input()
    lr = P.pil_bilinear_u8(hr, hr.shape[-2] // 4, hr.shape[-1] // 4).astype(np.float32)
    x1, f1 = R.gaussian(lr, 13.0, 0.0, 2.0, SEED_CHAIN, 0, R.CLIP)
    x2, f2, margin = R.poisson(x1, 0.5, 0.0, 0.1, (SEED_CHAIN + CHAIN_STEP) % (1 << 64), 0, R.ROUND_CLIP)
    return lr, Ref(x2, f1 | f2, margin)
