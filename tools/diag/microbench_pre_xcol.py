"""Reconstruction.pre's input-image source, backward, at the c2 shape (batch 32, 128^2, d(pre) 1024 wide, bf16): ops.flatk_bwd_pair (one pass
over d(pre)) against the two launches it replaces (1-tap weight gradient + flat-K data gradient).  us and GB/s of algorithmic bytes =
npix * (cout + 2 kx) * 2 plus the partial slabs written and read back."""
import sys; sys.path.insert(0, str(__import__('pathlib').Path(__file__).resolve().parents[2]))
import torch
from pssr2_amd import ops, _lib as L
N, H, W, COUT, KX, H0 = 32, 128, 128, 1024, 16, 64
if len(sys.argv) > 1:
    N = int(sys.argv[1])
code = L.BF16
npix = N * H * W
dy = (torch.randn(N, H, W, COUT, device="cuda") * (torch.rand(N, H, W, COUT, device="cuda") < 0.5)).to(torch.bfloat16)
img = torch.rand(N, 1, H, W, device="cuda") * 255
xcol = torch.empty(N, H, W, KX, dtype=torch.bfloat16, device="cuda")
ops.input_im2col(img, xcol, torch.ones(1, device="cuda"), torch.zeros(1, device="cuda"), code)
weight = torch.randn(COUT, H0 + 1, 3, 3, device="cuda") * 0.05
perm = torch.randperm(COUT, device="cuda").to(torch.int32)
dx = torch.empty_like(xcol)
slot = torch.zeros_like(weight)
pw1 = ops.pack_conv_weight(weight, code, mode=3, ci_begin=H0, ci_count=1, n_perm=perm)
spec = dict(mode=2, ci_begin=H0, ci_count=1, n_perm=perm, k_pad=KX)


def timeit(fn, n=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def old_wgrad():
    ops.unpack_conv_wgrad(ops.conv2d_wgrad_parts(dy, COUT, xcol, KX, 1, n=N, h=H, w=W, dtype=code), slot, **spec)


def old_dgrad():
    ops.conv2d(dy, COUT, pw1, dx, KX, n=N, h=H, w=W)


def new():
    ops.unpack_conv_wgrad(ops.flatk_bwd_pair(dy, COUT, xcol, dx, weight, code, ci_begin=H0, ci_count=1, n_perm=perm), slot, **spec)


slab = COUT * KX * 4
stream = npix * (COUT + 2 * KX) * 2
parts_new = L.lib().pssr_flatk_bwd_pair_parts(npix)
t_w, t_d, t_n = timeit(old_wgrad), timeit(old_dgrad), timeit(new)
b_w, b_d = npix * (COUT + KX) * 2 + 2 * 32 * slab, npix * (COUT + KX) * 2
b_n = stream + 2 * parts_new * slab
print(f"shape: {npix} px x {COUT} ch, d(pre) {npix * COUT * 2 / 1e9:.3f} GB")
print(f"old weight gradient + unpack {t_w:7.1f} us  {b_w / t_w / 1e3:7.1f} GB/s")
print(f"old data gradient            {t_d:7.1f} us  {b_d / t_d / 1e3:7.1f} GB/s")
print(f"old, both                    {t_w + t_d:7.1f} us")
print(f"flatk_bwd_pair + unpack      {t_n:7.1f} us  {b_n / t_n / 1e3:7.1f} GB/s   ({parts_new} slabs)   ratio to old {t_n / (t_w + t_d):.2f}")
