"""ops.flatk_bwd_pair (csrc/pre_xcol_bwd.hip): both gradients of Reconstruction.pre's input-image source from one pass over d(pre).

Op level: float64 numpy reference from the same 16-bit-rounded inputs (dx_ref = dy . W1, dW_ref = dy^T . x).  No tolerance is fixed in
advance: the two launches the kernel replaces (a flat-K conv2d and a 1-tap weight gradient) run on the same inputs and the new kernel's
error may be at most twice theirs (a different summation order and nothing more); dx is compared after both are rounded to storage.
Two runs of the new kernel must agree bit for bit.

Engine level: one training forward + backward with PSSR_XCOL_FUSE=1 and one with =0, each in its own process (the switch is read at
import).  Every parameter gradient is bit-identical except the input-source slice of reconstruction.pre.weight and norm.weight / bias
(which are sums over d(xcol)): those agree within twice the relative error the old path itself shows against float64 at the op level
on the same pixel count and width.  The default ResUNet runs at 48 x 48 (the smallest input its five levels train at: the deepest
feature map must be at least 3 pixels wide), RDResUNet at 32 x 32.

Measured on MI355X, max |error| against float64 (new kernel / the two old launches):
    bf16    64 px x  256   dW 6.9e-07 / 6.9e-07   dx (stored) 3.8e-03 / 3.8e-03
    f16     64 px x  256   dW 8.9e-07 / 8.9e-07   dx (stored) 4.8e-04 / 4.8e-04
    bf16   480 px x 1024   dW 3.9e-06 / 2.6e-06   dx (stored) 1.5e-02 / 1.5e-02
    f16    480 px x 1024   dW 4.0e-06 / 3.1e-06   dx (stored) 9.8e-04 / 9.8e-04
    bf16    64 px x  576   dW 6.0e-07 / 6.0e-07   dx (stored) 7.5e-03 / 7.5e-03
    bf16 32768 px x 1024   dW 4.5e-05 / 5.3e-05   dx (stored) 1.5e-02 / 1.5e-02
    bf16 41600 px x 1024   dW 5.0e-05 / 6.6e-05   dx (stored) 1.6e-02 / 1.6e-02
Engine level, max|new - old| / max|old|: reconstruction.pre.weight (input slice) 1.5e-07 (ResUNet, bound 3.1e-07) and 1.6e-07
(RDResUNet, bound 1.7e-07); norm.weight / norm.bias came out bit-identical in both."""
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
BF16, F16 = torch.bfloat16, torch.float16
KX = 16


@functools.lru_cache(maxsize=None)
def _case(n, h, w, cout, dt):
    """Inputs, the float64 reference and the results of the two old launches (computed once per case, never modified)."""
    from pssr2_amd import ops
    code = ops.dtype_code(dt)
    g = torch.Generator().manual_seed(1000 * n + 10 * h + w + cout)
    npix = n * h * w
    dy = torch.randn(npix, cout, generator=g)
    dy = (dy * (torch.rand(npix, cout, generator=g) < 0.5)).to(dt)            # about half exactly zero, like a ReLU-masked gradient
    img = (torch.rand(n, 1, h, w, generator=g) * 255).cuda()
    xcol = torch.empty(n, h, w, KX, dtype=dt, device="cuda")
    ops.input_im2col(img, xcol, torch.ones(1, device="cuda"), torch.zeros(1, device="cuda"), code)      # x / 128 - 1, zeros at the border taps
    weight = (torch.randn(cout, 1, 3, 3, generator=g) * 0.05).cuda()
    perm = torch.randperm(cout, generator=g).to(torch.int32).cuda()
    dy = dy.cuda().view(n, h, w, cout)
    # float64 reference
    dy64 = dy.view(npix, cout).double().cpu().numpy()
    x64 = xcol.view(npix, KX).double().cpu().numpy()
    assert (x64[:, 9:] == 0).all() and (x64[:w, :3] == 0).all()               # padding columns, and the top taps of the first image row
    w1 = np.zeros((cout, KX))
    w1[:, :9] = weight.view(cout, 9)[perm.long()].to(dt).double().cpu().numpy()          # rounded to storage as the packed weight is
    dx_ref = dy64 @ w1
    dw_ref = np.zeros((cout, 1, 3, 3))
    dw_ref.reshape(cout, 9)[perm.long().cpu().numpy()] = (dy64.T @ x64)[:, :9]
    # the two launches of today
    parts = ops.conv2d_wgrad_parts(dy, cout, xcol, KX, 1, n=n, h=h, w=w, dtype=code)
    dw_old = torch.zeros(cout, 1, 3, 3, device="cuda")
    ops.unpack_conv_wgrad(parts, dw_old, mode=2, ci_begin=0, ci_count=1, n_perm=perm, k_pad=KX)
    pw = ops.pack_conv_weight(weight, code, mode=3, ci_begin=0, ci_count=1, n_perm=perm)
    dx_old = torch.full((n, h, w, KX), 7.0, dtype=dt, device="cuda")
    ops.conv2d(dy, cout, pw, dx_old, KX, n=n, h=h, w=w)
    torch.cuda.synchronize()
    return dict(code=code, dy=dy, xcol=xcol, weight=weight, perm=perm, dx_ref=dx_ref, dw_ref=dw_ref,
                dw_old=dw_old.double().cpu().numpy(), dx_old=dx_old.view(npix, KX).double().cpu().numpy())


def _new(c, n, h, w, cout, dt):
    from pssr2_amd import ops
    dx = torch.full((n, h, w, KX), 7.0, dtype=dt, device="cuda")
    dw1 = ops.flatk_bwd_pair(c["dy"], cout, c["xcol"], dx, c["weight"], c["code"], ci_begin=0, ci_count=1, n_perm=c["perm"])
    dw = torch.zeros(cout, 1, 3, 3, device="cuda")
    ops.unpack_conv_wgrad(dw1, dw, mode=2, ci_begin=0, ci_count=1, n_perm=c["perm"], k_pad=KX)
    torch.cuda.synchronize()
    return dx, dw


def _errors(c, dx, dw):
    e_dw_new = np.abs(dw.double().cpu().numpy() - c["dw_ref"]).max()
    e_dw_old = np.abs(c["dw_old"] - c["dw_ref"]).max()
    e_dx_new = np.abs(dx.view(-1, KX).double().cpu().numpy() - c["dx_ref"]).max()
    e_dx_old = np.abs(c["dx_old"] - c["dx_ref"]).max()
    return e_dw_new, e_dw_old, e_dx_new, e_dx_old


CASES = [(1, 8, 8, 256, BF16), (1, 8, 8, 256, F16),                # 64 px: a single tile, a single workgroup
         (2, 12, 20, 1024, BF16), (2, 12, 20, 1024, F16),          # 480 px: a partial last tile
         (1, 8, 8, 576, BF16),                                     # a last chunk with 64 of its 256 channels
         (8, 64, 64, 1024, BF16)]                                  # 32768 px: one tile per workgroup


@pytest.mark.parametrize("n,h,w,cout,dt", CASES)
def test_op_against_f64_and_the_two_old_launches(n, h, w, cout, dt):
    from pssr2_amd import ops
    assert ops.flatk_bwd_pair_supported(ops.dtype_code(dt), cout, KX)
    c = _case(n, h, w, cout, dt)
    dx, dw = _new(c, n, h, w, cout, dt)
    e_dw_new, e_dw_old, e_dx_new, e_dx_old = _errors(c, dx, dw)
    print(f"[flatk_bwd_pair {dt} {n * h * w} px x {cout}] max|dW - ref| new {e_dw_new:.3e} old {e_dw_old:.3e}   "
          f"max|dx - ref| (stored) new {e_dx_new:.3e} old {e_dx_old:.3e}")
    assert np.isfinite(dx.float().cpu().numpy()).all()
    assert e_dw_new <= 2 * e_dw_old
    assert e_dx_new <= 2 * e_dx_old
    # bit-reproducible
    dx2, dw2 = _new(c, n, h, w, cout, dt)
    assert torch.equal(dx.view(torch.int16), dx2.view(torch.int16)) and torch.equal(dw, dw2)


def test_persistent_loop_several_tiles_per_workgroup():
    """More tiles than workgroups (32768 px = 512 tiles are one each on 256 CUs): 41600 px = 650 tiles, one or two per workgroup, so the
    prefetch crosses chunk and tile boundaries."""
    from pssr2_amd import _lib as L
    n, h, w, cout, dt = 5, 64, 130, 1024, BF16
    parts = L.lib().pssr_flatk_bwd_pair_parts(n * h * w)
    assert 0 < parts < n * h * w // 64
    c = _case(n, h, w, cout, dt)
    dx, dw = _new(c, n, h, w, cout, dt)
    e_dw_new, e_dw_old, e_dx_new, e_dx_old = _errors(c, dx, dw)
    print(f"[flatk_bwd_pair persistent, {parts} workgroups] dW new {e_dw_new:.3e} old {e_dw_old:.3e}   dx new {e_dx_new:.3e} old {e_dx_old:.3e}")
    assert e_dw_new <= 2 * e_dw_old and e_dx_new <= 2 * e_dx_old


def test_predicate_rejects_what_the_kernel_does_not_take():
    from pssr2_amd import _lib as L
    from pssr2_amd import ops
    assert not ops.flatk_bwd_pair_supported(L.F32, 1024, 16)
    assert not ops.flatk_bwd_pair_supported(L.BF16, 96, 16)          # not a multiple of 64
    assert not ops.flatk_bwd_pair_supported(L.BF16, 1088, 16)        # wider than four chunks
    assert not ops.flatk_bwd_pair_supported(L.BF16, 1024, 32)        # three input channels: 27 taps
    assert ops.flatk_bwd_pair_supported(L.F16, 256, 16) and ops.flatk_bwd_pair_supported(L.BF16, 1024, 16)
    # the entry point refuses too, before any launch
    t = torch.zeros(64, 1024, device="cuda")
    assert L.lib().pssr_flatk_bwd_pair(L.ptr(t), 1024, 0, 1024, L.ptr(t), 16, 0, L.ptr(t), 16, 0, 16, L.ptr(t), 9, 0, 9, None, L.ptr(t), 1, L.ptr(t), 64,
                                       L.F32, None) != 0


# ---------------------------------------------------------------------------------------------------------------------
# engine level
_WORKER = r"""
import sys
import torch
sys.path.insert(0, sys.argv[1])
from pssr2_amd import engine, models
kind, size, out = sys.argv[2], int(sys.argv[3]), sys.argv[4]
torch.manual_seed(11)
if kind == "resunet":
    model = models.ResUNet()
else:
    model = models.RDResUNet(channels=1, hidden=[64, 64, 64], scale=4, depth=1, rdnet_init=32, growth_rates=[16, 24, 32], ds_blocks=[False, True, True],
                             ese_blocks=[False, True, True], n_blocks=[2, 2, 1])
model.cuda().train()
model.compute_dtype = torch.bfloat16
g = torch.Generator().manual_seed(12)
x = (torch.rand(2, 1, size, size, generator=g) * 255).cuda()
target = (torch.rand(2, 1, 4 * size, 4 * size, generator=g) * 255).cuda()
y = model(x)
torch.nn.functional.mse_loss(y / 255, target / 255).backward()
torch.cuda.synchronize()
torch.save({"fuse": engine._XCOL_FUSE, "grads": {k: p.grad.detach().cpu() for k, p in model.named_parameters()}}, out)
"""


def _engine_grads(tmp_path, kind, size, fuse):
    out = tmp_path / f"{kind}_{fuse}.pt"
    env = dict(os.environ, PSSR_XCOL_FUSE=str(fuse))
    subprocess.run([sys.executable, "-c", _WORKER, str(ROOT), kind, str(size), str(out)], check=True, env=env, timeout=300)
    d = torch.load(out)
    assert d["fuse"] == bool(fuse)
    return d["grads"]


@pytest.mark.parametrize("kind,size", [("resunet", 48), ("rdresunet", 32)])
def test_engine_gradients_fused_against_separate_launches(tmp_path, kind, size):
    new = _engine_grads(tmp_path, kind, size, 1)
    old = _engine_grads(tmp_path, kind, size, 0)
    # the old path's own relative error against float64 at this pixel count and width (bf16): the yardstick for the three that change
    cout, h0 = new["reconstruction.pre.weight"].shape[0], new["reconstruction.pre.weight"].shape[1] - 1      # one input channel
    assert cout == 16 * h0
    c = _case(2, size, size, cout, BF16)
    rel_dw = np.abs(c["dw_old"] - c["dw_ref"]).max() / np.abs(c["dw_ref"]).max()
    rel_dx = np.abs(c["dx_old"] - c["dx_ref"]).max() / np.abs(c["dx_ref"]).max()
    changed = ("reconstruction.pre.weight", "norm.weight", "norm.bias")
    assert set(changed) <= set(new)
    for k in new:
        a, b = new[k], old[k]
        assert torch.isfinite(a).all(), k
        if k not in changed:
            assert torch.equal(a, b), k
            continue
        if k == "reconstruction.pre.weight":
            assert torch.equal(a[:, :h0], b[:, :h0])                 # the feature-map source is untouched
            a, b, bound = a[:, h0:], b[:, h0:], 2 * rel_dw
        else:
            bound = 2 * rel_dx
        rel = ((a - b).abs().max() / b.abs().max()).item()
        print(f"[{kind} {k}] max|new - old| / max|old| = {rel:.3e}  (bound {bound:.3e})")
        assert b.abs().max() > 0 and rel <= bound, k
