"""Thin Python wrappers over the C ABI (one function per entry point of include/pssr_mi355.h).

Tensors are only carriers of device memory here: every wrapper passes raw pointers, sizes and the
current HIP stream to libpssr_mi355.so.  Nothing in this module computes with torch.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L

TORCH_DTYPE = {L.F32: torch.float32, L.BF16: torch.bfloat16, L.F16: torch.float16}


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return L.F32
    if dt == torch.bfloat16:
        return L.BF16
    if dt == torch.float16:
        return L.F16
    raise ValueError(f"unsupported compute dtype {dt}; use torch.float32, torch.bfloat16 or torch.float16")


def pad_to(v: int, m: int) -> int:
    return (v + m - 1) // m * m


class PackedWeight:
    """A conv weight in the kernel's K-chunked layout plus the GEMM dims it was packed with."""
    __slots__ = ("data", "taps", "k_pad", "n_pad", "dtype")

    def __init__(self, data, taps, k_pad, n_pad, dtype):
        self.data, self.taps, self.k_pad, self.n_pad, self.dtype = data, taps, k_pad, n_pad, dtype


def pack_conv_weight(w: torch.Tensor, dtype: int, mode: int = 0, ci_begin: int = 0, ci_count: int | None = None,
                     n_perm: torch.Tensor | None = None, out: PackedWeight | None = None) -> PackedWeight:
    """OIHW f32 -> packed (mode 0 forward, 1 dgrad, 2 flat-K im2col, 3 flat-K dgrad)."""
    assert w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and w.dim() == 4
    cout, cin, ks, _ = w.shape
    ci_count = cin - ci_begin if ci_count is None else ci_count
    s2dk = ks * ks * pad_to(cin, 16)
    gk = ci_count if mode == 0 else cout if mode in (1, 3, 5) else s2dk if mode == 4 else ci_count * ks * ks
    gn = ci_count if mode == 1 else ci_count * ks * ks if mode == 3 else s2dk if mode == 5 else cout
    taps = 1 if mode >= 2 else ks * ks
    k_pad, n_pad = pad_to(gk, 16), pad_to(gn, 128)
    if out is None:
        nbytes = L.lib().pssr_packed_weight_bytes(taps, k_pad, n_pad, dtype)
        out = PackedWeight(torch.empty(nbytes, dtype=torch.uint8, device=w.device), taps, k_pad, n_pad, dtype)
    L.check(L.lib().pssr_pack_conv_weight(L.ptr(w), L.ptr(out.data), cout, cin, ks, ci_begin, ci_count, mode,
                                          L.ptr(n_perm), k_pad, n_pad, dtype, L.stream_ptr()), "pssr_pack_conv_weight")
    return out


# [True] while a forward pass issues its launches (Engine.forward): nothing runs beside them, which conv2d passes on as PSSR_FLAG_SOLO
SOLO = [False]


def conv2d(x, cin0, w0: PackedWeight, out, cout, *, n, h, w, in0_coff=0, out_coff=0, bias=None,
           x1=None, cin1=0, w1: PackedWeight | None = None, in1_coff=0,
           pro_scale=None, pro_shift=None, epilogue=L.EPI_STORE, flags=0,
           aux=None, aux_coff=0, aux_scale=None, aux_shift=None, aux_mean=None, aux_invstd=None, stats=None,
           in0_blk=0, out_blk=0, aux_blk=0, out_scale=1.0, out_shift=0.0, gelu_in=False, head_w=None, head_q=None):
    """x/out/aux: NHWC tensors [n, h, w, cstride] in the compute dtype (channel slices via *_coff).  EPI_HEADQ: ``out`` is unused (pass
    ``head_q``), the tap products go to ``head_q`` [9, 16, n, h, w] f32."""
    d = L.ConvDesc()
    d.dtype = w0.dtype
    d.n, d.h, d.w = n, h, w
    d.in0, d.in0_cstride, d.in0_coff, d.cin0, d.taps0, d.w0 = L.ptr(x), x.shape[-1], in0_coff, cin0, w0.taps, L.ptr(w0.data)
    if w1 is not None:
        d.in1, d.in1_cstride, d.in1_coff, d.cin1, d.taps1, d.w1 = L.ptr(x1), x1.shape[-1], in1_coff, cin1, w1.taps, L.ptr(w1.data)
        assert w1.n_pad == w0.n_pad and w1.dtype == w0.dtype
    d.prologue = L.PRO_GELU if gelu_in else L.PRO_BN_RELU if pro_scale is not None else L.PRO_NONE
    d.pro_scale, d.pro_shift = L.ptr(pro_scale), L.ptr(pro_shift)
    d.out, d.out_cstride, d.out_coff, d.cout, d.n_pad = L.ptr(out), out.shape[-1], out_coff, cout, w0.n_pad
    d.bias = L.ptr(bias)
    d.epilogue, d.flags = epilogue, flags | (L.FLAG_SOLO if SOLO[0] else 0)
    if aux is not None:
        d.aux, d.aux_cstride, d.aux_coff = L.ptr(aux), aux.shape[-1], aux_coff
    d.aux_scale, d.aux_shift, d.aux_mean, d.aux_invstd = L.ptr(aux_scale), L.ptr(aux_shift), L.ptr(aux_mean), L.ptr(aux_invstd)
    d.stats = L.ptr(stats)
    d.in0_blk, d.out_blk, d.aux_blk, d.out_scale, d.out_shift = in0_blk, out_blk, aux_blk, out_scale, out_shift
    if epilogue == L.EPI_FINAL:      # f32 NCHW output [n, cout, h, w]
        d.out_cstride, d.out_coff = cout, 0
    if epilogue == L.EPI_HEADQ:
        d.out_cstride, d.out_coff = cout, 0
    if epilogue == L.EPI_HEADQ or flags & L.FLAG_HEADQ:
        d.head_w, d.head_q = L.ptr(head_w), L.ptr(head_q)
    ws_bytes = L.lib().pssr_conv2d_workspace_bytes(C.byref(d))      # > 0: the library wants to split K (under-filled grid)
    if ws_bytes > 0:
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=out.device)
        d.workspace, d.workspace_bytes = L.ptr(ws), ws_bytes
    L.check(L.lib().pssr_conv2d(C.byref(d), L.stream_ptr()), "pssr_conv2d")
    return out


def _wgrad_desc(dy, cout, x, cin_pad, taps, *, n, h, w, dtype, dy_coff=0, in_coff=0, dy_blk=0, in_blk=0, pro_scale=None, pro_shift=None,
                gelu_in=False):
    d = L.WgradDesc()
    d.dtype, d.n, d.h, d.w = dtype, n, h, w
    d.dy, d.dy_cstride, d.dy_coff, d.dy_blk, d.cout = L.ptr(dy), dy.shape[-1], dy_coff, dy_blk, cout
    d.in_, d.in_cstride, d.in_coff, d.in_blk, d.cin_pad = L.ptr(x), x.shape[-1], in_coff, in_blk, cin_pad
    d.taps = taps
    d.prologue = L.PRO_GELU if gelu_in else L.PRO_BN_RELU if pro_scale is not None else L.PRO_NONE
    d.pro_scale, d.pro_shift = L.ptr(pro_scale), L.ptr(pro_shift)
    return d


def conv2d_wgrad(dy, cout, x, cin_pad, taps, dw, **kw):
    """Atomic mode: dw (f32 [cout, taps, cin_pad], zeroed by the caller) += dy^T (*) prologue(x)."""
    d = _wgrad_desc(dy, cout, x, cin_pad, taps, **kw)
    d.dw, d.dw_parts = L.ptr(dw), 0
    L.check(L.lib().pssr_conv2d_wgrad(C.byref(d), L.stream_ptr()), "pssr_conv2d_wgrad")
    return dw


def conv2d_wgrad_parts(dy, cout, x, cin_pad, taps, **kw):
    """Partial-slab mode: returns dw f32 [parts, cout, taps, cin_pad] (uninitialised workspace filled by the kernel); the
    parts are summed by ``unpack_conv_wgrad``."""
    d = _wgrad_desc(dy, cout, x, cin_pad, taps, **kw)
    parts = L.lib().pssr_conv2d_wgrad_parts(C.byref(d))
    if parts <= 0:
        L.check(parts if parts < 0 else -1, "pssr_conv2d_wgrad_parts")
    dw = torch.empty(parts, cout, taps, cin_pad, dtype=torch.float32, device=dy.device)
    d.dw, d.dw_parts = L.ptr(dw), parts
    L.check(L.lib().pssr_conv2d_wgrad(C.byref(d), L.stream_ptr()), "pssr_conv2d_wgrad")
    return dw


def unpack_conv_wgrad(dw_packed, dw_oihw, *, mode=0, ci_begin=0, ci_count=None, n_perm=None, k_pad, accumulate=False):
    """dw_packed: f32 [rows, taps, k_pad] or [parts, rows, taps, k_pad] (the parts are summed)."""
    cout, cin, ks, _ = dw_oihw.shape
    ci_count = cin - ci_begin if ci_count is None else ci_count
    parts, rows = (dw_packed.shape[0], dw_packed.shape[1]) if dw_packed.dim() == 4 else (1, dw_packed.shape[0])
    L.check(L.lib().pssr_unpack_conv_wgrad_parts(L.ptr(dw_packed), parts, rows, L.ptr(dw_oihw), cout, cin, ks, ci_begin, ci_count, mode,
                                                 L.ptr(n_perm), k_pad, int(accumulate), L.stream_ptr()), "pssr_unpack_conv_wgrad_parts")
    return dw_oihw


# ----------------------------------------------------------------------------------------------
# per-channel / pointwise kernels (csrc/elementwise.hip)
def _ref(t, coff=0):
    return L.ptr(t), t.shape[-1], coff


def channel_stats_nchw(x, stats, pre_scale=1.0, pre_shift=0.0):
    n, c, h, w = x.shape
    L.check(L.lib().pssr_channel_stats_nchw(L.ptr(x), n, c, C.c_int64(h * w), C.c_float(pre_scale), C.c_float(pre_shift),
                                            L.ptr(stats), L.stream_ptr()), "pssr_channel_stats_nchw")


def bn_finalize(stats, count, gamma, beta, eps, momentum, running_mean, running_var, scale, shift, mean, invstd):
    c = scale.numel()
    L.check(L.lib().pssr_bn_finalize(L.ptr(stats), C.c_double(count), L.ptr(gamma), L.ptr(beta), C.c_float(eps), C.c_float(momentum),
                                     L.ptr(running_mean), L.ptr(running_var), L.ptr(scale), L.ptr(shift), L.ptr(mean), L.ptr(invstd),
                                     c, L.stream_ptr()), "pssr_bn_finalize")


def bn_eval_affine(gamma, beta, running_mean, running_var, eps, scale, shift):
    L.check(L.lib().pssr_bn_eval_affine(L.ptr(gamma), L.ptr(beta), L.ptr(running_mean), L.ptr(running_var), C.c_float(eps),
                                        L.ptr(scale), L.ptr(shift), scale.numel(), L.stream_ptr()), "pssr_bn_eval_affine")


def bn_bwd_coefs(stats, count, gamma, mean, invstd, coef_a, coef_b, coef_c, dgamma, dbeta):
    L.check(L.lib().pssr_bn_bwd_coefs(L.ptr(stats), C.c_double(count), L.ptr(gamma), L.ptr(mean), L.ptr(invstd), L.ptr(coef_a),
                                      L.ptr(coef_b), L.ptr(coef_c), L.ptr(dgamma), L.ptr(dbeta), coef_a.numel(), L.stream_ptr()),
            "pssr_bn_bwd_coefs")


def bn_bwd_apply(g, y, coef_a, coef_b, coef_c, dy, npix, c, dtype, g_coff=0, y_coff=0, dy_coff=0):
    L.check(L.lib().pssr_bn_bwd_apply(*_ref(g, g_coff), *_ref(y, y_coff), L.ptr(coef_a), L.ptr(coef_b), L.ptr(coef_c),
                                      *_ref(dy, dy_coff), C.c_int64(npix), c, dtype, L.stream_ptr()), "pssr_bn_bwd_apply")


def bn_relu_apply(y, scale, shift, a, npix, c, dtype, y_coff=0, a_coff=0):
    """a = relu(scale * y + shift) in the storage type: pssr_bn_relu_apply (what a BatchNorm+ReLU prologue would stage, written out)."""
    L.check(L.lib().pssr_bn_relu_apply(L.ptr(y), y.shape[-1], y_coff, L.ptr(scale), L.ptr(shift), L.ptr(a), a.shape[-1], a_coff, C.c_int64(npix), c, dtype,
                                       L.stream_ptr()), "pssr_bn_relu_apply")


def input_im2col(x, xcol, scale, shift, dtype, pre_scale=1 / 128, pre_shift=-1.0):
    n, c, h, w = x.shape
    L.check(L.lib().pssr_input_im2col(L.ptr(x), L.ptr(xcol), n, c, h, w, xcol.shape[-1], C.c_float(pre_scale), C.c_float(pre_shift),
                                      L.ptr(scale), L.ptr(shift), dtype, L.stream_ptr()), "pssr_input_im2col")


def input_norm_bwd(dxcol_a, dxcol_b, x, mean, invstd, stats, dtype, pre_scale=1 / 128, pre_shift=-1.0):
    n, c, h, w = x.shape
    L.check(L.lib().pssr_input_norm_bwd(L.ptr(dxcol_a), L.ptr(dxcol_b), dxcol_a.shape[-1], L.ptr(x), C.c_float(pre_scale),
                                        C.c_float(pre_shift), L.ptr(mean), L.ptr(invstd), n, c, h, w, L.ptr(stats), dtype,
                                        L.stream_ptr()), "pssr_input_norm_bwd")


def maxpool2(x, out, n, h, w, c, dtype, in_coff=0, out_coff=0):
    L.check(L.lib().pssr_maxpool2(*_ref(x, in_coff), *_ref(out, out_coff), n, h, w, c, dtype, L.stream_ptr()), "pssr_maxpool2")


def maxpool2_bwd(act, dpool, dskip, dout, n, h, w, c, dtype, act_coff=0, dskip_coff=0):
    ds = _ref(dskip, dskip_coff) if dskip is not None else (None, 0, 0)
    L.check(L.lib().pssr_maxpool2_bwd(*_ref(act, act_coff), *_ref(dpool), *ds, *_ref(dout), n, h, w, c, dtype, L.stream_ptr()),
            "pssr_maxpool2_bwd")


def pixel_shuffle(lo, hi, n, h, w, c_hi, r, dtype, lo_coff=0, hi_coff=0, inverse=False):
    L.check(L.lib().pssr_pixel_shuffle(*_ref(lo, lo_coff), *_ref(hi, hi_coff), n, h, w, c_hi, r, int(inverse), dtype,
                                       L.stream_ptr()), "pssr_pixel_shuffle")


def relu_bwd_stats(dout, out, y, mean, invstd, dz, stats, npix, c, dtype, out_coff=0):
    L.check(L.lib().pssr_relu_bwd_stats(*_ref(dout), *_ref(out, out_coff), *_ref(y), L.ptr(mean), L.ptr(invstd), *_ref(dz),
                                        L.ptr(stats), C.c_int64(npix), c, dtype, L.stream_ptr()), "pssr_relu_bwd_stats")


def relu_bwd_stats_fused_ok(dtype, c, h=2, w=2, unshuffle=False):
    """The loader-fused forms below take 16-bit storage and power-of-two channel counts (every BatchNorm of the default models)."""
    return dtype != L.F32 and (c & (c - 1)) == 0 and c >= (32 if unshuffle else 8) and (unshuffle or (h % 2 == 0 and w % 2 == 0))


def relu_bwd_stats_pool(dpool, dskip, dskip_coff, out, out_coff, y, mean, invstd, dz, stats, n, h, w, c, dtype):
    """relu_bwd_stats whose d(out) = dskip + max-pool-backward(dpool) is formed in the loader (no maxpool2_bwd launch, no d(out) tensor)."""
    L.check(L.lib().pssr_relu_bwd_stats_pool(*_ref(dpool), *_ref(dskip, dskip_coff), *_ref(out, out_coff), *_ref(y), L.ptr(mean), L.ptr(invstd),
                                             *_ref(dz), L.ptr(stats), n, h, w, c, dtype, L.stream_ptr()), "pssr_relu_bwd_stats_pool")


def relu_bwd_stats_unshuffle(dhi, out, out_coff, y, mean, invstd, dz, stats, n, h, w, c, dtype):
    """relu_bwd_stats whose d(out) is the inverse pixel shuffle (r = 2) of channels [0, c / 4) of ``dhi`` (twice the resolution)."""
    L.check(L.lib().pssr_relu_bwd_stats_unshuffle(*_ref(dhi), *_ref(out, out_coff), *_ref(y), L.ptr(mean), L.ptr(invstd), *_ref(dz), L.ptr(stats),
                                                  n, h, w, c, dtype, L.stream_ptr()), "pssr_relu_bwd_stats_unshuffle")


def channel_sum_nhwc(x, npix, c, out, dtype, coff=0, cstride=None):
    cs = x.shape[-1] if cstride is None else cstride
    L.check(L.lib().pssr_channel_sum_nhwc(L.ptr(x), cs, coff, C.c_int64(npix), c, L.ptr(out), dtype, L.stream_ptr()),
            "pssr_channel_sum_nhwc")


def nchw_to_nhwc(x, out, scale, dtype):
    n, c, h, w = x.shape
    L.check(L.lib().pssr_nchw_to_nhwc(L.ptr(x), L.ptr(out), n, c, C.c_int64(h * w), out.shape[-1], C.c_float(scale), dtype,
                                      L.stream_ptr()), "pssr_nchw_to_nhwc")


def clip_u8(x, out):
    L.check(L.lib().pssr_clip_u8(L.ptr(x), L.ptr(out), C.c_int64(x.numel()), L.stream_ptr()), "pssr_clip_u8")


STAT_STRIPES = 64     # PSSR_STAT_ROWS: rows of every statistic buffer (32 stripes x {multiple-of-2^-20 part, remainder})


def f64_to_f32(src, dst, accumulate=False, stripes=STAT_STRIPES):
    L.check(L.lib().pssr_f64_to_f32(L.ptr(src), L.ptr(dst), dst.numel(), int(accumulate), stripes, L.stream_ptr()), "pssr_f64_to_f32")


def f64_to_f32_batch(items, stripes=STAT_STRIPES):
    """[(src f64 [stripes * n], dst f32 [n], accumulate), ...] folded by one launch per 16 items (pssr_f64_to_f32_batch)."""
    for k in range(0, len(items), L.COPY_BATCH_MAX):
        chunk = items[k:k + L.COPY_BATCH_MAX]
        fb = L.FoldBatch()
        for i, (src, dst, acc) in enumerate(chunk):
            if src.dtype != torch.float64 or dst.dtype != torch.float32 or src.numel() < stripes * dst.numel() or not (src.is_contiguous() and dst.is_contiguous()):
                raise ValueError("f64_to_f32_batch needs contiguous float64 [stripes * n] sources and float32 [n] destinations")
            fb.dst[i], fb.src[i], fb.n[i], fb.accumulate[i] = dst.data_ptr(), src.data_ptr(), dst.numel(), int(acc)
        L.check(L.lib().pssr_f64_to_f32_batch(C.byref(fb), len(chunk), stripes, L.stream_ptr()), "pssr_f64_to_f32_batch")


# ----------------------------------------------------------------------------------------------
# loss + optimizer (csrc/loss.hip, csrc/optim.hip)
def _win(win):
    arr = (C.c_float * len(win))(*[float(v) for v in win])
    return arr, len(win)


def ssim_level_fwd(x, y, planes, h, w, win, c1, c2, sums, l1_sum=None):
    arr, k = _win(win)
    L.check(L.lib().pssr_ssim_level_fwd(L.ptr(x), L.ptr(y), planes, h, w, arr, k, C.c_float(c1), C.c_float(c2), L.ptr(sums),
                                        L.ptr(l1_sum), L.stream_ptr()), "pssr_ssim_level_fwd")


def ssim_level_fwd_adj(x, y, planes, h, w, win, c1, c2, use_ssim, sums, l1_sum, stripes, stripe_stride, adj, in_div=1.0):
    k = len(win); arr = (C.c_float * k)(*win)
    L.check(L.lib().pssr_ssim_level_fwd_adj(L.ptr(x), L.ptr(y), C.c_float(in_div), planes, h, w, arr, k, C.c_float(c1), C.c_float(c2), int(use_ssim), L.ptr(sums),
                                            L.ptr(l1_sum), stripes, C.c_int64(stripe_stride), L.ptr(adj), L.stream_ptr()), "pssr_ssim_level_fwd_adj")


def msssim_weights_striped(sums, stripes, stripe_stride, folded, levels, planes, nvalid, level_weights, ms, mix, l1_sum, l1_numel, grad_out,
                           loss_out, wts, l1_coef):
    L.check(L.lib().pssr_msssim_weights_striped(L.ptr(sums), stripes, C.c_int64(stripe_stride), L.ptr(folded), levels, planes, L.ptr(nvalid),
                                                L.ptr(level_weights), int(ms), C.c_float(mix), L.ptr(l1_sum), C.c_double(l1_numel),
                                                L.ptr(grad_out), L.ptr(loss_out), L.ptr(wts), L.ptr(l1_coef), L.stream_ptr()),
            "pssr_msssim_weights_striped")


def ssim_level_bwd_adj(x, y, adj, planes, h, w, win, wts, dcoarse, hc, wc, l1_coef, dx, in_div=1.0):
    k = len(win); arr = (C.c_float * k)(*win)
    L.check(L.lib().pssr_ssim_level_bwd_adj(L.ptr(x), L.ptr(y), C.c_float(in_div), L.ptr(adj), planes, h, w, arr, k, L.ptr(wts), L.ptr(dcoarse), hc, wc,
                                            L.ptr(l1_coef), L.ptr(dx), L.stream_ptr()), "pssr_ssim_level_bwd_adj")


def avgpool2_planes(x, out, planes, h, w, in_div=1.0):
    L.check(L.lib().pssr_avgpool2_planes_div(L.ptr(x), C.c_float(in_div), L.ptr(out), planes, h, w, L.stream_ptr()), "pssr_avgpool2_planes_div")


def avgpool2_pair(x, y, xo, yo, planes, h, w, in_div=1.0):
    L.check(L.lib().pssr_avgpool2_pair_div(L.ptr(x), L.ptr(y), C.c_float(in_div), L.ptr(xo), L.ptr(yo), planes, h, w, L.stream_ptr()),
            "pssr_avgpool2_pair_div")


def msssim_weights(sums, levels, planes, nvalid, level_weights, ms, mix, l1_sum, l1_numel, grad_out, loss_out, wts, l1_coef):
    L.check(L.lib().pssr_msssim_weights(L.ptr(sums), levels, planes, L.ptr(nvalid), L.ptr(level_weights), int(ms), C.c_float(mix),
                                        L.ptr(l1_sum), C.c_double(l1_numel), L.ptr(grad_out), L.ptr(loss_out), L.ptr(wts),
                                        L.ptr(l1_coef), L.stream_ptr()), "pssr_msssim_weights")


def ssim_level_bwd(x, y, planes, h, w, win, c1, c2, wts, use_ssim, dcoarse, hc, wc, l1_coef, dx):
    arr, k = _win(win)
    L.check(L.lib().pssr_ssim_level_bwd(L.ptr(x), L.ptr(y), planes, h, w, arr, k, C.c_float(c1), C.c_float(c2), L.ptr(wts),
                                        int(use_ssim), L.ptr(dcoarse), hc, wc, L.ptr(l1_coef), L.ptr(dx), L.stream_ptr()),
            "pssr_ssim_level_bwd")


def adamw_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    L.check(L.lib().pssr_adamw_step(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), C.c_int64(p.numel()), C.c_float(lr), C.c_float(beta1),
                                    C.c_float(beta2), C.c_float(eps), C.c_float(weight_decay), C.c_int64(step), C.c_float(grad_scale),
                                    L.stream_ptr()), "pssr_adamw_step")


# ----------------------------------------------------------------------------------------------
# pair generation / crappifiers (csrc/crappify.hip)
ROUND_CLIP, CLIP = 2, 1


def bilinear_down_u8(hr, h, w):
    """uint8 [..., H, W] -> uint8 [..., h, w] (Pillow BILINEAR, bit-exact)."""
    assert hr.dtype == torch.uint8 and hr.is_cuda and hr.is_contiguous()
    H, W = hr.shape[-2:]
    planes = hr.numel() // (H * W)
    tmp = torch.empty(planes * H * w, dtype=torch.uint8, device=hr.device)
    lr = torch.empty(*hr.shape[:-2], h, w, dtype=torch.uint8, device=hr.device)
    L.check(L.lib().pssr_bilinear_down_u8(L.ptr(hr), L.ptr(tmp), L.ptr(lr), planes, H, W, h, w, L.stream_ptr()), "pssr_bilinear_down_u8")
    return lr


def u8_to_f32(x):
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    L.check(L.lib().pssr_u8_to_f32(L.ptr(x), L.ptr(out), C.c_int64(x.numel()), L.stream_ptr()), "pssr_u8_to_f32")
    return out


def crappify_gaussian(x, intensity, gain, spread, seed, tile_offset, flags, noise=None, out=None, tile_counter=None):
    out = torch.empty_like(x) if out is None else out
    tiles = x.shape[0]
    L.check(L.lib().pssr_crappify_gaussian(L.ptr(x), L.ptr(out), tiles, C.c_int64(x.numel() // tiles), C.c_float(intensity), C.c_float(gain),
                                           C.c_float(spread), C.c_uint64(seed), C.c_uint64(tile_offset), L.ptr(noise), flags,
                                           L.ptr(tile_counter), L.stream_ptr()), "pssr_crappify_gaussian")
    return out


def crappify_poisson(x, intensity, gain, spread, seed, tile_offset, flags, out=None, tile_counter=None):
    out = torch.empty_like(x) if out is None else out
    tiles = x.shape[0]
    L.check(L.lib().pssr_crappify_poisson(L.ptr(x), L.ptr(out), tiles, C.c_int64(x.numel() // tiles), C.c_float(intensity), C.c_float(gain),
                                          C.c_float(spread), C.c_uint64(seed), C.c_uint64(tile_offset), flags, L.ptr(tile_counter),
                                          L.stream_ptr()), "pssr_crappify_poisson")
    return out


def crappify_poisson_samples(x, samples, intensity, gain, flags, out=None):
    """Poisson mix with injected samples (f64, same shape as x): pssr_crappify_poisson_samples."""
    out = torch.empty_like(x) if out is None else out
    if samples.dtype != torch.float64 or samples.numel() != x.numel():
        raise ValueError("samples: float64, one per element of x")
    L.check(L.lib().pssr_crappify_poisson_samples(L.ptr(x), L.ptr(samples.contiguous()), L.ptr(out), C.c_int64(x.numel()), C.c_double(intensity),
                                                  C.c_double(gain), flags, L.stream_ptr()), "pssr_crappify_poisson_samples")
    return out


def gaussian_blur(x, sigma, gain, flags):
    h, w = x.shape[-2:]
    planes = x.numel() // (h * w)
    tmp, out = torch.empty_like(x), torch.empty_like(x)
    L.check(L.lib().pssr_gaussian_blur(L.ptr(x), L.ptr(tmp), L.ptr(out), planes, h, w, C.c_float(sigma), C.c_float(gain), flags,
                                       L.stream_ptr()), "pssr_gaussian_blur")
    return out


def counter_add(counter, inc):
    L.check(L.lib().pssr_counter_add(L.ptr(counter), C.c_uint64(inc), L.stream_ptr()), "pssr_counter_add")


def adamw_step_dev(p, g, m, v, state, beta1, beta2, eps, weight_decay, grad_scale=1.0):
    L.check(L.lib().pssr_adamw_step_dev(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), C.c_int64(p.numel()), L.ptr(state), C.c_float(beta1),
                                        C.c_float(beta2), C.c_float(eps), C.c_float(weight_decay), C.c_float(grad_scale),
                                        L.stream_ptr()), "pssr_adamw_step_dev")


def amp_check(g, amp):
    """amp[3] |= any(g is inf / NaN); amp: device int32[4] (see include/pssr_mi355.h)."""
    L.check(L.lib().pssr_amp_check(L.ptr(g), C.c_int64(g.numel()), L.ptr(amp), L.stream_ptr()), "pssr_amp_check")


def adamw_step_amp(p, g, m, v, state, beta1, beta2, eps, weight_decay, amp, growth, backoff, interval, grad_scale=1.0):
    L.check(L.lib().pssr_adamw_step_amp(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), C.c_int64(p.numel()), L.ptr(state), C.c_float(beta1),
                                        C.c_float(beta2), C.c_float(eps), C.c_float(weight_decay), C.c_float(grad_scale), L.ptr(amp),
                                        C.c_float(growth), C.c_float(backoff), int(interval), L.stream_ptr()), "pssr_adamw_step_amp")


# ----------------------------------------------------------------------------------------------
# RDNet encoder kernels (csrc/rdnet.hip)
def input_patchify(x, xpatch, scale, shift, patch, dtype, pre_scale=1 / 128, pre_shift=-1.0):
    n, c, h, w = x.shape
    L.check(L.lib().pssr_input_patchify(L.ptr(x), L.ptr(xpatch), n, c, h, w, patch, xpatch.shape[-1], C.c_float(pre_scale),
                                        C.c_float(pre_shift), L.ptr(scale), L.ptr(shift), dtype, L.stream_ptr()), "pssr_input_patchify")


def input_norm_bwd2(dxcol_a, dxcol_b, dpatch, patch, x, mean, invstd, stats, dtype, pre_scale=1 / 128, pre_shift=-1.0):
    n, c, h, w = x.shape
    col = dxcol_a if dxcol_a is not None else dxcol_b
    L.check(L.lib().pssr_input_norm_bwd2(L.ptr(dxcol_a), L.ptr(dxcol_b), col.shape[-1] if col is not None else 0, L.ptr(dpatch),
                                         dpatch.shape[-1] if dpatch is not None else 0, patch, L.ptr(x), C.c_float(pre_scale),
                                         C.c_float(pre_shift), L.ptr(mean), L.ptr(invstd), n, c, h, w, L.ptr(stats), dtype,
                                         L.stream_ptr()), "pssr_input_norm_bwd2")


def dwconv7_pack_batch(items):
    """[(weight [C,1,7,7] f32, packed [49, C] f32, flip), ...] by one launch per 48 items (pssr_dwconv7_pack_batch)."""
    for k in range(0, len(items), L.DWPACK_BATCH_MAX):
        chunk = items[k:k + L.DWPACK_BATCH_MAX]
        b = L.DwPackBatch()
        for i, (w, out, flip) in enumerate(chunk):
            c = w.shape[0]
            if w.dtype != torch.float32 or out.dtype != torch.float32 or not (w.is_contiguous() and out.is_contiguous()) or w.numel() != 49 * c \
                    or out.numel() < 49 * c:
                raise ValueError("dwconv7_pack_batch needs contiguous float32 [C,1,7,7] weights and [49, C] destinations")
            b.w[i], b.packed[i], b.c[i], b.flip[i] = w.data_ptr(), out.data_ptr(), c, int(flip)
        L.check(L.lib().pssr_dwconv7_pack_batch(C.byref(b), len(chunk), L.stream_ptr()), "pssr_dwconv7_pack_batch")


def dwconv7_pack(w, out, flip=False):
    """torch depthwise weight [C,1,7,7] f32 -> [49][C] f32 (flip: rotated 180 degrees for the input gradient)."""
    c = w.shape[0]
    L.check(L.lib().pssr_dwconv7_pack(L.ptr(w), L.ptr(out), c, int(flip), L.stream_ptr()), "pssr_dwconv7_pack")
    return out


def dwconv7(x, wp, bias, out, n, h, w, c, dtype, in_coff=0, out_coff=0, accumulate=False):
    L.check(L.lib().pssr_dwconv7(*_ref(x, in_coff), L.ptr(wp), L.ptr(bias), *_ref(out, out_coff), n, h, w, c, int(accumulate), dtype,
                                 L.stream_ptr()), "pssr_dwconv7")


def dwconv7_wgrad(dy, x, dw, n, h, w, c, dtype, dy_coff=0, x_coff=0):
    if w % 8 == 0:      # per-workgroup slabs summed in a fixed order (no atomics)
        lib = L.lib()
        lib.pssr_dwconv7_wgrad_workspace_bytes.restype = C.c_int64
        nbytes = lib.pssr_dwconv7_wgrad_workspace_bytes(n, h, w, c)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dw.device)
        L.check(lib.pssr_dwconv7_wgrad_ws(*_ref(dy, dy_coff), *_ref(x, x_coff), L.ptr(dw), n, h, w, c, dtype, L.ptr(ws), C.c_int64(nbytes),
                                          L.stream_ptr()), "pssr_dwconv7_wgrad_ws")
        return
    L.check(L.lib().pssr_dwconv7_wgrad(*_ref(dy, dy_coff), *_ref(x, x_coff), L.ptr(dw), n, h, w, c, dtype, L.stream_ptr()), "pssr_dwconv7_wgrad")


def layernorm2d_fwd(x, gamma, beta, eps, out, n, h, w, c, dtype, in_coff=0, out_coff=0, s2d=False, c_pad=None, mean=None, rstd=None):
    c_pad = pad_to(c, 16) if c_pad is None else c_pad
    L.check(L.lib().pssr_layernorm2d_fwd(*_ref(x, in_coff), L.ptr(gamma), L.ptr(beta), C.c_float(eps), *_ref(out, out_coff), int(s2d), c_pad,
                                         n, h, w, c, L.ptr(mean), L.ptr(rstd), dtype, L.stream_ptr()), "pssr_layernorm2d_fwd")


def layernorm2d_bwd(g, x, gamma, mean, rstd, dx, stats, n, h, w, c, dtype, g_coff=0, x_coff=0, dx_coff=0, s2d=False, c_pad=None,
                    accumulate=False):
    c_pad = pad_to(c, 16) if c_pad is None else c_pad
    L.check(L.lib().pssr_layernorm2d_bwd(*_ref(g, g_coff), int(s2d), c_pad, *_ref(x, x_coff), L.ptr(gamma), L.ptr(mean), L.ptr(rstd),
                                         *_ref(dx, dx_coff), int(accumulate), n, h, w, c, L.ptr(stats), dtype, L.stream_ptr()),
            "pssr_layernorm2d_bwd")


def image_channel_dot(a, b, n, hw, c, scale, out, dtype, a_coff=0, b_coff=0):
    """out[img][c] += scale * sum over the image's pixels of a * b, the same bits on every run (one workgroup per image and 32 channels,
    fixed summation order)."""
    bref = _ref(b, b_coff) if b is not None else (None, 0, 0)
    L.check(L.lib().pssr_image_channel_dot(*_ref(a, a_coff), *bref, n, hw, c, C.c_float(scale), L.ptr(out), dtype, L.stream_ptr()),
            "pssr_image_channel_dot")


def ese_gate(s_mean, w_fc, b_fc, u, gate):
    n, c = s_mean.shape
    L.check(L.lib().pssr_ese_gate(L.ptr(s_mean), L.ptr(w_fc), L.ptr(b_fc), n, c, L.ptr(u), L.ptr(gate), L.stream_ptr()), "pssr_ese_gate")


def scale_nc(t, gate, gamma, add, out, n, hw, c, dtype, t_coff=0, out_coff=0):
    L.check(L.lib().pssr_scale_nc(*_ref(t, t_coff), L.ptr(gate), L.ptr(gamma), L.ptr(add), *_ref(out, out_coff), n, hw, c, dtype,
                                  L.stream_ptr()), "pssr_scale_nc")


def ese_bwd(A, gate, u, gamma, s_mean, w_fc, hw, du, dgamma, db_fc, dw_fc, add):
    n, c = A.shape
    L.check(L.lib().pssr_ese_bwd(L.ptr(A), L.ptr(gate), L.ptr(u), L.ptr(gamma), L.ptr(s_mean), L.ptr(w_fc), n, c, hw, L.ptr(du),
                                 L.ptr(dgamma), L.ptr(db_fc), L.ptr(dw_fc), L.ptr(add), L.stream_ptr()), "pssr_ese_bwd")


# ----------------------------------------------------------------------------------------------
# Reconstruction.conv for C_out <= 3 (csrc/head_conv.hip), bf16 storage
def head_conv_supported(dtype, cin, cout):
    return dtype in (L.BF16, L.F16) and 1 <= cout <= 3 and cin % 32 == 0 and 32 <= cin <= 128


def head_conv_fwd(act, blk, weight, bias, out, n, h, w, cin, cout, out_scale, out_shift, dtype, act_coff=0):
    L.check(L.lib().pssr_head_conv_fwd(L.ptr(act), act.shape[-1], act_coff, blk, L.ptr(weight), L.ptr(bias), L.ptr(out), n, h, w, cin, cout,
                                       C.c_float(out_scale), C.c_float(out_shift), dtype, L.stream_ptr()), "pssr_head_conv_fwd")


def head_conv_dgrad(g, g_scale, weight, act, dact, blk, n, h, w, cin, cout, dtype, *, act_coff=0, dact_coff=0):
    L.check(L.lib().pssr_head_conv_dgrad(L.ptr(g), C.c_float(g_scale), L.ptr(weight), L.ptr(act), act.shape[-1], act_coff, L.ptr(dact), dact.shape[-1], dact_coff,
                                         blk, n, h, w, cin, cout, dtype, L.stream_ptr()), "pssr_head_conv_dgrad")


def head_conv_wgrad(g, g_scale, act, blk, dw, n, h, w, cin, cout, dtype, *, act_coff=0):
    L.check(L.lib().pssr_head_conv_wgrad(L.ptr(g), C.c_float(g_scale), L.ptr(act), act.shape[-1], act_coff, blk, L.ptr(dw), n, h, w, cin, cout, dtype,
                                         L.stream_ptr()), "pssr_head_conv_wgrad")


# ----------------------------------------------------------------------------------------------
# whole-sheet prediction (csrc/tiles.hip)
def sliding_tiles_u8(sheet, size, stride, tile0, ntile):
    """uint8 sheet [C,H,W] on the device -> float32 tiles [ntile, C, size, size] (row-major sliding windows)."""
    c, h, w = sheet.shape
    out = torch.empty(ntile, c, size, size, dtype=torch.float32, device=sheet.device)
    L.check(L.lib().pssr_sliding_tiles_u8(L.ptr(sheet), L.ptr(out), c, h, w, size, stride, tile0, ntile, L.stream_ptr()), "pssr_sliding_tiles_u8")
    return out


def patch_tiles_u8(tiles, n_rows, n_cols, overlap, margin):
    """uint8 tiles [n_rows*n_cols, C, S, S] -> uint8 sheet [C, n_rows*step+overlap, n_cols*step+overlap] (overlap-averaged)."""
    t, c, size, _ = tiles.shape
    assert t == n_rows * n_cols and tiles.dtype == torch.uint8 and tiles.is_contiguous()
    step = size - overlap
    out = torch.empty(c, n_rows * step + overlap, n_cols * step + overlap, dtype=torch.uint8, device=tiles.device)
    L.check(L.lib().pssr_patch_tiles_u8(L.ptr(tiles), L.ptr(out), c, n_rows, n_cols, size, overlap, margin, L.stream_ptr()), "pssr_patch_tiles_u8")
    return out


def stack_tiles_u8(stack, m, frame_step, size, stride, tiles_y, tiles_x, tile0, ntile):
    """uint8 stack [F,H,W] on the device -> float32 tiles [ntile, m, size, size]: tiles ``tile0 ..`` of the slice-major order over frame
    slices (``m`` frames every ``frame_step``) times a ``tiles_y`` x ``tiles_x`` grid, the sheet reflected where the grid leaves it."""
    assert stack.dtype == torch.uint8 and stack.is_contiguous()
    frames, h, w = stack.shape
    out = torch.empty(ntile, m, size, size, dtype=torch.float32, device=stack.device)
    L.check(L.lib().pssr_stack_tiles_u8(L.ptr(stack), L.ptr(out), frames, h, w, m, frame_step, size, stride, tiles_y, tiles_x, tile0, ntile,
                                        L.stream_ptr()), "pssr_stack_tiles_u8")
    return out


def patch_stack_u8(tiles, n_slices, n_rows, n_cols, overlap, margin, out_h, out_w):
    """uint8 tiles [n_slices*n_rows*n_cols, C, S, S] (slice-major) -> uint8 [n_slices, C, out_h, out_w]: every slice stitched as
    ``patch_tiles_u8`` and cut to its top-left ``out_h`` x ``out_w`` pixels, in one launch."""
    t, c, size, _ = tiles.shape
    assert t == n_slices * n_rows * n_cols and tiles.dtype == torch.uint8 and tiles.is_contiguous()
    out = torch.empty(n_slices, c, max(out_h, 0), max(out_w, 0), dtype=torch.uint8, device=tiles.device)
    L.check(L.lib().pssr_patch_stack_u8(L.ptr(tiles), L.ptr(out), n_slices, c, n_rows, n_cols, size, overlap, margin, out_h, out_w, L.stream_ptr()),
            "pssr_patch_stack_u8")
    return out


BLENDS = {"average": 0, "linear": 1}        # predict_sheet's / reassemble_sheets' ``blend`` -> pssr_blend_stack_u8's
ENSEMBLES = (1, 2, 4, 8)


def dihedral_tiles_u8(stack, m, frame_step, size, stride, tiles_y, tiles_x, ensemble, item0, nitem):
    """``stack_tiles_u8`` with the dihedral self-ensemble: float32 [nitem, m, size, size], items ``item0 ..`` of the sequence
    ``tile * ensemble + d`` whose member ``d`` is the tile with every frame plane turned by ``T_d`` (include/pssr_mi355.h)."""
    assert stack.dtype == torch.uint8 and stack.is_contiguous()
    frames, h, w = stack.shape
    out = torch.empty(nitem, m, size, size, dtype=torch.float32, device=stack.device)
    L.check(L.lib().pssr_dihedral_tiles_u8(L.ptr(stack), L.ptr(out), frames, h, w, m, frame_step, size, stride, tiles_y, tiles_x, ensemble, item0, nitem,
                                           L.stream_ptr()), "pssr_dihedral_tiles_u8")
    return out


def clip_u8_dihedral(x, out, ensemble, item0):
    """``clip_u8`` of float32 [n, C, S, S] into uint8 ``out`` of that shape, item ``i`` turned back by ``U_d``, ``d = (item0 + i) % ensemble``."""
    n, c, size, size_x = x.shape
    assert size == size_x and x.dtype == torch.float32 and x.is_contiguous()
    assert out.shape == x.shape and out.dtype == torch.uint8 and out.is_contiguous()
    L.check(L.lib().pssr_clip_u8_dihedral(L.ptr(x), L.ptr(out), n, c, size, ensemble, item0, L.stream_ptr()), "pssr_clip_u8_dihedral")


def blend_stack_u8(tiles, n_slices, n_rows, n_cols, overlap, margin, out_h, out_w, blend="average", ensemble=1):
    """uint8 member predictions [n_slices*n_rows*n_cols*ensemble, C, S, S] (item order, all in the sheet's orientation) -> uint8
    [n_slices, C, out_h, out_w]: the floored weighted mean over covering tiles and members (``blend``: a key of ``BLENDS``), cropped, in one
    launch.  ``blend="average", ensemble=1`` is ``patch_stack_u8``."""
    t, c, size, _ = tiles.shape
    assert t == n_slices * n_rows * n_cols * ensemble and tiles.dtype == torch.uint8 and tiles.is_contiguous()
    out = torch.empty(n_slices, c, max(out_h, 0), max(out_w, 0), dtype=torch.uint8, device=tiles.device)
    L.check(L.lib().pssr_blend_stack_u8(L.ptr(tiles), L.ptr(out), n_slices, c, n_rows, n_cols, size, overlap, margin, out_h, out_w, BLENDS[blend], ensemble,
                                        L.stream_ptr()), "pssr_blend_stack_u8")
    return out


def dihedral_batch(x, ensemble):
    """uint8 or float32 [n, m, s, s] on the device -> float32 [n * ensemble, m, s, s]: item ``i * ensemble + d`` is ``x[i]`` with every frame
    plane turned by ``T_d`` (include/pssr_mi355.h).  ``ensemble=1`` converts / copies."""
    n, m, size, size_x = x.shape
    assert size == size_x and x.dtype in (torch.uint8, torch.float32) and x.is_contiguous()
    out = torch.empty(n * ensemble, m, size, size, dtype=torch.float32, device=x.device)
    name = "pssr_dihedral_batch_u8" if x.dtype == torch.uint8 else "pssr_dihedral_batch_f32"
    L.check(getattr(L.lib(), name)(L.ptr(x), L.ptr(out), n, m, size, ensemble, L.stream_ptr()), name)
    return out


def ensemble_reduce_u8(y, ensemble, spread=False):
    """float32 member predictions [n * ensemble, C, S, S] (``dihedral_batch``'s order) -> uint8 [n, C, S, S]: the floored integer mean of the
    members, each quantised as ``clip_u8`` and turned back by ``U_d``; with ``spread`` also their max - min: ``(mean, spread)``.  One launch;
    the quantised members are never stored."""
    items, c, size, size_x = y.shape
    assert size == size_x and items % ensemble == 0 and y.dtype == torch.float32 and y.is_contiguous()
    mean = torch.empty(items // ensemble, c, size, size, dtype=torch.uint8, device=y.device)
    dif = torch.empty_like(mean) if spread else None
    L.check(L.lib().pssr_ensemble_reduce_u8(L.ptr(y), L.ptr(mean), L.ptr(dif), items // ensemble, c, size, ensemble, L.stream_ptr()),
            "pssr_ensemble_reduce_u8")
    return (mean, dif) if spread else mean


def spread_stack_u8(tiles, n_slices, n_rows, n_cols, overlap, margin, out_h, out_w, ensemble=1):
    """``blend_stack_u8``'s member predictions -> uint8 [n_slices, C, out_h, out_w]: max - min over every member of every tile that covers
    the pixel (the support of either blend), 0 where none does, cropped, in one launch."""
    t, c, size, _ = tiles.shape
    assert t == n_slices * n_rows * n_cols * ensemble and tiles.dtype == torch.uint8 and tiles.is_contiguous()
    out = torch.empty(n_slices, c, max(out_h, 0), max(out_w, 0), dtype=torch.uint8, device=tiles.device)
    L.check(L.lib().pssr_spread_stack_u8(L.ptr(tiles), L.ptr(out), n_slices, c, n_rows, n_cols, size, overlap, margin, out_h, out_w, ensemble,
                                         L.stream_ptr()), "pssr_spread_stack_u8")
    return out


def head_conv_bwd(g, g_scale, weight, act, dact, blk, dw, bias_sum, n, h, w, cin, cout, dtype, *, act_coff=0, dact_coff=0):
    """dgrad + wgrad (+ the bias sums of the pixel-shuffle conv in front) in one pass over the activation."""
    L.check(L.lib().pssr_head_conv_bwd(L.ptr(g), C.c_float(g_scale), L.ptr(weight), L.ptr(act), act.shape[-1], act_coff, L.ptr(dact), dact.shape[-1], dact_coff,
                                       blk, L.ptr(dw), L.ptr(bias_sum), n, h, w, cin, cout, dtype, L.stream_ptr()), "pssr_head_conv_bwd")


def head_q_supported(dtype, h0, cout, r, h, w):
    """The inference form of Reconstruction (EPI_HEADQ + head_q_gather): 16-bit storage, 64 hidden channels, one output channel, 4x."""
    return dtype != L.F32 and h0 == 64 and cout == 1 and r == 4 and h >= 16 and w >= 16 and L.lib().pssr_get_option(b"IGEMM_V3") > 0


def head_q_gather(q, bias, out, n, h, w, out_scale, out_shift):
    L.check(L.lib().pssr_head_q_gather(L.ptr(q), L.ptr(bias), L.ptr(out), n, h, w, C.c_float(out_scale), C.c_float(out_shift), L.stream_ptr()),
            "pssr_head_q_gather")


def head_conv_bwd_rows(g, g_scale, weight, act, dact, blk, dw_rows, bias_rows, n, h, w, cin, cout, dtype, *, act_coff=0, dact_coff=0):
    """head_conv_bwd with order-independent sums: dw_rows / bias_rows are zeroed f64 buffers of PSSR_STAT_ROWS = 64 rows ([STAT_STRIPES][cout * cin * 9]
    and [STAT_STRIPES][4^blk * cin]: 32 workgroup stripes of multiple-of-2^-20 pieces, then their 32 remainder rows), folded by f64_to_f32."""
    L.check(L.lib().pssr_head_conv_bwd_rows(L.ptr(g), C.c_float(g_scale), L.ptr(weight), L.ptr(act), act.shape[-1], act_coff, L.ptr(dact), dact.shape[-1], dact_coff,
                                            blk, L.ptr(dw_rows), L.ptr(bias_rows), n, h, w, cin, cout, dtype, L.stream_ptr()), "pssr_head_conv_bwd_rows")


def flatk_bwd_pair_supported(dtype, cout, kx):
    """One pass over dy for both gradients of a flat-K source (flatk_bwd_pair): 16-bit storage, cout a multiple of 64 up to 1024, kx = 16."""
    return bool(L.lib().pssr_flatk_bwd_pair_supported(dtype, cout, kx))


def flatk_bwd_pair(dy, cout, x, dx, weight, dtype, *, ci_begin, ci_count, n_perm=None, dy_coff=0):
    """dx = dy . W1 (rounded to storage) and dW1 = dy^T . x from ONE read of dy, for the flat-K window W1[k][j] = weight[n_perm[k], ci_begin
    + j // ks^2, j % ks^2] (j < ci_count * ks^2) of an OIHW f32 weight.  dy / x / dx: [..., cstride] tensors of equal pixel count.  Returns dW1 as
    f32 [1, cout, 1, kx]: one part for ``unpack_conv_wgrad(..., mode=2, k_pad=kx, ci_begin=, ci_count=, n_perm=)``."""
    kx = x.shape[-1]
    npix = dy.numel() // dy.shape[-1]
    assert x.numel() // kx == npix and dx.numel() // dx.shape[-1] == npix and dx.shape[-1] == kx
    assert weight.dtype == torch.float32 and weight.is_contiguous() and weight.dim() == 4
    kk = weight.shape[2] * weight.shape[3]
    parts = L.lib().pssr_flatk_bwd_pair_parts(npix)
    if parts <= 0:
        L.check(parts if parts < 0 else -1, "pssr_flatk_bwd_pair_parts")
    slabs = torch.empty(parts, cout, kx, dtype=torch.float32, device=dy.device)
    dw = torch.empty(1, cout, 1, kx, dtype=torch.float32, device=dy.device)
    L.check(L.lib().pssr_flatk_bwd_pair(L.ptr(dy), dy.shape[-1], dy_coff, cout, L.ptr(x), kx, 0, L.ptr(dx), kx, 0, kx, L.ptr(weight),
                                        weight.shape[1] * kk, ci_begin * kk, ci_count * kk, L.ptr(n_perm), L.ptr(slabs), parts, L.ptr(dw), npix, dtype,
                                        L.stream_ptr()), "pssr_flatk_bwd_pair")
    return dw


def crappify_saltpepper(x, amount, gain, spread, seed, tile_offset, flags, out=None, tile_counter=None):
    out = torch.empty_like(x) if out is None else out
    tiles = x.shape[0]
    L.check(L.lib().pssr_crappify_saltpepper(L.ptr(x), L.ptr(out), tiles, C.c_int64(x.numel() // tiles), C.c_float(amount), C.c_float(gain),
                                             C.c_float(spread), C.c_uint64(seed), C.c_uint64(tile_offset), flags, L.ptr(tile_counter),
                                             L.stream_ptr()), "pssr_crappify_saltpepper")
    return out


def gaussian_blur_tiles(x, sigma, spread, gain, seed, tile_offset, flags, tile_counter=None):
    """x: [tiles, frames, h, w] f32; every tile is blurred with its own sigma = max(N(sigma, spread), 0)."""
    tiles, h, w = x.shape[0], x.shape[-2], x.shape[-1]
    tmp, out = torch.empty_like(x), torch.empty_like(x)
    L.check(L.lib().pssr_gaussian_blur_tiles(L.ptr(x), L.ptr(tmp), L.ptr(out), tiles, x.numel() // (tiles * h * w), h, w, C.c_float(sigma),
                                             C.c_float(spread), C.c_float(gain), C.c_uint64(seed), C.c_uint64(tile_offset), flags,
                                             L.ptr(tile_counter), L.stream_ptr()), "pssr_gaussian_blur_tiles")
    return out


def gen_pair_geometry_u8(stacks, rotations, res):
    """_gen_pair's crop / reflect pad / rot90 / flip for a batch of uint8 stacks [c, h, w] resident on the device.
    rotations: per stack ``False`` or ``[rot, axis]`` as the reference draws them (axis 1, 2 or (1, 2))."""
    c = stacks[0].shape[0]
    items = (L.GatherItem * len(stacks))()
    for i, (st, rot) in enumerate(zip(stacks, rotations)):
        if st.dtype != torch.uint8 or not st.is_cuda or st.dim() != 3 or st.shape[0] != c or not st.is_contiguous():
            raise ValueError("gen_pair_geometry_u8 needs contiguous uint8 [c, h, w] stacks on the device")
        axis = -1
        if rot:
            axis = 3 if isinstance(rot[1], (tuple, list)) else int(rot[1])
        items[i].src, items[i].sh, items[i].sw = st.data_ptr(), st.shape[1], st.shape[2]
        items[i].rot, items[i].flip_axis = int(bool(rot and rot[0])), axis
    table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(stacks[0].device)
    out = torch.empty(len(stacks), c, res, res, dtype=torch.uint8, device=stacks[0].device)
    L.check(L.lib().pssr_gen_pair_geometry_u8(L.ptr(table), len(stacks), L.ptr(out), c, res, L.stream_ptr()), "pssr_gen_pair_geometry_u8")
    return out


def gather_windows_u8(sheet_table, n_sheets, items, c, res):
    """Windows [n, c, res, res] (uint8) out of uint8 sheets resident on the device: ``sheet_table`` holds ``n_sheets``
    ``pssr_sheet_desc`` and ``items`` n ``pssr_window_item`` (24 bytes each, any dtype), both on the device."""
    for t, size in ((sheet_table, n_sheets), (items, None)):
        if not t.is_cuda or not t.is_contiguous() or (t.numel() * t.element_size()) % 24 or (size is not None and t.numel() * t.element_size() != 24 * size):
            raise ValueError("gather_windows_u8 needs contiguous device tables of 24-byte records")
    n = items.numel() * items.element_size() // 24
    out = torch.empty(n, c, res, res, dtype=torch.uint8, device=items.device)
    L.check(L.lib().pssr_gather_windows_u8(L.ptr(sheet_table), n_sheets, L.ptr(items), n, L.ptr(out), c, res, L.stream_ptr()), "pssr_gather_windows_u8")
    return out


def nearest_index(src, dst):
    """int32 [dst]: the source index of every output pixel of ``PIL.Image.resize(NEAREST)`` from ``src`` to ``dst`` pixels along one
    axis (pssr/predict.py:228).  Pillow's affine nearest-neighbour path accumulates the source coordinate in double --
    ``xo = 0.5 * a; for x: idx = (int) xo; xo += a`` with ``a = src / dst`` -- and that accumulation is restated here: the closed form
    ``floor((x + 0.5) * src / dst)`` rounds differently for many non-integer ratios.  Host only (numpy)."""
    import numpy as np
    if src < 1 or dst < 1:
        raise ValueError(f"nearest_index needs positive sizes, got {src} -> {dst}")
    a = float(src) / float(dst)
    xo, out = 0.5 * a, np.empty(dst, dtype=np.int32)
    for x in range(dst):
        out[x] = int(xo)
        xo += a
    return out


_NEAREST_TABLES = {}


def nearest_table(src, dst, device):
    """``nearest_index(src, dst)`` as an int32 tensor on ``device``, made once per (src, dst, device)."""
    key = (int(src), int(dst), str(torch.device(device)))
    t = _NEAREST_TABLES.get(key)
    if t is None:
        t = _NEAREST_TABLES[key] = torch.from_numpy(nearest_index(int(src), int(dst))).to(device)
    return t


def collage_rows_u8(panels, canvas, row0=0):
    """Composes collage rows into ``canvas`` (uint8 [rows, columns] on the device, unit column stride): pssr_collage_rows_u8.
    ``panels``: 1..3 entries ``src`` or ``(src, yi, xi)``; ``src`` is a uint8 or float32 device tensor [n, src_h, src_w] (any view with
    unit column stride), ``yi`` [h] / ``xi`` [w] int32 device index tables (``nearest_table``), both None = identity (h x w = the
    source size).  All panels share n, h and w; image i fills canvas rows (row0 + i) * h .. + h - 1, panel p columns p * w .. + w - 1.
    float32 pixels are clipped to [0, 255] and truncated (``clip_u8``); a table entry outside the source gives 0."""
    if not 1 <= len(panels) <= 3:
        raise ValueError("collage_rows_u8 takes 1 to 3 panels")
    if canvas.dtype != torch.uint8 or not canvas.is_cuda or canvas.dim() != 2 or canvas.stride(1) != 1:
        raise ValueError("collage_rows_u8 needs a uint8 device canvas [rows, columns] with unit column stride")
    descs, keep, size, n = (L.CollagePanel * len(panels))(), [], None, None
    for d, panel in zip(descs, panels):
        src, yi, xi = panel if isinstance(panel, (tuple, list)) else (panel, None, None)
        if src.dtype not in (torch.uint8, torch.float32) or src.dim() != 3 or src.device != canvas.device or min(src.shape) < 1:
            raise ValueError("collage_rows_u8: a panel source is a non-empty uint8 or float32 tensor [n, h, w] on the canvas's device")
        if src.stride(2) != 1 or src.stride(1) < src.shape[2] or src.stride(0) < 0:
            src = src.contiguous()
        if (yi is None) != (xi is None):
            raise ValueError("collage_rows_u8: a panel has one index table but not the other")
        for t in (yi, xi):
            if t is not None and (t.dtype != torch.int32 or t.dim() != 1 or t.device != canvas.device or not t.is_contiguous()):
                raise ValueError("collage_rows_u8: index tables are contiguous int32 vectors on the canvas's device")
        hw = tuple(src.shape[1:]) if yi is None else (yi.numel(), xi.numel())
        if size not in (None, hw) or n not in (None, src.shape[0]):
            raise ValueError(f"collage_rows_u8: panels differ in output size or image count ({size} / {hw}, {n} / {src.shape[0]})")
        size, n = hw, src.shape[0]
        d.src, d.image_stride, d.row_pitch, d.src_h, d.src_w = src.data_ptr(), src.stride(0), src.stride(1), src.shape[1], src.shape[2]
        d.is_f32, d.yi, d.xi = int(src.dtype == torch.float32), None if yi is None else yi.data_ptr(), None if xi is None else xi.data_ptr()
        keep.append((src, yi, xi))
    h, w = size
    if row0 < 0 or (row0 + n) * h > canvas.shape[0] or len(panels) * w > canvas.shape[1]:
        raise ValueError(f"collage_rows_u8: {n} rows of {len(panels)} panels {h} x {w} from row {row0} do not fit a canvas {tuple(canvas.shape)}")
    pitch = canvas.stride(0) if canvas.shape[0] > 1 else canvas.shape[1]
    L.check(L.lib().pssr_collage_rows_u8(C.cast(descs, C.c_void_p), len(panels), L.ptr(canvas), pitch, row0, n, h, w, L.stream_ptr()),
            "pssr_collage_rows_u8")
    return canvas


def window_attn_supported(dtype, h, w, c, heads, ws, shift=0):
    """The shapes pssr_window_attn_fwd / _bwd take (include/pssr_mi355.h)."""
    return (dtype in (torch.float32, torch.bfloat16) and 1 <= ws <= 8 and h % ws == 0 and w % ws == 0 and 0 <= shift < ws
            and heads > 0 and c % heads == 0 and c // heads <= 32)


def _window_attn_args(qkv, bias_table, heads):
    if qkv.dim() != 4 or qkv.shape[3] % 3 or not qkv.is_cuda or not qkv.is_contiguous() or qkv.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("window attention needs a contiguous float32 or bfloat16 device tensor qkv [B, H, W, 3C]")
    if bias_table.dtype != torch.float32 or not bias_table.is_contiguous() or bias_table.device != qkv.device or bias_table.dim() != 2 \
            or bias_table.shape[1] != heads:
        raise ValueError("window attention needs a contiguous float32 bias_table [(2 ws - 1)^2, heads] on qkv's device")
    b, h, w, c3 = qkv.shape
    return b, h, w, c3 // 3


def window_attn_fwd(qkv, bias_table, heads, ws, shift, scale):
    """Shifted-window attention (pssr_window_attn_fwd): qkv [B, H, W, 3C] -> (out [B, H, W, C] in qkv's dtype, lse [B, heads, H, W]
    float32).  Shapes are checked by the library (RuntimeError on PSSR_ERR_ARG)."""
    b, h, w, c = _window_attn_args(qkv, bias_table, heads)
    if bias_table.shape[0] != (2 * ws - 1) ** 2:
        raise ValueError(f"bias_table has {bias_table.shape[0]} rows, window size {ws} needs {(2 * ws - 1) ** 2}")
    out = torch.empty(b, h, w, c, dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(b, heads, h, w, dtype=torch.float32, device=qkv.device)
    L.check(L.lib().pssr_window_attn_fwd(L.ptr(qkv), L.ptr(bias_table), L.ptr(out), L.ptr(lse), b, h, w, c, heads, ws, shift, float(scale),
                                         dtype_code(qkv.dtype), L.stream_ptr()), "pssr_window_attn_fwd")
    return out, lse


def window_attn_bwd(qkv, bias_table, lse, dout, heads, ws, shift, scale):
    """Backward of ``window_attn_fwd`` (pssr_window_attn_bwd): -> (dqkv like qkv, dbias_table like bias_table).  No atomics: the same
    bits on every call."""
    b, h, w, c = _window_attn_args(qkv, bias_table, heads)
    if bias_table.shape[0] != (2 * ws - 1) ** 2:
        raise ValueError(f"bias_table has {bias_table.shape[0]} rows, window size {ws} needs {(2 * ws - 1) ** 2}")
    if dout.shape != (b, h, w, c) or dout.dtype != qkv.dtype or dout.device != qkv.device or not dout.is_contiguous():
        raise ValueError("window_attn_bwd: dout must be contiguous [B, H, W, C] with qkv's dtype and device")
    if lse.shape != (b, heads, h, w) or lse.dtype != torch.float32 or lse.device != qkv.device or not lse.is_contiguous():
        raise ValueError("window_attn_bwd: lse must be the contiguous float32 [B, heads, H, W] tensor window_attn_fwd returned")
    dqkv = torch.empty_like(qkv)
    dbias = torch.empty_like(bias_table)
    nbytes = L.lib().pssr_window_attn_workspace_bytes(b, h, w, heads, ws)
    work = torch.empty(max(int(nbytes), 4) // 4, dtype=torch.float32, device=qkv.device)
    L.check(L.lib().pssr_window_attn_bwd(L.ptr(qkv), L.ptr(bias_table), L.ptr(lse), L.ptr(dout), L.ptr(dqkv), L.ptr(dbias), L.ptr(work),
                                         work.numel() * 4, b, h, w, c, heads, ws, shift, float(scale), dtype_code(qkv.dtype), L.stream_ptr()),
            "pssr_window_attn_bwd")
    return dqkv, dbias


def normalize_preds_u8(hr, hr_hat, pmin=0.1, pmax=99.9):
    """uint8 device tensors [..., H, W] of equal shape -> (hr_norm, hr_hat_norm) uint8, as pssr.util.normalize_preds (bit-exact).
    Degenerate images: a side whose reference value is NaN (a constant ground truth or prediction, or a ground truth so sparse that its
    ``pmax`` percentile is 0) comes out as byte 0 -- what numpy's undefined NaN -> uint8 cast happens to give on x86-64, fixed here."""
    if hr.dtype != torch.uint8 or hr_hat.dtype != torch.uint8 or hr.shape != hr_hat.shape or not hr.is_cuda:
        raise ValueError("normalize_preds_u8 needs two uint8 device tensors of the same shape")
    hr, hr_hat = hr.contiguous(), hr_hat.contiguous()
    px = hr.shape[-1] * hr.shape[-2]
    n = hr.numel() // px
    lib = L.lib()
    lib.pssr_normalize_preds_workspace_bytes.restype = C.c_int64
    ws = torch.empty(n * lib.pssr_normalize_preds_workspace_bytes(C.c_int64(px)), dtype=torch.uint8, device=hr.device)
    a, b = torch.empty_like(hr), torch.empty_like(hr_hat)
    L.check(lib.pssr_normalize_preds_u8(L.ptr(hr), L.ptr(hr_hat), L.ptr(a), L.ptr(b), n, C.c_int64(px), C.c_float(pmin), C.c_float(pmax), L.ptr(ws),
                                        L.stream_ptr()), "pssr_normalize_preds_u8")
    return a, b


def normalize_preds_resized_u8(hr, hr_hat, pmin=0.1, pmax=99.9):
    """uint8 device tensors [n, H, W] / [n, h, w] of different sizes (pssr/util.py:176-179): pssr_normalize_preds_resized_u8."""
    if hr.dtype != torch.uint8 or hr_hat.dtype != torch.uint8 or hr.dim() != 3 or hr_hat.dim() != 3 or hr.shape[0] != hr_hat.shape[0] or not hr.is_cuda:
        raise ValueError("normalize_preds_resized_u8 needs two uint8 device tensors [n, H, W] and [n, h, w]")
    hr, hr_hat = hr.contiguous(), hr_hat.contiguous()
    n, (H, W), (h, w) = hr.shape[0], hr.shape[1:], hr_hat.shape[1:]
    lib = L.lib()
    lib.pssr_normalize_preds_resized_workspace_bytes.restype = C.c_int64
    ws = torch.empty(lib.pssr_normalize_preds_resized_workspace_bytes(n, H, W, h, w), dtype=torch.uint8, device=hr.device)
    a, b = torch.empty_like(hr), torch.empty_like(hr_hat)
    L.check(lib.pssr_normalize_preds_resized_u8(L.ptr(hr), H, W, L.ptr(hr_hat), h, w, L.ptr(a), L.ptr(b), n, C.c_float(pmin), C.c_float(pmax), L.ptr(ws),
                                                L.stream_ptr()), "pssr_normalize_preds_resized_u8")
    return a, b


def image_metrics_u8(hr, hr_hat):
    """uint8 device tensors [..., H, W] of equal shape -> float64 device tensor [n, 2]: per image the exact sum of squared differences
    and the mean SSIM as skimage.metrics.structural_similarity(data_range=255) defines it (pssr/predict.py:199-203)."""
    if hr.dtype != torch.uint8 or hr_hat.dtype != torch.uint8 or hr.shape != hr_hat.shape or not hr.is_cuda or hr.dim() < 2:
        raise ValueError("image_metrics_u8 needs two uint8 device tensors of the same shape [..., H, W]")
    hr, hr_hat = hr.contiguous(), hr_hat.contiguous()
    h, w = hr.shape[-2:]
    if min(h, w) < 7:
        raise ValueError("win_size exceeds image extent: the 7x7 SSIM window needs images of at least 7x7 pixels")
    n = hr.numel() // (h * w)
    lib = L.lib()
    lib.pssr_image_metrics_workspace_bytes.restype = C.c_int64
    ws = torch.empty(lib.pssr_image_metrics_workspace_bytes(n, h, w), dtype=torch.uint8, device=hr.device)
    out = torch.empty(n, 2, dtype=torch.float64, device=hr.device)
    L.check(lib.pssr_image_metrics_u8(L.ptr(hr), L.ptr(hr_hat), L.ptr(out), n, h, w, L.ptr(ws), L.stream_ptr()), "pssr_image_metrics_u8")
    return out


def copy_f32_batch(pairs):
    """[(dst, src), ...] contiguous float32 device tensors of equal numel: all copied by one kernel launch per 16 pairs."""
    for k in range(0, len(pairs), L.COPY_BATCH_MAX):
        chunk = pairs[k:k + L.COPY_BATCH_MAX]
        items = L.CopyBatch()
        for i, (dst, src) in enumerate(chunk):
            if dst.dtype != torch.float32 or src.dtype != torch.float32 or dst.numel() != src.numel() or not (dst.is_contiguous() and src.is_contiguous()):
                raise ValueError("copy_f32_batch needs contiguous float32 tensors of equal size")
            items.dst[i], items.src[i], items.n[i] = dst.data_ptr(), src.data_ptr(), dst.numel()
        L.check(L.lib().pssr_copy_f32_batch(C.byref(items), len(chunk), L.stream_ptr()), "pssr_copy_f32_batch")


# ------------------------------------------------------------------ atrous / PSP variants (csrc/atrous.hip)
def input_plain(x, out, dtype, pre_scale=1 / 128, pre_shift=-1.0):
    n, c, h, w = x.shape
    L.check(L.lib().pssr_input_plain(L.ptr(x), L.ptr(out), n, c, h, w, out.shape[-1], C.c_float(pre_scale), C.c_float(pre_shift), dtype,
                                     L.stream_ptr()), "pssr_input_plain")


def im2col_dil(x, c, col, cp, n, h, w, dil, dtype, in_coff=0, scale=None, shift=None):
    L.check(L.lib().pssr_im2col_dil(L.ptr(x), x.shape[-1], in_coff, c, L.ptr(scale), L.ptr(shift), L.ptr(col), cp, n, h, w, dil, dtype,
                                    L.stream_ptr()), "pssr_im2col_dil")


def col2im_dil(dcol, cp, out, c, n, h, w, dil, dtype, out_coff=0, y=None, y_coff=0, scale=None, shift=None, mean=None, invstd=None, stats=None):
    L.check(L.lib().pssr_col2im_dil(L.ptr(dcol), cp, L.ptr(out), out.shape[-1], out_coff, c, n, h, w, dil, L.ptr(y),
                                    y.shape[-1] if y is not None else 0, y_coff, L.ptr(scale), L.ptr(shift), L.ptr(mean), L.ptr(invstd),
                                    L.ptr(stats), dtype, L.stream_ptr()), "pssr_col2im_dil")


def channel_stats_nhwc(x, c, npix, stats, dtype, coff=0):
    L.check(L.lib().pssr_channel_stats_nhwc(L.ptr(x), x.shape[-1], coff, c, C.c_int64(npix), L.ptr(stats), dtype, L.stream_ptr()),
            "pssr_channel_stats_nhwc")


def sum_relu(ins, out, npix, c, dtype, relu=True, out_coff=0):
    """ins: list of (tensor, channel offset)."""
    k = len(ins)
    ptrs = (C.c_void_p * k)(*[t.data_ptr() for t, _ in ins])
    css = (C.c_int * k)(*[t.shape[-1] for t, _ in ins])
    cos = (C.c_int * k)(*[o for _, o in ins])
    L.check(L.lib().pssr_sum_relu(ptrs, css, cos, k, L.ptr(out), out.shape[-1], out_coff, C.c_int64(npix), c, int(relu), dtype, L.stream_ptr()),
            "pssr_sum_relu")


def relu_mask(dout, out, dz, npix, c, dtype, do_coff=0, o_coff=0, dz_coff=0):
    L.check(L.lib().pssr_relu_mask(L.ptr(dout), dout.shape[-1], do_coff, L.ptr(out), out.shape[-1], o_coff, L.ptr(dz), dz.shape[-1], dz_coff,
                                   C.c_int64(npix), c, dtype, L.stream_ptr()), "pssr_relu_mask")


def affine_relu(x, scale, shift, out, npix, c, dtype, coff=0, out_coff=0):
    L.check(L.lib().pssr_affine_relu(L.ptr(x), x.shape[-1], coff, L.ptr(scale), L.ptr(shift), L.ptr(out), out.shape[-1], out_coff, C.c_int64(npix), c,
                                     dtype, L.stream_ptr()), "pssr_affine_relu")


def maxpool_k(x, out, n, h, w, c, k, dtype, in_coff=0, out_coff=0):
    L.check(L.lib().pssr_maxpool_k(L.ptr(x), x.shape[-1], in_coff, L.ptr(out), out.shape[-1], out_coff, n, h, w, c, k, dtype, L.stream_ptr()),
            "pssr_maxpool_k")


def maxpool_k_bwd(act, dpool, dx, n, h, w, c, k, dtype, act_coff=0, dp_coff=0, dx_coff=0):
    L.check(L.lib().pssr_maxpool_k_bwd(L.ptr(act), act.shape[-1], act_coff, L.ptr(dpool), dpool.shape[-1], dp_coff, L.ptr(dx), dx.shape[-1], dx_coff,
                                       n, h, w, c, k, dtype, L.stream_ptr()), "pssr_maxpool_k_bwd")


def bilinear_up(x, out, n, hs, ws, h, w, c, dtype, in_coff=0, out_coff=0):
    L.check(L.lib().pssr_bilinear_up(L.ptr(x), x.shape[-1], in_coff, L.ptr(out), out.shape[-1], out_coff, n, hs, ws, h, w, c, dtype, L.stream_ptr()),
            "pssr_bilinear_up")


def bilinear_up_bwd(dout, din, n, hs, ws, h, w, c, dtype, do_coff=0, di_coff=0):
    L.check(L.lib().pssr_bilinear_up_bwd(L.ptr(dout), dout.shape[-1], do_coff, L.ptr(din), din.shape[-1], di_coff, n, hs, ws, h, w, c, dtype,
                                         L.stream_ptr()), "pssr_bilinear_up_bwd")


HIST_CLAMP, HIST_ACCUMULATE = 1, 2


def gradhist_fwd(pairs, bins, lo, hi, sigma, clamp_first=False):
    """Soft histograms of up to two inputs in one launch (pssr_gradhist_fwd).  ``pairs``: [(a, b)] or [(a, b), (a1, b1)] of f32
    [batch, ...] tensors (b may be None: the histogram of a itself).  Returns one [batch, bins] f32 tensor per pair."""
    a0, b0 = pairs[0]
    a1, b1 = pairs[1] if len(pairs) > 1 else (None, None)
    batch, n = a0.shape[0], a0[0].numel()
    for t in (a0, b0, a1, b1):
        assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == batch * n)
    lib = L.lib()
    ws_bytes = lib.pssr_gradhist_workspace_bytes(batch, C.c_int64(n), bins)
    ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=a0.device)
    h0 = torch.empty(batch, bins, dtype=torch.float32, device=a0.device)
    h1 = torch.empty(batch, bins, dtype=torch.float32, device=a0.device) if a1 is not None else None
    L.check(lib.pssr_gradhist_fwd(L.ptr(a0), L.ptr(b0), L.ptr(a1), L.ptr(b1), L.ptr(h0), L.ptr(h1), L.ptr(ws), C.c_int64(ws_bytes), batch,
                                  C.c_int64(n), bins, C.c_float(lo), C.c_float(hi), C.c_float(sigma), HIST_CLAMP if clamp_first else 0,
                                  L.stream_ptr()), "pssr_gradhist_fwd")
    return [h0] if h1 is None else [h0, h1]


def gradhist_bwd(xa, xb, g, dx, bins, lo, hi, sigma, g_ref=None, dev_scale=None, g_scale=1.0, clamp=False, accumulate=False):
    batch, n = xa.shape[0], xa[0].numel()
    for t in (xa, xb, dx):
        assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == batch * n)
    for t in (g, g_ref):
        assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == batch * bins)
    flags = (HIST_CLAMP if clamp else 0) | (HIST_ACCUMULATE if accumulate else 0)
    L.check(L.lib().pssr_gradhist_bwd(L.ptr(xa), L.ptr(xb), L.ptr(g), L.ptr(g_ref), L.ptr(dev_scale), C.c_float(g_scale), L.ptr(dx), batch,
                                      C.c_int64(n), bins, C.c_float(lo), C.c_float(hi), C.c_float(sigma), flags, L.stream_ptr()),
            "pssr_gradhist_bwd")
    return dx


def crappifier_profiles(lr_hat, lr, ds_hr, pred, target, clamp=False):
    L.check(L.lib().pssr_crappifier_profiles(L.ptr(lr_hat), L.ptr(lr), L.ptr(ds_hr), L.ptr(pred), L.ptr(target), C.c_int64(lr.numel()),
                                             HIST_CLAMP if clamp else 0, L.stream_ptr()), "pssr_crappifier_profiles")


def subsample(src, stride, out=None):
    """``src[:, :, ::stride, ::stride]`` as a dense f32 tensor (pssr_subsample_f32)."""
    assert src.is_cuda and src.dtype == torch.float32 and src.is_contiguous() and src.dim() >= 2
    hh, ww = src.shape[-2:]
    shape = (*src.shape[:-2], -(-hh // stride), -(-ww // stride))
    out = torch.empty(shape, dtype=torch.float32, device=src.device) if out is None else out
    planes = src.numel() // (hh * ww)
    L.check(L.lib().pssr_subsample_f32(L.ptr(src), L.ptr(out), C.c_int64(planes), hh, ww, stride, L.stream_ptr()), "pssr_subsample_f32")
    return out


def crappifier_loss_combine(pred_hist, target_hist, ssim_loss, dist_scale, out):
    L.check(L.lib().pssr_crappifier_loss_combine(L.ptr(pred_hist), L.ptr(target_hist), C.c_int64(pred_hist.numel()), L.ptr(ssim_loss),
                                                 C.c_float(dist_scale), L.ptr(out), L.stream_ptr()), "pssr_crappifier_loss_combine")


def crappifier_loss_bwd_scalars(parts, grad_out, out):
    L.check(L.lib().pssr_crappifier_loss_bwd_scalars(L.ptr(parts), L.ptr(grad_out), L.ptr(out), L.stream_ptr()),
            "pssr_crappifier_loss_bwd_scalars")


def clamp_f32(x, lo, hi, out=None):
    """``torch.clamp(x, lo, hi)`` of a contiguous f32 tensor (in place when ``out is x``)."""
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
    out = torch.empty_like(x) if out is None else out
    if x.numel():
        L.check(L.lib().pssr_clamp_f32(L.ptr(x), L.ptr(out), C.c_int64(x.numel()), C.c_float(lo), C.c_float(hi), L.stream_ptr()),
                "pssr_clamp_f32")
    return out


# ----------------------------------------------------------------------------------------------
# noise-profile statistics of approximate_crappifier's objective (csrc/profile.hip)
PROFILE_BINS = 511


def noise_profile(a, b):
    """Per image (leading dimension) of ``a - b``: (int32 [images, 511] np.histogram(v, np.arange(-256, 256)) counts, float64 [images]
    sums of every v).  ``b``: uint8 (the reduced HR); ``a``: float32 (a crappified image, unrounded) or uint8 (the real LR)."""
    if b.dtype != torch.uint8 or a.dtype not in (torch.float32, torch.uint8) or a.shape != b.shape or not (a.is_cuda and b.is_cuda) or a.dim() < 2:
        raise ValueError("noise_profile needs a float32 or uint8 `a` and a uint8 `b` of the same shape [images, ...] on the device")
    a, b = a.contiguous(), b.contiguous()
    images = a.shape[0]
    per = a.numel() // images
    lib = L.lib()
    ws_bytes = lib.pssr_noise_profile_workspace_bytes(images, per)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=a.device) if ws_bytes else None
    hist = torch.empty(images, PROFILE_BINS, dtype=torch.int32, device=a.device)
    total = torch.empty(images, dtype=torch.float64, device=a.device)
    fn, name = (lib.pssr_noise_profile_f32, "pssr_noise_profile_f32") if a.dtype == torch.float32 else (lib.pssr_noise_profile_u8, "pssr_noise_profile_u8")
    L.check(fn(L.ptr(a), L.ptr(b), L.ptr(hist), L.ptr(total), images, per, L.ptr(ws), ws_bytes, L.stream_ptr()), name)
    return hist, total


def noise_profile_loss(pred_hist, pred_sum, target_hist, target_sum, per_image, width, terms=False):
    """(float64 [images] losses, float64 [1] mean over images[, float64 [images, 2] histogram and value terms]) of
    ``mean_k((t_k - p_k)**2) / width**2 + |mean(T) - mean(P)|`` (pssr/train.py:381-386)."""
    images = pred_hist.shape[0]
    for h, s in ((pred_hist, pred_sum), (target_hist, target_sum)):
        if h.dtype != torch.int32 or s.dtype != torch.float64 or tuple(h.shape) != (images, PROFILE_BINS) or s.numel() != images \
                or not (h.is_cuda and s.is_cuda and h.is_contiguous() and s.is_contiguous()):
            raise ValueError("noise_profile_loss needs contiguous int32 [images, 511] histograms and float64 [images] sums on the device")
    loss = torch.empty(images, dtype=torch.float64, device=pred_hist.device)
    mean = torch.empty(1, dtype=torch.float64, device=pred_hist.device)
    parts = torch.empty(images, 2, dtype=torch.float64, device=pred_hist.device) if terms else None
    L.check(L.lib().pssr_noise_profile_loss(L.ptr(pred_hist), L.ptr(pred_sum), L.ptr(target_hist), L.ptr(target_sum), images, per_image, width,
                                            L.ptr(loss), L.ptr(parts), L.ptr(mean), L.stream_ptr()), "pssr_noise_profile_loss")
    return (loss, mean, parts) if terms else (loss, mean)


# ----------------------------------------------------------------------------------------------
# consistency of a prediction with its own LR input (csrc/consistency.hip; definitions in include/pssr_mi355.h)
FITS = ("affine", "identity")        # consistency_map's ``fit``


def _u8_plane_pair(who, hi, lo, hi_name):
    """The checks of the ops that score an HR-side plane against an LR-side plane: uint8 device tensors ``hi`` [..., s*h, s*w] and ``lo``
    [..., h, w], the same leading dimensions, ``s`` an integer in 1 .. 16, at most 2**28 pixels per LR plane.  ``who`` and ``hi_name``
    name the op and its HR side in the messages.  -> ``(hi, lo, planes, h, w, s)`` with both tensors contiguous."""
    if hi.dtype != torch.uint8 or lo.dtype != torch.uint8 or not (hi.is_cuda and lo.is_cuda) or hi.dim() < 2 or hi.dim() != lo.dim() \
            or hi.shape[:-2] != lo.shape[:-2]:
        raise ValueError(f"{who} needs two uint8 device tensors [..., s*h, s*w] and [..., h, w] with the same leading dimensions")
    (H, W), (h, w) = hi.shape[-2:], lo.shape[-2:]
    s = H // h if h else 0
    if h < 1 or w < 1 or not 1 <= s <= 16 or H != s * h or W != s * w:
        raise ValueError(f"{who}: a {H}x{W} {hi_name} is no integer multiple (1 .. 16) of the {h}x{w} LR image")
    if h * w > 1 << 28:
        raise ValueError(f"{who}: {h * w} pixels per LR plane (at most 2**28)")
    planes = lo.numel() // (h * w)
    if planes < 1:
        raise ValueError(f"{who}: no planes")
    return hi.contiguous(), lo.contiguous(), planes, h, w, s


def reduce_moments_u8(y, l):
    """uint8 device tensors ``y`` [..., s*h, s*w] (the prediction) and ``l`` [..., h, w] (the LR input), the same leading dimensions, ``s`` an
    integer in 1 .. 16 -> ``(d, sums)``: ``d`` uint8 like ``l``, ``bilinear_down_u8(y, h, w)`` bit for bit, and ``sums`` int64 [planes, 5],
    the exact ``sum d, sum l, sum d*d, sum d*l, sum l*l`` of each plane (all below 2**63).  One fused pass over ``y``."""
    y, l, planes, h, w, s = _u8_plane_pair("reduce_moments_u8", y, l, "prediction")
    lib = L.lib()
    ws = torch.empty(lib.pssr_reduce_moments_workspace_bytes(planes, h, w, s), dtype=torch.uint8, device=y.device)
    d = torch.empty_like(l)
    sums = torch.empty(planes, 5, dtype=torch.int64, device=y.device)
    L.check(lib.pssr_reduce_moments_u8(L.ptr(y), L.ptr(l), L.ptr(d), L.ptr(sums), planes, h, w, s, L.ptr(ws), L.stream_ptr()), "pssr_reduce_moments_u8")
    return d, sums


def consistency_map_u8(d, l, lut):
    """uint8 device tensors ``d`` and ``l`` of the same shape [..., h, w] and the int32 device tables ``lut`` [planes, 256] (the fitted
    expected LR value of every reduced value, in 1/256 grey levels) -> ``(map, sse)``: ``map`` uint8 like ``d``,
    ``min(255, (|256 l - lut[d]| + 128) >> 8)``, and ``sse`` int64 [planes], the exact sum of ``|256 l - lut[d]|**2`` of each plane."""
    if d.dtype != torch.uint8 or l.dtype != torch.uint8 or d.shape != l.shape or not (d.is_cuda and l.is_cuda) or d.dim() < 2:
        raise ValueError("consistency_map_u8 needs two uint8 device tensors of the same shape [..., h, w]")
    pixels = d.shape[-1] * d.shape[-2]
    planes = d.numel() // pixels if pixels else 0
    if pixels < 1 or planes < 1 or pixels > 1 << 28:
        raise ValueError(f"consistency_map_u8: {planes} planes of {pixels} pixels (at least one, at most 2**28 pixels each)")
    if lut.dtype != torch.int32 or not lut.is_cuda or tuple(lut.shape) != (planes, 256):
        raise ValueError(f"consistency_map_u8 needs an int32 device table [{planes}, 256], one row per plane")
    d, l, lut = d.contiguous(), l.contiguous(), lut.contiguous()
    lib = L.lib()
    ws = torch.empty(lib.pssr_consistency_map_workspace_bytes(planes, pixels), dtype=torch.uint8, device=d.device)
    out = torch.empty_like(d)
    sse = torch.empty(planes, dtype=torch.int64, device=d.device)
    L.check(lib.pssr_consistency_map_u8(L.ptr(d), L.ptr(l), L.ptr(lut), L.ptr(out), L.ptr(sse), planes, pixels, L.ptr(ws), L.stream_ptr()),
            "pssr_consistency_map_u8")
    return out, sse


# ----------------------------------------------------------------------------------------------
# registration of real (HR, LR) pairs (csrc/register.hip; definitions in include/pssr_mi355.h)
MAX_REGISTER_RADIUS = 32


def register_margin(s, radius):
    """LR pixels a registration at scale ``s`` and ``radius`` HR pixels drops on every side: ``1 + ceil(radius / s)``."""
    return 1 + -(-radius // s)


def register_shifts_u8(hr, lr, radius):
    """uint8 device tensors ``hr`` [..., s*h, s*w] and ``lr`` [..., h, w], the same leading dimensions, ``s`` an integer in 1 .. 16, and a
    search radius of 0 .. 32 HR pixels -> int64 [planes, 3 T + 2], ``T = (2 radius + 1)**2``: per plane and shift ``(ty, tx)`` (row
    ``(ty + radius) (2 radius + 1) + tx + radius``) the exact ``sum D, sum D*D, sum D*Lc`` of the Pillow-bilinear reduction ``D`` of ``hr``
    sampled at that shift against ``Lc = lr[m:h-m, m:w-m]``, ``m = register_margin(s, radius)``, then ``sum Lc, sum Lc*Lc``.  One fused
    pass over ``hr``."""
    hr, lr, planes, h, w, s = _u8_plane_pair("register_shifts_u8", hr, lr, "HR image")
    if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= MAX_REGISTER_RADIUS:
        raise ValueError(f"register_shifts_u8: the radius must be an int in 0 .. {MAX_REGISTER_RADIUS} HR pixels. Given {radius!r}.")
    m = register_margin(s, radius)
    if h - 2 * m < 1 or w - 2 * m < 1:
        raise ValueError(f"register_shifts_u8: a {h}x{w} LR image leaves nothing inside the margin of {m} pixels on every side")
    lib = L.lib()
    ws = torch.empty(lib.pssr_register_shifts_workspace_bytes(planes, h, w, s, radius), dtype=torch.uint8, device=hr.device)
    sums = torch.empty(planes, 3 * (2 * radius + 1) ** 2 + 2, dtype=torch.int64, device=hr.device)
    L.check(lib.pssr_register_shifts_u8(L.ptr(hr), L.ptr(lr), L.ptr(sums), planes, h, w, s, radius, L.ptr(ws), L.stream_ptr()),
            "pssr_register_shifts_u8")
    return sums


def crop_shift_u8(x, origins, ho, wo, *, table=None):
    """uint8 device tensor ``x`` [..., H, W] and one origin ``(y0, x0)`` per plane (``origins``: host ints [planes, 2], checked here:
    a window must lie inside its plane) -> uint8 [..., ho, wo], ``x[p][y0:y0+ho, x0:x0+wo]``.  ``table``: an int32 device tensor
    [planes, 2] that already holds ``origins`` (a caller that crops several tensors uploads one table and passes its rows)."""
    if x.dtype != torch.uint8 or not x.is_cuda or x.dim() < 2:
        raise ValueError("crop_shift_u8 needs a uint8 device tensor [..., H, W]")
    H, W = x.shape[-2:]
    planes = x.numel() // (H * W) if H * W else 0
    if planes < 1 or not (1 <= ho <= H and 1 <= wo <= W):
        raise ValueError(f"crop_shift_u8: {planes} planes, a {ho}x{wo} window of a {H}x{W} plane")
    rows = [(int(y0), int(x0)) for y0, x0 in (origins.tolist() if hasattr(origins, "tolist") else origins)]
    if len(rows) != planes or any(not (0 <= y0 <= H - ho and 0 <= x0 <= W - wo) for y0, x0 in rows):
        raise ValueError(f"crop_shift_u8 needs {planes} origins (y0, x0) with 0 <= y0 <= {H - ho} and 0 <= x0 <= {W - wo}")
    if table is None:
        table = torch.tensor(rows, dtype=torch.int32).to(x.device)
    elif table.dtype != torch.int32 or not table.is_cuda or tuple(table.shape) != (planes, 2) or not table.is_contiguous():
        raise ValueError(f"crop_shift_u8: table must be a contiguous int32 device tensor [{planes}, 2]")
    x = x.contiguous()
    out = torch.empty(*x.shape[:-2], ho, wo, dtype=torch.uint8, device=x.device)
    L.check(L.lib().pssr_crop_shift_u8(L.ptr(x), L.ptr(out), L.ptr(table), planes, H, W, ho, wo, L.stream_ptr()), "pssr_crop_shift_u8")
    return out


# ----------------------------------------------------------------------------------------------
# estimate of the resolution-scaling function (csrc/rsf.hip; definitions in include/pssr_mi355.h)
MAX_RSF_CANDIDATES = 64
RSF_PRECISION_BITS = 22              # PRECISION_BITS of csrc/pil_taps.h: a row of a tap table of sigma > 0 sums to 1 << 22


def _interior_taps(s):
    """The ``2 s`` fixed-point coefficients of an interior output of Pillow's BILINEAR reduction by the integer ``s`` (step 1 of the
    registration block of include/pssr_mi355.h; the device copy is csrc/pil_taps.h): Pillow's precompute_coeffs + normalize_coeffs_8bpc
    for output 1 of 4 reduced from ``4 s``, in Python floats (C doubles) and Pillow's order of operations."""
    in_size, out_size = 4 * s, 4
    scale = in_size / out_size
    support = scale if scale > 1.0 else 1.0
    ss = 1.0 / support
    center = 1.5 * scale
    xmin, xmax = max(int(center - support + 0.5), 0), min(int(center + support + 0.5), in_size)
    ws = []
    for x in range(xmax - xmin):
        a = abs((x + xmin - center + 0.5) * ss)
        ws.append(1.0 - a if a < 1.0 else 0.0)
    ww = 0.0
    for v in ws:
        ww += v
    return [int(0.5 + (v / ww if ww != 0.0 else v) * (1 << RSF_PRECISION_BITS)) for v in ws]


def rsf_radius(sigma):
    """HR pixels the Gaussian of ``sigma`` reaches to either side in a tap table: 0 for ``sigma = 0``, else ``ceil(3 sigma)``."""
    import math
    return 0 if sigma == 0 else math.ceil(3 * sigma)


def rsf_taps(s, sigmas, radius=None):
    """The tap table of ``pssr_rsf_moments_u8`` (step 1 of include/pssr_mi355.h) for the scale ``s`` (1 .. 16) and the candidate widths
    ``sigmas`` (1 .. 64 finite numbers >= 0, in HR pixels, ``ceil(3 sigma) <= 32``) -> ``(taps, R)``: int32 numpy [K, 2 s + 2 R], every row
    non-negative with the sum ``1 << 22`` (the row of ``sigma = 0``: the sum of Pillow's own taps, which is ``(1 << 22) + 1`` at ``s = 3``),
    and ``R = max ceil(3 sigma)`` unless ``radius`` gives it.  Row ``k`` is Pillow's ``2 s`` interior
    taps convolved with the normalised float64 Gaussian of ``sigma_k`` (every sum the correctly rounded ``math.fsum``), rounded to 22 bits, the
    rounding's remainder added to the first largest tap; the row of ``sigma = 0`` is the interior taps themselves."""
    import math
    import numpy as np
    if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 1 <= s <= 16:
        raise ValueError(f"rsf_taps: the scale must be an int in 1 .. 16. Given {s!r}.")
    s = int(s)
    try:
        sig = [float(v) for v in sigmas]
    except (TypeError, ValueError):
        raise ValueError(f"rsf_taps: sigmas must be a sequence of numbers. Given {sigmas!r}.") from None
    if not 1 <= len(sig) <= MAX_RSF_CANDIDATES:
        raise ValueError(f"rsf_taps: 1 .. {MAX_RSF_CANDIDATES} candidate sigmas. Given {len(sig)}.")
    if any(not math.isfinite(v) or v < 0 for v in sig):
        raise ValueError(f"rsf_taps: every sigma must be finite and >= 0. Given {sig}.")
    rads = [rsf_radius(v) for v in sig]
    if max(rads) > MAX_REGISTER_RADIUS:
        raise ValueError(f"rsf_taps: ceil(3 sigma) must be at most {MAX_REGISTER_RADIUS} HR pixels. Given sigma = {max(sig)}.")
    if radius is None:
        radius = max(rads)
    elif isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not max(rads) <= radius <= MAX_REGISTER_RADIUS:
        raise ValueError(f"rsf_taps: radius must be an int from {max(rads)} (the largest ceil(3 sigma)) to {MAX_REGISTER_RADIUS}. Given {radius!r}.")
    radius, one = int(radius), 1 << RSF_PRECISION_BITS
    interior = _interior_taps(s)
    t = [k / one for k in interior]
    table = np.zeros((len(sig), 2 * s + 2 * radius), dtype=np.int32)
    for row, sigma, rad in zip(table, sig, rads):
        if sigma == 0:
            row[radius:radius + 2 * s] = interior
            continue
        g = [math.exp(-(i * i) / (2.0 * sigma * sigma)) for i in range(-rad, rad + 1)]
        total = math.fsum(g)
        g = [v / total for v in g]
        ks = []
        for n in range(2 * s + 2 * rad):
            c = math.fsum(g[i] * t[n - i] for i in range(max(0, n - 2 * s + 1), min(n, 2 * rad) + 1))
            ks.append(math.floor(c * one + 0.5))
        ks[ks.index(max(ks))] += one - sum(ks)
        row[radius - rad:radius + rad + 2 * s] = ks
    return table, radius


def _rsf_table(who, taps, radius, s=None):
    """The checks of a host tap table: int [K, 2 s + 2 radius], ``K`` in 1 .. 64, ``radius`` in 0 .. 32, rows non-negative with the sum
    ``1 << 22`` or that of Pillow's interior taps at this scale -> ``(int32 numpy table, K, s)``."""
    import numpy as np
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= radius <= MAX_REGISTER_RADIUS:
        raise ValueError(f"{who}: the radius must be an int in 0 .. {MAX_REGISTER_RADIUS} HR pixels. Given {radius!r}.")
    if torch.is_tensor(taps):
        if taps.is_cuda:
            raise ValueError(f"{who} takes the tap table on the host (it is checked there and uploaded)")
        taps = taps.numpy()
    taps = np.asarray(taps)
    if taps.ndim != 2 or taps.dtype.kind not in "iu" or not 1 <= taps.shape[0] <= MAX_RSF_CANDIDATES:
        raise ValueError(f"{who} needs an integer tap table [K, 2 s + 2 radius] with K in 1 .. {MAX_RSF_CANDIDATES} (ops.rsf_taps makes it)")
    nt = taps.shape[1] - 2 * int(radius)
    if nt < 2 or nt % 2 or nt // 2 > 16 or (s is not None and nt != 2 * s):
        want = f"2 * {s} + 2 * {radius}" if s is not None else f"2 s + 2 * {radius}, s in 1 .. 16,"
        raise ValueError(f"{who}: a tap table of {taps.shape[1]} columns does not have the {want} columns of radius {radius}")
    wide = taps.astype(np.int64)
    one, plain = 1 << RSF_PRECISION_BITS, sum(_interior_taps(nt // 2))
    if (wide < 0).any() or ((wide.sum(axis=1) != one) & (wide.sum(axis=1) != plain)).any():
        raise ValueError(f"{who}: every row of the tap table must be non-negative and sum to {one}"
                         + (f" (or to {plain}, as Pillow's own taps at this scale do)" if plain != one else ""))
    return np.ascontiguousarray(wide.astype(np.int32)), taps.shape[0], nt // 2


def rsf_moments_u8(y, l, taps, radius):
    """uint8 device tensors ``y`` [..., s*h, s*w] and ``l`` [..., h, w], the same leading dimensions, ``s`` an integer in 1 .. 16, the host
    tap table ``taps`` int [K, 2 s + 2 radius] of ``rsf_taps`` (checked here: shape, sign and row sums; then uploaded) -> int64
    [planes, 3 K + 2]: per plane and candidate ``k`` the exact ``sum D, sum D*D, sum D*Lc`` of ``D_k``, ``y`` blurred and reduced to the LR grid
    by row ``k`` in two strided passes, against ``Lc = l[m:h-m, m:w-m]``, ``m = register_margin(s, radius)``, then ``sum Lc, sum Lc*Lc``.
    One fused pass over ``y`` for all candidates."""
    y, l, planes, h, w, s = _u8_plane_pair("rsf_moments_u8", y, l, "sharp image")
    table, K, _ = _rsf_table("rsf_moments_u8", taps, radius, s)
    radius = int(radius)
    m = register_margin(s, radius)
    if h - 2 * m < 1 or w - 2 * m < 1:
        raise ValueError(f"rsf_moments_u8: a {h}x{w} LR image leaves nothing inside the margin of {m} pixels on every side")
    lib = L.lib()
    dev_taps = torch.from_numpy(table).to(y.device)
    ws = torch.empty(lib.pssr_rsf_moments_workspace_bytes(planes, h, w, s, K, radius), dtype=torch.uint8, device=y.device)
    sums = torch.empty(planes, 3 * K + 2, dtype=torch.int64, device=y.device)
    L.check(lib.pssr_rsf_moments_u8(L.ptr(y), L.ptr(l), L.ptr(dev_taps), L.ptr(sums), planes, h, w, s, K, radius, L.ptr(ws), L.stream_ptr()),
            "pssr_rsf_moments_u8")
    return sums


def rsf_reduce_u8(y, taps, radius, sel):
    """uint8 device tensor ``y`` [..., s*h, s*w], the host tap table ``taps`` int [K, 2 s + 2 radius] of ``rsf_taps`` (it fixes ``s``; checked
    as in ``rsf_moments_u8``) and one candidate index per plane (``sel``: host ints [planes], checked here: ``0 <= sel < K``) -> uint8
    [..., h - 2m, w - 2m], ``m = register_margin(s, radius)``: ``D_sel[p]`` of every plane, ``y`` blurred and reduced by that row."""
    import numpy as np
    if not torch.is_tensor(y) or y.dtype != torch.uint8 or not y.is_cuda or y.dim() < 2:
        raise ValueError("rsf_reduce_u8 needs a uint8 device tensor [..., s*h, s*w]")
    table, K, s = _rsf_table("rsf_reduce_u8", taps, radius)
    radius = int(radius)
    H, W = y.shape[-2:]
    h, w = H // s, W // s
    if h < 1 or w < 1 or H != s * h or W != s * w:
        raise ValueError(f"rsf_reduce_u8: a {H}x{W} image is no multiple of the scale {s} of the tap table")
    if h * w > 1 << 28:
        raise ValueError(f"rsf_reduce_u8: {h * w} pixels per LR plane (at most 2**28)")
    planes = y.numel() // (H * W)
    m = register_margin(s, radius)
    if planes < 1 or h - 2 * m < 1 or w - 2 * m < 1:
        raise ValueError(f"rsf_reduce_u8: {planes} planes; a {h}x{w} LR image leaves nothing inside the margin of {m} pixels on every side")
    rows = [int(v) for v in (sel.tolist() if hasattr(sel, "tolist") else sel)]
    if len(rows) != planes or any(not 0 <= v < K for v in rows):
        raise ValueError(f"rsf_reduce_u8 needs {planes} candidate indices sel with 0 <= sel < {K}")
    y = y.contiguous()
    dev_taps = torch.from_numpy(table).to(y.device)
    dev_sel = torch.from_numpy(np.asarray(rows, dtype=np.int32)).to(y.device)
    d = torch.empty(*y.shape[:-2], h - 2 * m, w - 2 * m, dtype=torch.uint8, device=y.device)
    L.check(L.lib().pssr_rsf_reduce_u8(L.ptr(y), L.ptr(dev_taps), L.ptr(dev_sel), L.ptr(d), planes, h, w, s, K, radius, L.stream_ptr()),
            "pssr_rsf_reduce_u8")
    return d


# ----------------------------------------------------------------------------------------------
# level-conditional moments of a pair (csrc/levels.hip; definitions in include/pssr_mi355.h)
LEVEL_MOMENTS = 5                    # per level of d: n, sum l, sum l*l, #{l == 0}, #{l == 255}


def level_moments_u8(d, l):
    """uint8 device tensors ``d`` and ``l`` of the same shape [planes, h, w] or [planes, n] (1 .. 2**28 pixels per plane) -> int64
    [planes, 256, 5]: per plane and grey level ``v`` of ``d``, over the pixels with ``d == v``, their number, the exact ``sum l`` and
    ``sum l*l``, and how many of them have ``l == 0`` and ``l == 255``.  One pass over both; the same bits on every run."""
    if not (torch.is_tensor(d) and torch.is_tensor(l)) or d.dtype != torch.uint8 or l.dtype != torch.uint8 or d.shape != l.shape \
            or not (d.is_cuda and l.is_cuda) or d.dim() not in (2, 3):
        raise ValueError("level_moments_u8 needs two uint8 device tensors of the same shape [planes, h, w] or [planes, n]")
    planes = d.shape[0]
    per_plane = d.numel() // planes if planes else 0
    if planes < 1 or per_plane < 1 or per_plane > 1 << 28:
        raise ValueError(f"level_moments_u8: {planes} planes of {per_plane} pixels (at least one, at most 2**28 pixels each)")
    d, l = d.contiguous(), l.contiguous()
    lib = L.lib()
    ws_bytes = lib.pssr_level_moments_workspace_bytes(planes, per_plane)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=d.device)
    table = torch.empty(planes, 256, LEVEL_MOMENTS, dtype=torch.int64, device=d.device)
    L.check(lib.pssr_level_moments_u8(L.ptr(d), L.ptr(l), L.ptr(table), planes, per_plane, L.ptr(ws), ws_bytes, L.stream_ptr()),
            "pssr_level_moments_u8")
    return table


# ----------------------------------------------------------------------------------------------
# Fourier ring correlation (csrc/frc.hip; definitions in include/pssr_mi355.h)
FRC_WINDOWS = ("hann", "none")       # frc's ``window``
FRC_MIN_BLOCK, FRC_MAX_BLOCK = 16, 1024

_FRC_TABLES = {}                     # (n, window) -> (ct, st) float32 numpy
_FRC_DEVICE_TABLES = {}              # (n, window, device) -> their device copies, kept for the life of the process (8 MB a pair at n = 1024)


def _check_frc_block(who, block):
    if isinstance(block, bool) or not isinstance(block, int) or block % 2 or not FRC_MIN_BLOCK <= block <= FRC_MAX_BLOCK:
        raise ValueError(f"{who}: block must be an even int in {FRC_MIN_BLOCK} .. {FRC_MAX_BLOCK}. Given {block!r}.")


def frc_tables(n, window="hann"):
    """The tables of ``pssr_frc_rings_u8`` (step 1 of include/pssr_mi355.h) -> ``(ct, st)``, float32 numpy [n, n]:
    ``ct[x, k] = w[x] cos(2 pi ((x k) mod n) / n)``, ``st[x, k] = -w[x] sin(2 pi ((x k) mod n) / n)`` with ``w[x] = sin(pi (x + 1/2) / n)**2``
    (``"hann"``) or 1 (``"none"``); float64 on the host, rounded once."""
    import numpy as np
    _check_frc_block("frc_tables", n)
    if window not in FRC_WINDOWS:
        raise ValueError(f"window must be one of {FRC_WINDOWS}. Given {window!r}.")
    if (n, window) not in _FRC_TABLES:
        x = np.arange(n, dtype=np.int64)
        w = np.sin(np.pi * (x + 0.5) / n) ** 2 if window == "hann" else np.ones(n)
        angle = 2.0 * np.pi * ((x[:, None] * x[None, :]) % n) / n
        _FRC_TABLES[n, window] = ((w[:, None] * np.cos(angle)).astype(np.float32), (-w[:, None] * np.sin(angle)).astype(np.float32))
    return _FRC_TABLES[n, window]


def _frc_device_tables(n, window, device):
    key = (n, window, torch.device(device))
    if key not in _FRC_DEVICE_TABLES:
        _FRC_DEVICE_TABLES[key] = tuple(torch.from_numpy(t).to(device) for t in frc_tables(n, window))
        torch.cuda.current_stream(key[2]).synchronize()        # uploaded once: whichever stream uses them later finds them written
    return _FRC_DEVICE_TABLES[key]


def _frc_sums_args(who, tensors, block, window):
    """The argument checks that the ring-sum and sector-sum drivers share -> ``(contiguous tensors, H, W, planes, blocks per plane)``."""
    first = tensors[0]
    if not all(torch.is_tensor(t) and t.dtype == torch.uint8 and t.is_cuda for t in tensors) or first.dim() < 2 \
            or any(t.shape != first.shape for t in tensors):
        raise ValueError(f"{who} needs two uint8 device tensors of the same shape [..., H, W]" if len(tensors) == 2 else
                         f"{who} needs a uint8 device tensor [..., H, W]")
    _check_frc_block(who, block)
    if window not in FRC_WINDOWS:
        raise ValueError(f"window must be one of {FRC_WINDOWS}. Given {window!r}.")
    H, W = first.shape[-2:]
    if block > min(H, W):
        raise ValueError(f"{who}: a block of {block} does not fit a {H}x{W} plane")
    planes = first.numel() // (H * W)
    nb = (H // block) * (W // block)
    if planes < 1 or planes * nb > 1 << 24:
        raise ValueError(f"{who}: {planes} planes of {nb} blocks (at least one plane, at most 2**24 blocks in all)")
    return [t.contiguous() for t in tensors], H, W, planes, nb


def frc_rings_u8(a, b, block, window="hann"):
    """uint8 device tensors ``a`` and ``b`` of the same shape [..., H, W], an even block side ``block`` in 16 .. 1024 (at most
    ``min(H, W)``) -> float64 device tensor [planes, nby * nbx, block // 2 + 1, 3]: per plane, per block of the centred grid of
    ``(H // block) x (W // block)`` blocks and per ring of spatial frequency the sums ``Re(Fa conj Fb), |Fa|**2, |Fb|**2`` over the
    windowed spectra of the two blocks.  Two matrix products per block on the f32-input MFMA and a fixed-order reduction: the same bits on
    every call."""
    (a, b), H, W, planes, nb = _frc_sums_args("frc_rings_u8", (a, b), block, window)
    ct, st = _frc_device_tables(block, window, a.device)
    lib = L.lib()
    ws = torch.empty(lib.pssr_frc_workspace_bytes(planes, H, W, block), dtype=torch.uint8, device=a.device)
    sums = torch.empty(planes, nb, block // 2 + 1, 3, dtype=torch.float64, device=a.device)
    L.check(lib.pssr_frc_rings_u8(L.ptr(a), L.ptr(b), L.ptr(ct), L.ptr(st), L.ptr(sums), planes, H, W, block, L.ptr(ws), L.stream_ptr()),
            "pssr_frc_rings_u8")
    return sums


def decorr_rings_u8(a, block, window="hann"):
    """uint8 device tensor ``a`` [..., H, W], an even block side ``block`` in 16 .. 1024 (at most ``min(H, W)``) -> float64 device tensor
    [planes, nby * nbx, block // 2 + 1, 2]: per plane, per block of the centred grid of ``(H // block) x (W // block)`` blocks and per ring
    of spatial frequency the sums ``|F|`` and ``|F|**2`` over the windowed spectrum of the block minus its own mean (steps 1 - 2 of
    "decorrelation analysis" in include/pssr_mi355.h).  The tables are ``frc_tables``' and so is their device cache; the same bits on every
    call."""
    (a,), H, W, planes, nb = _frc_sums_args("decorr_rings_u8", (a,), block, window)
    ct, st = _frc_device_tables(block, window, a.device)
    lib = L.lib()
    nbytes = lib.pssr_decorr_workspace_bytes(planes, H, W, block)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=a.device)
    sums = torch.empty(planes, nb, block // 2 + 1, 2, dtype=torch.float64, device=a.device)
    L.check(lib.pssr_decorr_rings_u8(L.ptr(a), L.ptr(ct), L.ptr(st), L.ptr(sums), planes, H, W, block, L.ptr(ws), nbytes, L.stream_ptr()),
            "pssr_decorr_rings_u8")
    return sums


# Directional resolution: the sums per (ring, sector) cell ("Directional resolution" in include/pssr_mi355.h)
FRC_MAX_SECTORS = 16

_FRC_SECTOR_BOUNDS = {}              # S -> (bx, by) int32 numpy
_FRC_DEVICE_BOUNDS = {}              # (S, device) -> their device copies
_FRC_SECTOR_POP = {}                 # (n, S) -> int64 [n // 2 + 1, S]


def _check_frc_sectors(who, sectors):
    if isinstance(sectors, bool) or not isinstance(sectors, int) or not 1 <= sectors <= FRC_MAX_SECTORS:
        raise ValueError(f"{who}: sectors must be an int in 1 .. {FRC_MAX_SECTORS}. Given {sectors!r}.")


def frc_sector_bounds(S):
    """The boundary vectors of step S1 of include/pssr_mi355.h -> ``(bx, by)``, int32 numpy [S]: ``rint(2**20 cos beta_j)`` and
    ``rint(2**20 sin beta_j)``, ``beta_j = (j + 1/2) pi / S``; float64 on the host, rounded once."""
    import numpy as np
    _check_frc_sectors("frc_sector_bounds", S)
    if S not in _FRC_SECTOR_BOUNDS:
        beta = (np.arange(S, dtype=np.float64) + 0.5) * np.pi / S
        _FRC_SECTOR_BOUNDS[S] = (np.rint(2.0 ** 20 * np.cos(beta)).astype(np.int32), np.rint(2.0 ** 20 * np.sin(beta)).astype(np.int32))
    return _FRC_SECTOR_BOUNDS[S]


def _frc_device_bounds(S, device):
    key = (S, torch.device(device))
    if key not in _FRC_DEVICE_BOUNDS:
        _FRC_DEVICE_BOUNDS[key] = tuple(torch.from_numpy(t).to(device) for t in frc_sector_bounds(S))
        torch.cuda.current_stream(key[1]).synchronize()        # as _frc_device_tables
    return _FRC_DEVICE_BOUNDS[key]


def frc_sector_pop(n, S):
    """int64 numpy [n // 2 + 1, S]: the coefficients of the full n x n spectrum per (ring, sector) cell (steps S2 and S4 of
    include/pssr_mi355.h; a coefficient with kx > n / 2 counts in the cell of its Hermitian mirror).  Host only."""
    import numpy as np
    _check_frc_block("frc_sector_pop", n)
    _check_frc_sectors("frc_sector_pop", S)
    if (n, S) not in _FRC_SECTOR_POP:
        R = n // 2
        ky, kx = np.meshgrid(np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64), indexing="ij")
        mirror = kx > R
        ky, kx = np.where(mirror, (n - ky) % n, ky), np.where(mirror, n - kx, kx)
        fy = np.where(ky <= R, ky, ky - n)
        q = fy * fy + kx * kx
        r = np.floor(np.sqrt(q.astype(np.float64)) + 0.5).astype(np.int64)
        r += (q > r * r + r).astype(np.int64) - ((r > 0) & (q < r * r - r + 1)).astype(np.int64)     # (isqrt(4 q) + 1) // 2 whatever the float root did
        gx, gy = np.where(fy >= 0, kx, -kx), np.abs(fy)
        bx, by = (t.astype(np.int64) for t in frc_sector_bounds(S))
        sector = (bx[:, None, None] * gy - by[:, None, None] * gx >= 0).sum(axis=0) % S
        keep = r <= R
        _FRC_SECTOR_POP[n, S] = np.bincount((r * S + sector)[keep], minlength=(R + 1) * S).reshape(R + 1, S)
    return _FRC_SECTOR_POP[n, S]


def frc_sectors_u8(a, b, block, sectors, window="hann"):
    """``frc_rings_u8`` per direction: -> float64 device tensor [planes, nby * nbx, block // 2 + 1, sectors, 3], the three sums of every
    ring cut into ``sectors`` (1 .. 16) sectors of the direction of the frequency vector, sector ``s`` centred on ``s pi / sectors``
    (0: along x).  The same transform; the reduction bins by (ring, sector) in one fixed order, and ``sectors=1`` gives the bits of
    ``frc_rings_u8``."""
    (a, b), H, W, planes, nb = _frc_sums_args("frc_sectors_u8", (a, b), block, window)
    _check_frc_sectors("frc_sectors_u8", sectors)
    ct, st = _frc_device_tables(block, window, a.device)
    bx, by = _frc_device_bounds(sectors, a.device)
    lib = L.lib()
    nbytes = lib.pssr_frc_sectors_workspace_bytes(planes, H, W, block, sectors)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=a.device)
    sums = torch.empty(planes, nb, block // 2 + 1, sectors, 3, dtype=torch.float64, device=a.device)
    L.check(lib.pssr_frc_sectors_u8(L.ptr(a), L.ptr(b), L.ptr(ct), L.ptr(st), L.ptr(bx), L.ptr(by), L.ptr(sums), planes, H, W, block, sectors,
                                    L.ptr(ws), nbytes, L.stream_ptr()), "pssr_frc_sectors_u8")
    return sums


def decorr_sectors_u8(a, block, sectors, window="hann"):
    """``decorr_rings_u8`` per direction: -> float64 device tensor [planes, nby * nbx, block // 2 + 1, sectors, 2], ``sum |F|`` and
    ``sum |F|**2`` per (ring, sector) cell, the sectors as in ``frc_sectors_u8``; ``sectors=1`` gives the bits of ``decorr_rings_u8``."""
    (a,), H, W, planes, nb = _frc_sums_args("decorr_sectors_u8", (a,), block, window)
    _check_frc_sectors("decorr_sectors_u8", sectors)
    ct, st = _frc_device_tables(block, window, a.device)
    bx, by = _frc_device_bounds(sectors, a.device)
    lib = L.lib()
    nbytes = lib.pssr_decorr_sectors_workspace_bytes(planes, H, W, block, sectors)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=a.device)
    sums = torch.empty(planes, nb, block // 2 + 1, sectors, 2, dtype=torch.float64, device=a.device)
    L.check(lib.pssr_decorr_sectors_u8(L.ptr(a), L.ptr(ct), L.ptr(st), L.ptr(bx), L.ptr(by), L.ptr(sums), planes, H, W, block, sectors, L.ptr(ws),
                                       nbytes, L.stream_ptr()), "pssr_decorr_sectors_u8")
    return sums


# ----------------------------------------------------------------------------------------------
# scan phase of a bidirectional scanner (csrc/scanline.hip, csrc/crappify.hip; definitions in include/pssr_mi355.h)
MAX_SCAN_RADIUS = 16


def line_moments_u8(x, radius):
    """uint8 device tensor ``x`` [..., H, W] (a non-contiguous one is copied), ``H >= 3``, ``W >= T = 2 radius + 1``, ``radius`` an int in
    0 .. 16 -> int64 [planes, H - 2, 3 T + 2]: per interior row ``y`` the exact ``sum O_k, sum O_k**2, sum O_k E`` for ``k = -radius ..
    radius`` with ``O_k = x[y, c + k]`` and ``E = x[y - 1, c] + x[y + 1, c]`` over the columns ``c`` in ``radius .. W - radius - 1``, then
    ``sum E, sum E**2``.  One launch for all planes."""
    if not torch.is_tensor(x) or x.dtype != torch.uint8 or not x.is_cuda or x.dim() < 2:
        raise ValueError("line_moments_u8 needs a uint8 device tensor [..., H, W]")
    if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= MAX_SCAN_RADIUS:
        raise ValueError(f"line_moments_u8: the radius must be an int in 0 .. {MAX_SCAN_RADIUS} pixels. Given {radius!r}.")
    H, W = x.shape[-2:]
    T = 2 * radius + 1
    planes = x.numel() // (H * W) if H * W else 0
    if planes < 1 or H < 3 or W < T or H * W > 1 << 28:
        raise ValueError(f"line_moments_u8: {planes} planes of {H}x{W} (at least 3 rows, at least {T} columns for radius={radius}, at most 2**28 pixels)")
    x = x.contiguous()
    sums = torch.empty(planes, H - 2, 3 * T + 2, dtype=torch.int64, device=x.device)
    L.check(L.lib().pssr_line_moments_u8(L.ptr(x), L.ptr(sums), planes, H, W, radius, L.stream_ptr()), "pssr_line_moments_u8")
    return sums


def _shift_rows_args(who, x, table, dtype):
    if not torch.is_tensor(x) or x.dtype != dtype or not x.is_cuda or x.dim() < 2:
        raise ValueError(f"{who} needs a {dtype} device tensor [..., H, W]")
    H, W = x.shape[-2:]
    planes = x.numel() // (H * W) if H * W else 0
    if planes < 1 or H * W > 1 << 28:
        raise ValueError(f"{who}: {planes} planes of {H}x{W} (at least one pixel, at most 2**28 per plane)")
    if not torch.is_tensor(table) or table.dtype != torch.int32 or not table.is_cuda or table.numel() != planes * H or not table.is_contiguous():
        raise ValueError(f"{who} needs a contiguous int32 device table of {planes * H} entries, one per plane and row")
    return x.contiguous(), planes, H, W


def shift_rows_u8(x, table):
    """uint8 device tensor ``x`` [..., H, W] and an int32 device ``table`` with one entry ``d`` per (plane, row), in 1/256 pixel -> uint8
    like ``x``: the content of every row moved right by ``d / 256`` with edge replication, ``((256 - f) a + f b + 128) >> 8``."""
    x, planes, H, W = _shift_rows_args("shift_rows_u8", x, table, torch.uint8)
    out = torch.empty_like(x)
    L.check(L.lib().pssr_shift_rows_u8(L.ptr(x), L.ptr(out), L.ptr(table), planes, H, W, L.stream_ptr()), "pssr_shift_rows_u8")
    return out


def shift_rows_f32(x, table, gain, flags):
    """float32 device tensor ``x`` [..., H, W] and a row ``table`` as for :func:`shift_rows_u8` -> float32 like ``x``: the rows moved,
    ``((256 - f) a + f b) / 256`` in float64, then ``+ gain`` and the crappifier stages' round / clip by ``flags``."""
    x, planes, H, W = _shift_rows_args("shift_rows_f32", x, table, torch.float32)
    out = torch.empty_like(x)
    L.check(L.lib().pssr_shift_rows_f32(L.ptr(x), L.ptr(out), L.ptr(table), planes, H, W, C.c_float(gain), flags, L.stream_ptr()),
            "pssr_shift_rows_f32")
    return out


def scan_rows_table(tiles, frames, h, intensity, spread, jitter, seed, tile_offset, tile_counter=None):
    """The ScanPhase crappifier's row table, int32 [tiles, frames, h] on the current device: ``rint(256 (phi_t (y & 1) + j))`` clamped to
    +-256 * 64 with the tile's phase ``phi_t = intensity (+ spread N)`` and the row's ``j = jitter N`` from the Philox stream of
    ``(seed, tile_offset + tile_counter + tile)``."""
    table = torch.empty(tiles, frames, h, dtype=torch.int32, device="cuda")
    L.check(L.lib().pssr_scan_rows_table(L.ptr(table), tiles, frames, h, C.c_float(intensity), C.c_float(spread), C.c_float(jitter),
                                         C.c_uint64(seed), C.c_uint64(tile_offset), L.ptr(tile_counter), L.stream_ptr()),
            "pssr_scan_rows_table")
    return table


# ----------------------------------------------------------------------------------------------
# classical baselines (csrc/baseline.hip; definitions B1 and B2 in include/pssr_mi355.h)
MAX_NLM_PATCH = 3
MAX_NLM_SEARCH = 10
MAX_UPSAMPLE = 8
UPSAMPLE_FILTERS = ("bilinear", "bicubic")


def __getattr__(name):
    if name == "NLM_LUT":                       # the library's table of 256 weights, read once
        table = (C.c_int32 * 256)()
        L.check(L.lib().pssr_nlm_lut(table), "pssr_nlm_lut")
        globals()["NLM_LUT"] = tuple(table)
        return globals()["NLM_LUT"]
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def _u8_planes_args(who, x):
    if not torch.is_tensor(x) or x.dtype != torch.uint8 or not x.is_cuda or x.dim() < 2:
        raise ValueError(f"{who} needs a uint8 device tensor [..., H, W]")
    H, W = x.shape[-2:]
    planes = x.numel() // (H * W) if H * W else 0
    if planes < 1 or H * W > 1 << 28:
        raise ValueError(f"{who}: {planes} planes of {H}x{W} (at least one pixel, at most 2**28 per plane)")
    return x.contiguous(), planes, H, W


def _int_in(v, lo, hi):
    return not isinstance(v, bool) and isinstance(v, int) and lo <= v <= hi


def nlm_u8(x, p, s, qmul, qshift, bias):
    """uint8 device tensor ``x`` [..., H, W] (a non-contiguous one is copied) -> uint8 like ``x``: the integer non-local means B2 of
    include/pssr_mi355.h with patch radius ``p`` (1 .. 3), search radius ``s`` (1 .. 10) and the three integers of
    ``util._nlm_params``.  One launch for all planes; the same bits on every run."""
    x, planes, H, W = _u8_planes_args("nlm_u8", x)
    if not _int_in(p, 1, MAX_NLM_PATCH) or not _int_in(s, 1, MAX_NLM_SEARCH):
        raise ValueError(f"nlm_u8: p must be an int in 1 .. {MAX_NLM_PATCH} and s one in 1 .. {MAX_NLM_SEARCH}. Given {p!r} and {s!r}.")
    if not _int_in(qmul, 1, 1023) or not _int_in(qshift, 0, 31) or not _int_in(bias, 0, (1 << 31) - 1):
        raise ValueError(f"nlm_u8: qmul must be an int in 1 .. 1023, qshift in 0 .. 31, bias in 0 .. 2**31 - 1. Given {qmul!r}, {qshift!r}, {bias!r}.")
    out = torch.empty_like(x)
    L.check(L.lib().pssr_nlm_u8(L.ptr(x), L.ptr(out), planes, H, W, p, s, qmul, qshift, bias, L.stream_ptr()), "pssr_nlm_u8")
    return out


def upsample_u8(x, r, filter):
    """uint8 device tensor ``x`` [..., h, w] (a non-contiguous one is copied) -> uint8 [..., h r, w r]: Pillow's 8-bit ``Image.resize``
    with ``filter`` ``"bilinear"`` or ``"bicubic"``, bit for bit (B1 of include/pssr_mi355.h), ``r`` an int in 1 .. 8.  One launch for
    all planes, both passes fused."""
    x, planes, h, w = _u8_planes_args("upsample_u8", x)
    if not _int_in(r, 1, MAX_UPSAMPLE):
        raise ValueError(f"upsample_u8: r must be an int in 1 .. {MAX_UPSAMPLE}. Given {r!r}.")
    if filter not in UPSAMPLE_FILTERS:
        raise ValueError(f"upsample_u8: filter must be one of {UPSAMPLE_FILTERS}. Given {filter!r}.")
    if h * r * w * r > 1 << 28:
        raise ValueError(f"upsample_u8: {h * r}x{w * r} output pixels per plane (at most 2**28)")
    out = torch.empty(*x.shape[:-2], h * r, w * r, dtype=torch.uint8, device=x.device)
    L.check(L.lib().pssr_upsample_u8(L.ptr(x), L.ptr(out), planes, h, w, r, UPSAMPLE_FILTERS.index(filter), L.stream_ptr()), "pssr_upsample_u8")
    return out
