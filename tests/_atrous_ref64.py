"""Plain float64 references of the operations of csrc/atrous.hip: torch / numpy on the CPU, no project imports, one function per
operation.  Tensors are channels-last ([n, h, w, c], or [npix, c] where the pixel grid does not matter) and whole: the references
know nothing about channel strides or offsets, the tests slice.  Pinned against torch by tests/test_atrous_ref64.py.

The bilinear resize takes its source coordinates in float32 (bilinear_taps), as torch and the kernel specify them: they are part
of the operation's definition, not an error to be bounded.  Everything else is float64."""
import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64


def _d(t):
    return torch.as_tensor(t).to(F64)


# ---- pointwise -------------------------------------------------------------------------------------------------------------------
def input_plain(x_nchw, out_c, a, b):
    """[n, c, h, w] -> [n, h, w, out_c]: x * a + b in the first c channels, zero in the rest."""
    x = _d(x_nchw)
    n, c, h, w = x.shape
    out = torch.zeros(n, h, w, out_c, dtype=F64)
    out[..., :c] = (x * float(a) + float(b)).permute(0, 2, 3, 1)
    return out


def preact(x, scale, shift):
    """x * scale + shift per channel (the pre-activation whose sign is the ReLU mask)."""
    return _d(x) * _d(scale) + _d(shift)


def affine_relu(x, scale, shift):
    return preact(x, scale, shift).clamp_min(0)


def sum_list(xs, relu):
    s = _d(xs[0]).clone()
    for x in xs[1:]:
        s = s + _d(x)
    return s.clamp_min(0) if relu else s


def relu_mask(dout, out):
    """dz = dout where out > 0, else 0."""
    dout = _d(dout)
    return torch.where(_d(out) > 0, dout, torch.zeros_like(dout))


def channel_stats(x):
    """(sum, sum of squares) per channel over every other axis."""
    x = _d(x).reshape(-1, x.shape[-1])
    return x.sum(0), (x * x).sum(0)


# ---- dilated 3x3 gather / fold -----------------------------------------------------------------------------------------------------
def _shifted(x, oy, ox):
    """out[:, y, x] = x[:, y + oy, x + ox], zero outside the image; x is [n, h, w, c]."""
    n, h, w, c = x.shape
    out = torch.zeros_like(x)
    ys0, ys1 = max(0, -oy), min(h, h - oy)
    xs0, xs1 = max(0, -ox), min(w, w - ox)
    if ys0 < ys1 and xs0 < xs1:
        out[:, ys0:ys1, xs0:xs1] = x[:, ys0 + oy:ys1 + oy, xs0 + ox:xs1 + ox]
    return out


def im2col_dil(x, dil, scale=None, shift=None, round_to=None):
    """[n, h, w, c] -> [n, h, w, 9, c]: nine zero-padded shifted copies, tap t = 3 (dy + 1) + (dx + 1) reads the pixel at
    (y + dy dil, x + dx dil).  With scale / shift the copies are of relu(x * scale + shift), rounded to `round_to` if given."""
    a = _d(x)
    if scale is not None:
        a = affine_relu(a, scale, shift)
        if round_to is not None:
            a = a.to(round_to).to(F64)
    return torch.stack([_shifted(a, (t // 3 - 1) * dil, (t % 3 - 1) * dil) for t in range(9)], dim=3)


def col2im_dil(dcol, dil):
    """Adjoint of im2col_dil: [n, h, w, 9, c] -> [n, h, w, c], out[p] = sum_t dcol[p - off_t][t]."""
    dcol = _d(dcol)
    out = torch.zeros_like(dcol[:, :, :, 0])
    for t in range(9):
        out = out + _shifted(dcol[:, :, :, t], -(t // 3 - 1) * dil, -(t % 3 - 1) * dil)
    return out


def preact_mask(y, scale, shift):
    return preact(y, scale, shift) > 0


def bn_bwd_stats(g, y, mean, invstd):
    """[sum g, sum g (y - mean) invstd] per channel."""
    g, y = _d(g), _d(y)
    c = g.shape[-1]
    xhat = (y - _d(mean)) * _d(invstd)
    return g.reshape(-1, c).sum(0), (g * xhat).reshape(-1, c).sum(0)


# ---- k x k max pooling -------------------------------------------------------------------------------------------------------------
def _windows(x, k):
    """[n, h, w, c] -> [n, h // k, w // k, c, k * k], the window in row-major order."""
    n, h, w, c = x.shape
    ho, wo = h // k, w // k
    v = x[:, :ho * k, :wo * k].reshape(n, ho, k, wo, k, c)
    return v.permute(0, 1, 3, 5, 2, 4).reshape(n, ho, wo, c, k * k)


def maxpool_k(x, k):
    """Floor mode: windows [k oy, k oy + k)."""
    return _windows(_d(x), k).amax(-1)


def maxpool_k_bwd(x, dpool, k):
    """The gradient goes to the first maximum of each window in row-major order; pixels outside every window get zero."""
    x, dpool = _d(x), _d(dpool)
    n, h, w, c = x.shape
    ho, wo = h // k, w // k
    first = torch.from_numpy(np.argmax(_windows(x, k).numpy(), axis=-1))          # numpy: the first occurrence
    hot = F.one_hot(first, k * k).to(F64) * dpool[..., None]                     # [n, ho, wo, c, k k]
    dx = torch.zeros_like(x)
    dx[:, :ho * k, :wo * k] = hot.reshape(n, ho, wo, c, k, k).permute(0, 1, 4, 2, 5, 3).reshape(n, ho * k, wo * k, c)
    return dx


# ---- bilinear resize, align_corners = False ----------------------------------------------------------------------------------------
def bilinear_taps(in_size, out_size):
    """(i0, i1, l1) of every destination index, in numpy float32 as torch specifies them: scale = f32(in) / f32(out),
    src = max((dst + 0.5) * scale - 0.5, 0), i0 = floor(src) (at most in - 1), i1 = min(i0 + 1, in - 1), l1 = src - i0.

    The product and the difference are ONE fused multiply-add, as in torch's vectorised CPU kernels, its device kernels and
    bil_src: with the product rounded on its own F.interpolate itself is missed by 2e-5 at 161 -> 323 (3e-7 fused); below
    about 16 source pixels the two agree to 2e-7.  numpy has no fma: the float64 product of two float32 is exact (48 bits), and where
    it is at least 0.5 so is the difference (below 0.5 the clamp gives 0 either way), hence one rounding to float32 is the fma."""
    f = np.float32
    scale = f(in_size) / f(out_size)
    dst = np.arange(out_size, dtype=f)
    src = ((dst + f(0.5)).astype(np.float64) * np.float64(scale) - 0.5).astype(f)
    src = np.maximum(src, f(0)).astype(f)
    i0 = np.minimum(src.astype(np.int64), in_size - 1)
    i1 = np.minimum(i0 + 1, in_size - 1)
    l1 = (src - i0.astype(f)).astype(f)
    assert src.dtype == f and l1.dtype == f
    return i0, i1, l1


def _tap_tensors(in_size, out_size):
    i0, i1, l1 = bilinear_taps(in_size, out_size)
    l1 = torch.from_numpy(l1.astype(np.float64))
    return torch.from_numpy(i0), torch.from_numpy(i1), 1.0 - l1, l1


def bilinear_up(x, h, w):
    """[n, hs, ws, c] -> [n, h, w, c] with the float32 taps and float64 interpolation."""
    x = _d(x)
    y0, y1, wy0, wy1 = _tap_tensors(x.shape[1], h)
    x0, x1, wx0, wx1 = _tap_tensors(x.shape[2], w)
    rows = x[:, y0] * wy0[None, :, None, None] + x[:, y1] * wy1[None, :, None, None]
    return rows[:, :, x0] * wx0[None, None, :, None] + rows[:, :, x1] * wx1[None, None, :, None]


def _scatter(t, dim, size, i0, i1, w0, w1):
    shape = [1] * t.dim()
    shape[dim] = -1
    out_shape = list(t.shape)
    out_shape[dim] = size
    out = torch.zeros(out_shape, dtype=F64)
    out.index_add_(dim, i0, t * w0.view(shape))
    out.index_add_(dim, i1, t * w1.view(shape))
    return out


def bilinear_weights(in_size, out_size):
    """[out, in] float64 matrix of the resize along one axis (scatter-add of the two taps of each destination index)."""
    i0, i1, w0, w1 = _tap_tensors(in_size, out_size)
    return _scatter(torch.eye(out_size, dtype=F64), 1, in_size, i0, i1, w0, w1)


def bilinear_up_bwd(dout, hs, ws):
    """The exact adjoint of bilinear_up by scatter-add in float64: (din [n, hs, ws, c], count [hs, ws], abs_sum [n, hs, ws, c]),
    count = destination pixels with a non-zero weight on the source pixel, abs_sum = sum |weight * dout| over them."""
    dout = _d(dout)
    n, h, w, c = dout.shape
    ty, tx = _tap_tensors(hs, h), _tap_tensors(ws, w)

    def adj(t):
        return _scatter(_scatter(t, 1, hs, *ty), 2, ws, *tx)
    cy = (bilinear_weights(hs, h) != 0).sum(0)
    cx = (bilinear_weights(ws, w) != 0).sum(0)
    return adj(dout), cy[:, None] * cx[None, :], adj(dout.abs())
