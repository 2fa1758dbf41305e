"""numpy restatements of predict_sheet's blend / ensemble path, in int64 throughout, written from the definitions (DESIGN.md §7 (14),
include/pssr_mi355.h) and not from the kernels: the dihedral members ``T_d`` / ``U_d``, the per-axis weight ``w1``, the stitched sheet
``blend_ref`` and the cut ``dihedral_tiles_ref``."""
import numpy as np


def T_d(a, d):
    """Member ``d`` of the last two (square) axes of ``a``."""
    return np.rot90(a[..., ::-1] if d & 4 else a, d & 3, axes=(-2, -1))


def U_d(b, d):
    """The inverse of ``T_d``."""
    c = np.rot90(b, -(d & 3), axes=(-2, -1))
    return c[..., ::-1] if d & 4 else c


def w1(l, S, O, M, first, last, blend):
    """Weight of local coordinate ``l`` on one axis of a tile of edge ``S`` (overlap ``O``, margin ``M``, both in output pixels) that is
    ``first`` / ``last`` of its grid row or column."""
    T = max(O - 2 * M, 0) + 1
    if (not first and l < M) or (not last and l >= S - M):
        return 0
    w = min(T, T if first else l - M + 1, T if last else S - M - l)
    return w if blend == "linear" else 1


def axis_weights(S, O, M, n, blend):
    """int64 [n, (n - 1) * (S - O) + S]: row ``r`` holds tile ``r``'s ``w1`` at the stitched coordinates it covers, 0 elsewhere."""
    step = S - O
    out = np.zeros((n, (n - 1) * step + S), dtype=np.int64)
    for r in range(n):
        out[r, r * step:r * step + S] = [w1(l, S, O, M, r == 0, r == n - 1, blend) for l in range(S)]
    return out


def blend_ref(preds, n_slices, n_rows, n_cols, overlap, margin, out_h, out_w, blend, ensemble):
    """uint8 [n_slices, C, out_h, out_w] from member predictions [n_slices * n_rows * n_cols * ensemble, C, S, S] in item order
    (tile * ensemble + d, tiles slice-major), all in the sheet's orientation: floor(num / den), 0 where den is 0."""
    preds = np.asarray(preds).astype(np.int64)
    n, c, S, _ = preds.shape
    per = n_rows * n_cols
    assert n == n_slices * per * ensemble
    step = S - overlap
    H, W = n_rows * step + overlap, n_cols * step + overlap
    wy, wx = axis_weights(S, overlap, margin, n_rows, blend), axis_weights(S, overlap, margin, n_cols, blend)
    num, den = np.zeros((n_slices, c, H, W), dtype=np.int64), np.zeros((H, W), dtype=np.int64)
    for r in range(n_rows):
        for q in range(n_cols):
            w = np.outer(wy[r, r * step:r * step + S], wx[q, q * step:q * step + S])
            den[r * step:r * step + S, q * step:q * step + S] += w
            for k in range(n_slices):
                g0 = (k * per + r * n_cols + q) * ensemble
                num[k, :, r * step:r * step + S, q * step:q * step + S] += w * preds[g0:g0 + ensemble].sum(0)
    den = den * ensemble
    out = np.where(den > 0, num // np.maximum(den, 1), 0)
    return out[:, :, :out_h, :out_w].astype(np.uint8)


def grid(n, size, stride):
    """Windows of the smallest grid that reaches the end of an axis of ``n`` pixels (predict_sheet's ``cover``)."""
    return -(-max(n - size, 0) // stride) + 1


def dihedral_tiles_ref(stack, m, frame_step, size, stride, tiles_y, tiles_x, n_slices, ensemble):
    """float32 [n_slices * tiles_y * tiles_x * ensemble, m, size, size] in item order: the stack reflect-padded (np.pad) at the bottom
    and the right to the grid's extent, the windows sliced slice-major, every frame plane of member ``d`` turned by ``T_d``."""
    f, h, w = stack.shape
    ext_h, ext_w = (tiles_y - 1) * stride + size, (tiles_x - 1) * stride + size
    pad = np.pad(stack, ((0, 0), (0, max(ext_h - h, 0)), (0, max(ext_w - w, 0))), mode="reflect")
    return np.stack([T_d(pad[k * frame_step:k * frame_step + m, ty * stride:ty * stride + size, tx * stride:tx * stride + size], d)
                     for k in range(n_slices) for ty in range(tiles_y) for tx in range(tiles_x) for d in range(ensemble)]).astype(np.float32)
