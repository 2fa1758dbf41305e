"""numpy restatements of the self-ensemble of predict_images / test_metrics and of the spread maps, in int64, written from the definitions
(include/pssr_mi355.h) and not from the kernels: the member sequence ``members_ref``, the reduction ``reduce_ref`` and the
stitched spread ``spread_stack_ref``."""
import numpy as np

from _blend_ref import T_d, U_d, axis_weights


def clip_u8(y):
    """pssr_clip_u8: clip to [0, 255], truncate; NaN gives 0."""
    y = np.asarray(y, dtype=np.float64)
    return np.clip(np.where(np.isnan(y), 0.0, y), 0, 255).astype(np.uint8)


def members_ref(x, E):
    """float32 [n * E, m, s, s]: item ``i * E + d`` is ``x[i]`` with every frame plane turned by ``T_d``."""
    x = np.asarray(x)
    return np.stack([T_d(x[i], d) for i in range(len(x)) for d in range(E)]).astype(np.float32)


def reduce_ref(y, E):
    """``(mean, spread)``, uint8 [n, C, S, S], of member predictions [n * E, C, S, S]: with ``q[i, d] = U_d(clip_u8(y[i * E + d]))``,
    ``mean = floor(sum_d q / E)`` and ``spread = max_d q - min_d q``."""
    q = clip_u8(y).astype(np.int64)
    n = len(q) // E
    assert len(q) == n * E
    q = np.stack([np.stack([U_d(q[i * E + d], d) for d in range(E)]) for i in range(n)])
    return (q.sum(1) // E).astype(np.uint8), (q.max(1) - q.min(1)).astype(np.uint8)


def spread_stack_ref(preds, n_slices, n_rows, n_cols, O, M, out_h, out_w, E):
    """uint8 [n_slices, C, out_h, out_w] from ``blend_ref``'s member predictions: max - min of ``preds[tile * E + d]`` over every member and
    every tile whose ``w1_y * w1_x`` is non-zero at the pixel; 0 where no tile covers it."""
    preds = np.asarray(preds).astype(np.int64)
    n, c, S, _ = preds.shape
    per = n_rows * n_cols
    assert n == n_slices * per * E
    step = S - O
    H, W = n_rows * step + O, n_cols * step + O
    wy, wx = axis_weights(S, O, M, n_rows, "average"), axis_weights(S, O, M, n_cols, "average")
    lo, hi = np.full((n_slices, c, H, W), 256, dtype=np.int64), np.full((n_slices, c, H, W), -1, dtype=np.int64)
    for r in range(n_rows):
        for q in range(n_cols):
            on = np.outer(wy[r, r * step:r * step + S], wx[q, q * step:q * step + S]) > 0
            ys, xs = slice(r * step, r * step + S), slice(q * step, q * step + S)
            for k in range(n_slices):
                g0 = (k * per + r * n_cols + q) * E
                mem = preds[g0:g0 + E]
                lo[k, :, ys, xs] = np.where(on, np.minimum(lo[k, :, ys, xs], mem.min(0)), lo[k, :, ys, xs])
                hi[k, :, ys, xs] = np.where(on, np.maximum(hi[k, :, ys, xs], mem.max(0)), hi[k, :, ys, xs])
    out = np.where(hi >= lo, hi - lo, 0)
    return out[:, :, :out_h, :out_w].astype(np.uint8)
