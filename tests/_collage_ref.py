"""numpy restatement of pssr_collage_rows_u8 (plain indexing with the tables) for tests/test_gpu_collage.py."""
import numpy as np


def to_u8(a):
    """uint8 as it is; float32 as ``np.clip(x, 0, 255).astype(np.uint8)`` (truncation toward zero: pssr/predict.py:245-246)."""
    a = np.asarray(a)
    return a if a.dtype == np.uint8 else np.clip(a, 0, 255).astype(np.uint8)


def panel(src, yi=None, xi=None):
    """[n, h, w] uint8: ``src[:, yi[y], xi[x]]`` of a [n, src_h, src_w] array; a row / column index outside the source gives 0."""
    src = to_u8(src)
    n, sh, sw = src.shape
    yi = np.arange(sh) if yi is None else np.asarray(yi, dtype=np.int64)
    xi = np.arange(sw) if xi is None else np.asarray(xi, dtype=np.int64)
    ok_y, ok_x = (yi >= 0) & (yi < sh), (xi >= 0) & (xi < sw)
    out = src[:, np.where(ok_y, yi, 0)][:, :, np.where(ok_x, xi, 0)].copy()
    out[:, ~ok_y, :] = 0
    out[:, :, ~ok_x] = 0
    return out


def compose(canvas, panels, row0=0):
    """Writes the rows into a copy of ``canvas`` [rows, columns]: image i at rows (row0 + i) * h, panel p at columns p * w.
    ``panels``: arrays or (array, yi, xi) tuples."""
    out = np.array(canvas, dtype=np.uint8, copy=True)
    for p, spec in enumerate(panels):
        block = panel(*spec) if isinstance(spec, (tuple, list)) else panel(spec)
        n, h, w = block.shape
        out[row0 * h:(row0 + n) * h, p * w:(p + 1) * w] = block.reshape(n * h, w)
    return out
