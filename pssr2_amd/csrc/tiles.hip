// Device-side tiling and reassembly for whole-sheet prediction (BASELINE config 5):
//   * sliding-window LR tiles straight from a uint8 sheet resident in HBM (pssr/data.py:629-638 `_sliding_window`, row-major
//     tiles, stride = size - overlap, trailing remainder dropped; `_tensor_ready`: float32 of the integer values);
//   * overlap-averaged stitching of the predicted uint8 tiles (pssr/util.py:116-137 `_patch_images` followed by the uint8
//     cast of `reassemble_sheets`, pssr/util.py:101): out = floor(sum / count) with `margin` pixels trimmed on inner edges.
// Both are pure index arithmetic + one integer divide per pixel, bit-exact.
// The stack forms (predict_sheet's n_frames / slide / cover) number the tiles slice-major over all frame slices of a stack, read a grid
// that leaves the sheet at the bottom / right through np.pad(mode="reflect")'s source index, and stitch every slice, cropped, in one launch.
// The dihedral forms (predict_sheet's blend / ensemble) cut every tile in up to 8 rotations and flips, store the quantised predictions
// turned back, and stitch them with feathered integer weights and the member average in one division.
// The batch forms (predict_images' / test_metrics' ensemble) turn a batch of square items into its members and reduce the members' predictions
// to their integer mean and spread without storing them; the spread of a stitched sheet is the stitch's gather with min / max (§7 (15)).
#include "common.h"

namespace {

__global__ void sliding_tiles_kernel(const uint8_t* __restrict__ sheet, float* __restrict__ out, int c, int h, int w, int size, int stride,
                                     int tiles_x, int tile0, int ntile) {
    const long total = (long)ntile * c * size * size;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = i % size;
        long t = i / size;
        const int y = t % size; t /= size;
        const int ch = t % c;
        const int tile = tile0 + (int)(t / c);
        const int ty = tile / tiles_x, tx = tile % tiles_x;
        out[i] = (float)sheet[((long)ch * h + ty * stride + y) * w + tx * stride + x];
    }
}

// gather formulation: every output pixel sums the tiles that cover it (after margin trimming) and divides
__global__ void patch_tiles_kernel(const uint8_t* __restrict__ tiles, uint8_t* __restrict__ out, int c, int n_rows, int n_cols, int size,
                                   int overlap, int margin) {
    const int step = size - overlap;
    const int H = n_rows * step + overlap, W = n_cols * step + overlap;
    const long total = (long)c * H * W;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = i % W;
        const int y = (i / W) % H;
        const int ch = i / ((long)W * H);
        // tile rows r with r*step <= y < r*step + size
        int r_lo = (y - size) / step + 1; if (r_lo < 0 || y < size) r_lo = (y >= size) ? r_lo : 0;
        int r_hi = y / step; if (r_hi > n_rows - 1) r_hi = n_rows - 1;
        int c_lo = (x - size) / step + 1; if (c_lo < 0 || x < size) c_lo = (x >= size) ? c_lo : 0;
        int c_hi = x / step; if (c_hi > n_cols - 1) c_hi = n_cols - 1;
        unsigned sum = 0, cnt = 0;
        for (int r = r_lo; r <= r_hi; ++r) {
            const int ly = y - r * step;
            if (ly < 0 || ly >= size) continue;
            const int top = r != 0 ? margin : 0, bot = r != n_rows - 1 ? margin : 0;
            if (ly < top || ly >= size - bot) continue;
            for (int q = c_lo; q <= c_hi; ++q) {
                const int lx = x - q * step;
                if (lx < 0 || lx >= size) continue;
                const int lef = q != 0 ? margin : 0, rig = q != n_cols - 1 ? margin : 0;
                if (lx < lef || lx >= size - rig) continue;
                sum += tiles[(((long)(r * n_cols + q) * c + ch) * size + ly) * size + lx];
                ++cnt;
            }
        }
        out[i] = cnt ? (uint8_t)(sum / cnt) : 0;
    }
}

// np.pad(mode="reflect") source index of extended coordinate i >= 0 on an axis of n >= 2 pixels (the edge pixel is not repeated)
__device__ __forceinline__ int fold_reflect(int i, int n) {
    const int p = 2 * (n - 1), j = i % p;
    return j < n ? j : p - j;
}

// One tile per blockIdx.y step, its m*size rows spread over blockIdx.x and the thread rows of a block; a thread keeps its V-pixel column
// group and walks rows: one 32-bit divide and one y fold per row, x folded only in tiles that cross the right edge (uniform per tile).
// V = 4: one 16-byte store per thread and row (size % 4 == 0, tiles 16-byte aligned); the sheet side is byte loads, w being arbitrary.
template <int V>
__global__ void __launch_bounds__(256) stack_tiles_kernel(const uint8_t* __restrict__ stack, float* __restrict__ out, int h, int w, int m,
                                                          int frame_step, int size, int stride, int per_slice, int tiles_x, int tile0, int ntile) {
    const int groups = size / V;                                  // column groups per row
    const int gx = groups < 256 ? groups : 256;                   // of which a block covers gx at a time,
    const int rows_per_pass = 256 / gx;                           // on rows_per_pass rows
    const int lx = threadIdx.x % gx, ly = threadIdx.x / gx;
    if (ly >= rows_per_pass) return;
    const int rows = m * size;
    for (int i = blockIdx.y; i < ntile; i += gridDim.y) {
        const int g = tile0 + i, k = g / per_slice, t = g % per_slice;
        const int y0 = (t / tiles_x) * stride, x0 = (t % tiles_x) * stride;
        const bool fold_x = x0 + size > w;
        const uint8_t* slice = stack + (long)k * frame_step * h * w;
        float* tile = out + (long)i * rows * size;
        for (int row = blockIdx.x * rows_per_pass + ly; row < rows; row += gridDim.x * rows_per_pass) {
            const int f = row / size;
            int sy = y0 + (row - f * size);
            if (sy >= h) sy = fold_reflect(sy, h);
            const uint8_t* src = slice + ((long)f * h + sy) * w;
            float* dst = tile + (long)row * size;
            for (int q = lx; q < groups; q += gx) {
                const int sx = x0 + q * V;
                float v[V];
                if (fold_x) {
#pragma unroll
                    for (int j = 0; j < V; ++j) v[j] = (float)src[sx + j < w ? sx + j : fold_reflect(sx + j, w)];
                } else {
#pragma unroll
                    for (int j = 0; j < V; ++j) v[j] = (float)src[sx + j];
                }
                if constexpr (V == 4) *reinterpret_cast<float4*>(dst + q * 4) = make_float4(v[0], v[1], v[2], v[3]);
                else dst[q] = v[0];
            }
        }
    }
}

// patch_tiles_kernel's value for the top-left out_h x out_w pixels of every slice: one output row per blockIdx.y step (the tile rows
// that cover it and their margins found once), threads along x
__global__ void __launch_bounds__(256) patch_stack_kernel(const uint8_t* __restrict__ tiles, uint8_t* __restrict__ out, long n_out_rows, int c,
                                                          int n_rows, int n_cols, int size, int overlap, int margin, int out_h, int out_w) {
    const int step = size - overlap;
    const int per_slice = n_rows * n_cols;
    for (long orow = blockIdx.y; orow < n_out_rows; orow += gridDim.y) {
        const int y = (int)(orow % out_h);
        const long sc = orow / out_h;                              // slice * c + channel
        const int ch = (int)(sc % c);
        const long first_tile = (sc / c) * per_slice;
        const int r_lo = y >= size ? (y - size) / step + 1 : 0;
        int r_hi = y / step; if (r_hi > n_rows - 1) r_hi = n_rows - 1;
        for (int x = blockIdx.x * 256 + threadIdx.x; x < out_w; x += gridDim.x * 256) {
            const int c_lo = x >= size ? (x - size) / step + 1 : 0;
            int c_hi = x / step; if (c_hi > n_cols - 1) c_hi = n_cols - 1;
            unsigned sum = 0, cnt = 0;
            for (int r = r_lo; r <= r_hi; ++r) {
                const int ly = y - r * step;
                const int top = r != 0 ? margin : 0, bot = r != n_rows - 1 ? margin : 0;
                if (ly < top || ly >= size - bot) continue;
                for (int q = c_lo; q <= c_hi; ++q) {
                    const int lx = x - q * step;
                    const int lef = q != 0 ? margin : 0, rig = q != n_cols - 1 ? margin : 0;
                    if (lx < lef || lx >= size - rig) continue;
                    sum += tiles[(((first_tile + r * n_cols + q) * c + ch) * size + ly) * size + lx];
                    ++cnt;
                }
            }
            out[orow * out_w + x] = cnt ? (uint8_t)(sum / cnt) : 0;
        }
    }
}

// ---- dihedral self-ensemble and weighted stitching (predict_sheet's blend / ensemble path; definitions: include/pssr_mi355.h)
// Element (r, c) of T_d(a) is a[rev_r ? n-1-p : p][rev_c ? n-1-q : q] with (p, q) = tr ? (c, r) : (r, c); U_d = T_d^-1 has the same form.
struct dihedral_map { int tr, rev_r, rev_c; };
__device__ __forceinline__ dihedral_map dihedral(int d, bool inverse) {
    const int rot = d & 3, tr = rot & 1, ry = rot >> 1, rx = (((rot + 1) >> 1) ^ (d >> 2)) & 1;
    return tr && inverse ? dihedral_map{tr, rx, ry} : dihedral_map{tr, ry, rx};
}

// One 32 x 32 block at (r0, c0) of an n x n destination plane, dst(r, c) = fetch(source row, source column) under `mp`, by 256 threads.
// Lanes run along destination rows when storing and along SOURCE rows when fetching: a transposing member goes through an LDS block of
// 33-dword pitch (row writes and column reads both touch 32 different banks per 32-lane group), the others map row to row directly.
// The gather half leaves a thread the values of its four destination pixels (r0 + ty + 8 k, c0 + tx), k < 4 (0 outside the plane); the store
// half writes them.  A kernel that reduces over members keeps the four in registers between the two (ensemble_reduce_kernel).
template <typename F>
__device__ __forceinline__ void dihedral_gather(float (&v)[4], int n, int r0, int c0, dihedral_map mp, float (*lds)[33], F fetch) {
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    if (!mp.tr) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = r0 + ty + 8 * k, c = c0 + tx;
            v[k] = r < n && c < n ? fetch(mp.rev_r ? n - 1 - r : r, mp.rev_c ? n - 1 - c : c) : 0.f;
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = r0 + tx, c = c0 + ty + 8 * k;               // lanes along r: along the source row
        if (r < n && c < n) lds[ty + 8 * k][tx] = fetch(mp.rev_r ? n - 1 - c : c, mp.rev_c ? n - 1 - r : r);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = r0 + ty + 8 * k, c = c0 + tx;
        v[k] = r < n && c < n ? lds[tx][ty + 8 * k] : 0.f;
    }
    __syncthreads();
}

template <typename T>
__device__ __forceinline__ void dihedral_store(T* __restrict__ dst, int n, int r0, int c0, const T (&v)[4]) {
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = r0 + ty + 8 * k, c = c0 + tx;
        if (r < n && c < n) dst[(long)r * n + c] = v[k];
    }
}

template <typename T, typename F>
__device__ __forceinline__ void dihedral_block(T* __restrict__ dst, int n, int r0, int c0, dihedral_map mp, float (*lds)[33], F fetch) {
    float v[4];
    dihedral_gather(v, n, r0, c0, mp, lds, fetch);
    const T t[4] = {(T)v[0], (T)v[1], (T)v[2], (T)v[3]};
    dihedral_store(dst, n, r0, c0, t);
}

// stack_tiles_kernel's window of tile g / ensemble, turned by T_(g % ensemble): one item per blockIdx.y step, its m planes' 32 x 32 blocks
// over blockIdx.x
__global__ void __launch_bounds__(256) dihedral_tiles_kernel(const uint8_t* __restrict__ stack, float* __restrict__ out, int h, int w, int m,
                                                             int frame_step, int size, int stride, int per_slice, int tiles_x, int ensemble,
                                                             int item0, int nitem) {
    __shared__ float lds[32][33];
    const int nb = (size + 31) / 32, blocks = m * nb * nb;
    for (int i = blockIdx.y; i < nitem; i += gridDim.y) {
        const int g = item0 + i, tile = g / ensemble, k = tile / per_slice, t = tile % per_slice;
        const dihedral_map mp = dihedral(g % ensemble, false);
        const int y0 = (t / tiles_x) * stride, x0 = (t % tiles_x) * stride;
        const uint8_t* slice = stack + (long)k * frame_step * h * w;
        for (int b = blockIdx.x; b < blocks; b += gridDim.x) {
            const int f = b / (nb * nb), br = b / nb % nb, bc = b % nb;
            const uint8_t* plane = slice + (long)f * h * w;
            dihedral_block(out + ((long)i * m + f) * size * size, size, br * 32, bc * 32, mp, lds, [&](int y, int x) {
                int sy = y0 + y, sx = x0 + x;
                if (sy >= h) sy = fold_reflect(sy, h);
                if (sx >= w) sx = fold_reflect(sx, w);
                return (float)plane[(long)sy * w + sx];
            });
        }
    }
}

// clip_u8_kernel's value of plane p = item * c + channel, stored through U_d, d = (phase + item) % ensemble
__global__ void __launch_bounds__(256) clip_u8_dihedral_kernel(const float* __restrict__ in, uint8_t* __restrict__ out, long planes, int c, int size,
                                                               int ensemble, int phase) {
    __shared__ float lds[32][33];
    const int nb = (size + 31) / 32;
    for (long p = blockIdx.y; p < planes; p += gridDim.y) {
        const dihedral_map mp = dihedral((int)((phase + p / c) % ensemble), true);
        const float* src = in + p * size * size;
        for (int b = blockIdx.x; b < nb * nb; b += gridDim.x)
            dihedral_block(out + p * size * size, size, (b / nb) * 32, (b % nb) * 32, mp, lds,
                           [&](int y, int x) { return fminf(fmaxf(src[(long)y * size + x], 0.f), 255.f); });   // the cast truncates toward zero
    }
}

// weight of local coordinate l on one axis of a tile that is first / last of its grid row or column; t = max(overlap - 2 margin, 0) + 1
__device__ __forceinline__ int blend_w1(int l, int size, int margin, int t, bool first, bool last, int blend) {
    if ((!first && l < margin) || (!last && l >= size - margin)) return 0;
    if (!blend) return 1;
    int v = t;
    if (!first && l - margin + 1 < v) v = l - margin + 1;
    if (!last && size - margin - l < v) v = size - margin - l;
    return v;
}

// patch_stack_kernel's gather with weights and ensemble members: one output row per blockIdx.y step (its covering tile rows and the sum
// of their weights found once), threads along x.  Acc holds 255 * ensemble * (largest weight sum)^2: the host picks 32 or 64 bits.
template <typename Acc>
__global__ void __launch_bounds__(256) blend_stack_kernel(const uint8_t* __restrict__ tiles, uint8_t* __restrict__ out, long n_out_rows, int c,
                                                          int n_rows, int n_cols, int size, int overlap, int margin, int out_h, int out_w,
                                                          int blend, int ensemble) {
    const int step = size - overlap;
    const int per_slice = n_rows * n_cols;
    const int t = (overlap > 2 * margin ? overlap - 2 * margin : 0) + 1;
    const long plane = (long)size * size, member = plane * c;
    for (long orow = blockIdx.y; orow < n_out_rows; orow += gridDim.y) {
        const int y = (int)(orow % out_h);
        const long sc = orow / out_h;                              // slice * c + channel
        const int ch = (int)(sc % c);
        const long first_tile = (sc / c) * per_slice;
        const int r_lo = y >= size ? (y - size) / step + 1 : 0;
        int r_hi = y / step; if (r_hi > n_rows - 1) r_hi = n_rows - 1;
        Acc sum_wy = 0;
        for (int r = r_lo; r <= r_hi; ++r) sum_wy += blend_w1(y - r * step, size, margin, t, r == 0, r == n_rows - 1, blend);
        for (int x = blockIdx.x * 256 + threadIdx.x; x < out_w; x += gridDim.x * 256) {
            const int c_lo = x >= size ? (x - size) / step + 1 : 0;
            int c_hi = x / step; if (c_hi > n_cols - 1) c_hi = n_cols - 1;
            Acc num = 0, sum_wx = 0;
            for (int r = r_lo; r <= r_hi; ++r) {
                const int ly = y - r * step;
                const int wy = blend_w1(ly, size, margin, t, r == 0, r == n_rows - 1, blend);
                if (!wy) continue;
                Acc row = 0;
                for (int q = c_lo; q <= c_hi; ++q) {
                    const int lx = x - q * step;
                    const int wx = blend_w1(lx, size, margin, t, q == 0, q == n_cols - 1, blend);
                    if (!wx) continue;
                    const uint8_t* px = tiles + (first_tile + r * n_cols + q) * ensemble * member + ch * plane + (long)ly * size + lx;
                    unsigned members = 0;
                    for (int d = 0; d < ensemble; ++d) members += px[d * member];
                    row += (Acc)wx * members;
                }
                num += (Acc)wy * row;
            }
            for (int q = c_lo; q <= c_hi; ++q) sum_wx += blend_w1(x - q * step, size, margin, t, q == 0, q == n_cols - 1, blend);
            const Acc den = (Acc)ensemble * sum_wy * sum_wx;
            out[orow * out_w + x] = den ? (uint8_t)(num / den) : 0;
        }
    }
}

// ---- the self-ensemble of a batch of square items (predict_images' / test_metrics' ensemble; definitions: include/pssr_mi355.h)
// Plane p = (i * ensemble + d) * m + f of the output is T_d of plane i * m + f of the input: one output plane per blockIdx.y step, its
// 32 x 32 blocks over blockIdx.x
template <typename In>
__global__ void __launch_bounds__(256) dihedral_batch_kernel(const In* __restrict__ in, float* __restrict__ out, long planes, int m, int size,
                                                             int ensemble) {
    __shared__ float lds[32][33];
    const int nb = (size + 31) / 32;
    const long plane = (long)size * size;
    for (long p = blockIdx.y; p < planes; p += gridDim.y) {
        const long item = p / m;
        const dihedral_map mp = dihedral((int)(item % ensemble), false);
        const In* src = in + (item / ensemble * m + p % m) * plane;
        for (int b = blockIdx.x; b < nb * nb; b += gridDim.x)
            dihedral_block(out + p * plane, size, (b / nb) * 32, (b % nb) * 32, mp, lds, [&](int y, int x) { return (float)src[(long)y * size + x]; });
    }
}

// Plane p = i * c + ch of mean / spread from planes (i * ensemble + d) * c + ch of the input, d < ensemble, each fetched through U_d with
// clip_u8_kernel's value: a thread keeps the integer sum, minimum and maximum of its four pixels of the 32 x 32 output block over the
// members and stores once (shift = log2 ensemble; spread may be null)
__global__ void __launch_bounds__(256) ensemble_reduce_kernel(const float* __restrict__ in, uint8_t* __restrict__ mean, uint8_t* __restrict__ spread,
                                                              long planes, int c, int size, int ensemble, int shift) {
    __shared__ float lds[32][33];
    const int nb = (size + 31) / 32;
    const long plane = (long)size * size;
    for (long p = blockIdx.y; p < planes; p += gridDim.y) {
        const float* first = in + (p / c * ensemble * c + p % c) * plane;
        for (int b = blockIdx.x; b < nb * nb; b += gridDim.x) {
            const int r0 = (b / nb) * 32, c0 = (b % nb) * 32;
            int sum[4] = {0, 0, 0, 0}, lo[4] = {255, 255, 255, 255}, hi[4] = {0, 0, 0, 0};
            for (int d = 0; d < ensemble; ++d) {
                const float* src = first + (long)d * c * plane;
                float v[4];
                dihedral_gather(v, size, r0, c0, dihedral(d, true), lds,
                                [&](int y, int x) { return fminf(fmaxf(src[(long)y * size + x], 0.f), 255.f); });
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int q = (int)v[k];                        // the cast truncates toward zero
                    sum[k] += q;
                    lo[k] = q < lo[k] ? q : lo[k];
                    hi[k] = q > hi[k] ? q : hi[k];
                }
            }
            const uint8_t avg[4] = {(uint8_t)(sum[0] >> shift), (uint8_t)(sum[1] >> shift), (uint8_t)(sum[2] >> shift), (uint8_t)(sum[3] >> shift)};
            dihedral_store(mean + p * plane, size, r0, c0, avg);
            if (spread) {
                const uint8_t dif[4] = {(uint8_t)(hi[0] - lo[0]), (uint8_t)(hi[1] - lo[1]), (uint8_t)(hi[2] - lo[2]), (uint8_t)(hi[3] - lo[3])};
                dihedral_store(spread + p * plane, size, r0, c0, dif);
            }
        }
    }
}

// blend_stack_kernel's gather with the minimum and the maximum in place of the weighted sum: over every member of every tile that covers the
// pixel with a non-zero weight (blend_w1's support does not depend on the blend)
__global__ void __launch_bounds__(256) spread_stack_kernel(const uint8_t* __restrict__ tiles, uint8_t* __restrict__ out, long n_out_rows, int c,
                                                           int n_rows, int n_cols, int size, int overlap, int margin, int out_h, int out_w,
                                                           int ensemble) {
    const int step = size - overlap;
    const int per_slice = n_rows * n_cols;
    const long plane = (long)size * size, member = plane * c;
    for (long orow = blockIdx.y; orow < n_out_rows; orow += gridDim.y) {
        const int y = (int)(orow % out_h);
        const long sc = orow / out_h;                              // slice * c + channel
        const int ch = (int)(sc % c);
        const long first_tile = (sc / c) * per_slice;
        const int r_lo = y >= size ? (y - size) / step + 1 : 0;
        int r_hi = y / step; if (r_hi > n_rows - 1) r_hi = n_rows - 1;
        for (int x = blockIdx.x * 256 + threadIdx.x; x < out_w; x += gridDim.x * 256) {
            const int c_lo = x >= size ? (x - size) / step + 1 : 0;
            int c_hi = x / step; if (c_hi > n_cols - 1) c_hi = n_cols - 1;
            int lo = 255, hi = 0;
            for (int r = r_lo; r <= r_hi; ++r) {
                const int ly = y - r * step;
                if (!blend_w1(ly, size, margin, 1, r == 0, r == n_rows - 1, 0)) continue;
                for (int q = c_lo; q <= c_hi; ++q) {
                    const int lx = x - q * step;
                    if (!blend_w1(lx, size, margin, 1, q == 0, q == n_cols - 1, 0)) continue;
                    const uint8_t* px = tiles + (first_tile + r * n_cols + q) * ensemble * member + ch * plane + (long)ly * size + lx;
                    for (int d = 0; d < ensemble; ++d) {
                        const int v = px[d * member];
                        lo = v < lo ? v : lo;
                        hi = v > hi ? v : hi;
                    }
                }
            }
            out[orow * out_w + x] = hi >= lo ? (uint8_t)(hi - lo) : 0;
        }
    }
}

}  // namespace

extern "C" {

int pssr_sliding_tiles_u8(const uint8_t* sheet, float* tiles, int c, int h, int w, int size, int stride, int tile0, int ntile, pssr_stream_t s) {
    PSSR_CHECK(sheet && tiles && c > 0 && size > 0 && stride > 0 && h >= size && w >= size && ntile > 0 && tile0 >= 0, PSSR_ERR_ARG, "sliding_tiles: bad args");
    const int tiles_y = (h - size) / stride + 1, tiles_x = (w - size) / stride + 1;
    PSSR_CHECK(tile0 + ntile <= tiles_x * tiles_y, PSSR_ERR_ARG, "sliding_tiles: tile range %d+%d exceeds %d", tile0, ntile, tiles_x * tiles_y);
    hipLaunchKernelGGL(sliding_tiles_kernel, dim3(grid1d((long)ntile * c * size * size, 16384)), dim3(256), 0, (hipStream_t)s, sheet, tiles, c, h, w, size,
                       stride, tiles_x, tile0, ntile);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

int pssr_patch_tiles_u8(const uint8_t* tiles, uint8_t* sheet, int c, int n_rows, int n_cols, int size, int overlap, int margin, pssr_stream_t s) {
    PSSR_CHECK(tiles && sheet && c > 0 && n_rows > 0 && n_cols > 0 && size > 0, PSSR_ERR_ARG, "patch_tiles: bad args");
    PSSR_CHECK(overlap >= 0 && overlap < size && margin >= 0 && margin <= overlap && 2 * margin < size, PSSR_ERR_ARG,
               "patch_tiles: need 0 <= margin <= overlap < size (margin=%d overlap=%d size=%d)", margin, overlap, size);
    const int step = size - overlap;
    const long total = (long)c * (n_rows * step + overlap) * (n_cols * step + overlap);
    hipLaunchKernelGGL(patch_tiles_kernel, dim3(grid1d(total, 16384)), dim3(256), 0, (hipStream_t)s, tiles, sheet, c, n_rows, n_cols, size, overlap, margin);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

// the argument checks the two cutting entry points share; tiles tile0 .. tile0 + ntile - 1 of the slice-major order are touched
static int check_stack_args(const char* who, const void* stack, const void* tiles, int frames, int h, int w, int m, int frame_step, int size, int stride,
                            int tiles_y, int tiles_x, long tile0, long ntile) {
    PSSR_CHECK(stack && tiles, PSSR_ERR_ARG, "%s: null pointer", who);
    PSSR_CHECK(frames > 0 && h > 0 && w > 0 && m > 0 && frame_step > 0 && size > 0 && stride > 0 && tiles_y > 0 && tiles_x > 0 && ntile > 0 && tile0 >= 0,
               PSSR_ERR_ARG, "%s: sizes must be positive and tile0 >= 0 (frames=%d h=%d w=%d m=%d frame_step=%d size=%d stride=%d grid=%dx%d tile0=%ld ntile=%ld)",
               who, frames, h, w, m, frame_step, size, stride, tiles_y, tiles_x, tile0, ntile);
    const long per_slice = (long)tiles_y * tiles_x, last = tile0 + ntile - 1;
    const long ext_h = (long)(tiles_y - 1) * stride + size, ext_w = (long)(tiles_x - 1) * stride + size;
    PSSR_CHECK(per_slice <= INT_MAX && last < INT_MAX && ext_h <= INT_MAX / 2 && ext_w <= INT_MAX / 2 && (long)m * size <= INT_MAX / 2,
               PSSR_ERR_ARG, "%s: tile grid %dx%d, tile range %ld+%ld or extents exceed 32-bit indexing", who, tiles_y, tiles_x, tile0, ntile);
    const long k_last = last / per_slice;
    PSSR_CHECK(k_last * frame_step + m <= frames, PSSR_ERR_ARG, "%s: slice %ld (frames %ld..%ld) leaves the stack of %d frames", who, k_last,
               k_last * frame_step, k_last * frame_step + m - 1, frames);
    PSSR_CHECK(ext_h <= h || h >= 2, PSSR_ERR_ARG, "%s: the grid is %ld rows high but an axis of length %d cannot be reflected", who, ext_h, h);
    PSSR_CHECK(ext_w <= w || w >= 2, PSSR_ERR_ARG, "%s: the grid is %ld columns wide but an axis of length %d cannot be reflected", who, ext_w, w);
    return PSSR_OK;
}

// ... and the two stitching entry points
static int check_patch_args(const char* who, const void* tiles, const void* out, int n_slices, int c, int n_rows, int n_cols, int size, int overlap,
                            int margin, int out_h, int out_w) {
    PSSR_CHECK(tiles && out, PSSR_ERR_ARG, "%s: null pointer", who);
    PSSR_CHECK(n_slices > 0 && c > 0 && n_rows > 0 && n_cols > 0 && size > 0, PSSR_ERR_ARG, "%s: bad args", who);
    PSSR_CHECK(overlap >= 0 && overlap < size && margin >= 0 && margin <= overlap && 2 * margin < size, PSSR_ERR_ARG,
               "%s: need 0 <= margin <= overlap < size (margin=%d overlap=%d size=%d)", who, margin, overlap, size);
    const int step = size - overlap;
    const long full_h = (long)n_rows * step + overlap, full_w = (long)n_cols * step + overlap;
    PSSR_CHECK((long)n_rows * n_cols <= INT_MAX && full_h <= INT_MAX && full_w <= INT_MAX, PSSR_ERR_ARG, "%s: tile grid %dx%d exceeds 32-bit indexing",
               who, n_rows, n_cols);
    PSSR_CHECK(out_h >= 1 && out_h <= full_h && out_w >= 1 && out_w <= full_w, PSSR_ERR_ARG,
               "%s: crop %dx%d must lie within the stitched sheet of %ldx%ld", who, out_h, out_w, full_h, full_w);
    return PSSR_OK;
}

static bool ensemble_ok(int e) { return e == 1 || e == 2 || e == 4 || e == 8; }

int pssr_stack_tiles_u8(const uint8_t* stack, float* tiles, int frames, int h, int w, int m, int frame_step, int size, int stride, int tiles_y,
                        int tiles_x, int tile0, int ntile, pssr_stream_t s) {
    if (const int e = check_stack_args("stack_tiles", stack, tiles, frames, h, w, m, frame_step, size, stride, tiles_y, tiles_x, tile0, ntile)) return e;
    const int per_slice = tiles_y * tiles_x;
    const bool vec = size % 4 == 0 && (uintptr_t)tiles % 16 == 0;
    const int groups = vec ? size / 4 : size, gx = groups < 256 ? groups : 256, rows_per_pass = 256 / gx;
    const int bx = cdiv(m * size, rows_per_pass);
    const dim3 grid(bx < 1024 ? bx : 1024, ntile < 65535 ? ntile : 65535);
    if (vec)
        hipLaunchKernelGGL(stack_tiles_kernel<4>, grid, dim3(256), 0, (hipStream_t)s, stack, tiles, h, w, m, frame_step, size, stride, per_slice,
                           tiles_x, tile0, ntile);
    else
        hipLaunchKernelGGL(stack_tiles_kernel<1>, grid, dim3(256), 0, (hipStream_t)s, stack, tiles, h, w, m, frame_step, size, stride, per_slice,
                           tiles_x, tile0, ntile);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

int pssr_patch_stack_u8(const uint8_t* tiles, uint8_t* out, int n_slices, int c, int n_rows, int n_cols, int size, int overlap, int margin, int out_h,
                        int out_w, pssr_stream_t s) {
    if (const int e = check_patch_args("patch_stack", tiles, out, n_slices, c, n_rows, n_cols, size, overlap, margin, out_h, out_w)) return e;
    const long n_out_rows = (long)n_slices * c * out_h;
    const int bx = cdiv(out_w, 256);
    hipLaunchKernelGGL(patch_stack_kernel, dim3(bx < 1024 ? bx : 1024, (unsigned)(n_out_rows < 65535 ? n_out_rows : 65535)), dim3(256), 0, (hipStream_t)s, tiles,
                       out, n_out_rows, c, n_rows, n_cols, size, overlap, margin, out_h, out_w);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

int pssr_dihedral_tiles_u8(const uint8_t* stack, float* tiles, int frames, int h, int w, int m, int frame_step, int size, int stride, int tiles_y,
                           int tiles_x, int ensemble, int item0, int nitem, pssr_stream_t s) {
    PSSR_CHECK(ensemble_ok(ensemble), PSSR_ERR_ARG, "dihedral_tiles: ensemble must be 1, 2, 4 or 8 (got %d)", ensemble);
    PSSR_CHECK(item0 >= 0 && nitem > 0 && (long)item0 + nitem - 1 < INT_MAX, PSSR_ERR_ARG,
               "dihedral_tiles: item range %d+%d must be non-empty, start at item0 >= 0 and stay within 32-bit indexing", item0, nitem);
    const long tile0 = item0 / ensemble, tile_last = ((long)item0 + nitem - 1) / ensemble;
    if (const int e = check_stack_args("dihedral_tiles", stack, tiles, frames, h, w, m, frame_step, size, stride, tiles_y, tiles_x, tile0,
                                       tile_last - tile0 + 1))
        return e;
    const int nb = cdiv(size, 32);
    const long blocks = (long)m * nb * nb;
    PSSR_CHECK(blocks <= INT_MAX, PSSR_ERR_ARG, "dihedral_tiles: %d planes of %d pixels square exceed 32-bit indexing", m, size);
    hipLaunchKernelGGL(dihedral_tiles_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024), nitem < 65535 ? nitem : 65535), dim3(256), 0, (hipStream_t)s,
                       stack, tiles, h, w, m, frame_step, size, stride, tiles_y * tiles_x, tiles_x, ensemble, item0, nitem);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

int pssr_clip_u8_dihedral(const float* in, uint8_t* out, int nitem, int c, int size, int ensemble, int item0, pssr_stream_t s) {
    PSSR_CHECK(in && out, PSSR_ERR_ARG, "clip_u8_dihedral: null pointer");
    PSSR_CHECK(ensemble_ok(ensemble), PSSR_ERR_ARG, "clip_u8_dihedral: ensemble must be 1, 2, 4 or 8 (got %d)", ensemble);
    PSSR_CHECK(nitem > 0 && c > 0 && size > 0 && item0 >= 0 && size <= INT_MAX - 31, PSSR_ERR_ARG,
               "clip_u8_dihedral: sizes must be positive and item0 >= 0 (nitem=%d c=%d size=%d item0=%d)", nitem, c, size, item0);
    const long planes = (long)nitem * c, nb = cdiv(size, 32);
    PSSR_CHECK(nb * nb <= INT_MAX, PSSR_ERR_ARG, "clip_u8_dihedral: planes of %d pixels square exceed 32-bit indexing", size);
    hipLaunchKernelGGL(clip_u8_dihedral_kernel, dim3((unsigned)(nb * nb < 1024 ? nb * nb : 1024), (unsigned)(planes < 65535 ? planes : 65535)), dim3(256), 0,
                       (hipStream_t)s, in, out, planes, c, size, ensemble, item0 % ensemble);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

int pssr_blend_stack_u8(const uint8_t* tiles, uint8_t* out, int n_slices, int c, int n_rows, int n_cols, int size, int overlap, int margin, int out_h,
                        int out_w, int blend, int ensemble, pssr_stream_t s) {
    if (const int e = check_patch_args("blend_stack", tiles, out, n_slices, c, n_rows, n_cols, size, overlap, margin, out_h, out_w)) return e;
    PSSR_CHECK(blend == 0 || blend == 1, PSSR_ERR_ARG, "blend_stack: blend must be 0 (average) or 1 (linear) (got %d)", blend);
    PSSR_CHECK(ensemble_ok(ensemble), PSSR_ERR_ARG, "blend_stack: ensemble must be 1, 2, 4 or 8 (got %d)", ensemble);
    // at most `over` tiles cover a pixel on an axis, each with a weight of at most t (1 for the average): the numerator is at most
    // 255 * ensemble * (weight sum on y) * (weight sum on x)
    const int step = size - overlap, over = cdiv(size, step), t = blend ? (overlap > 2 * margin ? overlap - 2 * margin : 0) + 1 : 1;
    const unsigned __int128 sum_y = (unsigned __int128)(over < n_rows ? over : n_rows) * t, sum_x = (unsigned __int128)(over < n_cols ? over : n_cols) * t;
    const unsigned __int128 bound = sum_y * sum_x * 255 * ensemble;
    PSSR_CHECK(bound >> 64 == 0, PSSR_ERR_ARG, "blend_stack: the weighted sum of overlap=%d margin=%d size=%d may exceed 64 bits", overlap, margin, size);
    const long n_out_rows = (long)n_slices * c * out_h;
    const int bx = cdiv(out_w, 256);
    const dim3 grid(bx < 1024 ? bx : 1024, (unsigned)(n_out_rows < 65535 ? n_out_rows : 65535));
    if (bound >> 32 == 0)
        hipLaunchKernelGGL(blend_stack_kernel<uint32_t>, grid, dim3(256), 0, (hipStream_t)s, tiles, out, n_out_rows, c, n_rows, n_cols, size, overlap, margin,
                           out_h, out_w, blend, ensemble);
    else
        hipLaunchKernelGGL(blend_stack_kernel<uint64_t>, grid, dim3(256), 0, (hipStream_t)s, tiles, out, n_out_rows, c, n_rows, n_cols, size, overlap, margin,
                           out_h, out_w, blend, ensemble);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

// the checks pssr_dihedral_batch_* and pssr_ensemble_reduce_u8 share: `items` square planes-of-`ch` times `ensemble` members
static int check_ensemble_args(const char* who, bool pointers, int items, int ch, int size, int ensemble) {
    PSSR_CHECK(pointers, PSSR_ERR_ARG, "%s: null pointer", who);
    PSSR_CHECK(ensemble_ok(ensemble), PSSR_ERR_ARG, "%s: ensemble must be 1, 2, 4 or 8 (got %d)", who, ensemble);
    PSSR_CHECK(items > 0 && ch > 0 && size > 0, PSSR_ERR_ARG, "%s: sizes must be positive (n=%d planes per item=%d size=%d)", who, items, ch, size);
    const long nb = ((long)size + 31) / 32;
    PSSR_CHECK((long)items * ensemble <= INT_MAX && size <= INT_MAX - 31 && nb * nb <= INT_MAX, PSSR_ERR_ARG,
               "%s: %d items of %d members or planes of %d pixels square exceed 32-bit indexing", who, items, ensemble, size);
    return PSSR_OK;
}

extern "C++" template <typename In>
static int dihedral_batch(const char* who, const In* in, float* out, int n, int m, int size, int ensemble, pssr_stream_t s) {
    if (const int e = check_ensemble_args(who, in && out, n, m, size, ensemble)) return e;
    const long planes = (long)n * ensemble * m, nb = cdiv(size, 32);
    hipLaunchKernelGGL(dihedral_batch_kernel<In>, dim3((unsigned)(nb * nb < 1024 ? nb * nb : 1024), (unsigned)(planes < 65535 ? planes : 65535)), dim3(256), 0,
                       (hipStream_t)s, in, out, planes, m, size, ensemble);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

int pssr_dihedral_batch_u8(const uint8_t* in, float* out, int n, int m, int size, int ensemble, pssr_stream_t s) {
    return dihedral_batch("dihedral_batch_u8", in, out, n, m, size, ensemble, s);
}

int pssr_dihedral_batch_f32(const float* in, float* out, int n, int m, int size, int ensemble, pssr_stream_t s) {
    return dihedral_batch("dihedral_batch_f32", in, out, n, m, size, ensemble, s);
}

int pssr_ensemble_reduce_u8(const float* in, uint8_t* mean, uint8_t* spread, int n, int c, int size, int ensemble, pssr_stream_t s) {
    if (const int e = check_ensemble_args("ensemble_reduce", in && mean, n, c, size, ensemble)) return e;
    const long planes = (long)n * c, nb = cdiv(size, 32);
    const int shift = ensemble == 8 ? 3 : ensemble >> 1;
    hipLaunchKernelGGL(ensemble_reduce_kernel, dim3((unsigned)(nb * nb < 1024 ? nb * nb : 1024), (unsigned)(planes < 65535 ? planes : 65535)), dim3(256), 0,
                       (hipStream_t)s, in, mean, spread, planes, c, size, ensemble, shift);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

int pssr_spread_stack_u8(const uint8_t* tiles, uint8_t* out, int n_slices, int c, int n_rows, int n_cols, int size, int overlap, int margin, int out_h,
                         int out_w, int ensemble, pssr_stream_t s) {
    if (const int e = check_patch_args("spread_stack", tiles, out, n_slices, c, n_rows, n_cols, size, overlap, margin, out_h, out_w)) return e;
    PSSR_CHECK(ensemble_ok(ensemble), PSSR_ERR_ARG, "spread_stack: ensemble must be 1, 2, 4 or 8 (got %d)", ensemble);
    const long n_out_rows = (long)n_slices * c * out_h;
    const int bx = cdiv(out_w, 256);
    hipLaunchKernelGGL(spread_stack_kernel, dim3(bx < 1024 ? bx : 1024, (unsigned)(n_out_rows < 65535 ? n_out_rows : 65535)), dim3(256), 0, (hipStream_t)s,
                       tiles, out, n_out_rows, c, n_rows, n_cols, size, overlap, margin, out_h, out_w, ensemble);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

}  // extern "C"
