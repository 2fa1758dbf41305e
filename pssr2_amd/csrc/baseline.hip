// The model-free rows of a super-resolution table, on uint8 planes (pssr2_amd.util.upsample / nlm_denoise, pssr2_amd.baselines.Baseline;
// include/pssr_mi355.h has the definitions B1 and B2).
//
// nlm_u8_kernel<P> (B2), grid (tiles, planes up to the cap), block 256 = one output pixel per thread of a 32 x 8 tile.
//   * The tile plus a halo of s + p pixels, every coordinate clamped into the plane, is staged once in LDS (T, at most 34 rows of 58
//     bytes); everything after it runs out of LDS and registers.
//   * ssd = sum a^2 + sum b^2 - 2 sum a b.  Both square sums come from one plane S in LDS, S[u][v] = the sum of the P x P squares of the
//     patch whose corner is T[u][v] (one entry per candidate centre of the tile, (8 + 2s) x (32 + 2s)).  sum a b comes from packed-byte dot
//     products: the thread keeps the P rows of its own patch as two dwords each (bytes beyond P are zero, which also masks whatever the
//     candidate's dwords hold there); per (dy, patch row) it reads the 9 aligned dwords of T that hold the bytes x - s - p .. x + s + p of
//     the candidate row, shifts them to its own byte phase (v_alignbyte_b32) and slides over them: candidate dx takes bytes
//     dx + s .. dx + s + 7 with two more v_alignbyte_b32 at compile-time phases and two v_dot4_u32_u8 (one for P = 3).  So a candidate costs
//     2 P dot products and 2 P byte alignments instead of P^2 subtract-multiply-adds, and an LDS dword is read once per 2s + 1 candidates.
//   * Then exactly B2's integers: q, the table, sum wgt v and sum wgt in uint32, one division per pixel.
//   * The 256 results go through LDS and leave as 16-byte pieces where the rows are whole aligned pieces, else as bytes.
//
// upsample_u8_kernel<FILTER> (B1), grid (tiles, planes up to the cap), block 256, a 64 x 64 tile of outputs.
//   * Prologue: 128 threads work out the integer taps (xmin, n <= 5, k[]) of the tile's 64 columns and 64 rows with pil_taps_f, in double
//     in Pillow's order, into LDS: 128 evaluations per 4096 outputs, none per pixel.
//   * The input window the taps name (at most 69 x 69 bytes) is staged in LDS; the x pass writes the uint8 intermediate [rows][64] to LDS
//     with Pillow's rounding and clipping; the y pass reads it 16 bytes per tap and writes 16 outputs per thread.  The intermediate
//     never goes to HBM.
// Integers only (but for the taps), no atomics, no workspace: the same bits on every run.
#include "u8_planes.h"

namespace {

// ---------------------------------------------------------------------------------------------- non-local means
constexpr int NLM_TW = 32, NLM_TH = 8;
constexpr int NLM_MAX_P = 3, NLM_MAX_S = 10, NLM_HALO = NLM_MAX_P + NLM_MAX_S;
constexpr int NLM_COLS = NLM_TW + 2 * NLM_HALO, NLM_ROWS = NLM_TH + 2 * NLM_HALO;      // 58 x 34
constexpr int NLM_PITCH = (NLM_COLS + 3) / 4 * 4;                                       // 60
constexpr int NLM_T_BYTES = NLM_ROWS * NLM_PITCH + 48;      // the 9 dwords of the last strip end 36 bytes behind their first
constexpr int NLM_SW = NLM_TW + 2 * NLM_MAX_S, NLM_SH = NLM_TH + 2 * NLM_MAX_S;        // 52 x 28 candidate centres
constexpr int NLM_NJ = 2 * NLM_MAX_S + 1;
static_assert(NLM_TW * NLM_TH == 256, "one output per thread");
static_assert(NLM_ROWS * NLM_PITCH < 2048, "the staged tile is under 2 KB");
static_assert(49ull * 255 * 255 < (1ull << 22), "ssd <= 49 * 255^2 < 2^22");
static_assert(49ull * 255 * 255 * 1023 < (1ull << 32), "ssd * qmul < 2^32");
static_assert(441ull * 16383 * 255 + 441ull * 16383 / 2 < (1ull << 32), "sum wgt v + (sum wgt >> 1) < 2^32");
static_assert((NLM_ROWS - 1) * NLM_PITCH + (NLM_TW - 1) / 4 * 4 + 36 <= NLM_T_BYTES, "the last strip stays inside T");

// LUT[q] = rint(16383 exp(-(q + 0.5) / 32)), LUT[255] = 0 (tests/test_baseline_host.py pins it to the formula)
#define PSSR_NLM_LUT_VALUES                                                                                             \
    16129, 15633, 15152, 14686, 14234, 13796, 13371, 12960, 12561, 12175, 11800, 11437, 11085, 10744, 10414, 10093,     \
    9783, 9482, 9190, 8907, 8633, 8368, 8110, 7861, 7619, 7384, 7157, 6937, 6724, 6517, 6316, 6122,                     \
    5934, 5751, 5574, 5403, 5236, 5075, 4919, 4768, 4621, 4479, 4341, 4208, 4078, 3953, 3831, 3713,                     \
    3599, 3488, 3381, 3277, 3176, 3078, 2984, 2892, 2803, 2717, 2633, 2552, 2473, 2397, 2324, 2252,                     \
    2183, 2116, 2051, 1987, 1926, 1867, 1810, 1754, 1700, 1648, 1597, 1548, 1500, 1454, 1409, 1366,                     \
    1324, 1283, 1244, 1205, 1168, 1132, 1098, 1064, 1031, 999, 969, 939, 910, 882, 855, 829,                            \
    803, 778, 754, 731, 709, 687, 666, 645, 625, 606, 587, 569, 552, 535, 518, 503,                                     \
    487, 472, 458, 443, 430, 417, 404, 391, 379, 368, 356, 345, 335, 324, 314, 305,                                     \
    295, 286, 278, 269, 261, 253, 245, 237, 230, 223, 216, 209, 203, 197, 191, 185,                                     \
    179, 174, 168, 163, 158, 153, 149, 144, 140, 135, 131, 127, 123, 119, 116, 112,                                     \
    109, 105, 102, 99, 96, 93, 90, 87, 85, 82, 80, 77, 75, 72, 70, 68,                                                  \
    66, 64, 62, 60, 58, 56, 55, 53, 51, 50, 48, 47, 45, 44, 43, 41,                                                     \
    40, 39, 38, 36, 35, 34, 33, 32, 31, 30, 29, 28, 27, 27, 26, 25,                                                     \
    24, 24, 23, 22, 21, 21, 20, 19, 19, 18, 18, 17, 17, 16, 16, 15,                                                     \
    15, 14, 14, 13, 13, 13, 12, 12, 11, 11, 11, 10, 10, 10, 9, 9,                                                       \
    9, 9, 8, 8, 8, 8, 7, 7, 7, 7, 7, 6, 6, 6, 6, 0
__device__ const uint16_t nlm_lut_dev[256] = {PSSR_NLM_LUT_VALUES};
const uint16_t nlm_lut_host[256] = {PSSR_NLM_LUT_VALUES};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// 16 bytes of an LDS row of results to out, or its bytes where the row is no whole aligned piece
template <int TW>
__device__ __forceinline__ void store_tile_u8(const uint8_t* res, uint8_t* __restrict__ out, long plane_out, int OW, int x0, int y0, int nx, int ny,
                                              bool wide) {
    const int tid = threadIdx.x;
    if (wide) {                                                 // OW and x0 are multiples of 16, out is aligned: nx is one too
        constexpr int PIECES = TW / 16;
        for (int i = tid; i < PIECES * ny; i += 256) {
            const int r = i / PIECES, c = (i - r * PIECES) * 16;
            if (c < nx) *reinterpret_cast<uint4*>(out + plane_out + (long)(y0 + r) * OW + x0 + c) = *reinterpret_cast<const uint4*>(res + r * TW + c);
        }
    } else {
        for (int i = tid; i < TW * ny; i += 256) {
            const int r = i / TW, c = i - r * TW;
            if (c < nx) out[plane_out + (long)(y0 + r) * OW + x0 + c] = res[r * TW + c];
        }
    }
}

template <int P>
__global__ __launch_bounds__(256) void nlm_u8_kernel(const uint8_t* __restrict__ x, uint8_t* __restrict__ out, int planes, int H, int W, int s,
                                                     uint32_t qmul, int qshift, uint32_t bias, int wide) {
    constexpr int PP = 2 * P + 1;
    __shared__ __attribute__((aligned(16))) uint32_t Tw[NLM_T_BYTES / 4];
    __shared__ uint32_t S[NLM_SH * NLM_SW];
    __shared__ uint16_t lut[256];
    __shared__ __attribute__((aligned(16))) uint8_t res[256];
    uint8_t* T = reinterpret_cast<uint8_t*>(Tw);
    const int tid = threadIdx.x, lx = tid & (NLM_TW - 1), ly = tid / NLM_TW;
    const int hl = s + P, rows = NLM_TH + 2 * hl, cols = NLM_TW + 2 * hl, srows = NLM_TH + 2 * s, scols = NLM_TW + 2 * s;
    const int tiles_x = (W + NLM_TW - 1) / NLM_TW;
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    const int x0 = tx * NLM_TW, y0 = ty * NLM_TH;
    const int nx = W - x0 < NLM_TW ? W - x0 : NLM_TW, ny = H - y0 < NLM_TH ? H - y0 : NLM_TH;
    lut[tid] = nlm_lut_dev[tid];
    for (int pl = blockIdx.y; pl < planes; pl += gridDim.y) {
        const long plane = (long)pl * H * W;
        for (int i = tid; i < rows * cols; i += 256) {
            const int r = i / cols, c = i - r * cols;
            T[r * NLM_PITCH + c] = x[plane + (long)clampi(y0 - hl + r, 0, H - 1) * W + clampi(x0 - hl + c, 0, W - 1)];
        }
        __syncthreads();
        for (int i = tid; i < srows * scols; i += 256) {
            const int r = i / scols, c = i - r * scols;
            uint32_t sum = 0;
#pragma unroll
            for (int py = 0; py < PP; ++py)
#pragma unroll
                for (int px = 0; px < PP; ++px) {
                    const uint32_t v = T[(r + py) * NLM_PITCH + c + px];
                    sum += v * v;
                }
            S[r * NLM_SW + c] = sum;
        }
        // the thread's own patch: row py as bytes 0 .. 3 and 4 .. PP - 1, zero beyond
        uint32_t alo[PP], ahi[PP];
#pragma unroll
        for (int py = 0; py < PP; ++py) {
            uint32_t lo = 0, hi = 0;
#pragma unroll
            for (int px = 0; px < PP; ++px) {
                const uint32_t v = T[(ly + s + py) * NLM_PITCH + lx + s + px];
                if (px < 4) lo |= v << (8 * px); else hi |= v << (8 * (px - 4));
            }
            alo[py] = lo; ahi[py] = hi;
        }
        __syncthreads();
        const uint32_t sa = S[(ly + s) * NLM_SW + lx + s];
        const int gx = x0 + lx, gy = y0 + ly;
        const uint32_t al = (uint32_t)lx & 3u;
        uint32_t num = 0, den = 0;
        for (int jy = 0; jy <= 2 * s; ++jy) {
            uint32_t ab[NLM_NJ];
#pragma unroll
            for (int j = 0; j < NLM_NJ; ++j) ab[j] = 0;
#pragma unroll
            for (int py = 0; py < PP; ++py) {
                const uint32_t* src = Tw + (((ly + jy + py) * NLM_PITCH + lx) >> 2);
                uint32_t w[9], st[8];
#pragma unroll
                for (int i = 0; i < 9; ++i) w[i] = src[i];
#pragma unroll
                for (int i = 0; i < 8; ++i) st[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], al);      // byte 0 of st = column lx of the row
#pragma unroll
                for (int j = 0; j < NLM_NJ; ++j) {
                    if (j <= 2 * s) {
                        const uint32_t lo = (j & 3) ? __builtin_amdgcn_alignbyte(st[j / 4 + 1], st[j / 4], (uint32_t)(j & 3)) : st[j / 4];
                        ab[j] = __builtin_amdgcn_udot4(alo[py], lo, ab[j], false);
                        if (PP > 4) {
                            const uint32_t hi = (j & 3) ? __builtin_amdgcn_alignbyte(st[j / 4 + 2], st[j / 4 + 1], (uint32_t)(j & 3)) : st[j / 4 + 1];
                            ab[j] = __builtin_amdgcn_udot4(ahi[py], hi, ab[j], false);
                        }
                    }
                }
            }
            const int cy = gy + jy - s;
            const bool row_in = cy >= 0 && cy < H;
#pragma unroll
            for (int j = 0; j < NLM_NJ; ++j) {
                if (j <= 2 * s) {
                    const int cx = gx + j - s;
                    const uint32_t ssd = sa + S[(ly + jy) * NLM_SW + lx + j] - 2u * ab[j];
                    const uint32_t d = ssd > bias ? ssd - bias : 0u;
                    uint32_t q = (d * qmul) >> qshift;
                    q = q < 255u ? q : 255u;
                    const uint32_t wgt = (row_in && cx >= 0 && cx < W) ? lut[q] : 0u;
                    const uint32_t v = T[(ly + P + jy) * NLM_PITCH + lx + P + j];
                    num += wgt * v; den += wgt;
                }
            }
        }
        // a thread outside the plane has no centre candidate: den = 0, and it stores nothing
        res[tid] = den ? (uint8_t)((num + (den >> 1)) / den) : 0;
        __syncthreads();
        store_tile_u8<NLM_TW>(res, out, plane, W, x0, y0, nx, ny, wide != 0);
        __syncthreads();                                        // T, S and res are rewritten for the next plane
    }
}

// ---------------------------------------------------------------------------------------------- enlargement
constexpr int UP_T = 64;                    // outputs of a tile on each axis
constexpr int UP_MAXN = 5;                  // taps of an output: ceil(support) * 2 + 1 for bicubic
constexpr int UP_IN = UP_T + UP_MAXN;       // input rows / columns a tile can name (r = 1: 64 + 4, one to spare)
constexpr int UP_PITCH = 72;
static_assert(UP_IN <= UP_PITCH, "an input row fits its LDS row");

struct UpTap { int xmin, n, k[UP_MAXN]; };

template <int FILTER>
__global__ __launch_bounds__(256) void upsample_u8_kernel(const uint8_t* __restrict__ x, uint8_t* __restrict__ out, int planes, int h, int w, int r,
                                                          int wide) {
    __shared__ UpTap taps[2 * UP_T];                            // columns, then rows
    __shared__ uint8_t src[UP_IN * UP_PITCH];
    __shared__ __attribute__((aligned(16))) uint8_t mid[UP_IN * UP_T];
    __shared__ __attribute__((aligned(16))) uint8_t res[UP_T * UP_T];
    const int tid = threadIdx.x;
    const int OW = w * r, OH = h * r;
    const int tiles_x = (OW + UP_T - 1) / UP_T;
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    const int X0 = tx * UP_T, Y0 = ty * UP_T;
    const int nx = OW - X0 < UP_T ? OW - X0 : UP_T, ny = OH - Y0 < UP_T ? OH - Y0 : UP_T;
    if (tid < 2 * UP_T) {
        const bool col = tid < UP_T;
        const int i = col ? tid : tid - UP_T, n_out = col ? nx : ny;
        UpTap t;
        t.xmin = 0; t.n = 0;
#pragma unroll
        for (int k = 0; k < UP_MAXN; ++k) t.k[k] = 0;
        if (i < n_out) pil_taps_f<FILTER, UP_MAXN>((col ? X0 : Y0) + i, col ? w : h, col ? OW : OH, t.xmin, t.n, t.k);
        taps[tid] = t;
    }
    __syncthreads();
    // the input window: the first output's xmin to the last one's xmin + n (both grow with the index), never more than UP_IN
    const int ix0 = taps[0].xmin, iy0 = taps[UP_T].xmin;
    int ncols = taps[nx - 1].xmin + taps[nx - 1].n - ix0, nrows = taps[UP_T + ny - 1].xmin + taps[UP_T + ny - 1].n - iy0;
    ncols = clampi(ncols, 1, UP_IN < w - ix0 ? UP_IN : w - ix0);
    nrows = clampi(nrows, 1, UP_IN < h - iy0 ? UP_IN : h - iy0);
    const int cx = tid & (UP_T - 1), cq = tid / UP_T;           // x pass: column cx, rows cq, cq + 4, ...
    const UpTap tc = taps[cx];
    const int yr = tid >> 2, xs = (tid & 3) * 16;               // y pass: row yr, columns xs .. xs + 15
    const UpTap tr = taps[UP_T + yr];
    for (int pl = blockIdx.y; pl < planes; pl += gridDim.y) {
        const long plane_in = (long)pl * h * w, plane_out = (long)pl * OH * OW;
        for (int i = tid; i < nrows * ncols; i += 256) {
            const int rr = i / ncols, c = i - rr * ncols;
            src[rr * UP_PITCH + c] = x[plane_in + (long)(iy0 + rr) * w + ix0 + c];
        }
        __syncthreads();
        if (cx < nx) {
            const int c0 = clampi(tc.xmin - ix0, 0, ncols - 1);
            for (int rr = cq; rr < nrows; rr += 256 / UP_T) {
                int acc = 1 << (PRECISION_BITS - 1);
#pragma unroll
                for (int k = 0; k < UP_MAXN; ++k)
                    if (k < tc.n) acc += tc.k[k] * (int)src[rr * UP_PITCH + (c0 + k < ncols ? c0 + k : ncols - 1)];
                mid[rr * UP_T + cx] = clip8(acc);
            }
        }
        __syncthreads();
        if (yr < ny) {
            const int r0 = clampi(tr.xmin - iy0, 0, nrows - 1);
            int acc[16];
#pragma unroll
            for (int b = 0; b < 16; ++b) acc[b] = 1 << (PRECISION_BITS - 1);
#pragma unroll
            for (int k = 0; k < UP_MAXN; ++k)
                if (k < tr.n) {
                    const int rr = r0 + k < nrows ? r0 + k : nrows - 1;
                    const uint4 m = *reinterpret_cast<const uint4*>(mid + rr * UP_T + xs);
                    const uint32_t mw[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
                    for (int b = 0; b < 16; ++b) acc[b] += tr.k[k] * (int)((mw[b >> 2] >> (8 * (b & 3))) & 255u);
                }
            uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                // The clipped byte is made opaque before it is packed: left to itself the compiler fuses the shift, the clip and the
                // packing of two neighbours into v_ashr_pk_u8_i32, which writes 16 bits of its destination, into a register whose
                // upper half still holds the previous dword's byte 2 (seen on the device: byte 2 of dwords 1 .. 3 came out OR-ed).
                uint32_t c = clip8(acc[b]);
                asm volatile("" : "+v"(c));
                o[b >> 2] |= c << (8 * (b & 3));
            }
            *reinterpret_cast<uint4*>(res + yr * UP_T + xs) = make_uint4(o[0], o[1], o[2], o[3]);
        }
        __syncthreads();
        store_tile_u8<UP_T>(res, out, plane_out, OW, X0, Y0, nx, ny, wide != 0);
        __syncthreads();                                        // src, mid and res are rewritten for the next plane
    }
}

}  // namespace

extern "C" int pssr_nlm_lut(int32_t* table) {
    PSSR_CHECK(table, PSSR_ERR_ARG, "nlm_lut: null pointer");
    for (int q = 0; q < 256; ++q) table[q] = nlm_lut_host[q];
    return PSSR_OK;
}

extern "C" int pssr_nlm_u8(const uint8_t* x, uint8_t* out, int planes, int H, int W, int p, int s, int qmul, int qshift, int bias,
                           pssr_stream_t stream) {
    PSSR_CHECK(x && out, PSSR_ERR_ARG, "nlm_u8: null pointer");
    PSSR_CHECK(x != out, PSSR_ERR_ARG, "nlm_u8: in place is not supported (a pixel is read by its neighbours' workgroups)");
    PSSR_CHECK(planes > 0 && H > 0 && W > 0, PSSR_ERR_ARG, "nlm_u8: planes, H and W must be positive (%d, %d, %d)", planes, H, W);
    PSSR_CHECK(p >= 1 && p <= NLM_MAX_P, PSSR_ERR_ARG, "nlm_u8: the patch radius must be 1 .. %d, given %d", NLM_MAX_P, p);
    PSSR_CHECK(s >= 1 && s <= NLM_MAX_S, PSSR_ERR_ARG, "nlm_u8: the search radius must be 1 .. %d, given %d", NLM_MAX_S, s);
    PSSR_CHECK(qmul >= 1 && qmul <= 1023, PSSR_ERR_ARG, "nlm_u8: qmul must be 1 .. 1023, given %d", qmul);
    PSSR_CHECK(qshift >= 0 && qshift <= 31, PSSR_ERR_ARG, "nlm_u8: qshift must be 0 .. 31, given %d", qshift);
    PSSR_CHECK(bias >= 0, PSSR_ERR_ARG, "nlm_u8: bias must not be negative, given %d", bias);
    PSSR_CHECK((long)H * W <= (1L << 28), PSSR_ERR_ARG, "nlm_u8: %ld pixels per plane (at most 2^28)", (long)H * W);
    const dim3 grid(cdiv(W, NLM_TW) * cdiv(H, NLM_TH), planes_grid_y(planes));
    const int wide = W % 16 == 0 && (uintptr_t)out % 16 == 0;
    const hipStream_t st = (hipStream_t)stream;
    if (p == 1) hipLaunchKernelGGL(nlm_u8_kernel<1>, grid, dim3(256), 0, st, x, out, planes, H, W, s, (uint32_t)qmul, qshift, (uint32_t)bias, wide);
    else if (p == 2) hipLaunchKernelGGL(nlm_u8_kernel<2>, grid, dim3(256), 0, st, x, out, planes, H, W, s, (uint32_t)qmul, qshift, (uint32_t)bias, wide);
    else hipLaunchKernelGGL(nlm_u8_kernel<3>, grid, dim3(256), 0, st, x, out, planes, H, W, s, (uint32_t)qmul, qshift, (uint32_t)bias, wide);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

extern "C" int pssr_upsample_u8(const uint8_t* x, uint8_t* out, int planes, int h, int w, int r, int filter, pssr_stream_t stream) {
    PSSR_CHECK(x && out, PSSR_ERR_ARG, "upsample_u8: null pointer");
    PSSR_CHECK(x != out, PSSR_ERR_ARG, "upsample_u8: in place is not supported");
    PSSR_CHECK(planes > 0 && h > 0 && w > 0, PSSR_ERR_ARG, "upsample_u8: planes, h and w must be positive (%d, %d, %d)", planes, h, w);
    PSSR_CHECK(r >= 1 && r <= 8, PSSR_ERR_ARG, "upsample_u8: the scale must be an integer in 1 .. 8, given %d", r);
    PSSR_CHECK(filter == PIL_BILINEAR || filter == PIL_BICUBIC, PSSR_ERR_ARG, "upsample_u8: unknown filter %d (0 bilinear, 1 bicubic)", filter);
    PSSR_CHECK((long)h * w <= (1L << 28), PSSR_ERR_ARG, "upsample_u8: %ld pixels per plane (at most 2^28)", (long)h * w);
    PSSR_CHECK((long)h * r * w * r <= (1L << 28), PSSR_ERR_ARG, "upsample_u8: %ld output pixels per plane (at most 2^28)", (long)h * r * w * r);
    const dim3 grid(cdiv(w * r, UP_T) * cdiv(h * r, UP_T), planes_grid_y(planes));
    const int wide = (w * r) % 16 == 0 && (uintptr_t)out % 16 == 0;
    const hipStream_t st = (hipStream_t)stream;
    if (filter == PIL_BILINEAR) hipLaunchKernelGGL(upsample_u8_kernel<PIL_BILINEAR>, grid, dim3(256), 0, st, x, out, planes, h, w, r, wide);
    else hipLaunchKernelGGL(upsample_u8_kernel<PIL_BICUBIC>, grid, dim3(256), 0, st, x, out, planes, h, w, r, wide);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}
