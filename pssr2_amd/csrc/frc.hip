// Fourier ring correlation of two uint8 plane stacks (pssr2_amd.util.frc; include/pssr_mi355.h has the definitions).  Per plane the
// centred grid of n x n blocks (n even, 16 .. 1024, any such n: the transform is two matrix products against the caller's tables
// Ct, St [n][n] -- window times cosine / minus sine -- on the f32-input MFMA, not a radix-2 FFT), K = n / 2 + 1 kept spectrum columns,
// R = n / 2 rings.  Per block, three launches' worth of work:
//
// frc_rows_kernel, grid (tiles, blocks of the chunk), block 256 = 2 x 2 waves, each wave a 32 x 32 tile of the 64 (y) x 64 (kx) outputs:
//   T = a (Ct + i St)[:, 0 .. n/2] for both images, four real products  a Ct, a St, b Ct, b St  that share their operands.  Per stage of
//   32 x: the 64 x 32 bytes of both images go to LDS as floats (converted on the way; pitch 33 words, the A operand reads down a
//   column of it), the 32 x 64 pieces of both tables beside them (the B operand reads along a row).  The bytes are loaded one per
//   lane: a stage's row is 32 bytes at an arbitrary address, so stage_rows_u8's aligned 16-byte pieces would need a second, shifting
//   pass through LDS (a stage is 4 KB of bytes against 64 MFMAs per wave; what the byte loads cost was not measured).  16 k-steps
//   of v_mfma_f32_32x32x2_f32 x 4 accumulators per stage.  T goes to the workspace, [4][n][K] floats per block (a Ct, a St, b Ct, b St).
// frc_cols_kernel, the same grid shape over 64 (ky) x 64 (kx) tiles of the spectrum: F = (Ct + i St)^T T, with the tables as the A
//   operand (read along a row of the staged piece) and the four planes of T as B; eight MFMAs per k-step into the four accumulators
//   Re Fa, Im Fa, Re Fb, Im Fb (- St as an operand gives the minus of the real part).  The tile of F stays in registers: each lane
//   forms Re(Fa conj Fb), |Fa|^2, |Fb|^2 of its 16 coefficients in float32, doubled for the columns 0 < kx < n/2 that stand for
//   their mirror images too, and puts the three products into LDS (in place of the stages).  Then thread r owns ring r: in a spectrum row
//   the ring index is non-decreasing in kx, so the ring's coefficients of a row are one run kx in [lo, hi] that follows from
//   integer square roots, and the thread adds the runs of the tile's rows, in row order and kx order, in float64.  It writes the
//   three sums (zeros for a ring that misses the tile) into the tile's row of partial sums.
// frc_fold_kernel: sums[block][r][3] = the partial rows of the block's tiles added in tile order, one thread per value.
//
// Padding: tiles and stages past n or K are zeros in LDS (tables and images both), never reads past a block, a table or T.
// Determinism: every float32 product and every float64 sum has one fixed order; no atomics, no fence between workgroups.
// Blocks are worked off in chunks that keep T and the partial rows inside FRC_WS_BYTES of workspace.
//
// Decorrelation analysis (pssr2_amd.util.decorr; "Resolution of one image by decorrelation analysis" in include/pssr_mi355.h) is the same
// transform of one image with the block's mean taken off, so the three kernels are templates on NI, the images per block: NI = 2 is
// everything above, NI = 1 has half the products (two MFMAs per k-step in the row pass, four in the column pass, T [2][n][K]) and
// another epilogue: |F|^2 and |F| = sqrtf(|F|^2) of every coefficient in place of the three products, two sums per ring.  In front of
// it frc_block_means_kernel, one workgroup per block: the integer sum of the block's bytes (a fixed tree in LDS, exact in any order)
// and m = float(S / n^2), the quotient in double; the row pass stages float(a) - m, zeros past the block as before.
//
// Sectorial sums (pssr2_amd.util.frc_sectors / decorr_sectors; "Directional resolution" in include/pssr_mi355.h): the same two passes, and a
// column pass whose epilogue (SECT) bins each coefficient by (ring, sector), S <= 16 sectors of the direction of the frequency vector.
// The sector is the count c of the caller's S integer boundary vectors b_j (ascending in angle, strictly inside the upper half plane) with
// b_j x g >= 0 for the upper-half-plane representative g of the coefficient, taken mod S: the counted j are a prefix 0 .. c - 1, so thread r,
// which walks ring r's runs as before, keeps c as a pointer and moves it down while b_(c-1) x g < 0 and up while b_c x g >= 0 (a step or
// two per coefficient: neighbours in a ring are neighbours in angle).  The tile's partial row is [R + 1][S][NS]; a cell's chain lives in
// its slot there, which only thread r touches: the thread zeroes its S slots, keeps the sums of the sector it is in in registers, and on
// a change of sector stores them and loads the new cell's, so every cell stays one float64 chain in row order and kx order and S = 1
// gives the bits of the unsectored kernel.  The boundary vectors sit in 128 bytes of LDS beside the products.
#include "common.h"

namespace {

constexpr int FRC_MIN_N = 16, FRC_MAX_N = 1024;
constexpr int FRC_TILE = 64;                    // outputs a side per workgroup (2 x 2 waves of 32 x 32)
constexpr int FRC_KT = 32;                      // summation indices per LDS stage
constexpr int FRC_APITCH = FRC_KT + 1;          // words per staged image row: the A operand reads down a column
constexpr long FRC_WS_BYTES = 256L << 20;       // workspace a chunk of blocks aims to stay below
constexpr int FRC_MAX_CHUNK = 32768;            // grid.y
constexpr long FRC_MAX_BLOCKS = 1L << 24;       // blocks per call
constexpr int FRC_MAX_SECTORS = 16;

struct FrcGeom {
    int n, K, R, nby, nbx, oy, ox, ty, tk, tiles;     // ty, tk: 64-tiles along y (or ky) and along kx; both passes have ty * tk tiles
    long nblocks, per_block_bytes;
    int chunk;
};

inline bool frc_args_ok(int planes, int H, int W, int n) {
    if (!(planes > 0 && H > 0 && W > 0 && n >= FRC_MIN_N && n <= FRC_MAX_N && n % 2 == 0 && n <= H && n <= W)) return false;
    return (long)planes * (H / n) * (W / n) <= FRC_MAX_BLOCKS;
}

// ni: images per block (2: the pair of FRC; 1: decorrelation analysis, which keeps a float mean per block beside T); S: sectors per ring
// of the partial rows (1: the unsectored calls)
inline FrcGeom frc_geom(int planes, int H, int W, int n, int ni, int S = 1) {
    FrcGeom g;
    g.n = n; g.K = n / 2 + 1; g.R = n / 2;
    g.nby = H / n; g.nbx = W / n;
    g.oy = (H - g.nby * n) / 2; g.ox = (W - g.nbx * n) / 2;
    g.ty = cdiv(n, FRC_TILE); g.tk = cdiv(g.K, FRC_TILE);
    g.tiles = g.ty * g.tk;
    g.nblocks = (long)planes * g.nby * g.nbx;
    g.per_block_bytes = (long)g.tiles * (g.R + 1) * S * (ni + 1) * (long)sizeof(double) + 2L * ni * n * g.K * (long)sizeof(float) +
                        (ni == 1 ? (long)sizeof(float) : 0L);
    long chunk = FRC_WS_BYTES / g.per_block_bytes;
    if (chunk < 1) chunk = 1;
    if (chunk > FRC_MAX_CHUNK) chunk = FRC_MAX_CHUNK;
    if (chunk > g.nblocks) chunk = g.nblocks;
    g.chunk = (int)chunk;
    return g;
}

// floor(sqrt(v)), v >= 0 and below 2^24 (exact as a float); the two loops mend the last place of the float root
__device__ __forceinline__ int isqrt_i(int v) {
    int k = (int)__builtin_sqrtf((float)v);
    while (k * k > v) --k;
    while ((k + 1) * (k + 1) <= v) ++k;
    return k;
}

__device__ __forceinline__ f32x16 mma(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
// row of element `reg` of a lane's 32 x 32 accumulator (its column is lane & 31)
__device__ __forceinline__ int acc_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

// A 32 x 64 piece of a row-major float matrix [rows][pitch] into lds[32][64]: rows row0 .., columns col0 .., zeros past rows / cols.
__device__ __forceinline__ void stage_f32_32x64(const float* __restrict__ src, long pitch, int row0, int rows, int col0, int cols, float* lds) {
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int idx = (int)threadIdx.x + 256 * it, r = idx >> 6, c = idx & 63;
        float v = 0.f;
        if (row0 + r < rows && col0 + c < cols) v = src[(long)(row0 + r) * pitch + col0 + c];
        lds[idx] = v;
    }
}

// The origin of block g of the call (plane, then row and column of the grid of blocks) in its stack of planes.
__device__ __forceinline__ long block_origin(long g, int H, int W, int n, int nby, int nbx, int oy, int ox) {
    const int nb = nby * nbx, blk = (int)(g % nb);
    return (g / nb * H + oy + blk / nbx * n) * (long)W + ox + blk % nbx * n;
}

// mean[block of the chunk] = float(S / n^2), S the sum of the block's bytes: partial sums per thread, then a fixed tree in LDS.
__global__ __launch_bounds__(256) void frc_block_means_kernel(const uint8_t* __restrict__ a, float* __restrict__ mean, long block0, int H, int W,
                                                              int n, int nby, int nbx, int oy, int ox) {
    __shared__ unsigned part[256];
    const int tid = threadIdx.x;
    const long origin = block_origin(block0 + blockIdx.x, H, W, n, nby, nbx, oy, ox);
    unsigned s = 0;                                             // at most 2^20 x 255 in all
    for (int y = tid >> 5; y < n; y += 8)
        for (int x = tid & 31; x < n; x += 32) s += a[origin + (long)y * W + x];
    part[tid] = s;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if (tid < half) part[tid] += part[tid + half];
        __syncthreads();
    }
    if (tid == 0) mean[blockIdx.x] = (float)((double)part[0] / (double)(n * n));
}

template <int NI>
__global__ __launch_bounds__(256) void frc_rows_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, const float* __restrict__ mean,
                                                       const float* __restrict__ ct, const float* __restrict__ st, float* __restrict__ T, long block0,
                                                       int H, int W, int n, int nby, int nbx, int oy, int ox, int tk) {
    __shared__ float limg[NI * FRC_TILE * FRC_APITCH], lc[FRC_KT * FRC_TILE], ls[FRC_KT * FRC_TILE];
    const int K = n / 2 + 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wy = wave >> 1, wx = wave & 1;
    const int y0 = (int)blockIdx.x / tk * FRC_TILE, k0 = (int)blockIdx.x % tk * FRC_TILE;
    const long origin = block_origin(block0 + blockIdx.y, H, W, n, nby, nbx, oy, ox);
    float m = 0.f;
    if constexpr (NI == 1) m = mean[blockIdx.y];
    f32x16 acc[2 * NI] = {};                                    // a Ct, a St (, b Ct, b St)
    for (int x0 = 0; x0 < n; x0 += FRC_KT) {
        uint8_t v[NI][8];
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int idx = tid + 256 * it, r = idx >> 5, c = idx & 31;
#pragma unroll
            for (int i = 0; i < NI; ++i) v[i][it] = 0;
            if (y0 + r < n && x0 + c < n) {
                const long at = origin + (long)(y0 + r) * W + x0 + c;
                v[0][it] = a[at];
                if constexpr (NI == 2) v[1][it] = b[at];
            }
        }
        stage_f32_32x64(ct, n, x0, n, k0, K, lc);
        stage_f32_32x64(st, n, x0, n, k0, K, ls);
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int idx = tid + 256 * it, r = idx >> 5, c = idx & 31;
            if constexpr (NI == 2) {
                limg[r * FRC_APITCH + c] = (float)v[0][it];
                limg[FRC_TILE * FRC_APITCH + r * FRC_APITCH + c] = (float)v[1][it];
            } else {
                limg[r * FRC_APITCH + c] = y0 + r < n && x0 + c < n ? (float)v[0][it] - m : 0.f;    // zeros past the block, not -m
            }
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < FRC_KT / 2; ++kk) {
            const int k = 2 * kk + (lane >> 5);
            float p[NI];
#pragma unroll
            for (int i = 0; i < NI; ++i) p[i] = limg[i * FRC_TILE * FRC_APITCH + (32 * wy + (lane & 31)) * FRC_APITCH + k];
            const float c = lc[k * FRC_TILE + 32 * wx + (lane & 31)], s = ls[k * FRC_TILE + 32 * wx + (lane & 31)];
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                acc[2 * i] = mma(p[i], c, acc[2 * i]);
                acc[2 * i + 1] = mma(p[i], s, acc[2 * i + 1]);
            }
        }
        __syncthreads();
    }
    float* const out = T + (long)blockIdx.y * 2 * NI * n * K;
    const int kx = k0 + 32 * wx + (lane & 31);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int y = y0 + 32 * wy + acc_row(reg, lane);
        if (y < n && kx < K)
#pragma unroll
            for (int q = 0; q < 2 * NI; ++q) out[((long)q * n + y) * K + kx] = acc[q][reg];
    }
}

// SECT: the sectorial epilogue, partial rows [R + 1][S][NS], bx, by [S] the boundary vectors (S, bx, by unused without it)
template <int NI, bool SECT = false>
__global__ __launch_bounds__(256) void frc_cols_kernel(const float* __restrict__ T, const float* __restrict__ ct, const float* __restrict__ st,
                                                       double* __restrict__ partial, int n, int tk, int S, const int* __restrict__ bx,
                                                       const int* __restrict__ by) {
    // stages: the tables' pieces [2][32][64] and T's 2 NI planes [32][64]; afterwards the NS = NI + 1 values per coefficient [NS][64][64]
    constexpr int NS = NI + 1;
    __shared__ float lds[(2 + 2 * NI) * FRC_KT * FRC_TILE];
    __shared__ int lb[SECT ? 2 * FRC_MAX_SECTORS : 1];           // bx, then by
    static_assert((2 + 2 * NI) * FRC_KT * FRC_TILE >= NS * FRC_TILE * FRC_TILE, "the products take the place of the stages");
    const int K = n / 2 + 1, R = n / 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wy = wave >> 1, wx = wave & 1;
    const int ky0 = (int)blockIdx.x / tk * FRC_TILE, k0 = (int)blockIdx.x % tk * FRC_TILE;
    const float* const Tb = T + (long)blockIdx.y * 2 * NI * n * K;
    float* const lc = lds, * const ls = lds + FRC_KT * FRC_TILE, * const lt = lds + 2 * FRC_KT * FRC_TILE;
    f32x16 acc[2 * NI] = {};                                    // Re Fa, Im Fa (, Re Fb, Im Fb)
    for (int yy = 0; yy < n; yy += FRC_KT) {
        stage_f32_32x64(ct, n, yy, n, ky0, n, lc);
        stage_f32_32x64(st, n, yy, n, ky0, n, ls);
#pragma unroll
        for (int q = 0; q < 2 * NI; ++q) stage_f32_32x64(Tb + (long)q * n * K, K, yy, n, k0, K, lt + q * FRC_KT * FRC_TILE);
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < FRC_KT / 2; ++kk) {
            const int k = 2 * kk + (lane >> 5);
            const float c = lc[k * FRC_TILE + 32 * wy + (lane & 31)], s = ls[k * FRC_TILE + 32 * wy + (lane & 31)];
            const float* t = lt + k * FRC_TILE + 32 * wx + (lane & 31);
            float tr[NI], ti[NI];
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                tr[i] = t[2 * i * FRC_KT * FRC_TILE];
                ti[i] = t[(2 * i + 1) * FRC_KT * FRC_TILE];
            }
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                acc[2 * i] = mma(c, tr[i], acc[2 * i]);
                acc[2 * i + 1] = mma(c, ti[i], acc[2 * i + 1]);
            }
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                acc[2 * i] = mma(-s, ti[i], acc[2 * i]);
                acc[2 * i + 1] = mma(s, tr[i], acc[2 * i + 1]);
            }
        }
        __syncthreads();
    }
    // the NS values of every coefficient of the tile, weighted, into LDS [NS][64][64]
    {
        const int col = 32 * wx + (lane & 31), kx = k0 + col;
        const float wgt = kx > 0 && kx < R ? 2.f : 1.f;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int row = 32 * wy + acc_row(reg, lane);
            if constexpr (NI == 2) {
                const float far = acc[0][reg], fai = acc[1][reg], fbr = acc[2][reg], fbi = acc[3][reg];
                lds[row * FRC_TILE + col] = wgt * (far * fbr + fai * fbi);
                lds[(FRC_TILE + row) * FRC_TILE + col] = wgt * (far * far + fai * fai);
                lds[(2 * FRC_TILE + row) * FRC_TILE + col] = wgt * (fbr * fbr + fbi * fbi);
            } else {
                const float fr = acc[0][reg], fi = acc[1][reg];
                const float p = __builtin_fmaf(fr, fr, fi * fi);            // |F|^2, the expression of include/pssr_mi355.h
                lds[row * FRC_TILE + col] = wgt * __builtin_sqrtf(p);      // |F|
                lds[(FRC_TILE + row) * FRC_TILE + col] = wgt * p;
            }
        }
    }
    if constexpr (SECT) {
        if (tid < S) {
            lb[tid] = bx[tid];
            lb[FRC_MAX_SECTORS + tid] = by[tid];
        }
    }
    __syncthreads();
    // ring r of the tile: per spectrum row the run of kx with floor(sqrt(fy^2 + kx^2) + 1/2) == r, that is
    // r^2 - r + 1 <= fy^2 + kx^2 <= r^2 + r (ring 0: the origin alone), cut to the tile's valid columns
    const int klast = k0 + FRC_TILE - 1 < K - 1 ? k0 + FRC_TILE - 1 : K - 1;
    if constexpr (SECT) {
        double* const prow = partial + ((long)blockIdx.y * gridDim.x + blockIdx.x) * (R + 1) * S * NS;
        for (int r = tid; r <= R; r += 256) {
            double* const cells = prow + (long)r * S * NS;     // this thread's alone
            for (int i = 0; i < S * NS; ++i) cells[i] = 0.;
            double sum[NS] = {};
            int c = 0, cur = -1;                                // boundaries below the direction; the sector whose sums are in registers
            for (int row = 0; row < FRC_TILE && ky0 + row < n; ++row) {
                const int ky = ky0 + row, fy = ky <= R ? ky : ky - n, f2 = fy * fy;
                const int hi2 = r * r + r - f2, lo2 = (r > 0 ? r * r - r + 1 : 0) - f2;
                if (hi2 < 0) continue;
                int lo = lo2 <= 0 ? 0 : isqrt_i(lo2 - 1) + 1, hi = isqrt_i(hi2);
                if (lo < k0) lo = k0;
                if (hi > klast) hi = klast;
                const int gy = fy >= 0 ? fy : -fy;
                for (int kx = lo; kx <= hi; ++kx) {
                    const int gx = fy >= 0 ? kx : -kx;
                    while (c > 0 && lb[c - 1] * gy - lb[FRC_MAX_SECTORS + c - 1] * gx < 0) --c;
                    while (c < S && lb[c] * gy - lb[FRC_MAX_SECTORS + c] * gx >= 0) ++c;
                    const int sector = c == S ? 0 : c;
                    if (sector != cur) {
                        if (cur >= 0)
#pragma unroll
                            for (int q = 0; q < NS; ++q) cells[cur * NS + q] = sum[q];
#pragma unroll
                        for (int q = 0; q < NS; ++q) sum[q] = cells[sector * NS + q];
                        cur = sector;
                    }
                    const int at = row * FRC_TILE + kx - k0;
#pragma unroll
                    for (int q = 0; q < NS; ++q) sum[q] += (double)lds[q * FRC_TILE * FRC_TILE + at];
                }
            }
            if (cur >= 0)
#pragma unroll
                for (int q = 0; q < NS; ++q) cells[cur * NS + q] = sum[q];
        }
        return;
    }
    double* const prow = partial + ((long)blockIdx.y * gridDim.x + blockIdx.x) * (R + 1) * NS;
    for (int r = tid; r <= R; r += 256) {
        double sum[NS] = {};
        for (int row = 0; row < FRC_TILE && ky0 + row < n; ++row) {
            const int ky = ky0 + row, fy = ky <= R ? ky : ky - n, f2 = fy * fy;
            const int hi2 = r * r + r - f2, lo2 = (r > 0 ? r * r - r + 1 : 0) - f2;
            if (hi2 < 0) continue;
            int lo = lo2 <= 0 ? 0 : isqrt_i(lo2 - 1) + 1, hi = isqrt_i(hi2);
            if (lo < k0) lo = k0;
            if (hi > klast) hi = klast;
            for (int at = row * FRC_TILE + lo - k0; at <= row * FRC_TILE + hi - k0; ++at)
#pragma unroll
                for (int q = 0; q < NS; ++q) sum[q] += (double)lds[q * FRC_TILE * FRC_TILE + at];
        }
#pragma unroll
        for (int q = 0; q < NS; ++q) prow[NS * r + q] = sum[q];
    }
}

// sums[block][q] = the partial rows [block][tile][q] added in tile order, q < k
__global__ __launch_bounds__(256) void frc_fold_kernel(const double* __restrict__ partial, double* __restrict__ sums, long values, int tiles, int k) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < values; i += (long)gridDim.x * 256) {
        const long blk = i / k;
        const int q = (int)(i - blk * k);
        double s = 0.;
        for (int t = 0; t < tiles; ++t) s += partial[(blk * tiles + t) * k + q];
        sums[i] = s;
    }
}

// The launches of one call: per chunk of blocks (the means,) the row pass, the column pass and the fold.
template <int NI>
int frc_launch(const uint8_t* a, const uint8_t* b, const float* ct, const float* st, double* sums, int H, int W, const FrcGeom& g, void* workspace,
               pssr_stream_t stream, int S = 0, const int* bx = nullptr, const int* by = nullptr) {        // S = 0: the unsectored column pass
    const int k = (g.R + 1) * (S ? S : 1) * (NI + 1);
    double* const partial = (double*)workspace;
    float* const T = (float*)((char*)workspace + (long)g.chunk * g.tiles * k * (long)sizeof(double));
    float* const mean = T + (long)g.chunk * 2 * NI * g.n * g.K;          // NI == 1 only
    hipStream_t s = (hipStream_t)stream;
    for (long block0 = 0; block0 < g.nblocks; block0 += g.chunk) {
        const int count = (int)(g.nblocks - block0 < g.chunk ? g.nblocks - block0 : g.chunk);
        if (NI == 1) {
            hipLaunchKernelGGL(frc_block_means_kernel, dim3(count), dim3(256), 0, s, a, mean, block0, H, W, g.n, g.nby, g.nbx, g.oy, g.ox);
            PSSR_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(frc_rows_kernel<NI>, dim3(g.tiles, count), dim3(256), 0, s, a, b, (const float*)mean, ct, st, T, block0, H, W, g.n, g.nby,
                           g.nbx, g.oy, g.ox, g.tk);
        PSSR_LAUNCH_CHECK();
        if (S)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(frc_cols_kernel<NI, true>), dim3(g.tiles, count), dim3(256), 0, s, (const float*)T, ct, st, partial, g.n,
                               g.tk, S, bx, by);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(frc_cols_kernel<NI, false>), dim3(g.tiles, count), dim3(256), 0, s, (const float*)T, ct, st, partial, g.n,
                               g.tk, 0, (const int*)nullptr, (const int*)nullptr);
        PSSR_LAUNCH_CHECK();
        const long values = (long)count * k;
        hipLaunchKernelGGL(frc_fold_kernel, dim3(grid1d(values, 4096)), dim3(256), 0, s, (const double*)partial, sums + block0 * k, values, g.tiles, k);
        PSSR_LAUNCH_CHECK();
    }
    return PSSR_OK;
}

}  // namespace

extern "C" int64_t pssr_frc_workspace_bytes(int planes, int H, int W, int n) {
    if (!frc_args_ok(planes, H, W, n)) return 0;
    const FrcGeom g = frc_geom(planes, H, W, n, 2);
    return (int64_t)g.chunk * g.per_block_bytes;
}

extern "C" int pssr_frc_rings_u8(const uint8_t* a, const uint8_t* b, const float* ct, const float* st, double* sums, int planes, int H, int W, int n,
                                 void* workspace, pssr_stream_t stream) {
    PSSR_CHECK(a && b && ct && st && sums && workspace, PSSR_ERR_ARG, "frc_rings_u8: null pointer");
    PSSR_CHECK(planes > 0 && H > 0 && W > 0, PSSR_ERR_ARG, "frc_rings_u8: planes, H and W must be positive (%d, %d, %d)", planes, H, W);
    PSSR_CHECK(n >= FRC_MIN_N && n <= FRC_MAX_N && n % 2 == 0, PSSR_ERR_ARG, "frc_rings_u8: the block side must be even and in %d .. %d, given %d",
               FRC_MIN_N, FRC_MAX_N, n);
    PSSR_CHECK(n <= H && n <= W, PSSR_ERR_ARG, "frc_rings_u8: a block of %d does not fit a %d x %d plane", n, H, W);
    PSSR_CHECK(frc_args_ok(planes, H, W, n), PSSR_ERR_ARG, "frc_rings_u8: %ld blocks in all (at most 2^24 per call)", (long)planes * (H / n) * (W / n));
    return frc_launch<2>(a, b, ct, st, sums, H, W, frc_geom(planes, H, W, n, 2), workspace, stream);
}

extern "C" int64_t pssr_decorr_workspace_bytes(int planes, int H, int W, int n) {
    if (!frc_args_ok(planes, H, W, n)) return 0;
    const FrcGeom g = frc_geom(planes, H, W, n, 1);
    return (int64_t)g.chunk * g.per_block_bytes;
}

extern "C" int pssr_decorr_rings_u8(const uint8_t* a, const float* ct, const float* st, double* sums, int planes, int H, int W, int n, void* workspace,
                                    int64_t workspace_bytes, pssr_stream_t stream) {
    PSSR_CHECK(a && ct && st && sums && workspace, PSSR_ERR_ARG, "decorr_rings_u8: null pointer");
    PSSR_CHECK(planes > 0 && H > 0 && W > 0, PSSR_ERR_ARG, "decorr_rings_u8: planes, H and W must be positive (%d, %d, %d)", planes, H, W);
    PSSR_CHECK(n >= FRC_MIN_N && n <= FRC_MAX_N && n % 2 == 0, PSSR_ERR_ARG, "decorr_rings_u8: the block side must be even and in %d .. %d, given %d",
               FRC_MIN_N, FRC_MAX_N, n);
    PSSR_CHECK(n <= H && n <= W, PSSR_ERR_ARG, "decorr_rings_u8: a block of %d does not fit a %d x %d plane", n, H, W);
    PSSR_CHECK(frc_args_ok(planes, H, W, n), PSSR_ERR_ARG, "decorr_rings_u8: %ld blocks in all (at most 2^24 per call)", (long)planes * (H / n) * (W / n));
    const FrcGeom g = frc_geom(planes, H, W, n, 1);
    PSSR_CHECK(workspace_bytes >= (int64_t)g.chunk * g.per_block_bytes, PSSR_ERR_ARG, "decorr_rings_u8: a workspace of %ld bytes is short of the %ld needed",
               (long)workspace_bytes, (long)((int64_t)g.chunk * g.per_block_bytes));
    return frc_launch<1>(a, nullptr, ct, st, sums, H, W, g, workspace, stream);
}

// ---------------------------------------------------------------------------------------------- sectorial sums
namespace {

// The checks that the four sector entry points share; 0 or the error code.
int frc_sectors_check(const char* who, int planes, int H, int W, int n, int S) {
    PSSR_CHECK(planes > 0 && H > 0 && W > 0, PSSR_ERR_ARG, "%s: planes, H and W must be positive (%d, %d, %d)", who, planes, H, W);
    PSSR_CHECK(n >= FRC_MIN_N && n <= FRC_MAX_N && n % 2 == 0, PSSR_ERR_ARG, "%s: the block side must be even and in %d .. %d, given %d", who,
               FRC_MIN_N, FRC_MAX_N, n);
    PSSR_CHECK(n <= H && n <= W, PSSR_ERR_ARG, "%s: a block of %d does not fit a %d x %d plane", who, n, H, W);
    PSSR_CHECK(frc_args_ok(planes, H, W, n), PSSR_ERR_ARG, "%s: %ld blocks in all (at most 2^24 per call)", who, (long)planes * (H / n) * (W / n));
    PSSR_CHECK(S >= 1 && S <= FRC_MAX_SECTORS, PSSR_ERR_ARG, "%s: the sector count must be in 1 .. %d, given %d", who, FRC_MAX_SECTORS, S);
    return PSSR_OK;
}

}  // namespace

extern "C" int64_t pssr_frc_sectors_workspace_bytes(int planes, int H, int W, int n, int S) {
    if (!frc_args_ok(planes, H, W, n) || S < 1 || S > FRC_MAX_SECTORS) return 0;
    const FrcGeom g = frc_geom(planes, H, W, n, 2, S);
    return (int64_t)g.chunk * g.per_block_bytes;
}

extern "C" int pssr_frc_sectors_u8(const uint8_t* a, const uint8_t* b, const float* ct, const float* st, const int32_t* bx, const int32_t* by,
                                   double* sums, int planes, int H, int W, int n, int S, void* workspace, int64_t workspace_bytes,
                                   pssr_stream_t stream) {
    PSSR_CHECK(a && b && ct && st && sums && workspace, PSSR_ERR_ARG, "frc_sectors_u8: null pointer");
    PSSR_CHECK(bx && by, PSSR_ERR_ARG, "frc_sectors_u8: null boundary table");
    if (const int e = frc_sectors_check("frc_sectors_u8", planes, H, W, n, S)) return e;
    const FrcGeom g = frc_geom(planes, H, W, n, 2, S);
    PSSR_CHECK(workspace_bytes >= (int64_t)g.chunk * g.per_block_bytes, PSSR_ERR_ARG, "frc_sectors_u8: a workspace of %ld bytes is short of the %ld needed",
               (long)workspace_bytes, (long)((int64_t)g.chunk * g.per_block_bytes));
    return frc_launch<2>(a, b, ct, st, sums, H, W, g, workspace, stream, S, bx, by);
}

extern "C" int64_t pssr_decorr_sectors_workspace_bytes(int planes, int H, int W, int n, int S) {
    if (!frc_args_ok(planes, H, W, n) || S < 1 || S > FRC_MAX_SECTORS) return 0;
    const FrcGeom g = frc_geom(planes, H, W, n, 1, S);
    return (int64_t)g.chunk * g.per_block_bytes;
}

extern "C" int pssr_decorr_sectors_u8(const uint8_t* a, const float* ct, const float* st, const int32_t* bx, const int32_t* by, double* sums,
                                      int planes, int H, int W, int n, int S, void* workspace, int64_t workspace_bytes, pssr_stream_t stream) {
    PSSR_CHECK(a && ct && st && sums && workspace, PSSR_ERR_ARG, "decorr_sectors_u8: null pointer");
    PSSR_CHECK(bx && by, PSSR_ERR_ARG, "decorr_sectors_u8: null boundary table");
    if (const int e = frc_sectors_check("decorr_sectors_u8", planes, H, W, n, S)) return e;
    const FrcGeom g = frc_geom(planes, H, W, n, 1, S);
    PSSR_CHECK(workspace_bytes >= (int64_t)g.chunk * g.per_block_bytes, PSSR_ERR_ARG, "decorr_sectors_u8: a workspace of %ld bytes is short of the %ld needed",
               (long)workspace_bytes, (long)((int64_t)g.chunk * g.per_block_bytes));
    return frc_launch<1>(a, nullptr, ct, st, sums, H, W, g, workspace, stream, S, bx, by);
}
