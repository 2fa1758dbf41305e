// The steps shared by the kernels that score a uint8 HR-side plane [s*h][s*w] against a uint8 LR-side plane [h][w] through Pillow's
// bilinear forward model: the fused reduction + moments and the map of consistency.hip, the shift search of register.hip, the blur search
// of rsf.hip.  The one
// copy of the argument checks of such a pair, of the grid sizing (workgroups per plane, a run of blocks of outputs per workgroup), of
// the staging of raw rows into LDS, of the workgroup sum and of the fold of the workgroups' partial rows.
#pragma once
#include "pil_taps.h"

namespace {   // internal linkage, as the kernels that use these

typedef unsigned long long u64;

// ---------------------------------------------------------------------------------------------- host: arguments and grids
constexpr int U8_PLANES_CAP = 1024;         // grid.y of every kernel over planes (planes beyond it: stride loop)
constexpr int U8_BLOCKS = 4096;             // workgroups a launch aims at (about two waves of 8 per CU)

// planes, LR size and scale of a pair that the entry points take: the sums are exact up to 2^28 pixels, indices are ints
inline bool u8_pair_ok(int planes, int h, int w, int s) {
    return planes > 0 && h > 0 && w > 0 && s >= 1 && s <= 16 && (long)h * s < (1L << 30) && (long)w * s < (1L << 30) && (long)h * w <= (1L << 28);
}
// ... with the message of the first check that fails, for the entry point `who`
inline int u8_pair_check(const char* who, int planes, int h, int w, int s) {
    PSSR_CHECK(planes > 0 && h > 0 && w > 0, PSSR_ERR_ARG, "%s: planes, h and w must be positive (%d, %d, %d)", who, planes, h, w);
    PSSR_CHECK(s >= 1 && s <= 16, PSSR_ERR_ARG, "%s: the scale must be an integer in 1 .. 16, given %d", who, s);
    PSSR_CHECK((long)h * w <= (1L << 28), PSSR_ERR_ARG, "%s: %ld pixels per LR plane (at most 2^28: the sums are exact up to there)", who, (long)h * w);
    PSSR_CHECK(u8_pair_ok(planes, h, w, s), PSSR_ERR_ARG, "%s: a %d x %d plane at scale %d has an axis of 2^30 or more", who, h, w, s);
    return PSSR_OK;
}

inline int planes_grid_y(int planes) { return planes < U8_PLANES_CAP ? planes : U8_PLANES_CAP; }
// workgroups per plane: enough to fill the part when there are few planes, never more than the plane has pieces of work or than `most`
inline int blocks_per_plane(int planes, long pieces, long most = U8_BLOCKS) {
    const int gy = planes_grid_y(planes);
    long want = (U8_BLOCKS + gy - 1) / gy;
    if (want > most) want = most;
    if (want > pieces) want = pieces;
    return (int)(want < 1 ? 1 : want);
}

// A workgroup walks a run of neighbouring blocks of outputs along x, [begin, end) of `tiles` dealt out in runs of tile_run(tiles, groups):
// the raw window of a block starts s/2 bytes before a 32 s-byte boundary, so its rows touch a cache line of each neighbour, which a run
// can find in this XCD's L2 (against blocks dealt out with a grid stride it measured the same at s = 4, where the reduction is not bound
// by HBM; the order costs nothing).  The last workgroups of a grid may be left without a block.
struct TileRun { int begin, end; };
__host__ __device__ inline int tile_run(int tiles, int groups) { return (tiles + groups - 1) / groups; }
__device__ __forceinline__ TileRun my_tile_run(int tiles) {
    const int run = tile_run(tiles, (int)gridDim.x);
    TileRun t;
    t.begin = (int)blockIdx.x * run;
    t.end = t.begin + run < tiles ? t.begin + run : tiles;
    return t;
}

// ---------------------------------------------------------------------------------------------- device: raw rows into LDS
// One round of the staging of `nrows` raw rows of `ncols` bytes of the buffer `src` of `total` bytes, by a workgroup of 256 threads.
// Row r starts at src[rowbase + (row0 + r) * W] and lands in lds[r * pitch ..] (16-byte aligned, pitch a multiple of 16) with its first
// byte at column (base15 + (row0 + r) * w15) & 15 -- base15 the low four bits of the address of src[rowbase], w15 = W & 15 -- so that
// the row arrives as whole aligned 16-byte pieces, pitch / 16 of them at most (pitch >= 15 + ncols rounded up).  A piece that straddles the
// buffer's first or last byte is put together from bytes; nothing outside [src, src + total) is read, bytes outside a row's ncols are
// whatever lies there (or zero).  Thread t takes the pieces piece0 + t + 256 i, i < PIECES, of the nrows * (pitch / 16): all their loads
// are issued first, then `meanwhile()` runs (work of the caller's that does not need the rows), then the LDS stores.  The caller
// synchronises.
template <int PIECES, class Meanwhile>
__device__ __forceinline__ void stage_rows_u8(const uint8_t* __restrict__ src, long total, long rowbase, int W, int base15, int w15, int row0, int nrows,
                                              int ncols, uint8_t* lds, int pitch, int piece0, Meanwhile&& meanwhile) {
    const int rq = pitch / 16;
    uint4 v[PIECES];
#pragma unroll
    for (int it = 0; it < PIECES; ++it) {
        const int idx = piece0 + (int)threadIdx.x + 256 * it, r = idx / rq, j = idx - r * rq;
        v[it] = make_uint4(0, 0, 0, 0);
        if (r < nrows) {
            const int shift = (base15 + (row0 + r) * w15) & 15;
            const long g = rowbase + (long)(row0 + r) * W - shift + 16 * j;       // an aligned piece; whole inside the buffer?
            if (16 * j < shift + ncols && g >= 0 && g + 16 <= total) v[it] = *reinterpret_cast<const uint4*>(src + g);
        }
    }
    meanwhile();
#pragma unroll
    for (int it = 0; it < PIECES; ++it) {
        const int idx = piece0 + (int)threadIdx.x + 256 * it, r = idx / rq, j = idx - r * rq;
        if (r < nrows) {
            const int shift = (base15 + (row0 + r) * w15) & 15;
            const long g = rowbase + (long)(row0 + r) * W - shift + 16 * j;
            if (16 * j < shift + ncols) {
                if (!(g >= 0 && g + 16 <= total)) {                               // the buffer's first or last piece: byte by byte
                    uint32_t p[4] = {0, 0, 0, 0};
                    for (int b = 0; b < 16; ++b)
                        if (g + b >= 0 && g + b < total) p[b >> 2] |= (uint32_t)src[g + b] << (8 * (b & 3));
                    v[it] = make_uint4(p[0], p[1], p[2], p[3]);
                }
                *reinterpret_cast<uint4*>(lds + r * pitch + 16 * j) = v[it];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- device: exact sums
// sum of v over the workgroup's 256 threads, valid in thread 0: fixed shuffle tree per wave, waves in order
__device__ __forceinline__ u64 block_sum_u64(u64 v, u64* red4) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
    __syncthreads();
    const u64 r = (red4[0] + red4[1]) + (red4[2] + red4[3]);
    __syncthreads();
    return r;
}

// An item's sums of one block of outputs into its three slots of the workgroup's partial row (the search kernels of register.hip and
// rsf.hip: an item is a shift or a candidate): the first block of a run writes them, the later ones add (a slot is written by one thread
// only, in program order).  The item "D = Lc" has no third slot.
__device__ __forceinline__ void slots_update(u64* slot, bool first, bool third, u64 sd, u64 sdd, u64 sdl) {
    if (first) {
        slot[0] = sd; slot[1] = sdd;
        if (third) slot[2] = sdl;
    } else {
        slot[0] += sd; slot[1] += sdd;
        if (third) slot[2] += sdl;
    }
}

// out[pl][q] = sum_row partial[pl][row][q], q < k: the second launch behind every kernel that leaves one row of 64-bit partial sums per
// workgroup and plane.  Grid (ceil(k / VALUES), planes up to the cap), block 256: a workgroup takes VALUES neighbouring values q of a
// plane and 256 / VALUES threads share the rows of each -- VALUES = 1 where k is small and the rows are thousands, 16 where k is in the
// thousands.  The sums wrap at 2^64, so the order of the additions does not change a bit.
template <int VALUES>
__global__ __launch_bounds__(256) void fold_u64_kernel(const u64* __restrict__ partial, u64* __restrict__ out, int planes, int rows, int k) {
    constexpr int SHARE = 256 / VALUES;                       // threads per value
    __shared__ u64 part[VALUES == 1 ? 4 : 256];
    const int ql = threadIdx.x % VALUES, rg = threadIdx.x / VALUES, q = blockIdx.x * VALUES + ql;
    for (int pl = blockIdx.y; pl < planes; pl += gridDim.y) {
        u64 sum = 0;
        if (q < k)
#pragma unroll 8
            for (int row = rg; row < rows; row += SHARE) sum += partial[((long)pl * rows + row) * k + q];
        if (VALUES == 1) {                                    // q < k: the grid has k workgroups per plane
            sum = block_sum_u64(sum, part);
            if (threadIdx.x == 0) out[(long)pl * k + q] = sum;
        } else {
            part[threadIdx.x] = sum;                          // [rg][ql]
            __syncthreads();
            if (rg == 0 && q < k) {
                u64 total = 0;
                for (int i = 0; i < SHARE; ++i) total += part[i * VALUES + ql];
                out[(long)pl * k + q] = total;
            }
            __syncthreads();
        }
    }
}
template <int VALUES>
inline void launch_fold_u64(const u64* partial, u64* out, int planes, int rows, int k, hipStream_t st) {
    hipLaunchKernelGGL(fold_u64_kernel<VALUES>, dim3(cdiv(k, VALUES), planes_grid_y(planes)), dim3(256), 0, st, partial, out, planes, rows, k);
}

}  // namespace
