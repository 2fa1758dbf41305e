// Consistency of a prediction with its own low-resolution input (pssr2_amd.util.consistency_map; include/pssr_mi355.h has the
// definitions).  Per plane pair Y [s*h][s*w] (uint8 prediction) and L [h][w] (uint8 LR input), s an integer in 1 .. 16:
//   D      = PIL.Image.resize(Y, (w, h), BILINEAR), bit for bit (the two-pass 22-bit fixed-point resampler of pil_taps.h),
//   sums   = { sum D, sum L, sum D^2, sum D L, sum L^2 } over the plane, exact unsigned 64-bit integers,
//   map    = min(255, (|256 L - P[D]| + 128) >> 8) with the host's fitted table P, sse = sum |256 L - P[D]|^2, exact.
//
// reduce_taps_kernel: the taps of every output column and row, once per call, into the workspace (w + h threads).  It is the only
// floating point here, and it is pil_taps -- Pillow's double arithmetic in Pillow's order.  One thread per output evaluating them for
// itself is what made pssr_bilinear_down_u8's horizontal pass slow (see the comment there).
//
// reduce_moments_kernel<MAXT> (MAXT >= 2 s: the longest tap window), grid (blocks, planes), block 256.  A workgroup owns 32 x 32
// outputs at a time.  For an integer ratio the window of output i is [i s - s/2, i s - s/2 + 2 s) clipped to the image, so a block
// reads at most 33 s rows x 33 s columns of Y: its own 32 s and a halo of s.  It
//   1. takes its column's taps into registers (thread t: column t & 31) and the 32 rows' taps into LDS,
//   2. stages Y in strips of raw rows -- about 22 KB of LDS: all 33 s rows of the block for s <= 4 -- with stage_rows_u8 of
//      u8_planes.h: whole aligned 16-byte pieces where the buffer has them (else bytes); a thread issues all its loads of a strip (and
//      of its four L bytes) before it waits, so that a workgroup has ~20 KB in flight (with one dword per lane and 16 rows per step
//      the kernel was latency-bound),
//   3. reduces every staged row horizontally into an LDS array [33 s][32] of bytes (clip8 between the passes, as Pillow),
//   4. runs the vertical pass on that array: a thread's four outputs (rows t >> 5, + 8, + 16, + 24) are stored to D, paired with
//      L and fed to 32-bit partial sums, which 64-bit accumulators take over after every block of outputs.
// Y comes from HBM about once (the halo is shared with the neighbours through L2); the [H][w] intermediate of the two-launch
// reduction never leaves LDS.  Windows are never assumed: the block's raw range is read from the tap table and clamped to the LDS
// arrays, taps beyond a window are zero.
//
// Determinism: integers only.  A wave's shuffle tree and the four waves' LDS sums (block_sum_u64) give one row of 64-bit partials per
// workgroup and plane in the workspace; fold_u64_kernel<1> (a second launch, one workgroup per value and plane) adds them.  No atomics,
// no fence, no floating-point sum: the same bits on every run, whatever the order.
//
// The argument checks of a plane pair, the workgroups per plane and their runs of blocks, the staging, the workgroup sum and the fold are
// u8_planes.h's, shared with register.hip.
//
// consistency_map_kernel: grid (blocks, planes), block 256, the plane's 256-entry table in LDS; 16 pixels per lane and step with
// 16-byte loads / stores where size and pointers allow, else one.  e < 2^18, so e^2 needs the 64-bit accumulator from the start.
#include "u8_planes.h"

namespace {

constexpr int RM_TILE = 32;                 // outputs per block and axis
constexpr int RM_RAW_BYTES = 22 * 1024;     // LDS for the raw rows staged per step
constexpr int RM_TAP_STRIDE = 2 + 32;       // ints per tap-table entry: xmin, n, k[32]
constexpr int CM_VEC = 16;

// entry i of `tab`: the taps of output i of an axis of `out_size` outputs reduced from `in_size` inputs
__global__ void reduce_taps_kernel(int* __restrict__ tab_x, int* __restrict__ tab_y, int W, int w, int H, int h) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= w + h) return;
    Taps t;
    if (i < w) pil_taps(i, W, w, t); else pil_taps(i - w, H, h, t);
    int* e = i < w ? tab_x + (long)i * RM_TAP_STRIDE : tab_y + (long)(i - w) * RM_TAP_STRIDE;
    const int n = t.n < 32 ? t.n : 32;
    e[0] = t.xmin; e[1] = n;
    for (int k = 0; k < 32; ++k) e[2 + k] = k < n ? t.k[k] : 0;
}

template <int MAXT>
__global__ __launch_bounds__(256) void reduce_moments_kernel(const uint8_t* __restrict__ y, const uint8_t* __restrict__ l, uint8_t* __restrict__ d,
                                                             u64* __restrict__ partial, const int* __restrict__ tab_x,
                                                             const int* __restrict__ tab_y, int planes, int h, int w, int H, int W,
                                                             int tiles_x, int tiles) {
    constexpr int SPAN = 33 * (MAXT / 2);                    // raw rows / columns a block of 32 outputs reads, at most
    constexpr int ROWB = (SPAN + 15 + MAXT + 15) / 16 * 16;  // + the alignment shift + a window of (zero) taps past the end
    constexpr int ROWQ = ROWB / 16;                          // 16-byte pieces per staged row
    constexpr int NDW = (MAXT + 3) / 4;                      // dwords of a tap window (one more is read for the byte shift)
    // raw rows staged per step: the whole block's rows when about 22 KB of LDS hold them (s <= 4), else as many as do, in eights
    constexpr int STRIP = (SPAN + 7) / 8 * 8 < RM_RAW_BYTES / ROWB / 8 * 8 ? (SPAN + 7) / 8 * 8 : RM_RAW_BYTES / ROWB / 8 * 8;
    constexpr int ITERS = (STRIP * ROWQ + 255) / 256;        // pieces per thread and step: all their loads are in flight together
    __shared__ __attribute__((aligned(16))) uint8_t raw[STRIP][ROWB];
    __shared__ uint8_t hbuf[SPAN + MAXT][RM_TILE];
    __shared__ int ky[RM_TILE][MAXT];
    __shared__ int yoff_s[RM_TILE];
    __shared__ u64 red4[4];
    const int tid = threadIdx.x, c = tid & 31, rg = tid >> 5;
    const long plane_in = (long)H * W, total = (long)planes * plane_in;
    const uintptr_t ybase = (uintptr_t)y;
    for (int pl = blockIdx.y; pl < planes; pl += gridDim.y) {
        u64 acc[5] = {0, 0, 0, 0, 0};
        const TileRun mine = my_tile_run(tiles);
        for (int tile = mine.begin; tile < mine.end; ++tile) {
            const int ty0 = tile / tiles_x * RM_TILE, tx0 = tile % tiles_x * RM_TILE;
            const int ncol = w - tx0 < RM_TILE ? w - tx0 : RM_TILE, nrow = h - ty0 < RM_TILE ? h - ty0 : RM_TILE;
            // the raw range of this block, from the table (never assumed), clamped to what the LDS arrays hold
            const int* ex = tab_x + (long)(tx0 + ncol - 1) * RM_TAP_STRIDE;
            const int* ey = tab_y + (long)(ty0 + nrow - 1) * RM_TAP_STRIDE;
            const int xlo = tab_x[(long)tx0 * RM_TAP_STRIDE], ylo = tab_y[(long)ty0 * RM_TAP_STRIDE];
            int xspan = ex[0] + ex[1] - xlo, yspan = ey[0] + ey[1] - ylo;
            xspan = xspan < SPAN ? (xspan > 1 ? xspan : 1) : SPAN;
            yspan = yspan < SPAN ? (yspan > 1 ? yspan : 1) : SPAN;
            int kx[MAXT], xoff = 0;
            {
                int xn = 0;
                const int* e = tab_x + (long)(tx0 + (c < ncol ? c : 0)) * RM_TAP_STRIDE;
                if (c < ncol) {
                    xoff = e[0] - xlo; xn = e[1] < MAXT ? e[1] : MAXT;
                    if (xoff < 0 || xoff > xspan) { xoff = 0; xn = 0; }
                    if (xoff + xn > xspan) xn = xspan - xoff;
                }
#pragma unroll
                for (int k = 0; k < MAXT; ++k) kx[k] = k < xn ? e[2 + k] : 0;
            }
            const long rowbase = (long)pl * plane_in + (long)ylo * W + xlo;            // the block's first raw byte
            const int base15 = (int)((ybase + (uintptr_t)rowbase) & 15), w15 = W & 15;
            // the block's own L bytes: asked for now, used after the vertical pass
            uint32_t lv[RM_TILE / 8];
#pragma unroll
            for (int q = 0; q < RM_TILE / 8; ++q) {
                const int ry = rg + 8 * q;
                lv[q] = ry < nrow && c < ncol ? l[((long)pl * h + ty0 + ry) * w + tx0 + c] : 0;
            }
            for (int y0 = 0; y0 < yspan; y0 += STRIP) {
                // the strip's raw rows, every piece of them in one round; the rows' taps go to LDS while the loads are in flight
                const int nstrip = yspan - y0 < STRIP ? yspan - y0 : STRIP;
                stage_rows_u8<ITERS>(y, total, rowbase, W, base15, w15, y0, nstrip, xspan, &raw[0][0], ROWB, 0, [&] {
                    if (y0 == 0 && tid < RM_TILE) {
                        int yoff = 0, yn = 0;
                        const int* e = tab_y + (long)(ty0 + (tid < nrow ? tid : 0)) * RM_TAP_STRIDE;
                        if (tid < nrow) {
                            yoff = e[0] - ylo; yn = e[1] < MAXT ? e[1] : MAXT;
                            if (yoff < 0 || yoff > yspan) { yoff = 0; yn = 0; }
                            if (yoff + yn > yspan) yn = yspan - yoff;
                        }
                        yoff_s[tid] = yoff;
                        for (int k = 0; k < MAXT; ++k) ky[tid][k] = k < yn ? e[2 + k] : 0;
                    }
                });
                __syncthreads();
                // read and multiply without a branch (a row beyond the strip's end is inside `raw`, its result is dropped), so that
                // several rows' LDS reads are in flight; 24-bit multiplies: a tap is at most 2^22, a byte 255
#pragma unroll 4
                for (int q = 0; q < STRIP / 8; ++q) {
                    const int r = rg + 8 * q;
                    const int shift = (base15 + (y0 + r) * w15) & 15;        // the low bits of the row's address
                    // the window starts at any byte: aligned dwords and v_alignbyte, since the compiler merges byte reads into
                    // unaligned ds_read_b64 (0.28 -> 0.21 ms on a 16384^2 plane at s = 4 without them)
                    const int b0 = shift + xoff;
                    const uint32_t* src = reinterpret_cast<const uint32_t*>(raw[r]) + (b0 >> 2);
                    uint32_t dw[NDW + 1];
#pragma unroll
                    for (int i = 0; i <= NDW; ++i) dw[i] = src[i];
                    int a = 1 << (PRECISION_BITS - 1);
#pragma unroll
                    for (int i = 0; i < NDW; ++i) {
                        const uint32_t four = __builtin_amdgcn_alignbyte(dw[i + 1], dw[i], (uint32_t)(b0 & 3));
#pragma unroll
                        for (int b = 0; b < 4; ++b)
                            if (4 * i + b < MAXT) a += __mul24((int)((four >> (8 * b)) & 0xffu), kx[4 * i + b]);
                    }
                    if (y0 + r < yspan) hbuf[y0 + r][c] = clip8(a);
                }
                __syncthreads();
            }
            uint32_t sd = 0, sl = 0, sdd = 0, sdl = 0, sll = 0;
#pragma unroll
            for (int q = 0; q < RM_TILE / 8; ++q) {
                // read and multiply without a branch (rows beyond the block have zero taps and offset 0): the four outputs' LDS reads
                // are in flight together; only the store and the sums are predicated
                const int ry = rg + 8 * q;
                const int yoff = yoff_s[ry];
                int a = 1 << (PRECISION_BITS - 1);
#pragma unroll
                for (int k = 0; k < MAXT; ++k) a += __mul24((int)hbuf[yoff + k][c], ky[ry][k]);
                if (ry < nrow && c < ncol) {
                    const uint32_t dv = clip8(a);
                    d[((long)pl * h + ty0 + ry) * w + tx0 + c] = (uint8_t)dv;
                    const uint32_t lq = lv[q];
                    sd += dv; sl += lq; sdd += dv * dv; sdl += dv * lq; sll += lq * lq;
                }
            }
            acc[0] += sd; acc[1] += sl; acc[2] += sdd; acc[3] += sdl; acc[4] += sll;
            __syncthreads();      // hbuf, ky and yoff_s are rewritten by the next block of outputs
        }
        for (int q = 0; q < 5; ++q) {
            const u64 s = block_sum_u64(acc[q], red4);
            if (tid == 0) partial[((long)pl * gridDim.x + blockIdx.x) * 5 + q] = s;
        }
    }
}

__device__ __forceinline__ uint32_t map_pixel(const int* P, uint32_t dv, uint32_t lv, u64& acc) {
    const int v = (int)(lv << 8) - P[dv];
    const uint32_t e = (uint32_t)(v < 0 ? -v : v);
    acc += (u64)e * e;
    const uint32_t m = (e + 128) >> 8;
    return m < 255 ? m : 255;
}

template <bool VEC>
__global__ __launch_bounds__(256) void consistency_map_kernel(const uint8_t* __restrict__ d, const uint8_t* __restrict__ l, const int* __restrict__ lut,
                                                              uint8_t* __restrict__ map, u64* __restrict__ partial, int planes, long n) {
    __shared__ int P[256];
    __shared__ u64 red4[4];
    const int tid = threadIdx.x;
    for (int pl = blockIdx.y; pl < planes; pl += gridDim.y) {
        __syncthreads();
        P[tid] = lut[(long)pl * 256 + tid];
        __syncthreads();
        const uint8_t* dp = d + (long)pl * n;
        const uint8_t* lp = l + (long)pl * n;
        uint8_t* mp = map + (long)pl * n;
        u64 acc = 0;
        if (VEC) {                                           // n % 16 == 0 and 16-byte aligned pointers: so is every plane
            for (long i = ((long)blockIdx.x * 256 + tid) * CM_VEC; i < n; i += (long)gridDim.x * 256 * CM_VEC) {
                const uint4 dq = *reinterpret_cast<const uint4*>(dp + i), lq = *reinterpret_cast<const uint4*>(lp + i);
                const uint32_t dw[4] = {dq.x, dq.y, dq.z, dq.w}, lw[4] = {lq.x, lq.y, lq.z, lq.w};
                uint32_t mw[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    mw[a] = 0;
#pragma unroll
                    for (int b = 0; b < 4; ++b) mw[a] |= map_pixel(P, (dw[a] >> (8 * b)) & 0xffu, (lw[a] >> (8 * b)) & 0xffu, acc) << (8 * b);
                }
                *reinterpret_cast<uint4*>(mp + i) = make_uint4(mw[0], mw[1], mw[2], mw[3]);
            }
        } else {
            for (long i = (long)blockIdx.x * 256 + tid; i < n; i += (long)gridDim.x * 256) mp[i] = (uint8_t)map_pixel(P, dp[i], lp[i], acc);
        }
        const u64 s = block_sum_u64(acc, red4);
        if (tid == 0) partial[(long)pl * gridDim.x + blockIdx.x] = s;
    }
}

long rm_tiles(int h, int w) { return (long)cdiv(h, RM_TILE) * cdiv(w, RM_TILE); }
long cm_pieces(long pixels) { return (pixels + 256 * CM_VEC - 1) / (256 * CM_VEC); }

}  // namespace

extern "C" int64_t pssr_reduce_moments_workspace_bytes(int planes, int h, int w, int s) {
    if (!u8_pair_ok(planes, h, w, s)) return 0;
    const int64_t part = (int64_t)planes * blocks_per_plane(planes, rm_tiles(h, w)) * 5 * (int64_t)sizeof(u64);
    return part + ((int64_t)w + h) * RM_TAP_STRIDE * (int64_t)sizeof(int);
}

extern "C" int pssr_reduce_moments_u8(const uint8_t* y, const uint8_t* l, uint8_t* d, uint64_t* sums, int planes, int h, int w, int s,
                                      void* workspace, pssr_stream_t stream) {
    PSSR_CHECK(y && l && d && sums && workspace, PSSR_ERR_ARG, "reduce_moments_u8: null pointer");
    if (const int status = u8_pair_check("reduce_moments_u8", planes, h, w, s)) return status;
    const int H = h * s, W = w * s;
    const long tiles = rm_tiles(h, w);
    const int gx = blocks_per_plane(planes, tiles), gy = planes_grid_y(planes);
    u64* partial = (u64*)workspace;
    int* tab_x = (int*)(partial + (long)planes * gx * 5);
    int* tab_y = tab_x + (long)w * RM_TAP_STRIDE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(reduce_taps_kernel, dim3(cdiv(w + h, 64)), dim3(64), 0, st, tab_x, tab_y, W, w, H, h);
    PSSR_LAUNCH_CHECK();
    const dim3 grid(gx, gy), block(256);
    const int tx = cdiv(w, RM_TILE);
#define RM_LAUNCH(T) hipLaunchKernelGGL(reduce_moments_kernel<T>, grid, block, 0, st, y, l, d, partial, (const int*)tab_x, (const int*)tab_y, planes, h, w, \
                                        H, W, tx, (int)tiles)
    if (s == 1) RM_LAUNCH(2);
    else if (s == 2) RM_LAUNCH(4);
    else if (s <= 4) RM_LAUNCH(8);
    else if (s <= 8) RM_LAUNCH(16);
    else RM_LAUNCH(32);
#undef RM_LAUNCH
    PSSR_LAUNCH_CHECK();
    launch_fold_u64<1>(partial, (u64*)sums, planes, gx, 5, st);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

extern "C" int64_t pssr_consistency_map_workspace_bytes(int planes, int64_t pixels) {
    if (planes <= 0 || pixels <= 0) return 0;
    return (int64_t)planes * blocks_per_plane(planes, cm_pieces((long)pixels)) * (int64_t)sizeof(u64);
}

extern "C" int pssr_consistency_map_u8(const uint8_t* d, const uint8_t* l, const int32_t* lut, uint8_t* map, uint64_t* sse, int planes, int64_t pixels,
                                       void* workspace, pssr_stream_t stream) {
    PSSR_CHECK(d && l && lut && map && sse && workspace, PSSR_ERR_ARG, "consistency_map_u8: null pointer");
    PSSR_CHECK(planes > 0 && pixels > 0, PSSR_ERR_ARG, "consistency_map_u8: planes and pixels must be positive (%d, %ld)", planes, (long)pixels);
    PSSR_CHECK(pixels <= (1L << 28), PSSR_ERR_ARG, "consistency_map_u8: %ld pixels per plane (at most 2^28: the squared-error sum is exact up to there)",
               (long)pixels);
    const int gx = blocks_per_plane(planes, cm_pieces((long)pixels)), gy = planes_grid_y(planes);
    const bool vec = pixels % CM_VEC == 0 && (uintptr_t)d % 16 == 0 && (uintptr_t)l % 16 == 0 && (uintptr_t)map % 16 == 0;
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(consistency_map_kernel<true>, dim3(gx, gy), dim3(256), 0, st, d, l, (const int*)lut, map, (u64*)workspace, planes, (long)pixels);
    else
        hipLaunchKernelGGL(consistency_map_kernel<false>, dim3(gx, gy), dim3(256), 0, st, d, l, (const int*)lut, map, (u64*)workspace, planes, (long)pixels);
    PSSR_LAUNCH_CHECK();
    launch_fold_u64<1>((const u64*)workspace, (u64*)sse, planes, gx, 1, st);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}
