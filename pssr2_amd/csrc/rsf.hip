// Estimate of the resolution-scaling function (RSF) between a sharp HR-side image and a measured LR-side one: an exhaustive search over
// K candidate blurs (pssr2_amd.util.estimate_rsf; include/pssr_mi355.h has the definitions).  Per plane pair Y [s*h][s*w] (uint8) and
// L [h][w] (uint8), s an integer in 1 .. 16, a radius R of 0 .. 32 HR pixels, a host-made table taps [K][NT], NT = 2 s + 2 R, of
// non-negative 22-bit fixed-point rows (Pillow's 2 s interior taps convolved with a Gaussian), a margin of m = 1 + ceil(R / s) LR pixels:
//   T_k[r][x] = clip8(2^21 + sum_j taps[k][j] Y[r][s (x + m) - s/2 - R + j])            (horizontal pass, stride s)
//   D_k[y][x] = clip8(2^21 + sum_j taps[k][j] T_k[s (y + m) - s/2 - R + j][x])          (vertical pass, stride s)
//   sums      = K triples (sum D_k, sum D_k^2, sum D_k Lc), then sum Lc, sum Lc^2, Lc = L[m : h - m, m : w - m]; exact 64-bit integers.
//
// rsf_kernel, grid (workgroups, planes), block 256, dynamic LDS.  A workgroup owns B x B outputs of the cropped LR grid at a time (B = 32,
// 28, .. 4, 2, 1: the largest whose arrays fit 60 KB of LDS, so that two or more workgroups share a CU).  It
//   1. stages the raw bytes of the block once -- (B-1) s + NT rows and columns -- with stage_rows_u8 of u8_planes.h (whole aligned 16-byte
//      pieces, four per thread in flight), and the block's Lc bytes, whose two sums it takes at once,
//   2. runs, for every candidate k, the horizontal pass into a strip of LDS, T_k [rows][B]: one work item per (raw row, output column),
//      neighbouring lanes read bytes s apart; only the rows that the vertical pass of this candidate reads, and only the taps between the
//      row's first and last non-zero column (found once per workgroup: a sigma of 1 does not pay for the taps of a sigma of 8),
//   3. runs the vertical pass out of the strip, one work item per output (neighbouring lanes read neighbouring bytes), and pairs D_k with
//      Lc in three 32-bit sums per thread (at most 1024 x 255^2 < 2^32 per block), which a fixed shuffle tree adds per wave.
//      Two strips: the horizontal pass of candidate k + 1 shares a barrier interval with the vertical pass of candidate k, so a
//      candidate costs one barrier.  The tap row is read with uniform addresses (scalar loads), never through LDS.
//   4. after the last candidate, thread k adds the four waves' parts of candidate k and adds them to the candidate's three 64-bit slots
//      of the workgroup's partial row in the workspace (slots_update: written by this thread only, in program order).
// Y comes from HBM about once for all K candidates (the halo is shared with the neighbours through L2); no intermediate leaves LDS.
// With REDUCE the same body runs for the one candidate sel[plane] and its epilogue stores D instead of summing it.
//
// Determinism: integers only; no atomics, no fence, no floating point.  fold_u64_kernel<16> (a second small launch) adds the workgroups'
// rows.  The argument checks of a plane pair, the grid sizing, the staging, the slots and the fold are u8_planes.h's, shared with
// consistency.hip and register.hip.
#include "u8_planes.h"

namespace {

constexpr int RF_MAX_R = 32, RF_MAX_K = 64;
constexpr int RF_LDS_BYTES = 60 * 1024;      // dynamic LDS a workgroup may take
constexpr long RF_PARTIAL_BYTES = 64L << 20; // partial rows a launch aims to stay below
constexpr int RF_STAGE = 4;                  // 16-byte pieces a thread has in flight

// the LDS arrays of a block of B x B outputs (bytes; all offsets multiples of 16)
struct RfLayout { int nt, rn, rp, tp, off_strip, strip, off_lc, bytes; };
__host__ __device__ inline RfLayout rf_layout(int B, int s, int R) {
    RfLayout g;
    g.nt = 2 * s + 2 * R;                          // taps of a row of the table
    g.rn = (B - 1) * s + g.nt;                     // raw rows / columns
    g.rp = (g.rn + 15 + 15) / 16 * 16;             // pitch of a raw row: + the alignment shift
    g.tp = (B + 3) / 4 * 4;                        // pitch of a strip
    g.off_strip = g.rn * g.rp;
    g.strip = (g.rn * g.tp + 15) / 16 * 16;        // one strip; there are two
    g.off_lc = g.off_strip + 2 * g.strip;
    g.bytes = g.off_lc + (B * B + 15) / 16 * 16;
    return g;
}
int rf_block(int s, int R) {
    for (int B = 32; B >= 4; B -= 4)
        if (rf_layout(B, s, R).bytes <= RF_LDS_BYTES) return B;
    return rf_layout(2, s, R).bytes <= RF_LDS_BYTES ? 2 : 1;
}
int rf_margin(int s, int R) { return 1 + (R + s - 1) / s; }

// sum over the wave's 64 lanes, valid in lane 0: a fixed shuffle tree
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

template <bool REDUCE>
__global__ __launch_bounds__(256) void rsf_kernel(const uint8_t* __restrict__ yin, const uint8_t* __restrict__ lr, const int* __restrict__ taps,
                                                  const int* __restrict__ sel, u64* __restrict__ partial, uint8_t* __restrict__ dout, int planes,
                                                  int h, int w, int s, int K, int R, int B, int tiles_x, int tiles) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ int span[RF_MAX_K];                          // first | last << 8 non-zero column of every row of the table
    __shared__ uint32_t parts[(RF_MAX_K + 1) * 4 * 3];      // [candidate, then "D = Lc"][wave][3]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = 1 + (R + s - 1) / s, hc = h - 2 * m, wc = w - 2 * m;
    const int k3 = 3 * K + 2;
    const RfLayout lay = rf_layout(B, s, R);
    const int NT = lay.nt, RP = lay.rp, TP = lay.tp;
    uint8_t* const raw = smem;                              // [rn][RP]
    uint8_t* const strips = smem + lay.off_strip;           // 2 x [rn][TP]
    uint8_t* const lc = smem + lay.off_lc;                  // [B][B]
    const int H = h * s, W = w * s;
    const long plane_in = (long)H * W, total = (long)planes * plane_in;
    const uintptr_t ybase = (uintptr_t)yin;
    if (tid < K) {
        int f = NT, last = -1;
        for (int j = 0; j < NT; ++j)
            if (taps[tid * NT + j] != 0) {
                if (f == NT) f = j;
                last = j;
            }
        span[tid] = last < 0 ? 1 : f | (last << 8);         // a row of zeros (not a table of the contract): an empty range, D = 0
    }
    __syncthreads();
    const TileRun mine = my_tile_run(tiles);
    for (int pl = blockIdx.y; pl < planes; pl += gridDim.y) {
        u64* const prow = REDUCE ? nullptr : partial + ((long)pl * gridDim.x + blockIdx.x) * k3;
        int kbegin = 0, kend = K;
        if (REDUCE) {
            kbegin = __builtin_amdgcn_readfirstlane(sel[pl]);
            kbegin = kbegin < 0 ? 0 : (kbegin > K - 1 ? K - 1 : kbegin);      // the caller's contract; no other row is read either way
            kend = kbegin + 1;
        } else if (mine.begin >= mine.end) {                // a workgroup without a block of outputs: its row is zero
            for (int i = tid; i < k3; i += 256) prow[i] = 0;
        }
        for (int tile = mine.begin; tile < mine.end; ++tile) {
            const int y0 = tile / tiles_x * B, x0 = tile % tiles_x * B;
            const int nrow = hc - y0 < B ? hc - y0 : B, ncol = wc - x0 < B ? wc - x0 : B;
            const int nout = nrow * ncol;
            const int rny = (nrow - 1) * s + NT, rnx = (ncol - 1) * s + NT;              // raw rows and columns
            const int yr = s * (y0 + m) - R - s / 2, xr = s * (x0 + m) - R - s / 2;      // the block's first raw row and column (>= 0 by m)
            const int step_r = 256 / ncol, step_x = 256 - step_r * ncol;                 // a thread's next work item: 256 further on
            const int r_first = tid / ncol, x_first = tid - r_first * ncol;
            // Lc of the block
            if (!REDUCE)
                for (int o = tid, yy = r_first, x = x_first; o < nout; o += 256) {
                    lc[yy * B + x] = lr[((long)pl * h + y0 + m + yy) * w + x0 + m + x];
                    yy += step_r; x += step_x;
                    if (x >= ncol) { x -= ncol; ++yy; }
                }
            // 1. the raw bytes, as aligned 16-byte pieces: row r lands at raw[r][0 ..] with its first byte at raw[r][shift_r]
            const long rowbase = (long)pl * plane_in + (long)yr * W + xr;
            const int base15 = (int)((ybase + (uintptr_t)rowbase) & 15), w15 = W & 15;
            for (int p0 = 0; p0 < rny * (RP / 16); p0 += 256 * RF_STAGE)
                stage_rows_u8<RF_STAGE>(yin, total, rowbase, W, base15, w15, 0, rny, rnx, raw, RP, p0, [] {});
            __syncthreads();
            // sum Lc, sum Lc^2: the item after the candidates
            if (!REDUCE) {
                uint32_t sl = 0, sll = 0;
                for (int o = tid, yy = r_first, x = x_first; o < nout; o += 256) {
                    const uint32_t v = lc[yy * B + x];
                    sl += v; sll += v * v;
                    yy += step_r; x += step_x;
                    if (x >= ncol) { x -= ncol; ++yy; }
                }
                sl = wave_sum_u32(sl); sll = wave_sum_u32(sll);
                if (lane == 0) { parts[(K * 4 + wave) * 3] = sl; parts[(K * 4 + wave) * 3 + 1] = sll; }
            }
            // 2. the horizontal pass of candidate k into `strip`: rows f .. (nrow - 1) s + last, the ones its vertical pass reads
            auto hpass = [&](int k, uint8_t* strip) {
                const int sp = __builtin_amdgcn_readfirstlane(span[k]);
                const int f = sp & 255, last = sp >> 8;
                const int* tk = taps + k * NT;
                const int items = last < f ? 0 : ((nrow - 1) * s + last - f + 1) * ncol;
                for (int o = tid, r = f + r_first, x = x_first; o < items; o += 256) {
                    const uint8_t* src = raw + r * RP + ((base15 + r * w15) & 15) + s * x;
                    int a = 1 << (PRECISION_BITS - 1);
#pragma unroll 4
                    for (int j = f; j <= last; ++j) a += __mul24((int)src[j], tk[j]);
                    strip[r * TP + x] = clip8(a);
                    r += step_r; x += step_x;
                    if (x >= ncol) { x -= ncol; ++r; }
                }
            };
            hpass(kbegin, strips);
            __syncthreads();
            for (int k = kbegin; k < kend; ++k) {
                const uint8_t* strip = strips + ((k - kbegin) & 1) * lay.strip;
                if (k + 1 < kend) hpass(k + 1, strips + ((k + 1 - kbegin) & 1) * lay.strip);
                // 3. the vertical pass of candidate k and its sums
                const int sp = __builtin_amdgcn_readfirstlane(span[k]);
                const int f = sp & 255, last = sp >> 8;
                const int* tk = taps + k * NT;
                uint32_t sd = 0, sdd = 0, sdl = 0;
                for (int o = tid, yy = r_first, x = x_first; o < nout; o += 256) {
                    const uint8_t* src = strip + s * yy * TP + x;
                    int a = 1 << (PRECISION_BITS - 1);
#pragma unroll 4
                    for (int j = f; j <= last; ++j) a += __mul24((int)src[j * TP], tk[j]);
                    const uint32_t dv = clip8(a);
                    if (REDUCE) {
                        dout[((long)pl * hc + y0 + yy) * wc + x0 + x] = (uint8_t)dv;
                    } else {
                        const uint32_t lv = lc[yy * B + x];
                        sd += dv; sdd += dv * dv; sdl += dv * lv;
                    }
                    yy += step_r; x += step_x;
                    if (x >= ncol) { x -= ncol; ++yy; }
                }
                if (!REDUCE) {
                    sd = wave_sum_u32(sd); sdd = wave_sum_u32(sdd); sdl = wave_sum_u32(sdl);
                    if (lane == 0) {
                        uint32_t* part = parts + (k * 4 + wave) * 3;
                        part[0] = sd; part[1] = sdd; part[2] = sdl;
                    }
                }
                __syncthreads();      // strip k is free for candidate k + 2; after the last candidate: `parts` is whole, the arrays are free
            }
            // 4. the four waves' parts of an item, in order, into its slots of this workgroup's row (written by this thread only)
            if (!REDUCE) {
                if (tid <= K) {
                    const uint32_t* part = parts + tid * 12;
                    const u64 a = ((u64)part[0] + part[3]) + ((u64)part[6] + part[9]);
                    const u64 b = ((u64)part[1] + part[4]) + ((u64)part[7] + part[10]);
                    const u64 c = ((u64)part[2] + part[5]) + ((u64)part[8] + part[11]);
                    slots_update(prow + 3 * tid, tile == mine.begin, tid < K, a, b, c);
                }
                __syncthreads();      // `parts` is rewritten by the next block of outputs
            }
        }
    }
}

bool rf_args_ok(int planes, int h, int w, int s, int K, int R) {
    if (!(u8_pair_ok(planes, h, w, s) && K >= 1 && K <= RF_MAX_K && R >= 0 && R <= RF_MAX_R)) return false;
    const int m = rf_margin(s, R);
    return h - 2 * m >= 1 && w - 2 * m >= 1;
}
// the checks of both entry points after the null pointers, with the message of the first that fails
int rf_check(const char* who, int planes, int h, int w, int s, int K, int R) {
    if (const int status = u8_pair_check(who, planes, h, w, s)) return status;
    PSSR_CHECK(K >= 1 && K <= RF_MAX_K, PSSR_ERR_ARG, "%s: 1 .. 64 candidates, given %d", who, K);
    PSSR_CHECK(R >= 0 && R <= RF_MAX_R, PSSR_ERR_ARG, "%s: the radius must be 0 .. 32 HR pixels, given %d", who, R);
    PSSR_CHECK(rf_args_ok(planes, h, w, s, K, R), PSSR_ERR_ARG,
               "%s: a %d x %d LR plane leaves nothing inside the margin of %d pixels (1 + ceil(radius / scale)) on every side", who, h, w, rf_margin(s, R));
    return PSSR_OK;
}

// workgroups per plane and what they walk
struct RfGrid { int gx, gy, B, tiles_x, tiles; };
RfGrid rf_grid(int planes, int h, int w, int s, int K, int R, bool reduce) {
    RfGrid g;
    const int m = rf_margin(s, R);
    g.B = rf_block(s, R);
    g.tiles_x = cdiv(w - 2 * m, g.B);
    g.tiles = cdiv(h - 2 * m, g.B) * g.tiles_x;
    g.gy = planes_grid_y(planes);
    const long row_bytes = (3L * K + 2) * (long)sizeof(u64);
    const int want = blocks_per_plane(planes, g.tiles, reduce ? U8_BLOCKS : RF_PARTIAL_BYTES / row_bytes / planes);
    g.gx = cdiv(g.tiles, tile_run(g.tiles, want));   // every workgroup has a block of outputs
    return g;
}

}  // namespace

extern "C" int pssr_rsf_block(int s, int radius) {
    return s >= 1 && s <= 16 && radius >= 0 && radius <= RF_MAX_R ? rf_block(s, radius) : 0;
}

extern "C" int64_t pssr_rsf_moments_workspace_bytes(int planes, int h, int w, int s, int K, int radius) {
    if (!rf_args_ok(planes, h, w, s, K, radius)) return 0;
    return (int64_t)planes * rf_grid(planes, h, w, s, K, radius, false).gx * (3 * K + 2) * (int64_t)sizeof(u64);
}

extern "C" int pssr_rsf_moments_u8(const uint8_t* y, const uint8_t* l, const int32_t* taps, uint64_t* sums, int planes, int h, int w, int s, int K,
                                   int radius, void* workspace, pssr_stream_t stream) {
    PSSR_CHECK(y && l && taps && sums && workspace, PSSR_ERR_ARG, "rsf_moments_u8: null pointer");
    if (const int status = rf_check("rsf_moments_u8", planes, h, w, s, K, radius)) return status;
    const RfGrid g = rf_grid(planes, h, w, s, K, radius, false);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rsf_kernel<false>, dim3(g.gx, g.gy), dim3(256), (size_t)rf_layout(g.B, s, radius).bytes, st, y, l, (const int*)taps,
                       (const int*)nullptr, (u64*)workspace, (uint8_t*)nullptr, planes, h, w, s, K, radius, g.B, g.tiles_x, g.tiles);
    PSSR_LAUNCH_CHECK();
    launch_fold_u64<16>((const u64*)workspace, (u64*)sums, planes, g.gx, 3 * K + 2, st);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

extern "C" int pssr_rsf_reduce_u8(const uint8_t* y, const int32_t* taps, const int32_t* sel, uint8_t* d, int planes, int h, int w, int s, int K,
                                  int radius, pssr_stream_t stream) {
    PSSR_CHECK(y && taps && sel && d, PSSR_ERR_ARG, "rsf_reduce_u8: null pointer");
    if (const int status = rf_check("rsf_reduce_u8", planes, h, w, s, K, radius)) return status;
    const RfGrid g = rf_grid(planes, h, w, s, K, radius, true);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rsf_kernel<true>, dim3(g.gx, g.gy), dim3(256), (size_t)rf_layout(g.B, s, radius).bytes, st, y, (const uint8_t*)nullptr,
                       (const int*)taps, (const int*)sel, (u64*)nullptr, d, planes, h, w, s, K, radius, g.B, g.tiles_x, g.tiles);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}
