// Registration of real LR / HR pairs by an exhaustive search over integer shifts (pssr2_amd.util.register_pairs; include/pssr_mi355.h
// has the definitions).  Per plane pair H [s*h][s*w] (uint8, the HR side) and L [h][w] (uint8, the LR side), s an integer in 1 .. 16, a
// radius R of 0 .. 32 HR pixels, T = (2R+1)^2 shifts t = (ty, tx), a margin of m = 1 + ceil(R / s) LR pixels:
//   D_t[y][x] = Pillow's two-pass BILINEAR reduction by s (the 2 s interior taps of pil_taps.h, clip8 after each pass) of H sampled at
//               HR origin (s (y + m) + ty, s (x + m) + tx), 0 <= y < h' = h - 2m, 0 <= x < w' = w - 2m,
//   sums      = T triples (sum D_t, sum D_t^2, sum D_t Lc), then sum Lc, sum Lc^2, Lc = L[m : h - m, m : w - m]; exact 64-bit integers.
//
// register_taps_kernel: the 2 s interior taps, once per call, into the workspace.  It is the only floating point here, and it is
// pil_taps -- Pillow's double arithmetic in Pillow's order -- for output 1 of 4 reduced from 4 s, an interior index.
//
// register_shifts_kernel, grid (workgroups, planes), block 256, dynamic LDS.  "Filter H densely at every HR position, then sample that map
// at stride s with offset t": a workgroup owns B x B outputs of the cropped LR grid at a time (B = 32 .. 4, the largest whose arrays
// fit 60 KB of LDS, so that two or more workgroups share a CU).  It
//   1. stages the raw HR bytes of the block -- (B-1) s + 2R + 2s rows and columns: the block, R on every side, the tap window -- with
//      stage_rows_u8 of u8_planes.h: whole aligned 16-byte pieces where the buffer has them (else bytes), four pieces per thread in
//      flight before the LDS stores, and the block's Lc bytes,
//   2. filters every staged row horizontally at every column position into `hbuf` (clip8), then `hbuf` vertically at every row position
//      into the dense image (clip8), which takes the place of the raw bytes: (B-1) s + 2R + 1 positions a side (filter_pass, twice),
//   3. gives each thread its own shifts (work item = shift; item T is "D = Lc" and yields sum Lc, sum Lc^2).  A thread walks the
//      block's outputs, four of a row per step with all their LDS reads issued together (one read per step was bound by the LDS
//      latency), reads dense[s y + ty + R][s x + tx + R] -- neighbouring lanes have neighbouring tx, so neighbouring bytes -- and
//      Lc[y][x .. x + 4) (one dword, an LDS broadcast), and keeps three 32-bit sums (at most 1024 x 255^2 < 2^32 per block).
//      An item is split over G threads, each with every G-th row of the block, G chosen on the host so that G (T + 1) fills whole
//      rounds of 256 threads (R = 8 at s = 4: 290 items, G = 5, 6 rounds of a fifth each instead of 2 whole ones).  The G x (T + 1) triples
//      go to LDS (in place of `hbuf`; G is 1 where they would not fit), and the thread of an item adds its G parts in order and
//      then adds them to the item's three 64-bit slots of the workgroup's partial row in the workspace (with G = 1 the item's only
//      thread does that itself).  No shuffle and no atomic anywhere.
// H comes from HBM about once (the halo is shared with the neighbours through L2); neither intermediate leaves LDS.
//
// Determinism: integers only.  A slot of the partial rows is written by one thread only, in program order (slots_update);
// fold_u64_kernel<16> (a second small launch: 16 values per workgroup, 16 threads share the rows of each) adds the rows.  No atomics, no
// fence, no floating-point sum: the same bits on every run.
//
// The argument checks of a plane pair, the workgroups per plane and their runs of blocks, the staging and the fold are u8_planes.h's,
// shared with consistency.hip.
//
// crop_shift_kernel: out[p] = in[p][y0 : y0 + ho, x0 : x0 + wo] with a per-plane origin table; 16 bytes per thread and step where the
// output rows are whole 16-byte pieces (the input piece as one, four or sixteen loads, by its address), else one byte.
#include "u8_planes.h"

namespace {

constexpr int RS_MAX_S = 16, RS_MAX_R = 32;
constexpr int RS_LDS_BYTES = 60 * 1024;     // dynamic LDS a workgroup may take
constexpr long RS_PARTIAL_BYTES = 64L << 20; // partial rows a launch aims to stay below (fewer workgroups at large radii)
constexpr int RS_MAX_SPLIT = 32;            // threads an item is split over at most (a block has at most 32 rows)
constexpr int RS_STAGE = 4;                 // 16-byte pieces a thread has in flight

// the LDS arrays of a block of B x B outputs (bytes; all offsets multiples of 16)
struct RsLayout { int rn, rp, dp, off_hbuf, off_lc, bytes; };
__host__ __device__ inline RsLayout rs_layout(int B, int s, int R) {
    RsLayout g;
    g.rn = (B - 1) * s + 2 * R + 2 * s;            // raw rows / columns
    g.rp = (g.rn + 15 + 15) / 16 * 16;             // pitch of a raw row: + the alignment shift
    g.dp = (g.rn + 3) / 4 * 4;                     // pitch of hbuf and of the dense image (<= rp: the dense image replaces the raw rows)
    g.off_hbuf = g.rn * g.rp;
    g.off_lc = g.off_hbuf + (g.rn * g.dp + 15) / 16 * 16;
    g.bytes = g.off_lc + (B * B + 15) / 16 * 16;
    return g;
}
int rs_block(int s, int R) {
    for (int B = 32; B > 1; B >>= 1)
        if (rs_layout(B, s, R).bytes <= RS_LDS_BYTES) return B;
    return 1;
}
int rs_margin(int s, int R) { return 1 + (R + s - 1) / s; }
// threads per item: the smallest G within 5 % of the fewest rounds of 256 threads per unit of work, ceil(G (T + 1) / 256) / G, among
// those whose G (T + 1) triples of 32-bit sums fit the LDS that `hbuf` leaves behind
int rs_split(int T, int B, const RsLayout& lay) {
    const int n = T + 1, room = (lay.off_lc - lay.off_hbuf) / 12;
    const int cap = B < RS_MAX_SPLIT ? B : RS_MAX_SPLIT;
    double best = (double)((n + 255) / 256);
    for (int g = 2; g <= cap && g * n <= room; ++g) {
        const double c = (double)((g * n + 255) / 256) / g;
        if (c < best) best = c;
    }
    for (int g = 1; g <= cap && (g == 1 || g * n <= room); ++g)
        if ((double)((g * n + 255) / 256) / g <= 1.05 * best) return g;
    return 1;
}

__global__ void register_taps_kernel(int* __restrict__ ks, int s) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    Taps t;
    pil_taps(1, 4 * s, 4, t);
    for (int k = 0; k < 2 * RS_MAX_S; ++k) ks[k] = k < t.n && k < 2 * s ? t.k[k] : 0;
}

// One pass of the `nt` taps `ks` at every position, a wave per row and a lane per column: dst[r][x] = clip8 of the taps on
// src[r][x + k * kstride], k < nt, for r < ny and x < nx.  Row r of `src` starts at column (base15 + r * w15) & 15 of its pitch: the raw
// rows as stage_rows_u8 leaves them, or 0, 0 for rows that start at column 0.
__device__ __forceinline__ void filter_pass(const uint8_t* src, int spitch, int base15, int w15, int kstride, uint8_t* dst, int dpitch, int ny, int nx,
                                            const int* ks, int nt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < ny; r += 4) {
        const uint8_t* row = src + r * spitch + ((base15 + r * w15) & 15);
        for (int x = lane; x < nx; x += 64) {
            int a = 1 << (PRECISION_BITS - 1);
            for (int k = 0; k < nt; ++k) a += __mul24((int)row[x + k * kstride], ks[k]);
            dst[r * dpitch + x] = clip8(a);
        }
    }
}

__global__ __launch_bounds__(256) void register_shifts_kernel(const uint8_t* __restrict__ hr, const uint8_t* __restrict__ lr, u64* __restrict__ partial,
                                                              const int* __restrict__ taps, int planes, int h, int w, int s, int R, int B,
                                                              int G, int tiles_x, int tiles) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ int ks[2 * RS_MAX_S];
    const int tid = threadIdx.x;
    const int m = 1 + (R + s - 1) / s, hc = h - 2 * m, wc = w - 2 * m;
    const int side = 2 * R + 1, T = side * side, nitems = T + 1, k3 = 3 * T + 2, nt = 2 * s;
    const int work = G * nitems;
    const RsLayout lay = rs_layout(B, s, R);
    const int RP = lay.rp, DP = lay.dp;
    uint8_t* const raw = smem;                      // [rn][RP], then the dense image [dn][DP]
    uint8_t* const hbuf = smem + lay.off_hbuf;      // [rn][DP]
    uint8_t* const lc = smem + lay.off_lc;          // [B][B]
    uint32_t* const parts = reinterpret_cast<uint32_t*>(hbuf);      // [G][T + 1][3] once hbuf is dead
    const int H = h * s, W = w * s;
    const long plane_in = (long)H * W, total = (long)planes * plane_in;
    const uintptr_t hbase = (uintptr_t)hr;
    if (tid < 2 * RS_MAX_S) ks[tid] = taps[tid];
    const TileRun mine = my_tile_run(tiles);
    for (int pl = blockIdx.y; pl < planes; pl += gridDim.y) {
        u64* const prow = partial + ((long)pl * gridDim.x + blockIdx.x) * k3;
        if (mine.begin >= mine.end)                 // a workgroup without a block of outputs: its row is zero
            for (int i = tid; i < k3; i += 256) prow[i] = 0;
        for (int tile = mine.begin; tile < mine.end; ++tile) {
            const int y0 = tile / tiles_x * B, x0 = tile % tiles_x * B;
            const int nrow = hc - y0 < B ? hc - y0 : B, ncol = wc - x0 < B ? wc - x0 : B;
            const int dny = (nrow - 1) * s + side, dnx = (ncol - 1) * s + side;          // dense positions
            const int rny = dny + nt - 1, rnx = dnx + nt - 1;                            // raw rows and columns
            const int yr = s * (y0 + m) - R - s / 2, xr = s * (x0 + m) - R - s / 2;      // the block's first raw row and column (>= 0 by m)
            // Lc of the block
            for (int o = tid; o < nrow * ncol; o += 256) {
                const int y = o / ncol, x = o - y * ncol;
                lc[y * B + x] = lr[((long)pl * h + y0 + m + y) * w + x0 + m + x];
            }
            // 1. the raw bytes, as aligned 16-byte pieces: row r lands at raw[r][0 ..] with its first byte at raw[r][shift_r]
            const long rowbase = (long)pl * plane_in + (long)yr * W + xr;
            const int base15 = (int)((hbase + (uintptr_t)rowbase) & 15), w15 = W & 15;
            for (int p0 = 0; p0 < rny * (RP / 16); p0 += 256 * RS_STAGE)
                stage_rows_u8<RS_STAGE>(hr, total, rowbase, W, base15, w15, 0, rny, rnx, raw, RP, p0, [] {});
            __syncthreads();
            // 2a. horizontal pass at every column position: hbuf[r][X] = the taps on raw[r][X .. X + 2s)
            filter_pass(raw, RP, base15, w15, 1, hbuf, DP, rny, dnx, ks, nt);
            __syncthreads();
            // 2b. vertical pass at every row position: dense[Y][X] = the taps on hbuf[Y .. Y + 2s)[X] (the raw bytes are dead)
            filter_pass(hbuf, DP, 0, 0, DP, raw, DP, dny, dnx, ks, nt);
            __syncthreads();
            // 3. the search: one work item per shift (and one for Lc itself), G threads per item with every G-th row each
            const bool first = tile == mine.begin;
            for (int wi = tid; wi < work; wi += 256) {
                const int g = wi / nitems, item = wi - g * nitems;
                const uint8_t* src = lc;
                int sx = 1, sy = B;
                if (item < T) {
                    const int ty = item / side, tx = item - ty * side;
                    src = raw + ty * DP + tx; sx = s; sy = s * DP;
                }
                uint32_t sd = 0, sdd = 0, sdl = 0;
                for (int y = g; y < nrow; y += G) {
                    const uint8_t* drow = src + y * sy;
                    const uint8_t* lrow = lc + y * B;           // 4-byte aligned: B is a multiple of 4 wherever a row has 4 outputs
                    int x = 0;
#pragma unroll 2
                    for (; x + 4 <= ncol; x += 4) {
                        const uint32_t l4 = *reinterpret_cast<const uint32_t*>(lrow + x);
                        const uint32_t d0 = drow[x * sx], d1 = drow[(x + 1) * sx], d2 = drow[(x + 2) * sx], d3 = drow[(x + 3) * sx];
                        const uint32_t l0 = l4 & 0xffu, l1 = (l4 >> 8) & 0xffu, l2 = (l4 >> 16) & 0xffu, l3 = l4 >> 24;
                        sd += (d0 + d1) + (d2 + d3);
                        sdd += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
                        sdl += (d0 * l0 + d1 * l1) + (d2 * l2 + d3 * l3);
                    }
                    for (; x < ncol; ++x) {
                        const uint32_t d = drow[x * sx], l = lrow[x];
                        sd += d; sdd += d * d; sdl += d * l;
                    }
                }
                if (G == 1) {                                   // the item's only thread: straight into its slots
                    slots_update(prow + 3 * item, first, item < T, sd, sdd, sdl);
                } else {
                    parts[3 * wi] = sd; parts[3 * wi + 1] = sdd; parts[3 * wi + 2] = sdl;
                }
            }
            if (G > 1) {
                __syncthreads();
                // an item's G parts, in order, into its three slots of this workgroup's row (written by this thread only)
                for (int item = tid; item < nitems; item += 256) {
                    u64 a = 0, b = 0, c = 0;
                    for (int g = 0; g < G; ++g) {
                        const uint32_t* part = parts + 3 * (g * nitems + item);
                        a += part[0]; b += part[1]; c += part[2];
                    }
                    slots_update(prow + 3 * item, first, item < T, a, b, c);
                }
            }
            __syncthreads();      // the LDS arrays are rewritten by the next block of outputs (`parts` by its horizontal pass)
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void crop_shift_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const int* __restrict__ origins,
                                                         int planes, int H, int W, int ho, int wo) {
    for (int pl = blockIdx.y; pl < planes; pl += gridDim.y) {
        int y0 = origins[2 * pl], x0 = origins[2 * pl + 1];
        y0 = y0 < 0 ? 0 : (y0 > H - ho ? H - ho : y0);          // the caller's contract; nothing is read outside the plane either way
        x0 = x0 < 0 ? 0 : (x0 > W - wo ? W - wo : x0);
        const uint8_t* src = in + (long)pl * H * W + (long)y0 * W + x0;
        uint8_t* dst = out + (long)pl * ho * wo;
        if (VEC) {                                               // wo % 16 == 0 and a 16-byte aligned `out`: so is every output piece
            const int q = wo / 16;
            const long n = (long)ho * q;
            for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
                const long y = i / q;
                const int j = (int)(i - y * q);
                const uint8_t* p = src + y * W + 16 * j;
                uint4 v;
                if (((uintptr_t)p & 15) == 0) {
                    v = *reinterpret_cast<const uint4*>(p);
                } else if (((uintptr_t)p & 3) == 0) {
                    const uint32_t* p4 = reinterpret_cast<const uint32_t*>(p);
                    v = make_uint4(p4[0], p4[1], p4[2], p4[3]);
                } else {
                    uint32_t d[4] = {0, 0, 0, 0};
#pragma unroll
                    for (int b = 0; b < 16; ++b) d[b >> 2] |= (uint32_t)p[b] << (8 * (b & 3));
                    v = make_uint4(d[0], d[1], d[2], d[3]);
                }
                *reinterpret_cast<uint4*>(dst + y * wo + 16 * j) = v;
            }
        } else {
            const long n = (long)ho * wo;
            for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
                const long y = i / wo;
                dst[i] = src[y * W + (i - y * wo)];
            }
        }
    }
}

bool rs_args_ok(int planes, int h, int w, int s, int R) {
    if (!(u8_pair_ok(planes, h, w, s) && R >= 0 && R <= RS_MAX_R)) return false;
    const int m = rs_margin(s, R);
    return h - 2 * m >= 1 && w - 2 * m >= 1;
}

// workgroups per plane and what they walk: (gx, B, tiles_x, tiles)
struct RsGrid { int gx, gy, B, tiles_x, tiles, G; };
RsGrid rs_grid(int planes, int h, int w, int s, int R) {
    RsGrid g;
    const int m = rs_margin(s, R), T = (2 * R + 1) * (2 * R + 1);
    g.B = rs_block(s, R);
    g.G = rs_split(T, g.B, rs_layout(g.B, s, R));
    g.tiles_x = cdiv(w - 2 * m, g.B);
    g.tiles = cdiv(h - 2 * m, g.B) * g.tiles_x;
    g.gy = planes_grid_y(planes);
    const long row_bytes = (3L * T + 2) * (long)sizeof(u64);
    const int want = blocks_per_plane(planes, g.tiles, RS_PARTIAL_BYTES / row_bytes / planes);
    g.gx = cdiv(g.tiles, tile_run(g.tiles, want));   // every workgroup has a block of outputs
    return g;
}
constexpr int64_t RS_TAP_BYTES = 2 * RS_MAX_S * (int64_t)sizeof(int);

}  // namespace

extern "C" int64_t pssr_register_shifts_workspace_bytes(int planes, int h, int w, int s, int radius) {
    if (!rs_args_ok(planes, h, w, s, radius)) return 0;
    const RsGrid g = rs_grid(planes, h, w, s, radius);
    const int T = (2 * radius + 1) * (2 * radius + 1);
    return RS_TAP_BYTES + (int64_t)planes * g.gx * (3 * T + 2) * (int64_t)sizeof(u64);
}

extern "C" int pssr_register_shifts_u8(const uint8_t* hr, const uint8_t* lr, uint64_t* sums, int planes, int h, int w, int s, int radius,
                                       void* workspace, pssr_stream_t stream) {
    PSSR_CHECK(hr && lr && sums && workspace, PSSR_ERR_ARG, "register_shifts_u8: null pointer");
    if (const int status = u8_pair_check("register_shifts_u8", planes, h, w, s)) return status;
    PSSR_CHECK(radius >= 0 && radius <= RS_MAX_R, PSSR_ERR_ARG, "register_shifts_u8: the radius must be 0 .. 32 HR pixels, given %d", radius);
    PSSR_CHECK(rs_args_ok(planes, h, w, s, radius), PSSR_ERR_ARG,
               "register_shifts_u8: a %d x %d LR plane leaves nothing inside the margin of %d pixels (1 + ceil(radius / scale)) on every side", h, w,
               rs_margin(s, radius));
    const RsGrid g = rs_grid(planes, h, w, s, radius);
    const int T = (2 * radius + 1) * (2 * radius + 1), k3 = 3 * T + 2;
    int* taps = (int*)workspace;
    u64* partial = (u64*)((char*)workspace + RS_TAP_BYTES);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(register_taps_kernel, dim3(1), dim3(64), 0, st, taps, s);
    PSSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(register_shifts_kernel, dim3(g.gx, g.gy), dim3(256), (size_t)rs_layout(g.B, s, radius).bytes, st, hr, lr, partial, (const int*)taps,
                       planes, h, w, s, radius, g.B, g.G, g.tiles_x, g.tiles);
    PSSR_LAUNCH_CHECK();
    launch_fold_u64<16>(partial, (u64*)sums, planes, g.gx, k3, st);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

extern "C" int pssr_crop_shift_u8(const uint8_t* in, uint8_t* out, const int32_t* origins, int planes, int H, int W, int ho, int wo,
                                  pssr_stream_t stream) {
    PSSR_CHECK(in && out && origins, PSSR_ERR_ARG, "crop_shift_u8: null pointer");
    PSSR_CHECK(planes > 0 && H > 0 && W > 0 && ho > 0 && wo > 0, PSSR_ERR_ARG, "crop_shift_u8: planes and sizes must be positive (%d; %d x %d -> %d x %d)",
               planes, H, W, ho, wo);
    PSSR_CHECK(ho <= H && wo <= W, PSSR_ERR_ARG, "crop_shift_u8: a %d x %d window does not fit a %d x %d plane", ho, wo, H, W);
    const bool vec = wo % 16 == 0 && (uintptr_t)out % 16 == 0;
    const long pieces = vec ? (long)ho * (wo / 16) : (long)ho * wo;
    const dim3 grid(blocks_per_plane(planes, (pieces + 255) / 256), planes_grid_y(planes));
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(crop_shift_kernel<true>, grid, dim3(256), 0, st, in, out, (const int*)origins, planes, H, W, ho, wo);
    else
        hipLaunchKernelGGL(crop_shift_kernel<false>, grid, dim3(256), 0, st, in, out, (const int*)origins, planes, H, W, ho, wo);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}
