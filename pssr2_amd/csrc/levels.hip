// Level-conditional moments of a uint8 plane pair (pssr2_amd.util.estimate_noise; include/pssr_mi355.h has the definitions): for each of
// the 256 grey levels v of D, over the pixels with D = v, the count n, sum L, sum L^2 and the counts of L = 0 and of L = 255 -- the
// photon-transfer table from which the host reads the shot-noise slope, the additive width, the gain and the salt-and-pepper amount.
// d, l uint8 [planes][per_plane], table uint64 [planes][256][5].
//
// level_moments_kernel, grid (workgroups, planes up to the cap), block 256, 20 KB of static LDS.  A plane is cut into aligned 16-byte
// pieces (the first starts at the 16-byte boundary at or before the plane's first byte) and into strips of 256 pieces; a workgroup walks
// a run of neighbouring strips (my_tile_run of u8_planes.h), LV_STAGE strips a step: every thread has LV_STAGE 16-byte loads of d and as
// many of l in flight, then bins their 16 pixel pairs each.
//   Binning: one private table [256][5] of uint32 per wave, LDS integer adds (exact in any order; ds_add_u32 without a return value).  A
//   level's five words are neighbours and 5 is odd, so the levels of a natural image spread over the banks; lanes of a wave that meet on
//   one level are serialised by the LDS unit -- a constant plane is the worst case and costs what DESIGN.md (21) reports.
//   Flush: after every step (256 * 16 * LV_STAGE = 2^14 pixels, so a word stays below 2^14 * 255^2 < 2^32) thread t adds the four waves'
//   words of level t into five 64-bit registers and clears them.  At the end of the plane it writes the five into its slots of the
//   workgroup's row in the workspace.
// The planes of a stack start at any address modulo 16; a piece that is not whole inside the buffer is put together from bytes, and the
// bytes of a piece outside the plane are not binned.  When d and l differ in their address modulo 16, no piece is aligned in both: the
// VEC = false instantiation of the same kernel cuts the plane from its first byte and puts every piece together from bytes (same strips,
// same lanes, same table).
//
// Determinism: integers only; no global atomics, no fence, no floating point.  fold_u64_kernel<16> (a second small launch) adds the
// workgroups' rows; the sums wrap at 2^64 and never get there (2^28 * 255^2 < 2^44).
#include "u8_planes.h"

namespace {

constexpr int LV_WORDS = 256 * 5;            // a table: [level][n, sum L, sum L^2, n0, n255]
constexpr int LV_STAGE = 4;                  // 16-byte pieces of each input a thread has in flight: a step is 2^14 pixels
constexpr int LV_MIN_RUN = 4;                // strips a workgroup takes at least: 32 KB read for the 10 KB row it leaves
constexpr long LV_MAX_PIXELS = 1L << 28;

__device__ __forceinline__ void level_add(uint32_t* table, uint32_t v, uint32_t x) {
    uint32_t* e = table + 5 * v;
    atomicAdd(e, 1u);
    atomicAdd(e + 1, x);
    atomicAdd(e + 2, x * x);
    if (x == 0) atomicAdd(e + 3, 1u);
    if (x == 255) atomicAdd(e + 4, 1u);
}

// the 16 bytes src[g .. g + 16) of a buffer of `total` bytes, one at a time; zero where the buffer is not
__device__ __forceinline__ uint4 piece_from_bytes(const uint8_t* __restrict__ src, long g, long total) {
    uint32_t p[4] = {0, 0, 0, 0};
#pragma unroll
    for (int b = 0; b < 16; ++b)
        if (g + b >= 0 && g + b < total) p[b >> 2] |= (uint32_t)src[g + b] << (8 * (b & 3));
    return make_uint4(p[0], p[1], p[2], p[3]);
}

template <bool VEC>
__global__ __launch_bounds__(256) void level_moments_kernel(const uint8_t* __restrict__ d, const uint8_t* __restrict__ l, u64* __restrict__ partial,
                                                            int planes, long per_plane, int strips) {
    __shared__ uint32_t tab[4 * LV_WORDS];                   // [wave][level][5]
    const int tid = threadIdx.x;
    uint32_t* const mine = tab + (tid >> 6) * LV_WORDS;
    for (int i = tid; i < 4 * LV_WORDS; i += 256) tab[i] = 0;
    __syncthreads();
    const long total = (long)planes * per_plane;
    const TileRun run = my_tile_run(strips);
    for (int pl = blockIdx.y; pl < planes; pl += gridDim.y) {
        const long base = (long)pl * per_plane;
        const int sh = VEC ? (int)(((uintptr_t)d + (uintptr_t)base) & 15) : 0;      // the plane's first byte inside its first piece
        const int pieces = (int)((sh + per_plane + 15) / 16);
        const int stop = run.end * 256 < pieces ? run.end * 256 : pieces;
        u64 acc[5] = {0, 0, 0, 0, 0};
        for (int p0 = run.begin * 256; p0 < run.end * 256; p0 += 256 * LV_STAGE) {
            uint4 vd[LV_STAGE], vl[LV_STAGE];
#pragma unroll
            for (int it = 0; it < LV_STAGE; ++it) {
                const int j = p0 + tid + 256 * it;
                const long g = base - sh + 16L * j;
                vd[it] = vl[it] = make_uint4(0, 0, 0, 0);
                if (VEC && j < stop && g >= 0 && g + 16 <= total) {
                    vd[it] = *reinterpret_cast<const uint4*>(d + g);
                    vl[it] = *reinterpret_cast<const uint4*>(l + g);
                }
            }
#pragma unroll
            for (int it = 0; it < LV_STAGE; ++it) {
                const int j = p0 + tid + 256 * it;
                if (j < stop) {
                    const long g = base - sh + 16L * j, first = 16L * j - sh;       // the piece's first byte in the buffer and in the plane
                    if (!(VEC && g >= 0 && g + 16 <= total)) {
                        vd[it] = piece_from_bytes(d, g, total);
                        vl[it] = piece_from_bytes(l, g, total);
                    }
                    const int lo = first < 0 ? (int)-first : 0, hi = per_plane - first < 16 ? (int)(per_plane - first) : 16;
                    const uint32_t wd[4] = {vd[it].x, vd[it].y, vd[it].z, vd[it].w}, wl[4] = {vl[it].x, vl[it].y, vl[it].z, vl[it].w};
#pragma unroll
                    for (int b = 0; b < 16; ++b)
                        if (b >= lo && b < hi) level_add(mine, (wd[b >> 2] >> (8 * (b & 3))) & 255u, (wl[b >> 2] >> (8 * (b & 3))) & 255u);
                }
            }
            __syncthreads();
            // flush: thread t owns level t
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                const int i = 5 * tid + q;
                acc[q] += ((u64)tab[i] + tab[LV_WORDS + i]) + ((u64)tab[2 * LV_WORDS + i] + tab[3 * LV_WORDS + i]);
                tab[i] = tab[LV_WORDS + i] = tab[2 * LV_WORDS + i] = tab[3 * LV_WORDS + i] = 0;
            }
            __syncthreads();
        }
        u64* const row = partial + ((long)pl * gridDim.x + blockIdx.x) * LV_WORDS + 5 * tid;      // zeros from a workgroup without a strip
#pragma unroll
        for (int q = 0; q < 5; ++q) row[q] = acc[q];
    }
}

bool lv_args_ok(int planes, int64_t per_plane) { return planes > 0 && per_plane >= 1 && per_plane <= LV_MAX_PIXELS; }

// workgroups per plane and the strips they share: the strips of the plane that starts latest in its first piece
struct LvGrid { int gx, gy, strips; };
LvGrid lv_grid(int planes, int64_t per_plane) {
    LvGrid g;
    const int pieces = (int)((15 + per_plane + 15) / 16);
    g.strips = cdiv(pieces, 256);
    g.gy = planes_grid_y(planes);
    g.gx = cdiv(g.strips, tile_run(g.strips, blocks_per_plane(planes, cdiv(g.strips, LV_MIN_RUN))));     // every workgroup has a strip
    return g;
}

}  // namespace

extern "C" int64_t pssr_level_moments_workspace_bytes(int planes, int64_t per_plane) {
    if (!lv_args_ok(planes, per_plane)) return 0;
    return (int64_t)planes * lv_grid(planes, per_plane).gx * LV_WORDS * (int64_t)sizeof(u64);
}

extern "C" int pssr_level_moments_u8(const uint8_t* d, const uint8_t* l, uint64_t* table, int planes, int64_t per_plane, void* workspace,
                                     int64_t workspace_bytes, pssr_stream_t stream) {
    PSSR_CHECK(d && l && table && workspace, PSSR_ERR_ARG, "level_moments_u8: null pointer");
    PSSR_CHECK(planes > 0, PSSR_ERR_ARG, "level_moments_u8: planes must be positive (%d)", planes);
    PSSR_CHECK(lv_args_ok(planes, per_plane), PSSR_ERR_ARG, "level_moments_u8: %ld pixels per plane (1 .. 2^28: the sums are exact up to there)",
               (long)per_plane);
    PSSR_CHECK(workspace_bytes >= pssr_level_moments_workspace_bytes(planes, per_plane), PSSR_ERR_ARG,
               "level_moments_u8: a workspace of %ld bytes is too small (%ld)", (long)workspace_bytes,
               (long)pssr_level_moments_workspace_bytes(planes, per_plane));
    const LvGrid g = lv_grid(planes, per_plane);
    hipStream_t st = (hipStream_t)stream;
    if ((((uintptr_t)d ^ (uintptr_t)l) & 15) == 0)
        hipLaunchKernelGGL(level_moments_kernel<true>, dim3(g.gx, g.gy), dim3(256), 0, st, d, l, (u64*)workspace, planes, (long)per_plane, g.strips);
    else
        hipLaunchKernelGGL(level_moments_kernel<false>, dim3(g.gx, g.gy), dim3(256), 0, st, d, l, (u64*)workspace, planes, (long)per_plane, g.strips);
    PSSR_LAUNCH_CHECK();
    launch_fold_u64<16>((const u64*)workspace, (u64*)table, planes, g.gx, LV_WORDS, st);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}
