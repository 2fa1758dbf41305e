// Scan phase of a bidirectional point scanner, the uint8 side (pssr2_amd.util.estimate_scan_phase / correct_scan_phase;
// include/pssr_mi355.h has the definitions): every second line is drawn on the way back, and a timing error moves the odd rows sideways
// against the even ones.
//
// line_moments_kernel (D3), grid (workgroups, planes), block 256.  Per plane X [H][W], radius R of 0 .. 16, T = 2R + 1, for every interior
// row y and every column x in R .. W-R-1: O_k = X[y][x + k], E = X[y-1][x] + X[y+1][x];  out[plane][y - 1] = T triples
// (sum O_k, sum O_k^2, sum O_k E), then sum E, sum E^2: exact 64-bit integers, the layout of pssr_register_shifts_u8 per row.
//   * A workgroup owns a run of neighbouring interior rows of one plane (u8_planes.h's runs) and walks the plane's columns in chunks of
//     at most LM_CHUNK.  Per chunk it stages the raw bytes of three rows with stage_rows_u8 -- whole aligned 16-byte pieces -- into a ring
//     of four LDS rows, then slides down: the loads of row y + 2 are issued before the sums of row y are taken and land in the ring's
//     fourth row afterwards, so a row comes from HBM once per run (plus the two rows a run shares with its neighbours).
//   * Per row: all threads write E (16-bit) to LDS; then thread g * (T + 1) + item takes the g-th of G = 256 / (T + 1) column segments
//     of one item -- a candidate k, or item T = "E itself" -- so R = 0 (2 items, 128 segments) and R = 16 (34 items, 7 segments) both
//     fill the group, and neighbouring lanes read neighbouring bytes of the row and the same E (an LDS broadcast).  Three 32-bit sums
//     per thread (at most LM_CHUNK columns: 255 * 510 * 4032 < 2^32), to LDS; the thread of an item adds its G parts in order as 64-bit
//     and writes the item's slots of the output row (the first chunk writes, later chunks add: one thread per slot, in program order).
// Integers only, no atomics, no fence, no second launch: the same bits on every run.
//
// shift_rows_kernel<uint8_t> (D1): shift_rows.h with the rounding ((256 - f) a + f b + 128) >> 8.
#include "u8_planes.h"
#include "shift_rows.h"

namespace {

constexpr int LM_MAX_R = 16;
constexpr int LM_CHUNK = 4032;                                  // columns of a chunk
constexpr int LM_PITCH = (LM_CHUNK + 2 * LM_MAX_R + 15 + 15) / 16 * 16;    // an LDS row: the chunk, R on both sides, the alignment shift (4080)
constexpr int LM_MIN_RUN = 8;                                   // rows a workgroup aims at, so that the shared rows stay a quarter
static_assert(LM_PITCH / 16 <= 256, "a row is staged in one round of 256 pieces");
static_assert(255ull * 510 * LM_CHUNK < (1ull << 32) && 510ull * 510 * LM_CHUNK < (1ull << 32), "32-bit sums of a thread");

__global__ __launch_bounds__(256) void line_moments_kernel(const uint8_t* __restrict__ x, u64* __restrict__ out, int planes, int H, int W, int R) {
    __shared__ __attribute__((aligned(16))) uint8_t ring[4][LM_PITCH];
    __shared__ uint16_t e16[LM_CHUNK];
    __shared__ uint32_t parts[256 * 3];
    const int tid = threadIdx.x;
    const int T = 2 * R + 1, nitems = T + 1, k3 = 3 * T + 2, G = 256 / nitems;
    const int g = tid / nitems, item = tid - g * nitems;
    const int rows = H - 2, wv = W - 2 * R;                     // interior rows, valid columns
    const long plane_in = (long)H * W, total = (long)planes * plane_in;
    const TileRun mine = my_tile_run(rows);                     // interior rows [begin, end): y = 1 + index
    if (mine.begin >= mine.end) return;
    const int ya = mine.begin + 1, yb = mine.end + 1;           // rows y in [ya, yb)
    for (int pl = blockIdx.y; pl < planes; pl += gridDim.y) {
        for (int c0 = 0; c0 < wv; c0 += LM_CHUNK) {
            const int ncol = wv - c0 < LM_CHUNK ? wv - c0 : LM_CHUNK, nraw = ncol + 2 * R;
            const long rowbase = (long)pl * plane_in + c0;      // raw column 0 of the chunk is column c0 of the plane (valid column c0 + R)
            const int base15 = (int)(((uintptr_t)x + (uintptr_t)rowbase) & 15), w15 = W & 15;
            const int seg = (ncol + G - 1) / G;
            const int j0 = g * seg < ncol ? g * seg : ncol, j1 = j0 + seg < ncol ? j0 + seg : ncol;
            auto shift_of = [&](int row) { return (base15 + row * w15) & 15; };
            auto sums_of = [&](int y) {
                const uint8_t* up = ring[(y - 1) & 3] + shift_of(y - 1) + R;
                const uint8_t* cur = ring[y & 3] + shift_of(y);
                const uint8_t* dn = ring[(y + 1) & 3] + shift_of(y + 1) + R;
                for (int j = tid; j < ncol; j += 256) e16[j] = (uint16_t)((uint32_t)up[j] + dn[j]);
                __syncthreads();
                if (g < G) {
                    uint32_t a = 0, b = 0, c = 0;
                    if (item < T) {
                        const uint8_t* src = cur + item;        // O_k at column j: raw column j + R + k, k = item - R
#pragma unroll 4
                        for (int j = j0; j < j1; ++j) {
                            const uint32_t o = src[j], e = e16[j];
                            a += o; b += o * o; c += o * e;
                        }
                    } else {
#pragma unroll 4
                        for (int j = j0; j < j1; ++j) {
                            const uint32_t e = e16[j];
                            a += e; b += e * e;
                        }
                    }
                    parts[3 * tid] = a; parts[3 * tid + 1] = b; parts[3 * tid + 2] = c;
                }
                __syncthreads();
                if (tid < nitems) {                             // g = 0: this thread's item
                    u64 a = 0, b = 0, c = 0;
                    for (int gg = 0; gg < G; ++gg) {
                        const uint32_t* part = parts + 3 * (gg * nitems + tid);
                        a += part[0]; b += part[1]; c += part[2];
                    }
                    slots_update(out + ((long)pl * rows + (y - 1)) * k3 + 3 * tid, c0 == 0, tid < T, a, b, c);
                }
            };
            // rows ya - 1, ya, ya + 1 of the chunk
            for (int r = ya - 1; r <= ya + 1; ++r)
                stage_rows_u8<1>(x, total, rowbase, W, base15, w15, r, 1, nraw, ring[r & 3], LM_PITCH, 0, [] {});
            __syncthreads();
            for (int y = ya; y < yb; ++y) {
                if (y + 1 < yb)                                 // row y + 2 <= H - 1 slides in behind the sums of row y
                    stage_rows_u8<1>(x, total, rowbase, W, base15, w15, y + 2, 1, nraw, ring[(y + 2) & 3], LM_PITCH, 0, [&] { sums_of(y); });
                else
                    sums_of(y);
                __syncthreads();                                // the ring row of y + 2 is read, and e16 / parts are rewritten, by the next row
            }
        }
    }
}

struct MixU8 {
    __device__ __forceinline__ uint8_t operator()(uint8_t a, uint8_t b, int f) const { return (uint8_t)(((256 - f) * (int)a + f * (int)b + 128) >> 8); }
};

}  // namespace

extern "C" int pssr_line_moments_u8(const uint8_t* x, uint64_t* sums, int planes, int H, int W, int radius, pssr_stream_t stream) {
    PSSR_CHECK(x && sums, PSSR_ERR_ARG, "line_moments_u8: null pointer");
    PSSR_CHECK(planes > 0 && H > 0 && W > 0, PSSR_ERR_ARG, "line_moments_u8: planes, H and W must be positive (%d, %d, %d)", planes, H, W);
    PSSR_CHECK(radius >= 0 && radius <= LM_MAX_R, PSSR_ERR_ARG, "line_moments_u8: the radius must be 0 .. 16 pixels, given %d", radius);
    PSSR_CHECK(H >= 3, PSSR_ERR_ARG, "line_moments_u8: a plane of %d rows has no row between two others (at least 3)", H);
    PSSR_CHECK(W >= 2 * radius + 1, PSSR_ERR_ARG, "line_moments_u8: a row of %d pixels is shorter than the 2 * %d + 1 of the window", W, radius);
    PSSR_CHECK((long)H * W <= (1L << 28), PSSR_ERR_ARG, "line_moments_u8: %ld pixels per plane (at most 2^28: the sums are exact up to there)", (long)H * W);
    const int rows = H - 2;
    const int gx = blocks_per_plane(planes, cdiv(rows, LM_MIN_RUN));
    hipLaunchKernelGGL(line_moments_kernel, dim3(cdiv(rows, tile_run(rows, gx)), planes_grid_y(planes)), dim3(256), 0, (hipStream_t)stream, x, (u64*)sums,
                       planes, H, W, radius);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

extern "C" int pssr_shift_rows_u8(const uint8_t* in, uint8_t* out, const int32_t* table, int planes, int H, int W, pssr_stream_t stream) {
    PSSR_CHECK(in && out && table, PSSR_ERR_ARG, "shift_rows_u8: null pointer");
    PSSR_CHECK(in != out, PSSR_ERR_ARG, "shift_rows_u8: in place is not supported (a row is read while it is written)");
    PSSR_CHECK(planes > 0 && H > 0 && W > 0, PSSR_ERR_ARG, "shift_rows_u8: planes, H and W must be positive (%d, %d, %d)", planes, H, W);
    PSSR_CHECK((long)H * W <= (1L << 28), PSSR_ERR_ARG, "shift_rows_u8: %ld pixels per plane (at most 2^28)", (long)H * W);
    launch_shift_rows<uint8_t>(in, out, (const int*)table, (long)planes * H, W, MixU8(), (hipStream_t)stream);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}
