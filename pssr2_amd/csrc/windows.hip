// Sliding-window gather for training from image sheets (pssr/data.py:629-660 `_sliding_window` / `_slice_image`, then the rot90 / flip of
// `_gen_pair`, pssr/data.py:477-480): out[i][f] = sheet[frame0 + f][y0 : y0 + res, x0 : x0 + res], np.rot90 in (H, W) when rot, np.flip
// along flip_axis (0 frames, 1 rows, 2 columns, 3 rows and columns, -1 none: the meaning they have in gen_pair_geometry_kernel,
// crappify.hip).  A sliding window is always full-size (`_n_tiles` counts whole windows only), so there is no crop / reflect-pad branch.
//
// gather_windows_kernel: grid (nb * nb * c, items), block 256, nb = ceil(res / 64).  A workgroup produces one 64 x 64 block (th x tw at
// the bottom / right edge) of one output frame.  Its pixels are one rectangle of the sheet whatever the orientation: th x tw, or
// tw x th when rotated.  That rectangle goes through LDS:
//
//   phase 1  the rectangle is read row by row (consecutive lanes take consecutive bytes of a sheet row) and written to lds[r][col];
//   phase 2  the output block is written row by row (consecutive lanes take consecutive bytes of an output row); output byte
//            (ly, lx + j) comes from lds address a0 + j * step, step = +1 / -1 (plain, column flip) or +P / -P (rotated).
//
// So both global accesses are row-contiguous in all seven orientations, and the transposition happens between the LDS write and the LDS
// read.
//
// LDS pitch P = 65 bytes.  A rotated read takes, per instruction, bytes of 4 rectangle rows that lie 16 rows apart (the four 16-byte
// segments of an output row) x 8 neighbouring columns per 32-lane half.  16 rows are 16 * 65 = 1040 bytes = 260 dwords = 4 banks
// (mod 32) apart and 8 neighbouring bytes cover at most 3 dwords, so the four segments fall on different banks; with a pitch that is
// a multiple of 8 bytes they would all meet on one.  Lanes that read different bytes of one dword share an address (broadcast).
//
// VEC = true (res % 16 == 0 and a 16-byte aligned `out`): a lane stores 16 bytes at a time, and phase 1 reads 16-byte aligned chunks.  Sheet rows
// are misaligned in general (odd widths, x0 = k * stride), so a row of the rectangle is read as the <= 5 aligned chunks that cover
// it, and every byte is put at its column in LDS (byte stores: the shift differs per row).  The first and last chunk of a row may
// start before / end after the rectangle's bytes: they still lie inside one aligned 16-byte granule that holds at least one byte of
// the sheet, i.e. in memory the sheet's own pages map.  VEC = false: the same kernel, one byte per load and per store.
//
// No atomics, no workspace: every output byte is written once, by one lane.
//
// Guard: an item whose sheet index, frame range or window does not lie inside its sheet is written as zeros and reads nothing (one
// test per workgroup, on values every lane holds in scalar registers).
#include "common.h"

#define WIN_BLOCK 64
#define WIN_PITCH 65
#define WIN_CHUNKS 5        // aligned 16-byte chunks that cover 64 bytes at any misalignment: ceil((15 + 64) / 16)

namespace {

struct SheetDesc { const uint8_t* base; int frames, h, w, reserved; };
struct WindowItem { int sheet, frame0, y0, x0, rot, flip_axis; };

template <bool VEC>
__global__ __launch_bounds__(256) void gather_windows_kernel(const SheetDesc* __restrict__ sheets, int n_sheets, const WindowItem* __restrict__ items,
                                                             uint8_t* __restrict__ out, int c, int res, int nb) {
    __shared__ uint8_t lds[WIN_BLOCK * WIN_PITCH];
    const int t = threadIdx.x;
    const WindowItem it = items[blockIdx.y];
    const unsigned bx = blockIdx.x;
    const int tx = (int)(bx % (unsigned)nb), ty = (int)((bx / (unsigned)nb) % (unsigned)nb), oc = (int)(bx / (unsigned)(nb * nb));
    const int oy0 = ty * WIN_BLOCK, ox0 = tx * WIN_BLOCK;
    const int th = min(WIN_BLOCK, res - oy0), tw = min(WIN_BLOCK, res - ox0);
    uint8_t* dst = out + (((long)blockIdx.y * c + oc) * res + oy0) * (long)res + ox0;

    bool ok = it.sheet >= 0 && it.sheet < n_sheets;
    SheetDesc sd = {nullptr, 0, 0, 0, 0};
    if (ok) {
        sd = sheets[it.sheet];
        ok = sd.base != nullptr && it.frame0 >= 0 && c <= sd.frames && it.frame0 <= sd.frames - c && it.y0 >= 0 && it.x0 >= 0 &&
             res <= sd.h && res <= sd.w && it.y0 <= sd.h - res && it.x0 <= sd.w - res;
    }
    if (!ok) {
        if (VEC) {
            const int ly = t >> 2, lx = (t & 3) * 16;
            if (ly < th && lx < tw) *reinterpret_cast<uint4*>(dst + (long)ly * res + lx) = make_uint4(0, 0, 0, 0);
        } else {
            for (int i = t; i < WIN_BLOCK * WIN_BLOCK; i += 256) {
                const int ly = i >> 6, lx = i & 63;
                if (ly < th && lx < tw) dst[(long)ly * res + lx] = 0;
            }
        }
        return;
    }

    const bool rot = it.rot != 0;
    const bool flip_r = it.flip_axis == 1 || it.flip_axis == 3, flip_c = it.flip_axis == 2 || it.flip_axis == 3;
    const int fc = it.flip_axis == 0 ? c - 1 - oc : oc;
    // the rectangle of the window this block is made of: rows [sy0, sy0 + nr), columns [sx0, sx0 + nc)
    const int fy0 = flip_r ? res - (oy0 + th) : oy0;                // first row / column of the block before the flips
    const int fx0 = flip_c ? res - (ox0 + tw) : ox0;
    const int sy0 = rot ? fx0 : fy0, nr = rot ? tw : th;            // np.rot90(m)[i][j] = m[j][n - 1 - i]
    const int sx0 = rot ? res - fy0 - th : fx0, nc = rot ? th : tw;
    const uint8_t* src = sd.base + (((long)(it.frame0 + fc) * sd.h + it.y0 + sy0) * (long)sd.w + it.x0 + sx0);

    // ---- phase 1: sheet rows -> lds[r][col]
    if (VEC) {
        for (int i = t; i < nr * WIN_CHUNKS; i += 256) {
            const int r = i / WIN_CHUNKS, q = i - r * WIN_CHUNKS;
            const uint8_t* row = src + (long)r * sd.w;
            const int a = (int)((uintptr_t)row & 15);               // the row starts `a` bytes into its first aligned chunk
            if (q * 16 < a + nc) {
                const uint4 u = *reinterpret_cast<const uint4*>(row - a + q * 16);
                const unsigned wv[4] = {u.x, u.y, u.z, u.w};
                uint8_t* l = lds + r * WIN_PITCH + q * 16 - a;
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int col = q * 16 + k - a;
                    if (col >= 0 && col < nc) l[k] = (uint8_t)(wv[k >> 2] >> (8 * (k & 3)));
                }
            }
        }
    } else {
        for (int i = t; i < WIN_BLOCK * WIN_BLOCK; i += 256) {
            const int r = i >> 6, col = i & 63;
            if (r < nr && col < nc) lds[r * WIN_PITCH + col] = src[(long)r * sd.w + col];
        }
    }
    __syncthreads();

    // ---- phase 2: output byte (ly, lx) = lds[r][col]:  plain  r = ly (th - 1 - ly under a row flip), col = lx (tw - 1 - lx under a column flip)
    //                                                     rotated r = lx (tw - 1 - lx under a column flip), col = th - 1 - ly (ly under a row flip)
    const int step = rot ? (flip_c ? -WIN_PITCH : WIN_PITCH) : (flip_c ? -1 : 1);
    if (VEC) {
        const int ly = t >> 2, lx = (t & 3) * 16;
        if (ly < th && lx < tw) {
            const int ux = flip_c ? tw - 1 - lx : lx;
            const int a0 = rot ? ux * WIN_PITCH + (flip_r ? ly : th - 1 - ly) : (flip_r ? th - 1 - ly : ly) * WIN_PITCH + ux;
            unsigned wv[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 16; ++j) wv[j >> 2] |= (unsigned)lds[a0 + j * step] << (8 * (j & 3));
            *reinterpret_cast<uint4*>(dst + (long)ly * res + lx) = make_uint4(wv[0], wv[1], wv[2], wv[3]);
        }
    } else {
        for (int i = t; i < WIN_BLOCK * WIN_BLOCK; i += 256) {
            const int ly = i >> 6, lx = i & 63;
            if (ly < th && lx < tw) {
                const int ux = flip_c ? tw - 1 - lx : lx;
                const int a0 = rot ? ux * WIN_PITCH + (flip_r ? ly : th - 1 - ly) : (flip_r ? th - 1 - ly : ly) * WIN_PITCH + ux;
                dst[(long)ly * res + lx] = lds[a0];
            }
        }
    }
}

}  // namespace

extern "C" int pssr_gather_windows_u8(const pssr_sheet_desc* sheets_dev, int n_sheets, const pssr_window_item* items_dev, int n_items, uint8_t* out,
                                      int c, int res, pssr_stream_t s) {
    static_assert(sizeof(pssr_sheet_desc) == 24 && sizeof(SheetDesc) == 24, "pssr_sheet_desc layout");
    static_assert(sizeof(pssr_window_item) == 24 && sizeof(WindowItem) == 24, "pssr_window_item layout");
    PSSR_CHECK(sheets_dev && items_dev && out, PSSR_ERR_ARG, "gather_windows: null pointer");
    PSSR_CHECK(n_sheets > 0 && c > 0 && res > 0, PSSR_ERR_ARG, "gather_windows: n_sheets, c and res must be positive");
    PSSR_CHECK(n_items > 0 && n_items <= 65535, PSSR_ERR_ARG, "gather_windows: n_items must be in [1, 65535]");
    const long nb = (res + WIN_BLOCK - 1) / WIN_BLOCK;
    PSSR_CHECK(nb * nb * c <= 0x7fffffffL, PSSR_ERR_ARG, "gather_windows: c * ceil(res / 64)^2 exceeds the grid limit");
    const dim3 grid((unsigned)(nb * nb * c), (unsigned)n_items);
    if (res % 16 == 0 && ((uintptr_t)out % 16) == 0)
        hipLaunchKernelGGL((gather_windows_kernel<true>), grid, dim3(256), 0, (hipStream_t)s, (const SheetDesc*)sheets_dev, n_sheets,
                           (const WindowItem*)items_dev, out, c, res, (int)nb);
    else
        hipLaunchKernelGGL((gather_windows_kernel<false>), grid, dim3(256), 0, (hipStream_t)s, (const SheetDesc*)sheets_dev, n_sheets,
                           (const WindowItem*)items_dev, out, c, res, (int)nb);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}
