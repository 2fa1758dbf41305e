// Collage rows of predict_collage (pssr/predict.py:85-142 with `_collage_preds` / `_image_stack`, :213-243): for every image one row of
// up to three panels side by side -- low-resolution input enlarged by Pillow's NEAREST map, prediction, ground truth -- composed
// straight into a uint8 canvas in HBM:
//
//   canvas[(row0 + i) * h + y][p * w + x] = panel_p(i)[ yi_p[y] ][ xi_p[x] ]          p < n_panels, y < h, x < w
//
// A panel is a strided view (pointer to its first pixel, image stride, row pitch: the centre frame and the crop of a [B, C, H, W]
// tensor need no copy), uint8 or float32; float32 pixels become fminf(fmaxf(v, 0), 255) truncated toward zero, the arithmetic of
// clip_u8_kernel (elementwise.hip), i.e. of `_pred_array` (pssr/predict.py:245-246).  yi[h] / xi[w] are int32 index tables on the
// device (PIL.Image.resize(NEAREST) as pssr2_amd/ops.py builds them); both null = the identity.
//
// collage_rows_kernel: grid (ceil(h * w / V / 256), n_panels, n_images), block 256; a thread makes V consecutive bytes of one panel row.
// The panel is chosen by blockIdx.y, so its descriptor (part of the kernel arguments) is read with scalar loads.
//   VEC = true  (V = 16; w % 16 == 0, canvas rows 16-byte aligned): the 16 bytes are assembled in registers and leave as one 16-byte
//               store.  An identity panel whose source row is 16-byte aligned at that position is read with one 16-byte load
//               (uint8) or four (float32); every other case reads pixel by pixel through the table, whose 16 entries come as four
//               16-byte loads when the table is aligned.  The enlarged panel reads each source pixel scale^2 times: from L1 / L2.
//   VEC = false (V = 1): the same kernel, one byte per thread.
// 32-bit index arithmetic; 64-bit only in the products that form a base address.  No atomics, no workspace, no LDS: every canvas
// byte is written once, by one lane.
//
// Guard: a row index outside [0, src_h) or a column index outside [0, src_w) -- a table entry, or the identity past the end of a
// source smaller than h x w -- writes 0 for that byte and reads nothing, as pssr_gather_windows_u8 does for a window that leaves its sheet.
#include "common.h"

namespace {

struct Panel { const void* src; long image_stride; int row_pitch, src_h, src_w, is_f32; const int* yi; const int* xi; };
struct Panels { Panel p[3]; };

__device__ __forceinline__ unsigned clip_byte(float v) { return (unsigned)(uint8_t)fminf(fmaxf(v, 0.f), 255.f); }

// pixel `sx` of the source row at element offset `row`; 0 (and no read) outside the row
__device__ __forceinline__ unsigned panel_px(const Panel& P, long row, int sx) {
    if ((unsigned)sx >= (unsigned)P.src_w) return 0;
    return P.is_f32 ? clip_byte(static_cast<const float*>(P.src)[row + sx]) : (unsigned)static_cast<const uint8_t*>(P.src)[row + sx];
}

template <bool VEC>
__global__ __launch_bounds__(256) void collage_rows_kernel(Panels ps, uint8_t* __restrict__ canvas, long pitch, int row0, int h, int w) {
    constexpr int V = VEC ? 16 : 1;
    const Panel P = ps.p[blockIdx.y];
    const int upr = w / V;                                          // units of V bytes per panel row
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= (unsigned)(h * upr)) return;
    const int y = (int)(u / (unsigned)upr), x0 = (int)(u % (unsigned)upr) * V;
    const int img = blockIdx.z;
    uint8_t* dst = canvas + ((long)(row0 + img) * h + y) * pitch + (long)blockIdx.y * w + x0;
    const int sy = P.yi ? P.yi[y] : y;
    const bool row_ok = sy >= 0 && sy < P.src_h;
    const long row = (long)img * P.image_stride + (long)(row_ok ? sy : 0) * P.row_pitch;

    if (!VEC) {
        *dst = row_ok ? (uint8_t)panel_px(P, row, P.xi ? P.xi[x0] : x0) : (uint8_t)0;
        return;
    }
    unsigned wv[4] = {0, 0, 0, 0};
    if (row_ok) {
        const uintptr_t at = (uintptr_t)P.src + (uintptr_t)(row + x0) * (P.is_f32 ? 4 : 1);
        if (!P.xi && x0 + 16 <= P.src_w && (at & 15) == 0) {
            if (P.is_f32) {
                const float4* r = reinterpret_cast<const float4*>(at);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float4 f = r[k];
                    wv[k] = clip_byte(f.x) | clip_byte(f.y) << 8 | clip_byte(f.z) << 16 | clip_byte(f.w) << 24;
                }
            } else {
                const uint4 q = *reinterpret_cast<const uint4*>(at);
                wv[0] = q.x, wv[1] = q.y, wv[2] = q.z, wv[3] = q.w;
            }
        } else {
            int sx[16];
            if (P.xi && ((uintptr_t)P.xi & 15) == 0) {
                const int4* t = reinterpret_cast<const int4*>(P.xi + x0);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int4 q = t[k];
                    sx[4 * k] = q.x, sx[4 * k + 1] = q.y, sx[4 * k + 2] = q.z, sx[4 * k + 3] = q.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 16; ++j) sx[j] = P.xi ? P.xi[x0 + j] : x0 + j;
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) wv[j >> 2] |= panel_px(P, row, sx[j]) << (8 * (j & 3));
        }
    }
    *reinterpret_cast<uint4*>(dst) = make_uint4(wv[0], wv[1], wv[2], wv[3]);
}

}  // namespace

extern "C" int pssr_collage_rows_u8(const pssr_collage_panel* panels, int n_panels, uint8_t* canvas, int64_t canvas_pitch, int row0,
                                    int n_images, int h, int w, pssr_stream_t s) {
    static_assert(sizeof(pssr_collage_panel) == 48 && sizeof(Panel) == 48, "pssr_collage_panel layout");
    PSSR_CHECK(panels && canvas, PSSR_ERR_ARG, "collage_rows: null pointer");
    PSSR_CHECK(n_panels >= 1 && n_panels <= 3, PSSR_ERR_ARG, "collage_rows: n_panels must be 1, 2 or 3");
    PSSR_CHECK(n_images > 0 && h > 0 && w > 0 && row0 >= 0, PSSR_ERR_ARG, "collage_rows: n_images, h and w must be positive, row0 non-negative");
    PSSR_CHECK(canvas_pitch >= (int64_t)n_panels * w, PSSR_ERR_ARG, "collage_rows: canvas_pitch is smaller than n_panels * w");
    PSSR_CHECK(n_images <= 65535, PSSR_ERR_ARG, "collage_rows: n_images exceeds the grid limit (65535)");
    PSSR_CHECK((int64_t)h * w <= 0x7fffffffL, PSSR_ERR_ARG, "collage_rows: h * w exceeds the grid limit");
    Panels ps = {};
    for (int p = 0; p < n_panels; ++p) {
        const pssr_collage_panel& a = panels[p];
        PSSR_CHECK(a.src, PSSR_ERR_ARG, "collage_rows: null pointer (panel source)");
        PSSR_CHECK(a.src_h > 0 && a.src_w > 0 && a.row_pitch >= a.src_w && a.image_stride >= 0, PSSR_ERR_ARG,
                   "collage_rows: a panel needs positive src_h / src_w, row_pitch >= src_w and a non-negative image stride");
        PSSR_CHECK((a.yi == nullptr) == (a.xi == nullptr), PSSR_ERR_ARG, "collage_rows: a panel has one index table but not the other");
        ps.p[p] = Panel{a.src, (long)a.image_stride, a.row_pitch, a.src_h, a.src_w, a.is_f32 != 0, a.yi, a.xi};
    }
    const bool vec = w % 16 == 0 && canvas_pitch % 16 == 0 && ((uintptr_t)canvas % 16) == 0;      // row0 * h * pitch is then a multiple of 16 too
    const long units = (long)h * (vec ? w / 16 : w);
    const dim3 grid((unsigned)((units + 255) / 256), (unsigned)n_panels, (unsigned)n_images);
    if (vec)
        hipLaunchKernelGGL((collage_rows_kernel<true>), grid, dim3(256), 0, (hipStream_t)s, ps, canvas, (long)canvas_pitch, row0, h, w);
    else
        hipLaunchKernelGGL((collage_rows_kernel<false>), grid, dim3(256), 0, (hipStream_t)s, ps, canvas, (long)canvas_pitch, row0, h, w);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}
