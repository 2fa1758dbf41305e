// Row resampling (D1 of the scan-phase block of include/pssr_mi355.h), shared by scanline.hip (uint8) and crappify.hip (float32 with the
// crappifier's gain and finish): the content of row `row` of [rows][W] moves right by d / 256 pixels, d = table[row], edge replicated.
//   p = 256 x - d,  i = p >> 8 = x + ((-d) >> 8),  f = p & 255 = (-d) & 255   (one i - x and one f per row)
//   out[x] = mix(in[clamp(i)], in[clamp(i + 1)], f)
// One thread per PER outputs: PER = 16 bytes' worth where the rows are whole aligned 16-byte pieces (one store), else 1.  The PER + 1
// inputs are single loads with clamped indices: nothing outside the row is read whatever the table holds.
#pragma once
#include "common.h"

namespace {

constexpr int SCAN_MAX_D = 256 * 64;        // |d| the definitions allow; a table entry beyond it is clamped

__device__ __forceinline__ uint4 pack16(const uint8_t* r) {
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int b = 0; b < 16; ++b) w[b >> 2] |= (uint32_t)r[b] << (8 * (b & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ uint4 pack16(const float* r) {
    return make_uint4(__float_as_uint(r[0]), __float_as_uint(r[1]), __float_as_uint(r[2]), __float_as_uint(r[3]));
}

template <class T, int PER, class Mix>
__global__ __launch_bounds__(256) void shift_rows_kernel(const T* __restrict__ in, T* __restrict__ out, const int* __restrict__ table, long rows, int W,
                                                         Mix mix) {
    const int q = W / PER;                  // PER > 1: W is a multiple of it
    const long n = rows * q;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const long row = i / q;
        const int x0 = (int)(i - row * q) * PER;
        int d = table[row];
        d = d < -SCAN_MAX_D ? -SCAN_MAX_D : (d > SCAN_MAX_D ? SCAN_MAX_D : d);
        const int s = (-d) >> 8, f = (-d) & 255;
        const T* src = in + row * W;
        T v[PER + 1];
#pragma unroll
        for (int t = 0; t <= PER; ++t) {
            int xi = x0 + s + t;
            xi = xi < 0 ? 0 : (xi > W - 1 ? W - 1 : xi);
            v[t] = src[xi];
        }
        if (PER == 1) {
            out[row * W + x0] = mix(v[0], v[1], f);
        } else {
            T r[PER];
#pragma unroll
            for (int t = 0; t < PER; ++t) r[t] = mix(v[t], v[t + 1], f);
            *reinterpret_cast<uint4*>(out + row * W + x0) = pack16(r);
        }
    }
}

// the launch: 16 bytes per thread where W and `out` allow, else one element
template <class T, class Mix>
inline void launch_shift_rows(const T* in, T* out, const int* table, long rows, int W, Mix mix, hipStream_t st) {
    constexpr int PER = 16 / (int)sizeof(T);
    if (W % PER == 0 && (uintptr_t)out % 16 == 0)
        hipLaunchKernelGGL((shift_rows_kernel<T, PER, Mix>), dim3(grid1d(rows * (W / PER), 8192)), dim3(256), 0, st, in, out, table, rows, W, mix);
    else
        hipLaunchKernelGGL((shift_rows_kernel<T, 1, Mix>), dim3(grid1d(rows * W, 8192)), dim3(256), 0, st, in, out, table, rows, W, mix);
}

}  // namespace
