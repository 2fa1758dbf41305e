// Noise-profile statistics of approximate_crappifier's objective (pssr/train.py:372-384) and the loss made of them.
//
// Per image over its n = C*H*W values, with b the reduced HR (uint8) and a the crappified image (f32, neither rounded nor clipped) or the
// real LR (uint8):
//   v_i   = a_i - b_i                         one f32 subtraction (for uint8 a: an exact integer)
//   hist  = np.histogram(v, np.arange(-256, 256)): 511 integer bins, bin k holds -256 + k <= v < -255 + k, bin 510 also v == 255;
//           v below -256, above 255, NaN or +-inf is counted nowhere
//   sum   = sum_i v_i in f64 (every value, also those outside the bins: the mean of the objective is over the whole image)
//
// noise_profile_kernel: grid (nwg, images), block 256.  A lane takes 16 consecutive values per step (one 16-byte load of b, and four
// 16-byte loads of an f32 a or one of a uint8 a); a workgroup takes strips of 256 * 16 values, strip = wg, wg + nwg, ...
//
// Privatisation: PROFILE_COPIES (8) LDS histograms per workgroup, chosen by lane (lane & 7), each padded to 513 words.  The profile's
// mass sits in a few dozen neighbouring bins (sigma 9 noise: +-3 sigma = 54 bins), so with ONE copy most of the 64 lanes of a
// ds_add hit a handful of words and the LDS unit serialises them.  Lane-indexed copies cut the lanes that can meet on one word to 8 and put
// the same bin of different copies into different banks (513 is odd); per-wave copies would leave all 64 lanes of a wave on one
// histogram, which is the case that serialises, and cost the same LDS for 4 waves x 2 copies.  8 copies are 16.4 KB: eight workgroups
// still fit a CU's 160 KB.  The copies are folded by the workgroup at the end (thread t: bins t and t + 256).
//
// Determinism: the counts are integers (LDS and global integer atomics: exact whatever the order).  The sum is a per-lane f64 chain
// in index order, a fixed shuffle tree per wave, the four waves added in wave order, and -- when an image is split over several
// workgroups -- one f64 partial per workgroup in the workspace, added in workgroup order by noise_profile_fold_kernel (a second
// launch; no floating-point atomics, no fences or tickets).  The same inputs give the same bits on every run.
//
// Images whose size is not a multiple of 16, or pointers that are not 16-byte aligned, take the scalar instantiation (VEC = false) of the
// same kernel: same strips, same lanes, same summation order, one value per load.
//
// noise_profile_loss_kernel (one workgroup per image): S = sum_k (t_k - p_k)^2 as an exact 64-bit integer, then
//   hist term  = (S / 511) / width^2          the reference's np.mean(int64) / (w**2): same two f64 divisions, so bit for bit
//   value term = |sum_T / n - sum_P / n|      f64 (the reference takes both means in f32 pairwise: it differs by that round-off)
// noise_profile_mean_kernel (second launch, one workgroup): mean over images, lane-strided f64 partials and a fixed tree.
#include "common.h"

#ifndef PROFILE_COPIES
#define PROFILE_COPIES 8
#endif
#define PROFILE_BINS PSSR_PROFILE_BINS
#define PROFILE_STRIDE 513
#define PROFILE_VEC 16
#define PROFILE_STRIP (256 * PROFILE_VEC)
#define PROFILE_MAX_WG 64

namespace {

__device__ __forceinline__ void profile_count(int* hist, float v) {
    // -256 <= v < 255 -> floor(v) + 256; v == 255 -> 510; NaN fails every comparison
    if (v >= -256.f && v <= 255.f) {
        const int k = v == 255.f ? PROFILE_BINS - 1 : (int)floorf(v) + 256;
        atomicAdd(&hist[k], 1);
    }
}

template <typename TA> struct ProfileLoad;
template <> struct ProfileLoad<float> {
    static __device__ __forceinline__ void vec(const float* a, float (&x)[PROFILE_VEC]) {
        const float4* p = reinterpret_cast<const float4*>(a);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 f = p[q];
            x[4 * q] = f.x; x[4 * q + 1] = f.y; x[4 * q + 2] = f.z; x[4 * q + 3] = f.w;
        }
    }
};
template <> struct ProfileLoad<uint8_t> {
    static __device__ __forceinline__ void vec(const uint8_t* a, float (&x)[PROFILE_VEC]) {
        const uint4 u = *reinterpret_cast<const uint4*>(a);
        const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int q = 0; q < PROFILE_VEC; ++q) x[q] = (float)((w[q >> 2] >> (8 * (q & 3))) & 0xffu);
    }
};

// grid (nwg, images), block 256.  nwg == 1: hist / sum rows are written directly; otherwise hist (zeroed by the caller) receives
// integer atomics and partial[image * nwg + wg] the workgroup's sum.
template <typename TA, bool VEC>
__global__ __launch_bounds__(256) void noise_profile_kernel(const TA* __restrict__ a, const uint8_t* __restrict__ b, int* __restrict__ hist,
                                                            double* __restrict__ sum, double* __restrict__ partial, long n) {
    __shared__ int lds[PROFILE_COPIES * PROFILE_STRIDE];
    __shared__ double wave_sum[4];
    const int nwg = gridDim.x, wg = blockIdx.x, img = blockIdx.y, t = threadIdx.x;
    for (int i = t; i < PROFILE_COPIES * PROFILE_STRIDE; i += 256) lds[i] = 0;
    __syncthreads();
    a += (long)img * n;
    b += (long)img * n;
    int* mine = lds + (t & (PROFILE_COPIES - 1)) * PROFILE_STRIDE;
    double acc = 0.0;
    const long strips = (n + PROFILE_STRIP - 1) / PROFILE_STRIP;
    for (long s = wg; s < strips; s += nwg) {
        const long base = s * PROFILE_STRIP + (long)t * PROFILE_VEC;
        if (VEC) {                                   // n % 16 == 0: a lane's 16 values are all inside or all outside
            if (base < n) {
                float x[PROFILE_VEC], y[PROFILE_VEC];
                ProfileLoad<TA>::vec(a + base, x);
                ProfileLoad<uint8_t>::vec(b + base, y);
#pragma unroll
                for (int q = 0; q < PROFILE_VEC; ++q) {
                    const float v = __fsub_rn(x[q], y[q]);
                    acc += (double)v;
                    profile_count(mine, v);
                }
            }
        } else {
            for (int q = 0; q < PROFILE_VEC; ++q) {
                if (base + q < n) {
                    const float v = __fsub_rn((float)a[base + q], (float)b[base + q]);
                    acc += (double)v;
                    profile_count(mine, v);
                }
            }
        }
    }
    // the sum: fixed shuffle tree per wave, waves in order
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((t & 63) == 0) wave_sum[t >> 6] = acc;
    __syncthreads();
    if (t == 0) {
        const double s = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
        if (nwg == 1) sum[img] = s;
        else partial[(long)img * nwg + wg] = s;
    }
    // the counts: fold the copies
    for (int k = t; k < PROFILE_BINS; k += 256) {
        int c = 0;
#pragma unroll
        for (int p = 0; p < PROFILE_COPIES; ++p) c += lds[p * PROFILE_STRIDE + k];
        int* dst = hist + (long)img * PROFILE_BINS + k;
        if (nwg == 1) *dst = c;
        else if (c) atomicAdd(dst, c);
    }
}

// sum[img] = partial[img][0] + partial[img][1] + ... in workgroup order
__global__ __launch_bounds__(256) void noise_profile_fold_kernel(const double* __restrict__ partial, double* __restrict__ sum, int images, int nwg) {
    const int img = blockIdx.x * 256 + threadIdx.x;
    if (img >= images) return;
    double s = 0.0;
    for (int w = 0; w < nwg; ++w) s += partial[(long)img * nwg + w];
    sum[img] = s;
}

// grid (images), block 256
__global__ __launch_bounds__(256) void noise_profile_loss_kernel(const int* __restrict__ ph, const double* __restrict__ ps, const int* __restrict__ th,
                                                                 const double* __restrict__ ts, long n, int width, double* __restrict__ loss,
                                                                 double* __restrict__ terms) {
    __shared__ unsigned long long part[256];
    const int img = blockIdx.x, t = threadIdx.x;
    unsigned long long s = 0;
    for (int k = t; k < PROFILE_BINS; k += 256) {
        const long long d = (long long)th[(long)img * PROFILE_BINS + k] - (long long)ph[(long)img * PROFILE_BINS + k];
        s += (unsigned long long)(d * d);
    }
    part[t] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) part[t] += part[t + w];
        __syncthreads();
    }
    if (t == 0) {
        const double dist = ((double)part[0] / (double)PROFILE_BINS) / ((double)width * (double)width);
        const double value = fabs(ts[img] / (double)n - ps[img] / (double)n);
        loss[img] = dist + value;
        if (terms) {
            terms[2 * img] = dist;
            terms[2 * img + 1] = value;
        }
    }
}

// one workgroup: mean[0] = (sum_i loss[i]) / images
__global__ __launch_bounds__(256) void noise_profile_mean_kernel(const double* __restrict__ loss, int images, double* __restrict__ mean) {
    __shared__ double part[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < images; i += 256) s += loss[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) mean[0] = part[0] / (double)images;
}

// workgroups per image: enough to fill the part when there are few images, never more than the image has strips
int profile_wgs(int images, long n) {
    const long strips = (n + PROFILE_STRIP - 1) / PROFILE_STRIP;
    long want = (2048 + images - 1) / images;
    if (want > PROFILE_MAX_WG) want = PROFILE_MAX_WG;
    if (want > strips) want = strips;
    return (int)(want < 1 ? 1 : want);
}

template <typename TA>
int noise_profile(const TA* a, const uint8_t* b, int32_t* hist, double* sum, int images, int64_t n, void* workspace, int64_t workspace_bytes,
                  pssr_stream_t s, const char* who) {
    PSSR_CHECK(a && b && hist && sum && images > 0 && n > 0, PSSR_ERR_ARG, "%s: bad args", who);
    PSSR_CHECK(images <= 65535 && n <= 0x7fffffffL, PSSR_ERR_ARG, "%s: more than 65535 images or 2^31 - 1 values per image", who);
    const int nwg = profile_wgs(images, (long)n);
    PSSR_CHECK(nwg == 1 || (workspace && workspace_bytes >= pssr_noise_profile_workspace_bytes(images, n)), PSSR_ERR_ARG,
               "%s: workspace too small", who);
    const bool vec = n % PROFILE_VEC == 0 && ((uintptr_t)a % 16) == 0 && ((uintptr_t)b % 16) == 0;
    hipStream_t st = (hipStream_t)s;
    if (nwg > 1) {
        hipError_t e = hipMemsetAsync(hist, 0, (size_t)images * PROFILE_BINS * sizeof(int32_t), st);
        PSSR_CHECK(e == hipSuccess, PSSR_ERR_LAUNCH, "%s: memset failed: %s", who, hipGetErrorString(e));
    }
    double* partial = (double*)workspace;
    if (vec)
        hipLaunchKernelGGL((noise_profile_kernel<TA, true>), dim3(nwg, images), dim3(256), 0, st, a, b, (int*)hist, sum, partial, (long)n);
    else
        hipLaunchKernelGGL((noise_profile_kernel<TA, false>), dim3(nwg, images), dim3(256), 0, st, a, b, (int*)hist, sum, partial, (long)n);
    if (nwg > 1)
        hipLaunchKernelGGL(noise_profile_fold_kernel, dim3((images + 255) / 256), dim3(256), 0, st, (const double*)partial, sum, images, nwg);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

}  // namespace

extern "C" int64_t pssr_noise_profile_workspace_bytes(int images, int64_t per_image) {
    if (images <= 0 || per_image <= 0) return 0;
    const int nwg = profile_wgs(images, (long)per_image);
    return nwg == 1 ? 0 : (int64_t)images * nwg * (int64_t)sizeof(double);
}

extern "C" int pssr_noise_profile_f32(const float* a, const uint8_t* b, int32_t* hist, double* sum, int images, int64_t per_image,
                                      void* workspace, int64_t workspace_bytes, pssr_stream_t s) {
    return noise_profile<float>(a, b, hist, sum, images, per_image, workspace, workspace_bytes, s, "noise_profile_f32");
}

extern "C" int pssr_noise_profile_u8(const uint8_t* a, const uint8_t* b, int32_t* hist, double* sum, int images, int64_t per_image,
                                     void* workspace, int64_t workspace_bytes, pssr_stream_t s) {
    return noise_profile<uint8_t>(a, b, hist, sum, images, per_image, workspace, workspace_bytes, s, "noise_profile_u8");
}

extern "C" int pssr_noise_profile_loss(const int32_t* pred_hist, const double* pred_sum, const int32_t* target_hist, const double* target_sum,
                                       int images, int64_t per_image, int width, double* loss, double* terms, double* mean, pssr_stream_t s) {
    PSSR_CHECK(pred_hist && pred_sum && target_hist && target_sum && loss && mean, PSSR_ERR_ARG, "noise_profile_loss: null pointer");
    PSSR_CHECK(images > 0 && per_image > 0 && width > 0, PSSR_ERR_ARG, "noise_profile_loss: images, per_image and width must be positive");
    // sum_k (t_k - p_k)^2 <= (2 per_image)^2 must stay below 2^53 for the f64 conversion to be exact
    PSSR_CHECK(per_image <= (1L << 25), PSSR_ERR_ARG, "noise_profile_loss: more than 2^25 values per image");
    hipLaunchKernelGGL(noise_profile_loss_kernel, dim3(images), dim3(256), 0, (hipStream_t)s, (const int*)pred_hist, pred_sum,
                       (const int*)target_hist, target_sum, (long)per_image, width, loss, terms);
    hipLaunchKernelGGL(noise_profile_mean_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, (const double*)loss, images, mean);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}
