// Soft histogram GradHist (pssr/models/_blocks.py:94-112) forward / backward, and the small kernels of the crappifier loss around it
// (pssr/train.py:388-402: profiles, strided subsample, mean squared histogram distance, product with the SSIM term) and of
// train_crappifier's gradient clipping (pssr/train.py:244).
//
// Per image b over its N = C*H*W values x_i, with delta = (hi - lo) / bins, c_k = lo + delta * (k + 1/2) (rounded as the reference's fp32
// tensor arithmetic rounds it), s_k(x) = sigmoid(sigma * (x - c_k)), s_{-1} = 1:
//   forward   h[b, j] = sum_i (s_{j-1}(x_i) - s_j(x_i)),  j = 0 .. bins-1          (every pixel differenced before the sum, as the reference)
//   backward  dx_i    = sigma * sum_k s_k (1 - s_k) (g[b, k+1] [k+1 < bins] - g[b, k])
//
// Forward: one thread per bin, the image's pixels staged through LDS in tiles of HIST_TILE (256: many short
// workgroups, so the few waves whose bins hold the mass do not serialise the launch); a workgroup covers 256 bins of one image and a
// fixed strided subset of its tiles, adds its f32 terms in double and writes one partial row rounded to f32 (no atomics);
// hist_reduce_kernel adds the partial rows in workgroup order in double.  Workspace: pairs * batch * HIST_MAX_WG * bins floats,
// independent of N.  Two runs give the same bits.
// Skipped work (per wave of 64 bins [j0, j1), decided for each pixel, uniform over the wave):
//   * x >= c_{j1-1} + 19 / sigma: every s_k of the wave (k = j0-1 .. j1-1) is exactly 1.0f (sigma (x - c) >= 18 > 17.4, where
//     exp(-z) is below half an ulp of 1), so every term is exactly 0 -- nothing is lost;
//   * j0 > 0 and x <= c_{j0-1} - 31 / sigma: every term is at most s_{j0-1}(x) <= e^-30, and the terms of ALL skipped bins above x add up
//     (telescoping) to at most e^-30 ~ 9.4e-14 per pixel, i.e. at most 9.4e-14 * N absolute per image summed over every bin.
//     The wave that holds bin 0 has no lower window: s_{-1} = 1 does not decay, so x = -inf adds its 1 to bin 0 as in the reference.
// The window is set in x by 1 / sigma, so a small sigma (wide sigmoids) keeps every bin of the range active.
// Non-finite pixels follow torch: NaN passes both window tests and makes its image's row NaN; +inf adds 0, -inf adds 1 to bin 0.
// Backward: one thread per pixel, the combined gradient G_k = g[k+1] [k+1 < bins] - g[k] in LDS, k restricted to
// sigma (x - c_k) in [-31, 19]: above, s_k(1 - s_k) is exactly 0; below, the dropped sum is at most
// sigma * max|G| * e^-30 / (1 - e^-(sigma delta)) per pixel.  A NaN x gives dx = NaN (0 under PSSR_HIST_CLAMP when xa itself is NaN:
// torch.clamp's gradient); x = +-inf gives 0.
#include "common.h"

#define HIST_TILE 256
#define HIST_MAX_WG 64
#define HIST_HI_Z 19.f
#define HIST_LO_Z 31.f

namespace {

__device__ __forceinline__ float hist_center(int k, float lo, float delta) {
#pragma clang fp contract(off)
    // torch: float(lo) + delta * (arange(bins).float() + 0.5): an fp32 multiply then an fp32 add.  The pragma keeps them apart:
    // __fmul_rn / __fadd_rn are plain operators to the compiler, and fused into one FMA (one rounding) they give another centre
    // wherever delta * (k + 1/2) is inexact (1000 bins over 512: off by up to 3e-5, 1e-4 in sigma (x - c))
    const float p = delta * ((float)k + 0.5f);
    return lo + p;
}

__device__ __forceinline__ float hist_sig(float x, float c, float sigma) {
    const float z = __fmul_rn(__fsub_rn(x, c), sigma);
    return __builtin_amdgcn_rcpf(1.f + expf(-z));        // v_rcp_f32 (1 ulp); exactly 1.0f when exp(-z) < half an ulp of 1
}

// torch.clamp: a NaN stays NaN (fminf / fmaxf alone would return a bound)
__device__ __forceinline__ float clamp_nan(float v, float lo, float hi) { return v != v ? v : fminf(fmaxf(v, lo), hi); }

__device__ __forceinline__ float load_x(const float* a, const float* b, long i, int clamp_a) {
    float v = a[i];
    if (clamp_a) v = clamp_nan(v, 0.f, 255.f);
    return b ? __fsub_rn(v, b[i]) : v;
}

struct HistPairs {
    const float* a[2];
    const float* b[2];
    int clamp_a0;
};

// grid (nwg, batch, pairs * chunks), block 256
__global__ __launch_bounds__(256) void hist_fwd_kernel(HistPairs in, float* __restrict__ work, long n, int bins, int chunks, float lo,
                                                       float delta, float sigma) {
    __shared__ float xs[HIST_TILE];
    const int nwg = gridDim.x, wg = blockIdx.x, b = blockIdx.y;
    const int pair = blockIdx.z / chunks, chunk = blockIdx.z % chunks;
    const float* a = in.a[pair];
    const float* bb = in.b[pair];
    const int clamp_a = pair == 0 ? in.clamp_a0 : 0;
    a += (long)b * n;
    if (bb) bb += (long)b * n;
    const int j = chunk * 256 + threadIdx.x;
    // the wave's bins [j0, j1) and its active x-window
    const int j0 = chunk * 256 + (threadIdx.x & ~63);
    const int j1 = min(j0 + 64, bins);
    const float x_hi = j0 < bins ? hist_center(j1 - 1, lo, delta) + HIST_HI_Z / sigma : -INFINITY;
    const float x_lo = j0 > 0 ? hist_center(j0 - 1, lo, delta) - HIST_LO_Z / sigma : -INFINITY;
    const float c_j = hist_center(j, lo, delta), c_jm = hist_center(j - 1, lo, delta);
    double acc = 0.0;       // not float: a run of equal pixels (clamped or integer profiles) adds one term again and again, and the
                            // roundings of a growing f32 sum then share a sign (8e-5 of 210 for 226 pixels at 255)
    const long ntiles = (n + HIST_TILE - 1) / HIST_TILE;
    for (long t = wg; t < ntiles; t += nwg) {
        const long base = t * HIST_TILE;
        const int cnt = (int)min((long)HIST_TILE, n - base);
        __syncthreads();
        for (int i = threadIdx.x; i < cnt; i += 256) xs[i] = load_x(a, bb, base + i, clamp_a);
        __syncthreads();
        if (j0 >= bins) continue;
        for (int i = 0; i < cnt; ++i) {
            const float x = xs[i];
            if (x >= x_hi || (j0 > 0 && x <= x_lo)) continue;       // wave-uniform; the wave of bin 0 has no lower window (x = -inf counts)
            const float sj = hist_sig(x, c_j, sigma);
            const float sm = j == 0 ? 1.f : hist_sig(x, c_jm, sigma);
            acc += (double)(sm - sj);
        }
    }
    if (j < bins) work[(((long)pair * gridDim.y + b) * nwg + wg) * bins + j] = (float)acc;
}

// h[pair][b][j] = sum over workgroups, in workgroup order, in double
__global__ __launch_bounds__(256) void hist_reduce_kernel(const float* __restrict__ work, float* __restrict__ h0, float* __restrict__ h1,
                                                          int batch, int nwg, int bins) {
    const long idx = blockIdx.x * 256L + threadIdx.x;
    const long per = (long)batch * bins;
    if (idx >= 2 * per) return;
    const int pair = (int)(idx / per);
    float* h = pair == 0 ? h0 : h1;
    if (!h) return;
    const long r = idx % per;
    const int b = (int)(r / bins), j = (int)(r % bins);
    const float* w = work + (((long)pair * batch + b) * nwg) * bins + j;
    double s = 0.0;
    for (int k = 0; k < nwg; ++k) s += (double)w[(long)k * bins];
    h[r] = (float)s;
}

// grid (ceil(n / 256), batch), block 256; LDS: G[bins]
__global__ __launch_bounds__(256) void hist_bwd_kernel(const float* __restrict__ xa, const float* __restrict__ xb, const float* __restrict__ g,
                                                       const float* __restrict__ g_ref, const float* __restrict__ dev_scale, float g_scale,
                                                       float* __restrict__ dx, long n, int bins, float lo, float delta, float sigma, int flags) {
    extern __shared__ float G[];
    const int b = blockIdx.y;
    const float sc = g_scale * (dev_scale ? dev_scale[0] : 1.f);
    const float* gb = g + (long)b * bins;
    const float* rb = g_ref ? g_ref + (long)b * bins : nullptr;
    for (int k = threadIdx.x; k < bins; k += 256) {
        const float gk = (rb ? gb[k] - rb[k] : gb[k]) * sc;
        const float gn = k + 1 < bins ? (rb ? gb[k + 1] - rb[k + 1] : gb[k + 1]) * sc : 0.f;
        G[k] = gn - gk;
    }
    __syncthreads();
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= n) return;
    const long gi = (long)b * n + i;
    const int clamp_a = flags & PSSR_HIST_CLAMP;
    const float a_raw = xa[gi];
    const float x = load_x(xa, xb, gi, clamp_a);
    // k window: sigma (x - c_k) in [-HIST_LO_Z, HIST_HI_Z]
    float klo_f = (x - HIST_HI_Z / sigma - lo) / delta - 1.5f, khi_f = (x + HIST_LO_Z / sigma - lo) / delta + 0.5f;
    klo_f = fminf(fmaxf(floorf(klo_f), 0.f), (float)bins);
    khi_f = fminf(fmaxf(floorf(khi_f), -1.f), (float)(bins - 1));
    const int klo = (int)klo_f, khi = (int)khi_f;
    float s = 0.f;
    for (int k = klo; k <= khi; ++k) {
        const float sk = hist_sig(x, hist_center(k, lo, delta), sigma);
        s += sk * (1.f - sk) * G[k];
    }
    if (x != x) s = x;                                  // the k window of a NaN is empty; torch's sum is NaN
    float d = sigma * s;
    if (flags & PSSR_HIST_ACCUMULATE) d += dx[gi];
    if (clamp_a && !(a_raw >= 0.f && a_raw <= 255.f)) d = 0.f;        // torch.clamp's gradient: min <= x <= max, inclusive
    dx[gi] = d;
}

// pred = clamp?(lr_hat) - ds_hr, target = lr - ds_hr
__global__ __launch_bounds__(256) void profiles_kernel(const float* __restrict__ lr_hat, const float* __restrict__ lr, const float* __restrict__ ds,
                                                       float* __restrict__ pred, float* __restrict__ target, long n, int clamp) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float d = ds[i];
        pred[i] = load_x(lr_hat, nullptr, i, clamp) - d;
        target[i] = lr[i] - d;
    }
}

// dst[p, y, x] = src[p, y * s, x * s]
__global__ __launch_bounds__(256) void subsample_kernel(const float* __restrict__ src, float* __restrict__ dst, long planes, int H, int W, int s,
                                                        int h, int w) {
    const long total = planes * h * w;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long p = i / ((long)h * w);
        const int r = (int)(i % ((long)h * w));
        const int y = r / w, x = r % w;
        dst[i] = src[(p * H + (long)y * s) * W + (long)x * s];
    }
}

// one workgroup: D = sum (p - t)^2 * dist_scale (double, fixed tree), out = [D * P, D, P]
__global__ __launch_bounds__(256) void loss_combine_kernel(const float* __restrict__ p, const float* __restrict__ t, long m,
                                                           const float* __restrict__ ssim_loss, float dist_scale, float* __restrict__ out) {
    __shared__ double part[256];
    double s = 0.0;
    for (long i = threadIdx.x; i < m; i += 256) {
        const double d = (double)p[i] - (double)t[i];
        s += d * d;
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float D = (float)(part[0] * (double)dist_scale);
        const float P = ssim_loss[0];
        out[0] = D * P;
        out[1] = D;
        out[2] = P;
    }
}

// parts = [L, D, P], dL -> out = [D * dL, P * dL]
__global__ void loss_bwd_scalars_kernel(const float* __restrict__ parts, const float* __restrict__ dL, float* __restrict__ out) {
    if (threadIdx.x == 0) {
        out[0] = parts[1] * dL[0];
        out[1] = parts[2] * dL[0];
    }
}

__global__ __launch_bounds__(256) void clamp_kernel(const float* __restrict__ x, float* __restrict__ y, long n, float lo, float hi) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) y[i] = clamp_nan(x[i], lo, hi);
}

unsigned grid_1d(long n, long cap = 4096) {
    long g = (n + 255) / 256;
    if (g > cap) g = cap;
    return (unsigned)(g < 1 ? 1 : g);
}

int hist_wgs(long n) {
    const long tiles = (n + HIST_TILE - 1) / HIST_TILE;
    return (int)(tiles < HIST_MAX_WG ? tiles : HIST_MAX_WG);
}

}  // namespace

extern "C" int64_t pssr_gradhist_workspace_bytes(int batch, int64_t n, int bins) {
    if (batch <= 0 || n <= 0 || bins <= 0) return 0;
    return (int64_t)2 * batch * hist_wgs(n) * bins * (int64_t)sizeof(float);
}

extern "C" int pssr_gradhist_fwd(const float* a0, const float* b0, const float* a1, const float* b1, float* h0, float* h1, float* workspace,
                                 int64_t workspace_bytes, int batch, int64_t n, int bins, float lo, float hi, float sigma, int flags,
                                 pssr_stream_t s) {
    PSSR_CHECK(a0 && h0 && workspace && batch > 0 && n > 0 && bins > 0 && bins <= PSSR_HIST_MAX_BINS, PSSR_ERR_ARG, "gradhist_fwd: bad args (bins 1 .. PSSR_HIST_MAX_BINS)");
    PSSR_CHECK((a1 == nullptr) == (h1 == nullptr) && (a1 != nullptr || b1 == nullptr), PSSR_ERR_ARG, "gradhist_fwd: second pair incomplete");
    PSSR_CHECK(hi > lo && sigma > 0.f, PSSR_ERR_ARG, "gradhist_fwd: needs range[1] > range[0] and sigma > 0");
    PSSR_CHECK(workspace_bytes >= pssr_gradhist_workspace_bytes(batch, n, bins), PSSR_ERR_ARG, "gradhist_fwd: workspace too small");
    PSSR_CHECK(batch <= 65535, PSSR_ERR_ARG, "gradhist_fwd: batch above 65535");
    const int pairs = a1 ? 2 : 1, chunks = (bins + 255) / 256, nwg = hist_wgs(n);
    HistPairs in;
    in.a[0] = a0; in.b[0] = b0; in.a[1] = a1; in.b[1] = b1;
    in.clamp_a0 = (flags & PSSR_HIST_CLAMP) ? 1 : 0;
    const float delta = (float)(((double)hi - (double)lo) / (double)bins);
    hipLaunchKernelGGL(hist_fwd_kernel, dim3(nwg, batch, pairs * chunks), dim3(256), 0, (hipStream_t)s, in, workspace, (long)n, bins, chunks,
                       lo, delta, sigma);
    const long outs = 2L * batch * bins;
    hipLaunchKernelGGL(hist_reduce_kernel, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, (hipStream_t)s, (const float*)workspace, h0,
                       pairs == 2 ? h1 : (float*)nullptr, batch, nwg, bins);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

extern "C" int pssr_gradhist_bwd(const float* xa, const float* xb, const float* g, const float* g_ref, const float* dev_scale, float g_scale,
                                 float* dx, int batch, int64_t n, int bins, float lo, float hi, float sigma, int flags, pssr_stream_t s) {
    PSSR_CHECK(xa && g && dx && batch > 0 && n > 0 && bins > 0 && bins <= PSSR_HIST_MAX_BINS, PSSR_ERR_ARG, "gradhist_bwd: bad args (bins 1 .. PSSR_HIST_MAX_BINS)");
    PSSR_CHECK(hi > lo && sigma > 0.f, PSSR_ERR_ARG, "gradhist_bwd: needs range[1] > range[0] and sigma > 0");
    PSSR_CHECK(batch <= 65535 && (n + 255) / 256 <= 0x7fffffffL, PSSR_ERR_ARG, "gradhist_bwd: shape too large");
    const float delta = (float)(((double)hi - (double)lo) / (double)bins);
    hipLaunchKernelGGL(hist_bwd_kernel, dim3((unsigned)((n + 255) / 256), batch), dim3(256), bins * sizeof(float), (hipStream_t)s, xa, xb, g,
                       g_ref, dev_scale, g_scale, dx, (long)n, bins, lo, delta, sigma, flags);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

extern "C" int pssr_crappifier_profiles(const float* lr_hat, const float* lr, const float* ds_hr, float* pred, float* target, int64_t n,
                                        int flags, pssr_stream_t s) {
    PSSR_CHECK(lr_hat && lr && ds_hr && pred && target && n > 0, PSSR_ERR_ARG, "crappifier_profiles: bad args");
    hipLaunchKernelGGL(profiles_kernel, dim3(grid_1d(n)), dim3(256), 0, (hipStream_t)s, lr_hat, lr, ds_hr, pred, target, (long)n,
                       (flags & PSSR_HIST_CLAMP) ? 1 : 0);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

extern "C" int pssr_subsample_f32(const float* src, float* dst, int64_t planes, int h_in, int w_in, int stride, pssr_stream_t s) {
    PSSR_CHECK(src && dst && planes > 0 && h_in > 0 && w_in > 0 && stride > 0, PSSR_ERR_ARG, "subsample_f32: bad args");
    const int h = (h_in + stride - 1) / stride, w = (w_in + stride - 1) / stride;
    hipLaunchKernelGGL(subsample_kernel, dim3(grid_1d(planes * h * w)), dim3(256), 0, (hipStream_t)s, src, dst, (long)planes, h_in, w_in, stride,
                       h, w);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

extern "C" int pssr_crappifier_loss_combine(const float* pred_hist, const float* target_hist, int64_t m, const float* ssim_loss,
                                            float dist_scale, float* out, pssr_stream_t s) {
    PSSR_CHECK(pred_hist && target_hist && ssim_loss && out && m > 0, PSSR_ERR_ARG, "crappifier_loss_combine: bad args");
    hipLaunchKernelGGL(loss_combine_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, pred_hist, target_hist, (long)m, ssim_loss, dist_scale, out);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

extern "C" int pssr_crappifier_loss_bwd_scalars(const float* parts, const float* grad_out, float* out, pssr_stream_t s) {
    PSSR_CHECK(parts && grad_out && out, PSSR_ERR_ARG, "crappifier_loss_bwd_scalars: bad args");
    hipLaunchKernelGGL(loss_bwd_scalars_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, parts, grad_out, out);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

extern "C" int pssr_clamp_f32(const float* x, float* y, int64_t n, float lo, float hi, pssr_stream_t s) {
    PSSR_CHECK(x && y && n > 0 && lo <= hi, PSSR_ERR_ARG, "clamp_f32: bad args");
    hipLaunchKernelGGL(clamp_kernel, dim3(grid_1d(n)), dim3(256), 0, (hipStream_t)s, x, y, (long)n, lo, hi);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}
