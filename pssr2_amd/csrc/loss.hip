// SSIM / MS-SSIM + Gaussian-weighted L1 loss (pssr/util.py:10-52 -> pytorch_msssim), forward and
// backward, on f32 NCHW planes.  HBM-bound: every level reads its two maps once per pass; the five
// Gaussian-filtered maps (mu_x, mu_y, E[x^2], E[y^2], E[xy]) exist only in LDS.
//
// forward  (per level): tile of TS x TS *valid* positions; separable 11-tap filter through LDS;
//                       per-plane f64 sums of the cs map and the ssim map (+ weighted |x-y| at level 0).
// weights  (tiny)     : loss value and d loss / d(map element) per plane and level, on device.
// backward (per level): recompute the filtered maps on a (TS+10)^2 halo, form the three adjoint maps
//                       (wrt mu_x, E[x^2], E[xy]), apply the transposed filter, add the avg-pool
//                       gradient arriving from the coarser level and the L1 term.
//
// Six level kernels: the generic pair (ssim_fwd_kernel / ssim_bwd_kernel: any odd window up to MAXW, one output per thread -- the
// readable form of the algorithm), the register-blocked pair for a compile-time window (ssim_fwd_k / ssim_bwd_k) and the training
// pair (ssim_fwd_adj_k / ssim_bwd_adj_k).  Every step that more than one of them performs is one helper below.
#include "common.h"

namespace {

constexpr int TS = 32;       // tile side
constexpr int MAXW = 33;     // largest supported window
constexpr int SEG = 8, NS = TS / SEG;      // register-blocked kernels: outputs per thread of a 1-D pass, segments per tile row / column

struct Win { float g[MAXW]; int k; };

// ------------------------------------------------------------------------------------------------
// LDS layouts (in floats): each kernel lays its dynamic LDS out by one of these and its launcher sizes it from the same one.
struct FwdLds {      // ssim_fwd_kernel: xs, ys [IN][IN]; hp [5][IN][TS]
    int halo, IN, ys, hp, floats;
    __host__ __device__ explicit FwdLds(int k) : halo(k - 1), IN(TS + halo), ys(IN * IN), hp(2 * IN * IN), floats(hp + 5 * IN * TS) {}
};
struct BwdLds {      // ssim_bwd_kernel: xs, ys [IN][IN]; hp [5][IN][AD], later th [3][AD][TS]; ad [3][AD][AD]
    int halo, AD, IN, ys, hp, ad, floats;
    __host__ __device__ explicit BwdLds(int k)
        : halo(k - 1), AD(TS + halo), IN(TS + 2 * halo), ys(IN * IN), hp(2 * IN * IN), ad(hp + 5 * IN * AD), floats(ad + 3 * AD * AD) {}
};
template <int K, int MAPS> struct FwdGeom {      // ssim_fwd_k (MAPS = 5), ssim_fwd_adj_k (MAPS = 1): xs, ys [IN][IN]; hp [MAPS][IN][HPW]
    static constexpr int halo = K - 1, IN = TS + halo;
    static constexpr int HPW = TS + 1;           // row pitch of the h-pass images: the 8 rows a lane group writes fall on different banks
    static constexpr int YS = IN * IN, HP = 2 * IN * IN, FLOATS = HP + MAPS * IN * HPW;
};
template <int K> struct BwdAdjGeom {             // ssim_bwd_adj_k: ad [AD][ADC]; th [THR][THW]
    static constexpr int halo = K - 1, AD = TS + halo;
    static constexpr int ADC = AD + 1;                            // row pitch of the adjoint tile (odd: the rows of a lane group on different banks)
    static constexpr int THR = AD + SEG, THW = TS + 1;
    static constexpr int NL = (AD * AD + 255) / 256;              // tile elements per thread
    static constexpr int TH = AD * ADC, FLOATS = TH + THR * THW;
};
template <int K> struct BwdGeom {                // ssim_bwd_k: xs, ys [IN][INP]; hp [5][IN][ADP], later th [3][THR][TS]; ad [3][AD][AD] over xs / ys
    static constexpr int halo = K - 1, AD = TS + halo, IN = TS + 2 * halo;
    static constexpr int SA = 7, NSA = (AD + SA - 1) / SA;        // segments over the AD-wide adjoint region (42 = 6 x 7 for K = 11)
    static constexpr int ADP = NSA * SA;                          // padded row length of the h-pass image
    static constexpr int INP = IN + SA;                           // row pitch with room for the last (partial) segment's window
    static constexpr int THR = AD + SEG;
    static constexpr int YS = IN * INP, HP = 2 * IN * INP, FLOATS = HP + 5 * IN * ADP;
    static_assert(3 * AD * AD <= 2 * IN * INP, "adjoint maps must fit into the input images");
    static_assert(3 * THR * TS <= 5 * IN * ADP, "transposed h-pass images must fit into the h-pass images");
};

// ------------------------------------------------------------------------------------------------
// Steps shared by the level kernels.  Small structs go by value; Win goes by reference so that the taps stay in scalar registers.

// The x / y tile at image position (gy0, gx0) -> xs / ys: `rows` rows of `pitch` floats, the first `cols` of each from the image,
// zero outside the image and in the pad columns.  Forward tiles start at the tile origin, backward tiles `halo` before it.
// in_mul = 1 / divisor in f32: the loss of x / divisor and y / divisor without materialising the quotients -- train_paired passes
// images / 255, two full passes over 33 MB tensors per step and a third one for the gradient; torch divides a tensor by a scalar
// as a multiplication by the f32 reciprocal, so do these kernels.
__device__ __forceinline__ void stage_tile(const float* __restrict__ xp, const float* __restrict__ yp, int H, int W, int gy0, int gx0,
                                           int rows, int cols, int pitch, float in_mul, float* xs, float* ys, int tid) {
    for (int i = tid; i < rows * pitch; i += 256) {
        const int r = i / pitch, c = i % pitch;
        const int gy = gy0 + r, gx = gx0 + c;
        float xv = 0.f, yv = 0.f;
        if (c < cols && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) {
            xv = __fmul_rn(xp[(long)gy * W + gx], in_mul); yv = __fmul_rn(yp[(long)gy * W + gx], in_mul);
        }
        xs[i] = xv; ys[i] = yv;
    }
}

// The helpers that walk the window take its length as K where it is a compile-time constant (loops unrolled), else (K = 0) from
// win.k (loops left rolled).
template <int K> __device__ __forceinline__ float win_sum(const Win& win) {
    constexpr int UNR = K ? K : 1;
    const int k = K ? K : win.k;
    float s = 0.f;
#pragma unroll UNR
    for (int t = 0; t < k; ++t) s += win.g[t];
    return s;
}

// Border weight of the Gaussian-weighted L1 term along one axis: the mass of the window centred on coordinate p that lies inside
// [0, n).  For an interior p that is the whole window sum `wsum`, added in the same order as the clipped sum, so the same float.
template <int K> __device__ __forceinline__ float border_mass(const Win& win, float wsum, int p, int n) {
    constexpr int UNR = K ? K : 1;
    const int k = K ? K : win.k, r5 = k / 2;
    float s = wsum;
    if (p < r5 || p >= n - r5) {
        s = 0.f;
#pragma unroll UNR
        for (int t = 0; t < k; ++t) { const int q = p + t - r5; if (q >= 0 && q < n) s += win.g[t]; }
    }
    return s;
}

// L1 partial of this thread over the TS x TS pixels at the origin of a staged forward tile (its origin is the tile origin): each
// pixel once, since the tiles partition the image when the grid covers it (see level_grid)
template <int K> __device__ __forceinline__ float l1_tile(const Win& win, const float* xs, const float* ys, int pitch, int oy0, int ox0,
                                                          int H, int W, int tid) {
    const float wsum = win_sum<K>(win);
    float l1 = 0.f;
    for (int i = tid; i < TS * TS; i += 256) {
        const int r = i / TS, c = i % TS;
        const int gy = oy0 + r, gx = ox0 + c;
        if (gy < H && gx < W) {
            const float sy = border_mass<K>(win, wsum, gy, H), sx = border_mass<K>(win, wsum, gx, W);
            l1 += fabsf(xs[r * pitch + c] - ys[r * pitch + c]) * sy * sx;
        }
    }
    return l1;
}

// SSIM at one position from the five filtered values: cs = contrast-structure term, lum = luminance term, with their denominators
struct SsimPt { float cs, lum, Dcs, Dl; };
__device__ __forceinline__ SsimPt ssim_point(float mx, float my, float exx, float eyy, float exy, float C1, float C2) {
    const float sxx = exx - mx * mx, syy = eyy - my * my, sxy = exy - mx * my;
    SsimPt p;
    p.Dcs = sxx + syy + C2; p.cs = (2.f * sxy + C2) / p.Dcs;
    p.Dl = mx * mx + my * my + C1; p.lum = (2.f * mx * my + C1) / p.Dl;
    return p;
}

// The derivatives of the cs map (use_ssim = 0) or the ssim map (1) at that position wrt (mu_x, E[x^2], E[xy]), times `wt` as the
// leading factor of each product.  Two routes use it, and they round differently: ssim_bwd_kernel / ssim_bwd_k pass the plane's
// upstream weight and so compute (wt * lum) * d; ssim_fwd_adj_k passes 1 and stores lum * d per unit of weight, from which
// ssim_bwd_adj_k computes wt * (lum * d).
struct SsimAdj { float a, b, cc; };
__device__ __forceinline__ SsimAdj ssim_adjoint(const SsimPt p, float mx, float my, int use_ssim, float wt) {
    const float dcs_dmx = 2.f * (p.cs * mx - my) / p.Dcs, dcs_dexx = -p.cs / p.Dcs, dcs_dexy = 2.f / p.Dcs;
    SsimAdj d;
    if (use_ssim) {
        const float dl_dmx = 2.f * (my - p.lum * mx) / p.Dl;
        d.a = wt * (p.lum * dcs_dmx + p.cs * dl_dmx); d.b = wt * p.lum * dcs_dexx; d.cc = wt * p.lum * dcs_dexy;
    } else {
        d.a = wt * dcs_dmx; d.b = wt * dcs_dexx; d.cc = wt * dcs_dexy;
    }
    return d;
}

// Sum of the three forward partials over the workgroup; true in the one thread that then holds the sums in (cs, ss, l1)
__device__ __forceinline__ bool block_sum3(float& cs, float& ss, float& l1, int tid) {
    __shared__ float red[3][256];
    red[0][tid] = cs; red[1][tid] = ss; red[2][tid] = l1;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; red[2][tid] += red[2][tid + o]; }
        __syncthreads();
    }
    if (tid != 0) return false;
    cs = red[0][0]; ss = red[1][0]; l1 = red[2][0];
    return true;
}

// ... into the plane's f64 sums with plain atomics (ssim_fwd_kernel, ssim_fwd_k; ssim_fwd_adj_k adds striped exact pieces instead)
__device__ __forceinline__ void add_sums(double* sums, double* l1_sum, int plane, float cs, float ss, float l1) {
    atomicAdd(sums + plane * 2, (double)cs);
    atomicAdd(sums + plane * 2 + 1, (double)ss);
    if (l1_sum) atomicAdd(l1_sum, (double)l1);
}

// What the backward kernels add to a pixel's filtered gradient g: the gradient of the coarser level through the 2 x 2 average
// pooling (padding = size % 2) and the L1 term l1_coef * border weight * sign(x - y)
struct PixTerms { const float* dc; int WC, H, W; float l1c, wsum; };
template <int K> __device__ __forceinline__ PixTerms pix_terms(const Win& win, const float* dcoarse, int plane, int HC, int WC, int H, int W,
                                                               const float* l1_coef_p) {
    return PixTerms{dcoarse ? dcoarse + (long)plane * HC * WC : nullptr, WC, H, W, l1_coef_p ? l1_coef_p[0] : 0.f, win_sum<K>(win)};
}
template <int K> __device__ __forceinline__ float pixel_grad(const PixTerms e, const Win& win, float g, float xv, float yv, int gy, int gx) {
    if (e.dc) {
        const int cy = (gy + (e.H & 1)) >> 1, cx = (gx + (e.W & 1)) >> 1;
        g += 0.25f * e.dc[(long)cy * e.WC + cx];
    }
    if (e.l1c != 0.f) {
        const float sy = border_mass<K>(win, e.wsum, gy, e.H), sx = border_mass<K>(win, e.wsum, gx, e.W);
        const float d = xv - yv;
        g += e.l1c * sy * sx * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
    }
    return g;
}

// Register-blocked 1-D passes for a compile-time window K: a thread produces N consecutive outputs from a sliding window of
// N + K - 1 inputs held in registers (6x fewer LDS reads than one output per thread), all tap loops unrolled (window weights come
// from scalar registers).  Same LDS images and arithmetic order per output as the generic kernels.
template <int K, int N, int NQ>
__device__ __forceinline__ void fir_seg(const float (*v)[N + K - 1], const Win& win, float (*out)[N]) {
#pragma unroll
    for (int o = 0; o < N; ++o)
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            float s = 0.f;
#pragma unroll
            for (int t = 0; t < K; ++t) s = fmaf(win.g[t], v[q][o + t], s);
            out[q][o] = s;
        }
}
// transposed, one output: sum_t g[t] * v[halo - t], where v[j] is the adjoint value `halo - j` before the output.  Per output, not
// per segment as fir_seg: with the N results collected in an array first, the vertical pass of ssim_bwd_adj_k took 2 VGPRs more
template <int K> __device__ __forceinline__ float fir_t(const float* v, const Win& win) {
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < K; ++t) s = fmaf(win.g[t], v[K - 1 - t], s);
    return s;
}
// the five maps to filter (x, y, x^2, y^2, xy) on a row segment of the staged tile
template <int N> __device__ __forceinline__ void moments_seg(const float* xr, const float* yr, float (*v)[N]) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const float a = xr[j], b = yr[j];
        v[0][j] = a; v[1][j] = b; v[2][j] = a * a; v[3][j] = b * b; v[4][j] = a * b;
    }
}

// The two filter passes of the generic pair.  Horizontal: the five maps (x, y, x^2, y^2, xy) filtered along the `rows` rows of the
// staged tile (row pitch `pitch`), `cols` outputs per row -> hp [5][rows][cols].  Vertical: the five filtered values at (r, c) from hp.
__device__ __forceinline__ void hpass5(const Win& win, const float* xs, const float* ys, int pitch, int rows, int cols, float* hp, int tid) {
    for (int i = tid; i < rows * cols; i += 256) {
        const int r = i / cols, c = i % cols;
        float mx = 0, my = 0, xx = 0, yy = 0, xy = 0;
        for (int t = 0; t < win.k; ++t) {
            const float a = xs[r * pitch + c + t], b = ys[r * pitch + c + t], gw = win.g[t];
            mx = fmaf(gw, a, mx); my = fmaf(gw, b, my);
            xx = fmaf(gw, a * a, xx); yy = fmaf(gw, b * b, yy); xy = fmaf(gw, a * b, xy);
        }
        hp[0 * rows * cols + i] = mx; hp[1 * rows * cols + i] = my; hp[2 * rows * cols + i] = xx; hp[3 * rows * cols + i] = yy; hp[4 * rows * cols + i] = xy;
    }
}
__device__ __forceinline__ void vpass5(const Win& win, const float* hp, int rows, int cols, int r, int c, float (&m)[5]) {
#pragma unroll
    for (int q = 0; q < 5; ++q) m[q] = 0.f;
    for (int t = 0; t < win.k; ++t) {
        const float gw = win.g[t];
#pragma unroll
        for (int q = 0; q < 5; ++q) m[q] = fmaf(gw, hp[q * rows * cols + (r + t) * cols + c], m[q]);
    }
}

// ------------------------------------------------------------------------------------------------
// Generic pair: any window, one output per thread and pass.
__global__ __launch_bounds__(256) void ssim_fwd_kernel(const float* __restrict__ X, const float* __restrict__ Y, int H, int W,
                                                       Win win, float C1, float C2, double* sums /*[planes][2]*/,
                                                       double* l1_sum /*nullable*/) {
    extern __shared__ float lds[];
    const FwdLds G(win.k);
    const int halo = G.halo, IN = G.IN;
    float* xs = lds;
    float* ys = lds + G.ys;
    float* hp = lds + G.hp;
    const int plane = blockIdx.z;
    const int oy0 = blockIdx.y * TS, ox0 = blockIdx.x * TS;       // valid-map tile origin == input origin
    const int VH = H - halo, VW = W - halo;
    const int tid = threadIdx.x;
    stage_tile(X + (long)plane * H * W, Y + (long)plane * H * W, H, W, oy0, ox0, IN, IN, IN, 1.f, xs, ys, tid);
    __syncthreads();
    float l1 = l1_sum ? l1_tile<0>(win, xs, ys, IN, oy0, ox0, H, W, tid) : 0.f;
    hpass5(win, xs, ys, IN, IN, TS, hp, tid);
    __syncthreads();
    float cs_acc = 0.f, ss_acc = 0.f;
    for (int i = tid; i < TS * TS; i += 256) {
        const int r = i / TS, c = i % TS;
        if (oy0 + r >= VH || ox0 + c >= VW) continue;
        float m[5];
        vpass5(win, hp, IN, TS, r, c, m);
        const SsimPt p = ssim_point(m[0], m[1], m[2], m[3], m[4], C1, C2);
        cs_acc += p.cs; ss_acc += p.lum * p.cs;
    }
    if (block_sum3(cs_acc, ss_acc, l1, tid)) add_sums(sums, l1_sum, plane, cs_acc, ss_acc, l1);
}

__global__ __launch_bounds__(256) void ssim_bwd_kernel(const float* __restrict__ X, const float* __restrict__ Y, int H, int W, Win win,
                                                       float C1, float C2, const float* __restrict__ wts /*[planes]*/, int use_ssim,
                                                       const float* __restrict__ dcoarse, int HC, int WC,
                                                       const float* l1_coef_p, float* __restrict__ dX) {
    // output tile: TS x TS pixels at (qy0, qx0); adjoint maps needed at valid positions p in [q0-halo, q0+TS-1]
    extern __shared__ float lds[];
    const BwdLds G(win.k);
    const int k = win.k, halo = G.halo, AD = G.AD, IN = G.IN;
    float* xs = lds;                       // [IN][IN]
    float* ys = lds + G.ys;                // [IN][IN]
    float* hp = lds + G.hp;                // [5][IN][AD]  (horizontal pass)  -> later reused for adjoint h-pass [3][AD][TS]
    float* ad = lds + G.ad;                // [3][AD][AD]  adjoint maps a, b, c
    const int plane = blockIdx.z;
    const int qy0 = blockIdx.y * TS, qx0 = blockIdx.x * TS;
    const int VH = H - halo, VW = W - halo;
    const int tid = threadIdx.x;
    const float wt = wts[plane];
    // inputs rows [qy0-halo, qy0+TS+halo)
    stage_tile(X + (long)plane * H * W, Y + (long)plane * H * W, H, W, qy0 - halo, qx0 - halo, IN, IN, IN, 1.f, xs, ys, tid);
    __syncthreads();
    hpass5(win, xs, ys, IN, IN, AD, hp, tid);      // IN rows, AD cols
    __syncthreads();
    for (int i = tid; i < AD * AD; i += 256) {
        const int r = i / AD, c = i % AD;
        const int py = qy0 - halo + r, px = qx0 - halo + c;     // valid-map position
        SsimAdj d = {0.f, 0.f, 0.f};
        if (py >= 0 && py < VH && px >= 0 && px < VW) {
            float m[5];
            vpass5(win, hp, IN, AD, r, c, m);
            d = ssim_adjoint(ssim_point(m[0], m[1], m[2], m[3], m[4], C1, C2), m[0], m[1], use_ssim, wt);
        }
        ad[0 * AD * AD + i] = d.a; ad[1 * AD * AD + i] = d.b; ad[2 * AD * AD + i] = d.cc;
    }
    __syncthreads();
    // transposed filter, horizontal: out col q gets sum_t g[t] * ad[.., q + halo - t]  (ad col index = p - (q0-halo))
    float* th = hp;                        // [3][AD][TS]
    for (int i = tid; i < AD * TS; i += 256) {
        const int r = i / TS, c = i % TS;
        float s0 = 0, s1 = 0, s2 = 0;
        for (int t = 0; t < k; ++t) {
            const float gw = win.g[t];
            const int src = r * AD + c + halo - t;
            s0 = fmaf(gw, ad[src], s0); s1 = fmaf(gw, ad[AD * AD + src], s1); s2 = fmaf(gw, ad[2 * AD * AD + src], s2);
        }
        th[i] = s0; th[AD * TS + i] = s1; th[2 * AD * TS + i] = s2;
    }
    __syncthreads();
    const PixTerms e = pix_terms<0>(win, dcoarse, plane, HC, WC, H, W, l1_coef_p);
    float* dxp = dX + (long)plane * H * W;
    for (int i = tid; i < TS * TS; i += 256) {
        const int r = i / TS, c = i % TS;
        const int gy = qy0 + r, gx = qx0 + c;
        if (gy >= H || gx >= W) continue;
        float s0 = 0, s1 = 0, s2 = 0;
        for (int t = 0; t < k; ++t) {
            const float gw = win.g[t];
            const int src = (r + halo - t) * TS + c;
            s0 = fmaf(gw, th[src], s0); s1 = fmaf(gw, th[AD * TS + src], s1); s2 = fmaf(gw, th[2 * AD * TS + src], s2);
        }
        const float xv = xs[(r + halo) * IN + c + halo], yv = ys[(r + halo) * IN + c + halo];
        dxp[(long)gy * W + gx] = pixel_grad<0>(e, win, s0 + 2.f * xv * s1 + yv * s2, xv, yv, gy, gx);
    }
}

// ------------------------------------------------------------------------------------------------
// avg_pool2d(kernel 2, stride 2, padding = size % 2, count_include_pad) on planes
__global__ void avgpool_kernel(const float* __restrict__ in0, float* __restrict__ out0, const float* __restrict__ in1, float* __restrict__ out1,
                               int planes, int H, int W, int HO, int WO, float in_mul) {
#pragma clang fp contract(off)          // the scaled inputs are rounded products (what the quotient tensor would hold), not FMA operands
    const float* in = blockIdx.y ? in1 : in0;          // (two tensors per launch: the x and y pyramids of the loss)
    float* out = blockIdx.y ? out1 : out0;
    const int py = H & 1, px = W & 1;
    const long total = (long)planes * HO * WO;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int ox = i % WO, oy = (i / WO) % HO;
        const long pl = i / ((long)WO * HO);
        const float* src = in + pl * H * W;
        float s = 0.f;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int y = 2 * oy - py + dy, x = 2 * ox - px + dx;
                if (y >= 0 && y < H && x >= 0 && x < W) s += __fmul_rn(src[(long)y * W + x], in_mul);      // (a rounded product, as the quotient tensor would hold: no FMA contraction)
            }
        out[i] = 0.25f * s;
    }
}

// loss and upstream weights.  sums: [levels][planes][2] (cs sum, ssim sum); nvalid[l] = valid positions per plane.
__global__ void weights_kernel(const double* sums_in, int levels, int planes, const double* nvalid, const float* lvl_w, int ms,
                               float mix, const double* l1_sum_in, double l1_numel, const float* grad_out,
                               float* loss_out, float* wts /*[levels][planes]*/, float* l1_coef, int stripes, long stripe_stride,
                               double* folded /* [levels * planes * 2 + 1] scratch of the striped entry, else null */) {
    // striped sums (ssim_fwd_adj_k): fold the copies first, in a fixed order -- with one stripe too: that kernel writes every sum as
    // two pieces whatever the stripe count
    const double* sums = sums_in;
    const double* l1_sum = l1_sum_in;
    if (folded) {
        // (fixed order; the loads of a value are independent and issued together: the serial loop cost 24 us on the step's chain)
        const int nvals = levels * planes * 2;
        for (int i = threadIdx.x; i <= nvals; i += 256) {
            const double* src = i < nvals ? sums_in + i : l1_sum_in;
            double t = 0.0;
            if (src) {
                int k = 0;
                for (; k + 8 <= 2 * stripes; k += 8) {
                    double v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) v[u] = src[(long)(k + u) * stripe_stride];
#pragma unroll
                    for (int u = 0; u < 8; ++u) t += v[u];
                }
                for (; k < 2 * stripes; ++k) t += src[(long)k * stripe_stride];
            }
            folded[i] = t;
        }
        __syncthreads();
        sums = folded;
        if (l1_sum_in) l1_sum = folded + nvals;
    }
    __shared__ double acc[256];
    const int tid = threadIdx.x;
    const float go = grad_out ? grad_out[0] : 1.f;
    double local = 0.0;
    for (int p = tid; p < planes; p += 256) {
        if (ms) {
            double prod = 1.0;
            double v[8];
            for (int l = 0; l < levels; ++l) {
                const double mean = sums[((long)l * planes + p) * 2 + (l == levels - 1 ? 1 : 0)] / nvalid[l];
                v[l] = mean > 0 ? mean : 0.0;
                prod *= pow(v[l], (double)lvl_w[l]);
            }
            local += prod;
            for (int l = 0; l < levels; ++l) {
                // d loss / d v_l = -mix/planes * w_l * prod / v_l ; spread over nvalid[l] map elements
                const double d = v[l] > 0 ? -(double)mix / planes * lvl_w[l] * prod / v[l] : 0.0;
                wts[(long)l * planes + p] = (float)(d / nvalid[l] * go);
            }
        } else {
            const double mean = sums[(long)p * 2 + 1] / nvalid[0];
            local += mean;      // nonnegative_ssim=False: no relu on plain SSIM
            wts[p] = (float)(-(double)mix / planes / nvalid[0] * go);
        }
    }
    acc[tid] = local;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) acc[tid] += acc[tid + o]; __syncthreads(); }
    if (tid == 0) {
        double loss = mix * (1.0 - acc[0] / planes);
        double lc = 0.0;
        if (l1_sum) { loss = loss + (1.0 - mix) * l1_sum[0] / l1_numel; lc = (1.0 - mix) / l1_numel * go; }
        else loss = (1.0 - acc[0] / planes);          // mix == 1: the reference skips the L1 branch entirely
        loss_out[0] = (float)loss;
        l1_coef[0] = (float)lc;
    }
}

// ------------------------------------------------------------------------------------------------
// Register-blocked pair for a compile-time window K (see fir_seg).
template <int K>
__global__ __launch_bounds__(256) void ssim_fwd_k(const float* __restrict__ X, const float* __restrict__ Y, int H, int W,
                                                  Win win, float C1, float C2, double* sums, double* l1_sum) {
    using G = FwdGeom<K, 5>;
    constexpr int halo = G::halo, IN = G::IN, HPW = G::HPW;
    extern __shared__ float lds[];
    float* xs = lds;
    float* ys = lds + G::YS;
    float* hp = lds + G::HP;                   // [5][IN][HPW]
    const int plane = blockIdx.z;
    const int oy0 = blockIdx.y * TS, ox0 = blockIdx.x * TS;
    const int VH = H - halo, VW = W - halo;
    const int tid = threadIdx.x;
    stage_tile(X + (long)plane * H * W, Y + (long)plane * H * W, H, W, oy0, ox0, IN, IN, IN, 1.f, xs, ys, tid);
    __syncthreads();
    float l1 = l1_sum ? l1_tile<K>(win, xs, ys, IN, oy0, ox0, H, W, tid) : 0.f;
    // horizontal pass: item = (row, segment of SEG output columns)
    for (int it = tid; it < IN * NS; it += 256) {
        const int r = it / NS, c0 = (it % NS) * SEG;
        float v[5][SEG + K - 1];
        moments_seg<SEG + K - 1>(xs + r * IN + c0, ys + r * IN + c0, v);
        float o[5][SEG];
        fir_seg<K, SEG, 5>(v, win, o);
#pragma unroll
        for (int q = 0; q < 5; ++q)
#pragma unroll
            for (int j = 0; j < SEG; ++j) hp[q * IN * HPW + r * HPW + c0 + j] = o[q][j];
    }
    __syncthreads();
    float cs_acc = 0.f, ss_acc = 0.f;
    // vertical pass: item = (column, segment of SEG output rows)
    for (int it = tid; it < TS * NS; it += 256) {
        const int c = it % TS, r0 = (it / TS) * SEG;
        float v[5][SEG + K - 1];
#pragma unroll
        for (int q = 0; q < 5; ++q)
#pragma unroll
            for (int j = 0; j < SEG + K - 1; ++j) v[q][j] = hp[q * IN * HPW + (r0 + j) * HPW + c];
        float m[5][SEG];
        fir_seg<K, SEG, 5>(v, win, m);
#pragma unroll
        for (int j = 0; j < SEG; ++j) {
            if (oy0 + r0 + j >= VH || ox0 + c >= VW) continue;
            const SsimPt p = ssim_point(m[0][j], m[1][j], m[2][j], m[3][j], m[4][j], C1, C2);
            cs_acc += p.cs; ss_acc += p.lum * p.cs;
        }
    }
    if (block_sum3(cs_acc, ss_acc, l1, tid)) add_sums(sums, l1_sum, plane, cs_acc, ss_acc, l1);
}

template <int K>
__global__ __launch_bounds__(256, 2) void ssim_bwd_k(const float* __restrict__ X, const float* __restrict__ Y, int H, int W, Win win,
                                                  float C1, float C2, const float* __restrict__ wts, int use_ssim,
                                                  const float* __restrict__ dcoarse, int HC, int WC, const float* l1_coef_p,
                                                  float* __restrict__ dX) {
    using G = BwdGeom<K>;
    constexpr int halo = G::halo, AD = G::AD, IN = G::IN, SA = G::SA, NSA = G::NSA, ADP = G::ADP, INP = G::INP, THR = G::THR;
    extern __shared__ float lds[];
    float* xs = lds;                       // [IN][INP]
    float* ys = lds + G::YS;
    float* hp = lds + G::HP;               // [5][IN][ADP]  -> later th [3][THR][TS]
    float* ad = lds;                       // [3][AD][AD] adjoint maps: alias xs / ys, which are dead after the horizontal pass
    const int plane = blockIdx.z;
    const int qy0 = blockIdx.y * TS, qx0 = blockIdx.x * TS;
    const int VH = H - halo, VW = W - halo;
    const float* xp = X + (long)plane * H * W;
    const float* yp = Y + (long)plane * H * W;
    const int tid = threadIdx.x;
    const float wt = wts[plane];
    stage_tile(xp, yp, H, W, qy0 - halo, qx0 - halo, IN, IN, INP, 1.f, xs, ys, tid);
    __syncthreads();
    // horizontal pass over [IN rows][AD cols]
    for (int it = tid; it < IN * NSA; it += 256) {
        const int r = it / NSA, c0 = (it % NSA) * SA;
        float v[5][SA + K - 1];
        moments_seg<SA + K - 1>(xs + r * INP + c0, ys + r * INP + c0, v);
        float o[5][SA];
        fir_seg<K, SA, 5>(v, win, o);
#pragma unroll
        for (int q = 0; q < 5; ++q)
#pragma unroll
            for (int j = 0; j < SA; ++j) hp[q * IN * ADP + r * ADP + c0 + j] = o[q][j];
    }
    __syncthreads();
    // vertical pass + adjoint maps at [AD rows][AD cols]; stored at column offset 0, rows 0..AD-1 of the padded image
    for (int it = tid; it < AD * NSA; it += 256) {
        const int c = it % AD, r0 = (it / AD) * SA;
        float v[5][SA + K - 1];
#pragma unroll
        for (int q = 0; q < 5; ++q)
#pragma unroll
            for (int j = 0; j < SA + K - 1; ++j) {
                const int rr = r0 + j;
                v[q][j] = rr < IN ? hp[q * IN * ADP + rr * ADP + c] : 0.f;
            }
        float m[5][SA];
        fir_seg<K, SA, 5>(v, win, m);
#pragma unroll
        for (int j = 0; j < SA; ++j) {
            const int r = r0 + j;
            if (r >= AD) continue;
            const int py = qy0 - halo + r, px = qx0 - halo + c;
            SsimAdj d = {0.f, 0.f, 0.f};
            if (py >= 0 && py < VH && px >= 0 && px < VW)
                d = ssim_adjoint(ssim_point(m[0][j], m[1][j], m[2][j], m[3][j], m[4][j], C1, C2), m[0][j], m[1][j], use_ssim, wt);
            ad[0 * AD * AD + r * AD + c] = d.a; ad[1 * AD * AD + r * AD + c] = d.b; ad[2 * AD * AD + r * AD + c] = d.cc;
        }
    }
    __syncthreads();
    // transposed filter, horizontal: th[r][q] = sum_t g[t] * ad[r][q + halo - t] = sum_u g[K-1-u] * ad[r][q + u]
    float* th = hp;                        // [3][THR][TS]
    for (int it = tid; it < AD * NS; it += 256) {
        const int r = it / NS, c0 = (it % NS) * SEG;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            float v[SEG + K - 1];
#pragma unroll
            for (int j = 0; j < SEG + K - 1; ++j) v[j] = ad[q * AD * AD + r * AD + c0 + j];
#pragma unroll
            for (int o = 0; o < SEG; ++o) th[q * THR * TS + r * TS + c0 + o] = fir_t<K>(v + o, win);
        }
    }
    __syncthreads();
    const PixTerms e = pix_terms<K>(win, dcoarse, plane, HC, WC, H, W, l1_coef_p);
    float* dxp = dX + (long)plane * H * W;
    for (int it = tid; it < TS * NS; it += 256) {
        const int c = it % TS, r0 = (it / TS) * SEG;
        float s[3][SEG];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            float v[SEG + K - 1];
#pragma unroll
            for (int j = 0; j < SEG + K - 1; ++j) v[j] = th[q * THR * TS + (r0 + j) * TS + c];
#pragma unroll
            for (int o = 0; o < SEG; ++o) s[q][o] = fir_t<K>(v + o, win);
        }
#pragma unroll
        for (int o = 0; o < SEG; ++o) {
            const int gy = qy0 + r0 + o, gx = qx0 + c;
            if (gy >= H || gx >= W) continue;
            const float xv = xp[(long)gy * W + gx], yv = yp[(long)gy * W + gx];      // (the LDS copies were overwritten by `ad`)
            dxp[(long)gy * W + gx] = pixel_grad<K>(e, win, s[0][o] + 2.f * xv * s[1][o] + yv * s[2][o], xv, yv, gy, gx);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Training pair (11-tap window).
// Forward: as ssim_fwd_k, plus the adjoint maps for ssim_bwd_adj_k.  The five filtered maps go through ONE
// horizontal-pass image one after the other (xs / ys + one map: 19.7 KB per workgroup instead of 41.6 KB, so 5-8 workgroups per CU
// instead of 3: this kernel, too, spent most of its wave cycles in waits), the vertical results stay in registers; the per-plane sums
// are spread over `stripes` copies (a level-0 launch ended with 256 f64 atomics per address and 8192 on the L1 sum: 59 of 217 us).
template <int K>
__global__ __launch_bounds__(256) void ssim_fwd_adj_k(const float* __restrict__ X, const float* __restrict__ Y, int H, int W,
                                                      Win win, float C1, float C2, double* sums, double* l1_sum, int stripes, long stripe_stride,
                                                      float* __restrict__ adj, int use_ssim, float in_mul) {
    using G = FwdGeom<K, 1>;
    constexpr int halo = G::halo, IN = G::IN, HPW = G::HPW;
    extern __shared__ float lds[];
    float* xs = lds;
    float* ys = lds + G::YS;
    float* hp = lds + G::HP;                   // [IN][HPW]: one map at a time
    const int plane = blockIdx.z;
    const int oy0 = blockIdx.y * TS, ox0 = blockIdx.x * TS;
    const int VH = H - halo, VW = W - halo;
    const int tid = threadIdx.x;
    stage_tile(X + (long)plane * H * W, Y + (long)plane * H * W, H, W, oy0, ox0, IN, IN, IN, in_mul, xs, ys, tid);
    __syncthreads();
    float l1 = l1_sum ? l1_tile<K>(win, xs, ys, IN, oy0, ox0, H, W, tid) : 0.f;
    // vertical item of this thread (the first TS * NS threads): column vc, rows vr0 .. vr0 + SEG - 1; its five filtered values
    const bool vitem = tid < TS * NS;
    const int vc = tid % TS, vr0 = (tid / TS) * SEG;
    float m[5][SEG];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        // horizontal pass of map q (x, y, x^2, y^2, xy): item = (row, segment of SEG output columns)
        for (int it = tid; it < IN * NS; it += 256) {
            const int r = it / NS, c0 = (it % NS) * SEG;
            float v[1][SEG + K - 1];
#pragma unroll
            for (int j = 0; j < SEG + K - 1; ++j) {
                const float a = (q == 1 || q == 3) ? 0.f : xs[r * IN + c0 + j];
                const float b = (q == 0 || q == 2) ? 0.f : ys[r * IN + c0 + j];
                v[0][j] = q == 0 ? a : q == 1 ? b : q == 2 ? a * a : q == 3 ? b * b : a * b;
            }
            float o[1][SEG];
            fir_seg<K, SEG, 1>(v, win, o);
#pragma unroll
            for (int j = 0; j < SEG; ++j) hp[r * HPW + c0 + j] = o[0][j];
        }
        __syncthreads();
        if (vitem) {
            float v[1][SEG + K - 1];
#pragma unroll
            for (int j = 0; j < SEG + K - 1; ++j) v[0][j] = hp[(vr0 + j) * HPW + vc];
            fir_seg<K, SEG, 1>(v, win, &m[q]);
        }
        if (q < 4) __syncthreads();
    }
    float cs_acc = 0.f, ss_acc = 0.f;
    if (vitem) {
#pragma unroll
        for (int j = 0; j < SEG; ++j) {
            if (oy0 + vr0 + j >= VH || ox0 + vc >= VW) continue;
            const SsimPt p = ssim_point(m[0][j], m[1][j], m[2][j], m[3][j], m[4][j], C1, C2);
            cs_acc += p.cs; ss_acc += p.lum * p.cs;
            // the map's derivatives wrt (mu_x, E[x^2], E[xy]) at this position, per unit of upstream weight: what the backward
            // pass used to recompute from x and y on a (TS + 20) x (TS + 10) halo (5 filtered maps) before its own 3 filters
            const SsimAdj d = ssim_adjoint(p, m[0][j], m[1][j], use_ssim, 1.f);
            float* ap = adj + ((long)plane * 3 * H + (oy0 + vr0 + j)) * W + ox0 + vc;
            ap[0] = d.a; ap[(long)H * W] = d.b; ap[2L * H * W] = d.cc;
        }
    }
    if (block_sum3(cs_acc, ss_acc, l1, tid)) {
        // (two exact pieces per sum, as stat_add: rows [0, stripes) and [stripes, 2 stripes) -- order-independent)
        const long so = (long)((blockIdx.x + blockIdx.y * 5) % stripes) * stripe_stride, lo = (long)stripes * stripe_stride;
        stat_add(sums + so + plane * 2, lo, cs_acc);
        stat_add(sums + so + plane * 2 + 1, lo, ss_acc);
        if (l1_sum) stat_add(l1_sum + so, lo, l1);
    }
}

// Backward from the adjoint maps the forward pass stored ([plane][3][H][W], valid positions only): scale by the plane's upstream
// weight, apply the transposed separable filter, add the chain-rule factors (1, 2x, y), the avg-pool gradient of the coarser level
// and the L1 term.  3 filtered maps on a (TS + 10)^2 halo instead of 5 + 3: 78 k instead of 295 k FMAs per 32 x 32 tile.
// The three maps go through ONE pair of LDS images one after the other (13.8 KB per workgroup: 8 workgroups per CU instead of 3 --
// the counters of the all-at-once version: 71 % of the wave cycles in waits, 15 % issuing vector instructions), the next map's tile
// is requested before the current one is filtered, and the per-tile index arithmetic is done once.
template <int K>
__global__ __launch_bounds__(256) void ssim_bwd_adj_k(const float* __restrict__ X, const float* __restrict__ Y, const float* __restrict__ ADJ,
                                                      int H, int W, Win win, const float* __restrict__ wts,
                                                      const float* __restrict__ dcoarse, int HC, int WC, const float* l1_coef_p,
                                                      float* __restrict__ dX, float in_mul) {
    using G = BwdAdjGeom<K>;
    constexpr int halo = G::halo, AD = G::AD, ADC = G::ADC, THW = G::THW, NL = G::NL;
    extern __shared__ float lds[];
    float* ad = lds;                       // [AD][ADC]
    float* th = lds + G::TH;               // [THR][THW]
    const int plane = blockIdx.z;
    const int qy0 = blockIdx.y * TS, qx0 = blockIdx.x * TS;
    const int VH = H - halo, VW = W - halo;
    const float* xp = X + (long)plane * H * W;
    const float* yp = Y + (long)plane * H * W;
    const float* ap = ADJ + (long)plane * 3 * H * W;
    const int tid = threadIdx.x;
    const float wt = wts[plane];
    // tile elements of this thread: offset in a map (or -1 outside the valid region) and LDS slot
    int goff[NL], lslot[NL];
#pragma unroll
    for (int u = 0; u < NL; ++u) {
        const int i = tid + u * 256;
        const int r = i / AD, c = i - r * AD;
        const int py = qy0 - halo + r, px = qx0 - halo + c;
        lslot[u] = i < AD * AD ? r * ADC + c : -1;
        goff[u] = (i < AD * AD && py >= 0 && py < VH && px >= 0 && px < VW) ? py * W + px : -1;
    }
    float pre[NL];
#define SB_LOAD(Q)                                                                                                \
    _Pragma("unroll") for (int u = 0; u < NL; ++u) pre[u] = goff[u] >= 0 ? wt * ap[(long)(Q) * H * W + goff[u]] : 0.f;
    SB_LOAD(0)
    // vertical item of this thread (the first TS * NS threads): column c, rows r0 .. r0 + SEG - 1; its x / y values
    const bool vitem = tid < TS * NS;
    const int vc = tid % TS, vr0 = (tid / TS) * SEG;
    float xv[SEG], yv[SEG], gsum[SEG];
#pragma unroll
    for (int o = 0; o < SEG; ++o) {
        const int gy = qy0 + vr0 + o, gx = qx0 + vc;
        const bool ok = vitem && gy < H && gx < W;
        xv[o] = ok ? __fmul_rn(xp[(long)gy * W + gx], in_mul) : 0.f;
        yv[o] = ok ? __fmul_rn(yp[(long)gy * W + gx], in_mul) : 0.f;
        gsum[o] = 0.f;
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
#pragma unroll
        for (int u = 0; u < NL; ++u) if (lslot[u] >= 0) ad[lslot[u]] = pre[u];
        __syncthreads();
        if (q < 2) { SB_LOAD(q + 1) }
        // transposed filter, horizontal: th[r][x] = sum_t g[t] * ad[r][x + halo - t]
        for (int it = tid; it < AD * NS; it += 256) {
            const int r = it / NS, c0 = (it % NS) * SEG;
            float v[SEG + K - 1];
#pragma unroll
            for (int j = 0; j < SEG + K - 1; ++j) v[j] = ad[r * ADC + c0 + j];
#pragma unroll
            for (int o = 0; o < SEG; ++o) th[r * THW + c0 + o] = fir_t<K>(v + o, win);
        }
        __syncthreads();
        if (vitem) {
            float v[SEG + K - 1];
#pragma unroll
            for (int j = 0; j < SEG + K - 1; ++j) v[j] = th[(vr0 + j) * THW + vc];
#pragma unroll
            for (int o = 0; o < SEG; ++o) {
                const float a = fir_t<K>(v + o, win);
                // g = s0 + 2 x s1 + y s2, summed in that order (as the all-at-once kernel did)
                if (q == 0) gsum[o] = a;
                else if (q == 1) gsum[o] = gsum[o] + 2.f * xv[o] * a;
                else gsum[o] = gsum[o] + yv[o] * a;
            }
        }
    }
#undef SB_LOAD
    if (!vitem) return;
    const PixTerms e = pix_terms<K>(win, dcoarse, plane, HC, WC, H, W, l1_coef_p);
    float* dxp = dX + (long)plane * H * W;
#pragma unroll
    for (int o = 0; o < SEG; ++o) {
        const int gy = qy0 + vr0 + o, gx = qx0 + vc;
        if (gy >= H || gx >= W) continue;
        // (* in_mul: chain rule of x * in_mul, what autograd does for x / divisor)
        dxp[(long)gy * W + gx] = __fmul_rn(pixel_grad<K>(e, win, gsum[o], xv[o], yv[o], gy, gx), in_mul);
    }
}

// ------------------------------------------------------------------------------------------------
// host side
Win make_win(const float* g, int k) {
    Win w; w.k = k;
    for (int i = 0; i < MAXW; ++i) w.g[i] = i < k ? g[i] : 0.f;
    return w;
}

// Grid of TS x TS tiles over a level: over the whole image where every pixel gets a value (the L1 term, the gradient), else over
// the valid positions of the window only
dim3 level_grid(int planes, int h, int w, int k, bool whole) {
    const int eh = whole ? h : h - k + 1, ew = whole ? w : w - k + 1;
    return dim3(cdiv(ew, TS), cdiv(eh, TS), planes);
}

float in_mul_of(float in_div) { return in_div == 1.f ? 1.f : 1.f / in_div; }      // (see stage_tile)

size_t lds_bytes(int floats) { return (size_t)floats * sizeof(float); }

int launch_pool(const float* in0, float* out0, const float* in1, float* out1, int tensors, float in_div, int planes, int h, int w, pssr_stream_t s) {
    const int ho = (h + 2 * (h & 1) - 2) / 2 + 1, wo = (w + 2 * (w & 1) - 2) / 2 + 1;
    const long total = (long)planes * ho * wo;
    int blocks = (int)((total + 255) / 256); if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(avgpool_kernel, dim3(blocks, tensors), dim3(256), 0, (hipStream_t)s, in0, out0, in1, out1, planes, h, w, ho, wo, in_mul_of(in_div));
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

int launch_weights(const double* sums, int stripes, long stripe_stride, double* folded, int levels, int planes, const double* nvalid,
                   const float* level_weights, int ms, float mix, const double* l1_sum, double l1_numel, const float* grad_out,
                   float* loss_out, float* wts, float* l1_coef, pssr_stream_t s) {
    hipLaunchKernelGGL(weights_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, sums, levels, planes, nvalid, level_weights, ms, mix,
                       l1_sum, l1_numel, grad_out, loss_out, wts, l1_coef, stripes, stripe_stride, folded);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

}  // namespace

extern "C" {

int pssr_ssim_level_fwd(const float* x, const float* y, int planes, int h, int w, const float* win_host, int k,
                        float c1, float c2, double* sums, double* l1_sum, pssr_stream_t s) {
    PSSR_CHECK(x && y && sums && win_host && planes > 0 && k > 0 && k <= MAXW && (k & 1), PSSR_ERR_ARG, "ssim_level_fwd: bad args");
    PSSR_CHECK(h >= k && w >= k, PSSR_ERR_ARG, "ssim_level_fwd: image %dx%d smaller than window %d", h, w, k);
    // when the L1 term is requested the tiles must cover the whole image, not only the valid region
    const dim3 grid = level_grid(planes, h, w, k, l1_sum != nullptr);
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute((const void*)ssim_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096);
        (void)hipFuncSetAttribute((const void*)ssim_fwd_k<11>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096);
        attr = true;
    }
    if (k == 11)
        hipLaunchKernelGGL(ssim_fwd_k<11>, grid, dim3(256), lds_bytes(FwdGeom<11, 5>::FLOATS), (hipStream_t)s, x, y, h, w,
                           make_win(win_host, k), c1, c2, sums, l1_sum);
    else
        hipLaunchKernelGGL(ssim_fwd_kernel, grid, dim3(256), lds_bytes(FwdLds(k).floats), (hipStream_t)s, x, y, h, w,
                           make_win(win_host, k), c1, c2, sums, l1_sum);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

int pssr_ssim_level_fwd_adj(const float* x, const float* y, float in_div, int planes, int h, int w, const float* win_host, int k, float c1,
                            float c2, int use_ssim, double* sums, double* l1_sum, int stripes, int64_t stripe_stride, float* adj,
                            pssr_stream_t s) {
    PSSR_CHECK(x && y && sums && win_host && planes > 0 && adj && k == 11, PSSR_ERR_ARG,
               "ssim_level_fwd_adj: needs the adjoint buffer and the 11-tap window (k=%d)", k);
    PSSR_CHECK(h >= k && w >= k && stripes >= 1 && (stripes == 1 || stripe_stride > 0) && in_div > 0.f, PSSR_ERR_ARG, "ssim_level_fwd_adj: bad size / stripes / in_div");
    hipLaunchKernelGGL(ssim_fwd_adj_k<11>, level_grid(planes, h, w, k, l1_sum != nullptr), dim3(256), lds_bytes(FwdGeom<11, 1>::FLOATS),
                       (hipStream_t)s, x, y, h, w, make_win(win_host, k), c1, c2, sums, l1_sum, stripes, (long)stripe_stride, adj, use_ssim,
                       in_mul_of(in_div));
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

int pssr_ssim_level_bwd_adj(const float* x, const float* y, float in_div, const float* adj, int planes, int h, int w, const float* win_host,
                            int k, const float* wts, const float* dcoarse, int hc, int wc, const float* l1_coef, float* dx, pssr_stream_t s) {
    PSSR_CHECK(x && y && adj && wts && dx && win_host && planes > 0 && k == 11, PSSR_ERR_ARG, "ssim_level_bwd_adj: bad args (k=%d)", k);
    hipLaunchKernelGGL(ssim_bwd_adj_k<11>, level_grid(planes, h, w, k, true), dim3(256), lds_bytes(BwdAdjGeom<11>::FLOATS), (hipStream_t)s,
                       x, y, adj, h, w, make_win(win_host, k), wts, dcoarse, hc, wc, l1_coef, dx, in_mul_of(in_div));
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

int pssr_avgpool2_planes(const float* in, float* out, int planes, int h, int w, pssr_stream_t s) {
    return pssr_avgpool2_planes_div(in, 1.f, out, planes, h, w, s);
}

int pssr_avgpool2_planes_div(const float* in, float in_div, float* out, int planes, int h, int w, pssr_stream_t s) {
    PSSR_CHECK(in && out && planes > 0 && h > 0 && w > 0 && in_div > 0.f, PSSR_ERR_ARG, "avgpool2_planes: bad args");
    return launch_pool(in, out, in, out, 1, in_div, planes, h, w, s);
}

int pssr_avgpool2_pair_div(const float* x, const float* y, float in_div, float* xo, float* yo, int planes, int h, int w, pssr_stream_t s) {
    PSSR_CHECK(x && y && xo && yo && planes > 0 && h > 0 && w > 0 && in_div > 0.f, PSSR_ERR_ARG, "avgpool2_pair: bad args");
    return launch_pool(x, xo, y, yo, 2, in_div, planes, h, w, s);
}

int pssr_msssim_weights(const double* sums, int levels, int planes, const double* nvalid, const float* level_weights, int ms,
                        float mix, const double* l1_sum, double l1_numel, const float* grad_out, float* loss_out, float* wts,
                        float* l1_coef, pssr_stream_t s) {
    PSSR_CHECK(sums && nvalid && loss_out && wts && l1_coef && levels > 0 && levels <= 8 && planes > 0, PSSR_ERR_ARG, "msssim_weights: bad args");
    return launch_weights(sums, 1, 0L, nullptr, levels, planes, nvalid, level_weights, ms, mix, l1_sum, l1_numel, grad_out, loss_out, wts, l1_coef, s);
}

int pssr_msssim_weights_striped(const double* sums, int stripes, int64_t stripe_stride, double* folded, int levels, int planes,
                                const double* nvalid, const float* level_weights, int ms, float mix, const double* l1_sum,
                                double l1_numel, const float* grad_out, float* loss_out, float* wts, float* l1_coef, pssr_stream_t s) {
    PSSR_CHECK(sums && folded && stripes >= 1 && stripe_stride > 0 && nvalid && loss_out && wts && l1_coef && levels > 0 && levels <= 8 && planes > 0,
               PSSR_ERR_ARG, "msssim_weights_striped: bad args");
    return launch_weights(sums, stripes, (long)stripe_stride, folded, levels, planes, nvalid, level_weights, ms, mix, l1_sum, l1_numel, grad_out,
                          loss_out, wts, l1_coef, s);
}

int pssr_ssim_level_bwd(const float* x, const float* y, int planes, int h, int w, const float* win_host, int k, float c1, float c2,
                        const float* wts, int use_ssim, const float* dcoarse, int hc, int wc, const float* l1_coef, float* dx,
                        pssr_stream_t s) {
    PSSR_CHECK(x && y && wts && dx && win_host && planes > 0 && k > 0 && k <= MAXW && (k & 1), PSSR_ERR_ARG, "ssim_level_bwd: bad args");
    const size_t lds = lds_bytes(BwdLds(k).floats);
    PSSR_CHECK(lds <= 156 * 1024, PSSR_ERR_UNSUPPORTED, "ssim_level_bwd: window %d needs %zu bytes of LDS", k, lds);
    const dim3 grid = level_grid(planes, h, w, k, true);
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute((const void*)ssim_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096);
        (void)hipFuncSetAttribute((const void*)ssim_bwd_k<11>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096);
        attr = true;
    }
    if (k == 11)
        hipLaunchKernelGGL(ssim_bwd_k<11>, grid, dim3(256), lds_bytes(BwdGeom<11>::FLOATS), (hipStream_t)s, x, y, h, w,
                           make_win(win_host, k), c1, c2, wts, use_ssim, dcoarse, hc, wc, l1_coef, dx);
    else
        hipLaunchKernelGGL(ssim_bwd_kernel, grid, dim3(256), lds, (hipStream_t)s, x, y, h, w,
                           make_win(win_host, k), c1, c2, wts, use_ssim, dcoarse, hc, wc, l1_coef, dx);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

}  // extern "C"
