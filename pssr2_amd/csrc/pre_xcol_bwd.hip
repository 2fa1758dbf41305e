// Backward of a flat-K (im2col) source of a wide convolution in ONE pass over the output gradient (gfx950, 16-bit storage):
//
//     dx[p][j]  = sum_k dy[p][k] * W1[k][j]        (data gradient of the im2col tensor, rounded to storage)
//     dW1[k][j] = sum_p dy[p][k] * x[p][j]         (weight gradient, f32)
//
// for dy [npix][cout] (cout up to 1024: Reconstruction.pre's r^2 * h0 channels), x [npix][16] and W1 [cout][16].  Both products are
// 16 wide, so each is a pure streaming pass over dy -- the largest tensor of the training step -- with next to no arithmetic; done as
// two launches (a flat-K conv2d and a 1-tap weight gradient) dy is fetched twice.  Here a workgroup walks a contiguous run of
// 64-pixel tiles; per tile it streams dy in chunks of 256 channels through LDS ([32-channel sub-tile][64 px][64 B], the layout of
// conv_wgrad.hip) while the next chunk's global loads are in flight in registers, and multiplies every chunk twice:
//   * dW1: K = pixels, so both operands are read transposed (ds_read_b64_tr_b16); a wave owns two 32-channel sub-tiles of every
//     chunk and keeps their 32 x 32 results (x padded to 32 columns with zeros) in accumulators for the life of the workgroup;
//   * dx:  K = channels, the A fragment is 8 consecutive channels of a pixel (a plain 16-byte LDS read), the B fragment comes from a
//     transposed, storage-rounded copy of W1 the workgroup builds in LDS once; waves 0/1 and 2/3 sum over different halves of a
//     chunk's channels and meet in LDS at the end of the tile (fixed order).
// Every workgroup ends with one plain-store partial slab of dW1; a second small launch sums the slabs in a fixed order (no
// floating-point atomics anywhere: the result does not depend on scheduling).

#include "common.h"

namespace {

constexpr int PX_PIX = 64;                 // pixels per tile
constexpr int PX_CH = 256;                 // channels per chunk
constexpr int PX_KX = 16;                  // width of x / dx / W1
constexpr int PX_ROWB = 64;                // bytes per LDS row (32 channels)
constexpr int PX_SUB = PX_PIX * PX_ROWB;   // bytes per 32-channel sub-tile
constexpr int PX_DY_BYTES = (PX_CH / 32) * PX_SUB;
constexpr int PX_XT_BYTES = PX_PIX * PX_ROWB;
constexpr int PX_DX_BYTES = 2 * PX_PIX * PX_KX * 4;
constexpr int PX_ITEMS = PX_DY_BYTES / 16 / 256;      // 16-byte pieces of a chunk per thread
constexpr int PX_RED_LANES = 16;           // part lanes of the slab reduction

struct PairArgs {
    const void* dy; int dy_cs, dy_co, cout;
    const void* x; int x_cs, x_co;
    void* dx; int dx_cs, dx_co;
    const float* w; int w_row, w_off, nk;          // W1[k][j] = w[n_perm[k] * w_row + w_off + j] for j < nk, else 0
    const int32_t* n_perm;
    float* slabs;                                  // [gridDim.x][cout][16] f32
    long npix; int n_tiles;
};

template <typename T> constexpr int px_w1_stride(int nch) { return (nch * PX_CH + 8) * (int)sizeof(T); }
template <typename T> constexpr int px_lds_bytes(int nch) { return PX_DY_BYTES + PX_XT_BYTES + PX_DX_BYTES + PX_KX * px_w1_stride<T>(nch); }

__device__ __forceinline__ u32x4 px_tr_frag(const char* a0, const char* a1) {      // two ds_read_b64_tr_b16 (see conv_wgrad.hip)
    typedef __attribute__((ext_vector_type(4))) short s16x4;
    typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
    const u32x2 lo = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a0));
    const u32x2 hi = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a1));
    u32x4 r = {lo[0], lo[1], hi[0], hi[1]};
    return r;
}

template <typename T, int NCH>        // NCH = 256-channel chunks per pixel: cout <= 256 * NCH
__global__ __launch_bounds__(256, 2) void flatk_bwd_pair_kernel(const PairArgs p) {
    using X = TT<T>;
    constexpr int ESZ = 2;
    constexpr int W1S = px_w1_stride<T>(NCH);
    static_assert(sizeof(T) == 2, "16-bit storage");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const Dy = smem;
    char* const Xt = smem + PX_DY_BYTES;
    float* const Dxs = (float*)(smem + PX_DY_BYTES + PX_XT_BYTES);
    char* const W1t = smem + PX_DY_BYTES + PX_XT_BYTES + PX_DX_BYTES;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // this workgroup's run of tiles (contiguous in memory)
    const int t_begin = (int)((long)blockIdx.x * p.n_tiles / gridDim.x), t_end = (int)((long)(blockIdx.x + 1) * p.n_tiles / gridDim.x);

    // ---- W1 transposed and rounded to storage: W1t[j][k], rows padded by 16 bytes (conflict-free 16-byte fragment reads); channels
    // past cout hold zeros (their dy is zero-filled, and 0 * garbage could be NaN)
    for (int i = tid; i < NCH * PX_CH * PX_KX; i += 256) {
        const int k = i / PX_KX, j = i % PX_KX;
        float v = 0.f;
        if (k < p.cout && j < p.nk) v = p.w[(long)(p.n_perm ? p.n_perm[k] : k) * p.w_row + p.w_off + j];
        *(T*)(W1t + j * W1S + k * ESZ) = (T)v;
    }
    // x occupies the lower 32 bytes of its 64-byte rows; the upper 16 columns of the 32-wide operand are zeroed here and never written again
    if (tid < 2 * PX_PIX) *(u32x4*)(Xt + (tid >> 1) * PX_ROWB + 32 + (tid & 1) * 16) = u32x4{0u, 0u, 0u, 0u};

    f32x16 accw[NCH][2];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int e = 0; e < 16; ++e) accw[c][a][e] = 0.f;

    // ---- tile-independent item descriptors.  dy piece `it` of a chunk: pixel tid / 8 + 32 (it & 1), channels 64 (it >> 1) + 8 (tid % 8)
    // (a wave instruction fetches whole 128-byte lines); x piece (threads 0..127): pixel tid / 2, 16-byte half tid % 2
    const int ipix = tid >> 3, ipc = tid & 7;
    const unsigned dy_off0 = (unsigned)((ipix * p.dy_cs + ipc * 8) * ESZ), dy_off1 = dy_off0 + (unsigned)(32 * p.dy_cs * ESZ);
    const int dy_lds = (ipc >> 2) * PX_SUB + ipix * PX_ROWB + (ipc & 3) * 16;
    const unsigned x_off = (unsigned)(((tid >> 1) * p.x_cs + (tid & 1) * 8) * ESZ);
    const int x_lds = (tid >> 1) * PX_ROWB + (tid & 1) * 16;
    // ---- fragment read bases.  Transposed reads: lane 4q+p of each 16-lane group addresses row q, columns 4p..4p+3
    const int g = lane >> 4, li = lane & 15;
    const int fr_off = ((g >> 1) * 8 + (li >> 2)) * PX_ROWB + ((g & 1) * 16 + (li & 3) * 4) * 2;
    const char* const dyw_rd = Dy + (2 * wave) * PX_SUB + fr_off;
    const char* const x_rd = Xt + fr_off;
    // data gradient: wave -> pixel block wave & 1 (32 pixels), channel group wave >> 1 (four sub-tiles of every chunk)
    const int mblk = wave & 1, kgrp = wave >> 1;
    const char* const dyd_rd = Dy + (kgrp * 4) * PX_SUB + (mblk * 32 + (lane & 31)) * PX_ROWB + (lane >> 5) * 16;
    const char* const w1_rd = W1t + (lane & 15) * W1S + (kgrp * 128 + (lane >> 5) * 8) * ESZ;

    u32x4 dy_reg[PX_ITEMS], x_reg = {0u, 0u, 0u, 0u};

    // requests chunk CH of tile TILE (and with chunk 0 the tile's x rows); pixels past npix and channels past cout are redirected to an
    // out-of-range offset: the buffer load returns zeros and touches no memory
#define PX_ISSUE(TILE, CH)                                                                                        \
    {                                                                                                             \
        const long pix0_ = (long)(TILE) * PX_PIX;                                                                 \
        const int left_ = (int)(p.npix - pix0_ < PX_PIX ? p.npix - pix0_ : PX_PIX);                               \
        const __amdgpu_buffer_rsrc_t rdy_ = __builtin_amdgcn_make_buffer_rsrc(                                    \
            (void*)((const char*)p.dy + (pix0_ * p.dy_cs + p.dy_co + (CH) * PX_CH) * ESZ), 0, (int)0xfffffff0u, 0x00020000); \
        _Pragma("unroll") for (int it = 0; it < PX_ITEMS; ++it) {                                                 \
            const bool ok_ = ipix + 32 * (it & 1) < left_ && (CH) * PX_CH + 64 * (it >> 1) < p.cout;              \
            const unsigned off_ = ok_ ? ((it & 1) ? dy_off1 : dy_off0) + (unsigned)(128 * (it >> 1)) : 0xffffffffu; \
            dy_reg[it] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rdy_, (int)off_, 0, 0)); \
        }                                                                                                         \
        if ((CH) == 0 && tid < 128) {                                                                             \
            const __amdgpu_buffer_rsrc_t rx_ = __builtin_amdgcn_make_buffer_rsrc(                                 \
                (void*)((const char*)p.x + (pix0_ * p.x_cs + p.x_co) * ESZ), 0, (int)0xfffffff0u, 0x00020000);    \
            x_reg = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rx_, (int)((tid >> 1) < left_ ? x_off : 0xffffffffu), 0, 0)); \
        }                                                                                                         \
    }

    if (t_begin < t_end) PX_ISSUE(t_begin, 0)
    for (int tile = t_begin; tile < t_end; ++tile) {
        f32x16 accd;
#pragma unroll
        for (int e = 0; e < 16; ++e) accd[e] = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            // ---- commit the staged chunk
#pragma unroll
            for (int it = 0; it < PX_ITEMS; ++it) *(u32x4*)(Dy + dy_lds + (it >> 1) * 2 * PX_SUB + (it & 1) * 32 * PX_ROWB) = dy_reg[it];
            if (c == 0 && tid < 128) *(u32x4*)(Xt + x_lds) = x_reg;
            __syncthreads();
            if (c + 1 < NCH) PX_ISSUE(tile, c + 1)
            else if (tile + 1 < t_end) PX_ISSUE(tile + 1, 0)

            // ---- dW1: 4 k-steps of 16 pixels, this wave's two sub-tiles
#pragma unroll
            for (int s = 0; s < PX_PIX / 16; ++s) {
                const u32x4 bf = px_tr_frag(x_rd + s * 16 * PX_ROWB, x_rd + (s * 16 + 4) * PX_ROWB);
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    const u32x4 af = px_tr_frag(dyw_rd + a * PX_SUB + s * 16 * PX_ROWB, dyw_rd + a * PX_SUB + (s * 16 + 4) * PX_ROWB);
                    X::mma(accw[c][a], af, bf);
                }
            }
            // ---- dx: this wave's 32 pixels x its four sub-tiles, 2 k-steps of 16 channels each
#pragma unroll
            for (int ss = 0; ss < 4; ++ss)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const u32x4 af = *(const u32x4*)(dyd_rd + ss * PX_SUB + t * 32);
                    const u32x4 bf = *(const u32x4*)(w1_rd + (c * PX_CH + ss * 32 + t * 16) * ESZ);
                    X::mma(accd, af, bf);
                }
            __syncthreads();
        }
        // ---- dx of the tile: the two channel groups meet in LDS, group 0 + group 1, rounded to storage
        if ((lane & 31) < PX_KX) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = mblk * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                Dxs[(kgrp * PX_PIX + row) * PX_KX + (lane & 31)] = accd[e];
            }
        }
        __syncthreads();
        {
            const int row = tid >> 2, j0 = (tid & 3) * 4;
            const long pix = (long)tile * PX_PIX + row;
            if (pix < p.npix) {
                const float4 a = *(const float4*)(Dxs + row * PX_KX + j0);
                const float4 b = *(const float4*)(Dxs + (PX_PIX + row) * PX_KX + j0);
                const float v[4] = {a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w};
                store4((T*)p.dx + pix * p.dx_cs + p.dx_co + j0, v);
            }
        }
        // (Dxs is written again only behind the barriers of the next tile's chunks)
    }
#undef PX_ISSUE

    // ---- this workgroup's partial slab [cout][16], plain stores (a workgroup without tiles stores zeros)
    if ((lane & 31) < PX_KX) {
        float* const dst = p.slabs + (long)blockIdx.x * p.cout * PX_KX;
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int n = c * PX_CH + (2 * wave + a) * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                    if (n < p.cout) dst[n * PX_KX + (lane & 31)] = accw[c][a][e];
                }
    }
}

// dw[i] = sum over the slabs, in a fixed order: 16 part lanes per position of 4 floats, every lane sums its slabs q = lane, lane + 16,
// ... one after the other, then the lanes are summed 0..15
__global__ __launch_bounds__(256) void flatk_slab_sum_kernel(const float* __restrict__ slabs, int parts, int total4, float* __restrict__ dw) {
    __shared__ float4 buf[256];
    const int pos = threadIdx.x & 15, pl = threadIdx.x >> 4;
    const int i4 = blockIdx.x * 16 + pos;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i4 < total4)
        for (int q = pl; q < parts; q += PX_RED_LANES) {
            const float4 a = *(const float4*)(slabs + ((long)q * total4 + i4) * 4);
            v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
        }
    buf[pl * 16 + pos] = v;
    __syncthreads();
    if (pl == 0 && i4 < total4) {
        float4 s = buf[pos];
        for (int l = 1; l < PX_RED_LANES; ++l) {
            const float4 a = buf[l * 16 + pos];
            s.x += a.x; s.y += a.y; s.z += a.z; s.w += a.w;
        }
        *(float4*)(dw + (long)i4 * 4) = s;
    }
}

int px_cus() {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) cus = n;
        else cus = 256;
    }
    return cus;
}

int px_parts(long npix) {
    const long tiles = (npix + PX_PIX - 1) / PX_PIX;
    const long target = 2L * px_cus();
    return (int)(tiles < target ? tiles : target);
}

template <typename T, int NCH>
int px_launch(const PairArgs& a, int parts, hipStream_t s) {
    constexpr int LDS = px_lds_bytes<T>(NCH);
    static_assert(2 * LDS <= 160 * 1024, "two workgroups per CU");
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void*)flatk_bwd_pair_kernel<T, NCH>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
        attr_done = true;
    }
    hipLaunchKernelGGL((flatk_bwd_pair_kernel<T, NCH>), dim3(parts), dim3(256), LDS, s, a);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

template <typename T>
int px_launch_nch(const PairArgs& a, int parts, hipStream_t s) {
    const int nch = cdiv(a.cout, PX_CH);
    return nch == 1 ? px_launch<T, 1>(a, parts, s) : nch == 2 ? px_launch<T, 2>(a, parts, s)
         : nch == 3 ? px_launch<T, 3>(a, parts, s) : px_launch<T, 4>(a, parts, s);
}

}  // namespace

extern "C" int pssr_flatk_bwd_pair_supported(int dtype, int cout, int kx) {
    return (dtype == PSSR_BF16 || dtype == PSSR_F16) && cout >= 64 && cout <= 4 * PX_CH && cout % 64 == 0 && kx == PX_KX;
}

extern "C" int pssr_flatk_bwd_pair_parts(int64_t npix) {
    PSSR_CHECK(npix > 0 && npix < (1LL << 31) * PX_PIX, PSSR_ERR_ARG, "flatk_bwd_pair: npix=%lld", (long long)npix);
    return px_parts((long)npix);
}

extern "C" int pssr_flatk_bwd_pair(const void* dy, int dy_cs, int dy_co, int cout, const void* x, int x_cs, int x_co, void* dx, int dx_cs,
                                   int dx_co, int kx, const float* w, int w_row, int w_off, int nk, const int32_t* n_perm, float* slabs,
                                   int parts, float* dw, int64_t npix, int dtype, pssr_stream_t stream) {
    PSSR_CHECK(dy && x && dx && w && slabs && dw, PSSR_ERR_ARG, "flatk_bwd_pair: null pointer");
    PSSR_CHECK(pssr_flatk_bwd_pair_supported(dtype, cout, kx), PSSR_ERR_UNSUPPORTED,
               "flatk_bwd_pair: dtype=%d cout=%d kx=%d (16-bit storage, cout a multiple of 64 up to 1024, kx = 16)", dtype, cout, kx);
    PSSR_CHECK(npix > 0 && npix < (1LL << 31) * PX_PIX, PSSR_ERR_ARG, "flatk_bwd_pair: npix=%lld", (long long)npix);
    PSSR_CHECK(dy_cs % 8 == 0 && dy_co % 8 == 0 && dy_co >= 0 && dy_co + cout <= dy_cs, PSSR_ERR_ARG, "flatk_bwd_pair: dy stride/offset");
    PSSR_CHECK(x_cs % 8 == 0 && x_co % 8 == 0 && x_co >= 0 && x_co + kx <= x_cs, PSSR_ERR_ARG, "flatk_bwd_pair: x stride/offset");
    PSSR_CHECK(dx_cs % 4 == 0 && dx_co % 4 == 0 && dx_co >= 0 && dx_co + kx <= dx_cs, PSSR_ERR_ARG, "flatk_bwd_pair: dx stride/offset");
    PSSR_CHECK((long)PX_PIX * dy_cs * 2 < (1L << 30) && (long)PX_PIX * x_cs * 2 < (1L << 30), PSSR_ERR_ARG, "flatk_bwd_pair: channel stride too large");
    PSSR_CHECK(nk > 0 && nk <= kx && w_row >= w_off + nk && w_off >= 0, PSSR_ERR_ARG, "flatk_bwd_pair: weight window");
    PSSR_CHECK(parts == px_parts((long)npix), PSSR_ERR_ARG, "flatk_bwd_pair: parts=%d but this shape needs %d (ask pssr_flatk_bwd_pair_parts)", parts,
               px_parts((long)npix));
    PairArgs a;
    a.dy = dy; a.dy_cs = dy_cs; a.dy_co = dy_co; a.cout = cout;
    a.x = x; a.x_cs = x_cs; a.x_co = x_co;
    a.dx = dx; a.dx_cs = dx_cs; a.dx_co = dx_co;
    a.w = w; a.w_row = w_row; a.w_off = w_off; a.nk = nk; a.n_perm = n_perm;
    a.slabs = slabs; a.npix = (long)npix; a.n_tiles = (int)((npix + PX_PIX - 1) / PX_PIX);
    hipStream_t s = (hipStream_t)stream;
    const int rc = dtype == PSSR_BF16 ? px_launch_nch<bf16_t>(a, parts, s) : px_launch_nch<f16_t>(a, parts, s);
    if (rc != PSSR_OK) return rc;
    const int total4 = cout * PX_KX / 4;
    hipLaunchKernelGGL(flatk_slab_sum_kernel, dim3(cdiv(total4, 16)), dim3(256), 0, s, (const float*)slabs, parts, total4, dw);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}
