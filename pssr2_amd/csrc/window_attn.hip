// Shifted-window attention of SwinIR (pssr/models/swinir.py:345-385 `SwinTransformerBlock.forward`, :563-594 `WindowAttention.forward`)
// as one forward and one backward kernel over the un-rolled, un-windowed token tensor:
//
//   qkv [B, H, W, 3C]   channel which * C + head * hd + d   (the qkv Linear applied per token; which = 0 q, 1 k, 2 v)
//   out [B, H, W, C]    channel head * hd + d, original token order
//   lse [B, heads, H, W] float32: log-sum-exp of every query row, original token order
//
//   S = (q * scale) k^T + bias_table[rel(i, j)] + mask(i, j),   P = softmax_j S,   O = P v            per (window, head)
//
// The cyclic shift (-shift, -shift), window_partition's token order (row-major inside the window), window_reverse and the shift back
// are addressing only: token n = r * ws + c of window (wr, wc) sits at shifted position (wr * ws + r, wc * ws + c), i.e. at original
// position ((y + shift) mod H, (x + shift) mod W).  No rolled or windowed copy of anything exists.  The relative-position index is
// (ri - rj + ws - 1) * (2 ws - 1) + (ci - cj + ws - 1).  The mask of `calculate_mask` is not materialised: along an axis of length L the
// region of shifted position p is 0 for p < L - ws, 1 for p < L - shift, else 2; region = 3 * rh + rw; exactly -100.0f is ADDED where
// the regions of the two tokens differ and shift > 0 (it is not -inf: with large logits masked entries keep weight).
//
// Launch: grid B * nWindows * heads (head fastest: neighbouring workgroups read neighbouring channel segments of the same tokens),
// block 256 = 4 waves, one (window, head) pair per workgroup.  N = ws^2 <= 64 tokens, hd <= 32; everything is padded with zeros to
// 64 x 32 in LDS and kept there in float32 whatever the storage type, so both storage types run the exact-f32
// v_mfma_f32_32x32x2_f32 (a k-ordered fma chain): S, the softmax and the sums are required in float32 anyway, one code path serves
// both types, and at the default SwinIR shape it is 3.5-4.9x faster than the torch composition (bound by
// the LDS round trips and the dependent MFMA chains, not by HBM: a bf16 MFMA build is the next step there).
//
//   LDS rows of q / k / v / dO: pitch 33 floats, of S / P / dS: pitch 65.  An MFMA operand read is one ds_read_b32 per lane at
//   row * pitch (+ k) or k * pitch + row; both pitches are odd, so the 32 lanes of a group fall on 32 different banks.
//
// Forward:  1 tokens, regions, the head's bias column -> LDS     2 q * scale, k, v -> LDS (VEC: 16-byte loads; else element loads:
//           rows of hd elements are not 16-byte aligned in general)     3 S: one 32 x 32 tile per wave -> LDS
//           4 row pass, 4 lanes per row: + bias + mask, max, exp, sum (__shfl_xor), P -> LDS, lse -> HBM
//           5 O = P v: 2 tiles x 2 halves of the j sum; waves 2, 3 hand their half over through LDS, waves 0, 1 add and store.
// Backward: P is recomputed from q, k and lse.  S and dP = dO v^T tiles stay in the wave's registers; P~ = exp(S - lse);
//           the row sums of P~ and of dP o P~ are reduced over the 32 lanes of a half and exchanged between the two waves of a row
//           through LDS; P = P~ / rowsum(P~) (1 up to the rounding of lse: one ulp of |lse| in every entry of a row otherwise);
//           dV = P^T dO (split like O), then dS = P o (dP - rowsum(dP o P)) replaces P in LDS, dq = scale dS k and
//           dk = dS^T (q scale) take one tile per wave.  All three go to dqkv [B, H, W, 3C]: every element is owned by one (window, head) pair, no atomics.
//           dbias: each workgroup writes its (2 ws - 1)^2 sums of dS (token pairs in a fixed order, added in double) to
//           workspace[pair][rel]; window_attn_dbias_kernel adds them over windows and batch items in a fixed order, in double: the
//           same bits on every run.
//
// The kernels clamp nothing: the host checks that every index they form lies inside its tensor.
#include "common.h"

#define WA_N 64          // padded tokens per window
#define WA_D 32          // padded head dim
#define WA_QP 33         // LDS pitch of q / k / v / dO rows (floats)
#define WA_SP 65         // LDS pitch of S / P / dS rows
#define WA_MAXREL 225    // (2 * 8 - 1)^2

namespace {

struct WaGeom { int B, H, W, C, heads, ws, shift, hd, nwh, nww; float scale; };

// row of accumulator register e of a 32 x 32 tile (the column is lane & 31)
__device__ __forceinline__ int wa_row(int e, int lane) { return (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5); }

// acc[i][j] = sum_k A[i][k] B[k][j], k < K (even): A[i][k] at A[i * a_rs + k * a_ks], B[k][j] at B[k * b_ks + j * b_cs]
__device__ __forceinline__ f32x16 wa_mma(const float* A, int a_rs, int a_ks, const float* B, int b_ks, int b_cs, int K, int lane) {
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    const int r = lane & 31, h = lane >> 5;
    const float* a = A + r * a_rs + h * a_ks;
    const float* b = B + h * b_ks + r * b_cs;
    for (int k = 0; k < K; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k * a_ks], b[k * b_ks], acc, 0, 0, 0);
    return acc;
}

// tokens of the window (offset inside the batch item, original order) and their mask regions
__device__ __forceinline__ void wa_tokens(const WaGeom& g, int win, int t, int* stok, int* sreg) {
    if (t >= WA_N) return;
    int tok = 0, reg = 0;
    if (t < g.ws * g.ws) {
        const int wr = win / g.nww, wc = win - wr * g.nww;
        const int r = t / g.ws, c = t - r * g.ws;
        const int y = wr * g.ws + r, x = wc * g.ws + c;             // shifted coordinates
        int oy = y + g.shift, ox = x + g.shift;                       // torch.roll(x, -shift): shifted[y] = x[(y + shift) mod H]
        if (oy >= g.H) oy -= g.H;
        if (ox >= g.W) ox -= g.W;
        tok = oy * g.W + ox;
        const int rh = y < g.H - g.ws ? 0 : y < g.H - g.shift ? 1 : 2;
        const int rw = x < g.W - g.ws ? 0 : x < g.W - g.shift ? 1 : 2;
        reg = 3 * rh + rw;
    }
    stok[t] = tok;
    sreg[t] = reg;
}

// dst[n][d] = mul * src[tok[n] * tstride + d] for n < N, d < hd; zeros up to 64 x 32
template <typename T, bool VEC>
__device__ __forceinline__ void wa_load_rows(float* dst, const T* __restrict__ src, const int* stok, long tstride, int N, int hd, float mul, int t) {
    if (VEC) {
        constexpr int EPV = 16 / sizeof(T), CPR = WA_D / EPV;
        const int cpr = hd / EPV;
        for (int i = t; i < WA_N * CPR; i += 256) {
            const int n = i / CPR, c = i - n * CPR;
            float f[EPV];
#pragma unroll
            for (int e = 0; e < EPV; ++e) f[e] = 0.f;
            if (n < N && c < cpr) TT<T>::unpack(*reinterpret_cast<const u32x4*>(src + (long)stok[n] * tstride + c * EPV), f);
#pragma unroll
            for (int e = 0; e < EPV; ++e) dst[n * WA_QP + c * EPV + e] = f[e] * mul;
        }
    } else {
        for (int i = t; i < WA_N * WA_D; i += 256) {
            const int n = i >> 5, d = i & 31;
            float v = 0.f;
            if (n < N && d < hd) v = to_f32(src[(long)stok[n] * tstride + d]);
            dst[n * WA_QP + d] = v * mul;
        }
    }
}

// logit of the pair (i, j), both < N: (s + bias) + mask, in the order WindowAttention.forward adds them
__device__ __forceinline__ float wa_logit(const WaGeom& g, const float* sbias, const int* sreg, float s, int i, int j) {
    const int ri = i / g.ws, ci = i - ri * g.ws, rj = j / g.ws, cj = j - rj * g.ws;
    s += sbias[(ri - rj + g.ws - 1) * (2 * g.ws - 1) + (ci - cj + g.ws - 1)];
    return (g.shift > 0 && sreg[i] != sreg[j]) ? s + -100.0f : s;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void window_attn_fwd_kernel(const T* __restrict__ qkv, const float* __restrict__ bias_table, T* __restrict__ out,
                                                              float* __restrict__ lse, WaGeom g) {
    __shared__ float sq[WA_N * WA_QP], sk[WA_N * WA_QP], sv[WA_N * WA_QP], sp[WA_N * WA_SP], sbias[WA_MAXREL];
    __shared__ int stok[WA_N], sreg[WA_N];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int nwin = g.nwh * g.nww, N = g.ws * g.ws, nrel = (2 * g.ws - 1) * (2 * g.ws - 1);
    const unsigned bid = blockIdx.x;
    const int head = (int)(bid % (unsigned)g.heads);
    const unsigned bw = bid / (unsigned)g.heads;
    const int win = (int)(bw % (unsigned)nwin), b = (int)(bw / (unsigned)nwin);
    const long npix = (long)g.H * g.W;

    wa_tokens(g, win, t, stok, sreg);
    for (int i = t; i < nrel; i += 256) sbias[i] = bias_table[i * g.heads + head];
    __syncthreads();

    const T* base = qkv + (long)b * npix * 3 * g.C + head * g.hd;
    wa_load_rows<T, VEC>(sq, base, stok, 3L * g.C, N, g.hd, g.scale, t);
    wa_load_rows<T, VEC>(sk, base + g.C, stok, 3L * g.C, N, g.hd, 1.f, t);
    wa_load_rows<T, VEC>(sv, base + 2 * g.C, stok, 3L * g.C, N, g.hd, 1.f, t);
    __syncthreads();

    const int ti = wave & 1, tj = wave >> 1;
    {   // S tile (ti, tj)
        const f32x16 acc = wa_mma(sq + ti * 32 * WA_QP, WA_QP, 1, sk + tj * 32 * WA_QP, 1, WA_QP, (g.hd + 1) & ~1, lane);
#pragma unroll
        for (int e = 0; e < 16; ++e) sp[(ti * 32 + wa_row(e, lane)) * WA_SP + tj * 32 + (lane & 31)] = acc[e];
    }
    __syncthreads();

    {   // row pass: row i on 4 neighbouring lanes, columns sub + 4 m
        const int i = t >> 2, sub = t & 3;
        float s[16], mx = -INFINITY;
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            const int j = sub + 4 * m;
            s[m] = (i < N && j < N) ? wa_logit(g, sbias, sreg, sp[i * WA_SP + j], i, j) : -INFINITY;
            mx = fmaxf(mx, s[m]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 1));
        mx = fmaxf(mx, __shfl_xor(mx, 2));
        float sum = 0.f;
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            s[m] = (i < N && sub + 4 * m < N) ? expf(s[m] - mx) : 0.f;
            sum += s[m];
        }
        sum += __shfl_xor(sum, 1);
        sum += __shfl_xor(sum, 2);
        const float inv = i < N ? 1.f / sum : 0.f;
#pragma unroll
        for (int m = 0; m < 16; ++m) sp[i * WA_SP + sub + 4 * m] = s[m] * inv;
        if (sub == 0 && i < N) lse[((long)b * g.heads + head) * npix + stok[i]] = mx + logf(sum);
    }
    __syncthreads();

    // O = P v: tile row ti, half tj of the sum over j
    f32x16 acc = wa_mma(sp + ti * 32 * WA_SP + tj * 32, WA_SP, 1, sv + tj * 32 * WA_QP, WA_QP, 1, 32, lane);
    if (wave >= 2) {
#pragma unroll
        for (int e = 0; e < 16; ++e) sq[(ti * 32 + wa_row(e, lane)) * WA_QP + (lane & 31)] = acc[e];      // q is no longer read
    }
    __syncthreads();
    if (wave < 2) {
        const int d = lane & 31;
        T* obase = out + (long)b * npix * g.C + head * g.hd + d;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int i = ti * 32 + wa_row(e, lane);
            if (i < N && d < g.hd) obase[(long)stok[i] * g.C] = from_f32<T>(acc[e] + sq[i * WA_QP + d]);
        }
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void window_attn_bwd_kernel(const T* __restrict__ qkv, const float* __restrict__ bias_table, const float* __restrict__ lse,
                                                              const T* __restrict__ dout, T* __restrict__ dqkv, float* __restrict__ part, WaGeom g) {
    __shared__ float sq[WA_N * WA_QP], sk[WA_N * WA_QP], sv[WA_N * WA_QP], sdo[WA_N * WA_QP], sp[WA_N * WA_SP], sbias[WA_MAXREL];
    __shared__ float slse[WA_N], sdelta[2 * WA_N], ssum[2 * WA_N];
    __shared__ int stok[WA_N], sreg[WA_N];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int nwin = g.nwh * g.nww, N = g.ws * g.ws, nrel = (2 * g.ws - 1) * (2 * g.ws - 1);
    const unsigned bid = blockIdx.x;
    const int head = (int)(bid % (unsigned)g.heads);
    const unsigned bw = bid / (unsigned)g.heads;
    const int win = (int)(bw % (unsigned)nwin), b = (int)(bw / (unsigned)nwin);
    const long npix = (long)g.H * g.W;

    wa_tokens(g, win, t, stok, sreg);
    for (int i = t; i < nrel; i += 256) sbias[i] = bias_table[i * g.heads + head];
    __syncthreads();

    const T* base = qkv + (long)b * npix * 3 * g.C + head * g.hd;
    wa_load_rows<T, VEC>(sq, base, stok, 3L * g.C, N, g.hd, g.scale, t);
    wa_load_rows<T, VEC>(sk, base + g.C, stok, 3L * g.C, N, g.hd, 1.f, t);
    wa_load_rows<T, VEC>(sv, base + 2 * g.C, stok, 3L * g.C, N, g.hd, 1.f, t);
    wa_load_rows<T, VEC>(sdo, dout + (long)b * npix * g.C + head * g.hd, stok, (long)g.C, N, g.hd, 1.f, t);
    if (t < WA_N) slse[t] = t < N ? lse[((long)b * g.heads + head) * npix + stok[t]] : 0.f;
    __syncthreads();

    const int ti = wave & 1, tj = wave >> 1, kp = (g.hd + 1) & ~1;
    const int j = tj * 32 + (lane & 31);
    float p[16], dp[16];
    {   // S and dP = dO v^T, tile (ti, tj); P~ = exp(S + bias + mask - lse); partial row sums of P~ and of dP o P~
        const f32x16 as = wa_mma(sq + ti * 32 * WA_QP, WA_QP, 1, sk + tj * 32 * WA_QP, 1, WA_QP, kp, lane);
        const f32x16 ad = wa_mma(sdo + ti * 32 * WA_QP, WA_QP, 1, sv + tj * 32 * WA_QP, 1, WA_QP, kp, lane);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int i = ti * 32 + wa_row(e, lane);
            p[e] = (i < N && j < N) ? expf(wa_logit(g, sbias, sreg, as[e], i, j) - slse[i]) : 0.f;
            dp[e] = ad[e];
            float v = p[e] * dp[e], u = p[e];
#pragma unroll
            for (int m = 1; m < 32; m <<= 1) {
                v += __shfl_xor(v, m);
                u += __shfl_xor(u, m);
            }
            if ((lane & 31) == 0) {
                sdelta[tj * WA_N + i] = v;
                ssum[tj * WA_N + i] = u;
            }
        }
    }
    __syncthreads();
    // The row sum of P~ is 1 up to the rounding of lse and of S - lse (an error of one ulp of |lse| in every entry of the row, which
    // matters when logits are large); dividing by it takes that common factor out again.  P -> LDS, dS = P o (dP - rowsum(dP o P)) stays
    // in registers until P has been read.
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int i = ti * 32 + wa_row(e, lane);
        const float r = ssum[i] + ssum[WA_N + i];
        const float inv = r > 0.f ? 1.f / r : 0.f;
        p[e] *= inv;
        sp[i * WA_SP + j] = p[e];
        dp[e] = p[e] * (dp[e] - (sdelta[i] + sdelta[WA_N + i]) * inv);
    }
    __syncthreads();

    {   // dV = P^T dO: tile row ti (tokens j), half tj of the sum over i
        f32x16 acc = wa_mma(sp + tj * 32 * WA_SP + ti * 32, 1, WA_SP, sdo + tj * 32 * WA_QP, WA_QP, 1, 32, lane);
        if (wave >= 2) {
#pragma unroll
            for (int e = 0; e < 16; ++e) sv[(ti * 32 + wa_row(e, lane)) * WA_QP + (lane & 31)] = acc[e];      // v is no longer read
        }
        __syncthreads();
        if (wave < 2) {
            const int d = lane & 31;
            T* obase = dqkv + (long)b * npix * 3 * g.C + 2 * g.C + head * g.hd + d;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int n = ti * 32 + wa_row(e, lane);
                if (n < N && d < g.hd) obase[(long)stok[n] * 3 * g.C] = from_f32<T>(acc[e] + sv[n * WA_QP + d]);
            }
        }
    }
    // dS replaces P (every wave has passed the barrier above after its last read of P)
#pragma unroll
    for (int e = 0; e < 16; ++e) sp[(ti * 32 + wa_row(e, lane)) * WA_SP + j] = dp[e];
    __syncthreads();

    {   // waves 0, 1: dq = scale dS k (tokens i); waves 2, 3: dk = dS^T (q scale) (tokens j); tile row ti
        const bool is_k = wave >= 2;
        const f32x16 acc = is_k ? wa_mma(sp + ti * 32, 1, WA_SP, sq, WA_QP, 1, WA_N, lane)
                                : wa_mma(sp + ti * 32 * WA_SP, WA_SP, 1, sk, WA_QP, 1, WA_N, lane);
        const float mul = is_k ? 1.f : g.scale;
        const int d = lane & 31;
        T* obase = dqkv + (long)b * npix * 3 * g.C + (is_k ? g.C : 0) + head * g.hd + d;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int n = ti * 32 + wa_row(e, lane);
            if (n < N && d < g.hd) obase[(long)stok[n] * 3 * g.C] = from_f32<T>(acc[e] * mul);
        }
    }
    if (t < nrel) {   // this pair's share of dbias_table[t]: the token pairs with that relative position, i ascending
        const int w2 = 2 * g.ws - 1;
        const int dr = t / w2 - (g.ws - 1), dc = t % w2 - (g.ws - 1);
        double sum = 0.;
        for (int i = 0; i < N; ++i) {
            const int ri = i / g.ws, ci = i - ri * g.ws, rj = ri - dr, cj = ci - dc;
            if (rj >= 0 && rj < g.ws && cj >= 0 && cj < g.ws) sum += (double)sp[i * WA_SP + rj * g.ws + cj];
        }
        part[(long)bid * nrel + t] = (float)sum;
    }
}

// dbias_table[rel][head] = sum over batch items and windows of part[(bw * heads + head) * nrel + rel]; grid (ceil(nrel / 32), heads),
// block 256: lane group wl adds bw = wl, wl + 8, ... in ascending order, then the 8 groups are added in ascending order
__global__ __launch_bounds__(256) void window_attn_dbias_kernel(const float* __restrict__ part, float* __restrict__ dbias, int nbw, int heads, int nrel) {
    __shared__ double red[8][32];
    const int rl = threadIdx.x & 31, wl = threadIdx.x >> 5;
    const int rel = blockIdx.x * 32 + rl, head = blockIdx.y;
    double acc = 0.;
    if (rel < nrel) {
#pragma unroll 4
        for (int bw = wl; bw < nbw; bw += 8) acc += (double)part[((long)bw * heads + head) * nrel + rel];
    }
    red[wl][rl] = acc;
    __syncthreads();
    if (wl == 0 && rel < nrel) {
        double total = red[0][rl];
#pragma unroll
        for (int k = 1; k < 8; ++k) total += red[k][rl];
        dbias[rel * heads + head] = (float)total;
    }
}

// shape checks shared by the entry points; fills g
int wa_check(const char* what, int B, int H, int W, int C, int heads, int ws, int shift, float scale, int dtype, WaGeom* g) {
    PSSR_CHECK(dtype == PSSR_F32 || dtype == PSSR_BF16, PSSR_ERR_ARG, "%s: dtype must be PSSR_F32 or PSSR_BF16", what);
    PSSR_CHECK(B > 0 && H > 0 && W > 0 && C > 0 && heads > 0, PSSR_ERR_ARG, "%s: B, H, W, C and heads must be positive", what);
    PSSR_CHECK(ws >= 1 && ws <= 8, PSSR_ERR_ARG, "%s: window size %d outside [1, 8] (at most 64 tokens per window)", what, ws);
    PSSR_CHECK(shift >= 0 && shift < ws, PSSR_ERR_ARG, "%s: shift %d outside [0, window size %d)", what, shift, ws);
    PSSR_CHECK(H % ws == 0 && W % ws == 0, PSSR_ERR_ARG, "%s: H %d and W %d must be multiples of the window size %d", what, H, W, ws);
    PSSR_CHECK(C % heads == 0, PSSR_ERR_ARG, "%s: C %d is not a multiple of heads %d", what, C, heads);
    PSSR_CHECK(C / heads <= WA_D, PSSR_ERR_ARG, "%s: head dim %d exceeds %d", what, C / heads, WA_D);
    PSSR_CHECK(scale == scale, PSSR_ERR_ARG, "%s: scale is NaN", what);
    // every index the kernels form: token offsets oy * W + ox < H * W and bias_table offsets < 225 * heads in int; element offsets
    // below B * H * W * 3C and workspace offsets below grid * 225 in 64 bits
    PSSR_CHECK((int64_t)H * W <= 0x7fffffffL && (int64_t)heads * WA_MAXREL <= 0x7fffffffL, PSSR_ERR_ARG, "%s: H * W or heads exceeds 32-bit indexing", what);
    PSSR_CHECK((int64_t)B * H * W <= ((int64_t)1 << 40) && C <= (1 << 20), PSSR_ERR_ARG, "%s: tensor too large for 64-bit element offsets", what);
    const int64_t blocks = (int64_t)B * (H / ws) * (W / ws) * heads;
    PSSR_CHECK(blocks <= 0x7fffffffL, PSSR_ERR_ARG, "%s: B * windows * heads exceeds the grid limit", what);
    *g = WaGeom{B, H, W, C, heads, ws, shift, C / heads, H / ws, W / ws, scale};
    return PSSR_OK;
}

template <typename T> bool wa_vec(int hd, const void* a, const void* b) {
    return (hd * sizeof(T)) % 16 == 0 && ((uintptr_t)a % 16) == 0 && ((uintptr_t)b % 16) == 0;       // 3C and C elements are then multiples of 16 bytes too
}

}  // namespace

extern "C" int64_t pssr_window_attn_workspace_bytes(int B, int H, int W, int heads, int ws) {
    if (B <= 0 || H <= 0 || W <= 0 || heads <= 0 || ws < 1 || ws > 8 || H % ws || W % ws) return PSSR_ERR_ARG;
    return (int64_t)B * (H / ws) * (W / ws) * heads * (2 * ws - 1) * (2 * ws - 1) * (int64_t)sizeof(float);
}

extern "C" int pssr_window_attn_fwd(const void* qkv, const float* bias_table, void* out, float* lse, int B, int H, int W, int C, int heads, int ws,
                                    int shift, float scale, int dtype, pssr_stream_t s) {
    PSSR_CHECK(qkv && bias_table && out && lse, PSSR_ERR_ARG, "window_attn_fwd: null pointer");
    WaGeom g;
    if (int rc = wa_check("window_attn_fwd", B, H, W, C, heads, ws, shift, scale, dtype, &g)) return rc;
    const dim3 grid((unsigned)(B * g.nwh * g.nww * heads));
#define WA_FWD(T, V) hipLaunchKernelGGL((window_attn_fwd_kernel<T, V>), grid, dim3(256), 0, (hipStream_t)s, (const T*)qkv, bias_table, (T*)out, lse, g)
    if (dtype == PSSR_F32) {
        if (wa_vec<float>(g.hd, qkv, qkv)) WA_FWD(float, true); else WA_FWD(float, false);
    } else {
        if (wa_vec<bf16_t>(g.hd, qkv, qkv)) WA_FWD(bf16_t, true); else WA_FWD(bf16_t, false);
    }
#undef WA_FWD
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}

extern "C" int pssr_window_attn_bwd(const void* qkv, const float* bias_table, const float* lse, const void* dout, void* dqkv, float* dbias_table,
                                    void* workspace, int64_t workspace_bytes, int B, int H, int W, int C, int heads, int ws, int shift, float scale,
                                    int dtype, pssr_stream_t s) {
    PSSR_CHECK(qkv && bias_table && lse && dout && dqkv && dbias_table && workspace, PSSR_ERR_ARG, "window_attn_bwd: null pointer");
    WaGeom g;
    if (int rc = wa_check("window_attn_bwd", B, H, W, C, heads, ws, shift, scale, dtype, &g)) return rc;
    PSSR_CHECK(workspace_bytes >= pssr_window_attn_workspace_bytes(B, H, W, heads, ws), PSSR_ERR_ARG,
               "window_attn_bwd: workspace smaller than pssr_window_attn_workspace_bytes");
    const int nbw = B * g.nwh * g.nww, nrel = (2 * ws - 1) * (2 * ws - 1);
    const dim3 grid((unsigned)(nbw * heads));
    float* part = (float*)workspace;
#define WA_BWD(T, V) hipLaunchKernelGGL((window_attn_bwd_kernel<T, V>), grid, dim3(256), 0, (hipStream_t)s, (const T*)qkv, bias_table, lse, (const T*)dout, (T*)dqkv, part, g)
    if (dtype == PSSR_F32) {
        if (wa_vec<float>(g.hd, qkv, dout)) WA_BWD(float, true); else WA_BWD(float, false);
    } else {
        if (wa_vec<bf16_t>(g.hd, qkv, dout)) WA_BWD(bf16_t, true); else WA_BWD(bf16_t, false);
    }
#undef WA_BWD
    PSSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(window_attn_dbias_kernel, dim3((unsigned)cdiv(nrel, 32), (unsigned)heads), dim3(256), 0, (hipStream_t)s, part, dbias_table, nbw,
                       heads, nrel);
    PSSR_LAUNCH_CHECK();
    return PSSR_OK;
}
