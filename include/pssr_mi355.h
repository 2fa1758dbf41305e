/* pssr_mi355.h — C ABI of libpssr_mi355.so, the MI355X (gfx950) kernels behind pssr2_amd.
 *
 * The reference (ucsdmanorlab/PSSR2) is pure Python and has no FFI layer; its hot path is the
 * torch.nn ops listed in SURVEY.md §8a.  Each entry point below replaces one (or a fused group) of
 * those ops; the reference file:line it stands for is cited next to it.  Conventions:
 *   - every pointer is a DEVICE pointer unless marked "host"; the caller owns all memory,
 *     the library allocates nothing persistent;
 *   - every call takes the HIP stream to launch on (pssr_stream_t == hipStream_t) and never
 *     synchronises it;
 *   - return value: 0 on success, a negative PSSR_ERR_* otherwise (never throws across the ABI);
 *     pssr_last_error() returns a thread-local message for the last failure;
 *   - activations are NHWC ("pixel-major") with an explicit channel stride so that an op can read
 *     or write a channel slice of a wider buffer (this is how torch.cat is elided);
 *   - dtype of activations / packed weights: PSSR_F32 (exact-f32 MFMA path, parity), PSSR_BF16 or PSSR_F16
 *     (16-bit storage, f32 accumulate; fp16 needs loss scaling by the caller).  Parameters, statistics and
 *     gradients are f32/f64.
 */
#ifndef PSSR_MI355_H
#define PSSR_MI355_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* pssr_stream_t; /* hipStream_t */

enum { PSSR_F32 = 0, PSSR_BF16 = 1, PSSR_F16 = 2 };

enum {
    PSSR_OK = 0,
    PSSR_ERR_ARG = -1,     /* invalid shape / alignment / enum */
    PSSR_ERR_LAUNCH = -2,  /* HIP launch failure */
    PSSR_ERR_UNSUPPORTED = -3
};

int pssr_abi_version(void);
const char* pssr_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Weight packing.  torch keeps Conv2d weights OIHW f32 (pssr/models/_blocks.py:10-11,28,35); the
 * conv kernels consume a K-chunked, LDS-image-ordered copy in the compute dtype:
 *   packed[chunk][tap][n (padded to 128)][32 bytes = 2 swizzled 16-byte slots of K]
 * A chunk is KCH consecutive K indices and a slot holds EPS = KCH / 2 of them in order: EPS = 4, KCH = 8 for PSSR_F32, EPS = 8,
 * KCH = 16 for PSSR_BF16 and PSSR_F16.  K elements [0, EPS) of a chunk are in slot (n >> 3) & 1 of column n and elements
 * [EPS, KCH) in the other one, i.e. the slot at byte offset 16 s holds the half h = s ^ ((n >> 3) & 1) (the conv kernels read
 * half h of column n at n * 32 + ((h ^ ((n >> 3) & 1)) << 4): conflict-free LDS reads).
 * mode 0 (forward):  GEMM-K = input channels  [ci_begin, ci_begin+ci_count) of the OIHW tensor,
 *                    GEMM-N = output channels (optionally permuted by `n_perm`: n_src = n_perm[n]).
 * mode 1 (dgrad):    GEMM-K = output channels, GEMM-N = input channels of the range, taps flipped.
 * mode 2 (flat-K):   a KxK conv seen as 1x1 over im2col'ed channels: K index = (ci-ci_begin)*ks*ks + tap.
 * mode 3 (flat-K dgrad): the transpose of mode 2: GEMM-K = output channels, GEMM-N = flat index.
 * mode 4 (space-to-depth): a KxK stride-K conv (RDNet transition, pssr/models/_rdnet.py:54-62) seen as 1x1 over the
 *                    space-to-depth input written by pssr_layernorm2d_fwd(s2d=1): K index = tap*cpad + ci,
 *                    cpad = cin rounded up to 16.   mode 5: its transpose (dgrad).
 * `k_pad` = GEMM-K rounded up to 16, `n_pad` = GEMM-N rounded up to 128 (zero filled).
 */
int pssr_pack_conv_weight(const float* w_oihw, void* packed, int cout, int cin, int ks,
                          int ci_begin, int ci_count, int mode, const int32_t* n_perm,
                          int k_pad, int n_pad, int dtype, pssr_stream_t stream);
/* The same for many weights in one launch (a training step re-packs every conv weight, forward and dgrad form).
 * `items_dev` is a DEVICE array; fields as the arguments above; `center` != 0 (modes 2/3, ks = 3): `w_oihw` is a 1x1
 * weight [cout][cin] standing for the centre tap of a 3x3 kernel (ResBlock.respass consumed through the im2col'ed input). */
typedef struct pssr_pack_item {
    const float* w; void* packed; const int32_t* n_perm;
    int32_t cout, cin, ks, ci_begin, ci_count, mode, k_pad, n_pad, dtype, center;
} pssr_pack_item;
int pssr_pack_conv_weight_batch(const pssr_pack_item* items_dev, int n_items, pssr_stream_t stream);
/* bytes needed for a packed weight */
int64_t pssr_packed_weight_bytes(int taps, int k_pad, int n_pad, int dtype);

/* Inverse of mode 0 / mode 2 for gradients: wgrad writes dW as f32 [n][tap][k_pad]; this scatters
 * (adds when `accumulate`) into the OIHW f32 gradient of the parameter. */
int pssr_unpack_conv_wgrad(const float* dw_packed, float* dw_oihw, int cout, int cin, int ks,
                           int ci_begin, int ci_count, int mode, const int32_t* n_perm,
                           int k_pad, int accumulate, pssr_stream_t stream);
/* same, summing `parts` partial slabs laid out [parts][rows][taps][k_pad] (rows = the wgrad's cout) first */
int pssr_unpack_conv_wgrad_parts(const float* dw_parts, int parts, int rows, float* dw_oihw, int cout, int cin, int ks,
                                 int ci_begin, int ci_count, int mode, const int32_t* n_perm,
                                 int k_pad, int accumulate, pssr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution, stride 1, "same" zero padding, NHWC, MFMA 32x32 tiles.
 * Replaces nn.Conv2d forward (pssr/models/_blocks.py:16-17,39-40) and, with mode-1 packed
 * weights, its input-gradient; BatchNorm2d+ReLU of the *previous* layer is applied while the
 * input tile is staged (prologue), and BatchNorm statistics / residual tail / ReLU-mask are
 * applied while the output tile is written (epilogue), so no normalised tensor is materialised.
 */
enum { PSSR_PRO_NONE = 0, PSSR_PRO_BN_RELU = 1,
       PSSR_PRO_GELU = 2 /* in = gelu(in): nn.GELU between the two 1x1 convs of an RDNet block, pssr/models/_rdnet.py:185,200 */ };
enum {
    PSSR_EPI_STORE = 0,      /* out = acc + bias                                             */
    PSSR_EPI_TAIL = 1,       /* out = relu(acc + bias + aux*aux_scale + aux_shift)  (ResBlock tail, _blocks.py:40) */
    PSSR_EPI_DGRAD_MASK = 2, /* out = (aux*aux_scale+aux_shift > 0) ? acc : 0   (ReLU backward) */
    PSSR_EPI_DGRAD_GELU = 4, /* out = acc * gelu'(aux)   (GELU backward; with FLAG_STATS stats[0..cout) += sum out)  */
    PSSR_EPI_HEADQ = 5,      /* inference form of Reconstruction (_blocks.py:15-18) for 64 hidden channels and ONE output channel: the
                              * epilogue of `pre` (FLAG_RELU implied, channels sub-pixel major, cout = 16 * 64) does not store its
                              * activation but the nine per-tap dot products of relu(acc + bias) with Reconstruction.conv's weights:
                              * head_q[tap][sub][n][h][w] (f32) for sub-pixel sub of low-resolution pixel (n, y, x);
                              * pssr_head_q_gather sums, for every output pixel, the nine products of its shifted neighbours.
                              * 16-bit storage, the conv_v3 tiles (h, w >= 16); PSSR_ERR_UNSUPPORTED otherwise */
    PSSR_EPI_FINAL = 3       /* out_f32_nchw = (acc + bias)*out_scale + out_shift; any cout <= 32
                                (Reconstruction.conv + "x*128+128", _blocks.py:17, resunet.py:95)  */
};
/* Per-channel f64 statistics are accumulated into PSSR_STAT_STRIPES interleaved copies
 * (stats[stripe][2*C], stripe = workgroup index mod PSSR_STAT_STRIPES) so that thousands of workgroups do
 * not serialise on 2*C addresses; the finalisers sum the stripes. */
#define PSSR_STAT_STRIPES 32
/* Every statistic buffer has PSSR_STAT_ROWS = 2 x PSSR_STAT_STRIPES rows: a workgroup adds each of its f32 partial sums v to stripe
 * s = workgroup index mod PSSR_STAT_STRIPES as TWO exact pieces -- row s gets v rounded to a multiple of 2^-20, row
 * PSSR_STAT_STRIPES + s the remainder rounded to a multiple of 2^-64.  Sums of such pieces are exact in f64 (no rounding, hence
 * independent of the order in which the atomics arrive) while a row stays below 2^33 resp. holds fewer than 2^10 addends; the
 * consumers (pssr_bn_finalize, pssr_bn_bwd_coefs, pssr_f64_to_f32, ...) add the rows in a fixed order.  Training steps are therefore
 * bit-reproducible; beyond those magnitudes the sums merely round like ordinary f64 atomics again. */
#define PSSR_STAT_ROWS (2 * PSSR_STAT_STRIPES)

enum {
    PSSR_FLAG_RELU = 1,   /* EPI_STORE: relu after bias (Reconstruction.pre, _blocks.py:16)   */
    PSSR_FLAG_STATS = 2,  /* accumulate per-channel f64 sums into `stats`:
                             EPI_STORE: [sum v, sum v^2]; EPI_DGRAD_MASK: [sum g, sum g*xhat] */
    PSSR_FLAG_HEADQ = 8,  /* EPI_STORE (with FLAG_RELU): store the activation AND the tap planes of PSSR_EPI_HEADQ (same conditions, head_w /
                             head_q set): the training form -- `pre`'s activation is kept for the backward pass, Reconstruction.conv's
                             forward still needs no pass over it */
    PSSR_FLAG_AFFINE = 4, /* EPI_STORE, 16-bit storage, not with FLAG_STATS: out = (acc + bias) * aux_scale + aux_shift (then FLAG_RELU):
                             an eval-mode BatchNorm (+ ReLU) applied by the PRODUCING convolution on its f32 accumulators
                             (_blocks.py:28-32 in eval mode), so that the next layer's loader needs no prologue */
    PSSR_FLAG_SOLO = 32,  /* hint, any epilogue: nothing else runs beside this launch (a forward pass on one stream): tilings that fill the
                             chip by themselves are preferred -- 128 x 64 tiles where 128 x 128 would leave one workgroup per CU.  Launches
                             of a backward pass, which share the chip with the weight-gradient stream, measured better without it */
    PSSR_FLAG_SHUF2 = 16  /* EPI_STORE, 16-bit storage, cout % 32 == 0, not with FLAG_STATS / FLAG_HEADQ: F.pixel_shuffle(out, 2)
                             (resunet.py:82) done by the store.  `out` is the [n, 2h, 2w, out_cstride] buffer the shuffled map belongs
                             into (channels out_coff .. out_coff + cout / 4); the weights (and bias) arrive with their output channels
                             in sub-pixel-major order (packed row s * cout / 4 + c = torch channel 4 c + s, s = 2 i + j), and the
                             8-channel piece c of sub-pixel (i, j) of pixel (y, x) goes to pixel (2 y + i, 2 x + j), channel c */
};

typedef struct pssr_conv_desc {
    int32_t dtype;
    int32_t n, h, w;            /* batch and spatial size (input == output)                    */
    /* up to two input sources accumulated into one output; source 1 is optional (cin1 == 0)    */
    const void* in0; int32_t in0_cstride, in0_coff, cin0, taps0;   /* taps: 9 (3x3) or 1 (1x1)  */
    const void* w0;             /* packed (pssr_pack_conv_weight), K padded to 16               */
    const void* in1; int32_t in1_cstride, in1_coff, cin1, taps1;
    const void* w1;
    int32_t prologue;           /* applies to source 0 only                                    */
    const float* pro_scale;     /* [cin0] gamma*invstd                                         */
    const float* pro_shift;     /* [cin0] beta - mean*gamma*invstd                             */
    void* out; int32_t out_cstride, out_coff, cout, n_pad;
    const float* bias;          /* [cout] or NULL                                              */
    int32_t epilogue, flags;
    const void* aux; int32_t aux_cstride, aux_coff;
    const float* aux_scale; const float* aux_shift;      /* [cout]                              */
    const float* aux_mean; const float* aux_invstd;      /* [cout] (DGRAD_MASK + STATS)         */
    double* stats;              /* [PSSR_STAT_ROWS][2*cout], caller-zeroed                     */
    /* "blocked" pixel order (log2 r, 0 = plain NHWC): pixel (y,x) of an r-times upsampled image
     * lives at ((y/r*W/r + x/r)*r*r + (y%r)*r + x%r), i.e. F.pixel_shuffle (_blocks.py:17) of an
     * NHWC tensor whose channels were ordered sub-pixel-major needs no data movement at all.    */
    int32_t in0_blk, out_blk, aux_blk;
    float out_scale, out_shift; /* EPI_FINAL only                                              */
    /* optional scratch for split-K (layers whose tiles do not fill the chip): pssr_conv2d_workspace_bytes(desc) bytes,
     * uninitialised, caller-owned; NULL (or too small) simply disables the split                                   */
    void* workspace; int64_t workspace_bytes;
    /* EPI_HEADQ only (appended in ABI version 3; other epilogues never read them): Reconstruction.conv's weight [1][64][3][3] f32 and
     * the tap products [9][16][n][h][w] f32 */
    const float* head_w; float* head_q;
} pssr_conv_desc;

int pssr_conv2d(const pssr_conv_desc* desc, pssr_stream_t stream);
/* bytes of `workspace` with which pssr_conv2d would split K for this shape (0: no split); negative = PSSR_ERR_*.  Pointers
 * in `desc` are ignored. */
int64_t pssr_conv2d_workspace_bytes(const pssr_conv_desc* desc);
/* Deprecated (ABI version 1): selected the round-1 pipelined 256-pixel loop, which conv_v3_kernel replaced (tunable IGEMM_V3
 * below).  Kept so that old bindings load; ignores its argument and returns 0. */
int pssr_conv2d_pipeline_mode(int mode);

/* Kernel-selection tunables (no reference counterpart: the reference has no native code).  ONE process-wide table, filled once
 * from the environment variables PSSR_<NAME> on first use and changed afterwards only through pssr_set_option(); no launch
 * path reads the environment.  Names: IGEMM_V3 (1: LDS-DMA / counted-wait 3x3 loop for 16-bit layers with > 64 output
 * channels on >= 16x16 images when its 256-pixel tiles fill the chip; 2: whenever the shape allows; 0: the 128-pixel loop), IGEMM_V3_64
 * (the same loop in 64-channel tiles for 33..64 output channels), IGEMM_N64 (128 x 64 tiles for FLAG_SOLO launches whose 128 x 128
 * tiles leave one workgroup per CU), IGEMM_FLAT, IGEMM_BIG, IGEMM_KSPLIT, CONV_EPI8, WGRAD_LEAN, WGRAD_X2 (0 in production),
 * WGRAD_DMA, WGRAD_BLOCKS, WGRAD_BLOCKS_1X1, DWCONV_TILE, DWWG_BLOCKS, LN_BWD_BLOCKS (and the diagnostic IGEMM_DBG, LN_DBG,
 * V3_LDS_PAD: 0 in production).  pssr_set_option returns the previous value (>= 0) or PSSR_ERR_ARG
 * for an unknown name / out-of-range value; pssr_get_option returns the value or PSSR_ERR_ARG. */
int pssr_set_option(const char* name, int value);
int pssr_get_option(const char* name);

/* Weight gradient of the same convolution (autograd of nn.Conv2d.weight):
 *   dw[n][tap][k] = sum_pixels dy[p][n] * prologue(in)[p + tap][k]      (f32)
 * The pixel reduction is split over workgroups.  dw_parts > 0 (preferred): the caller provides
 * dw[dw_parts][cout][taps][cin_pad] (no initialisation needed), dw_parts = pssr_conv2d_wgrad_parts(desc); every
 * workgroup stores its partial slab once and pssr_unpack_conv_wgrad_parts sums the parts while scattering to OIHW.
 * dw_parts == 0: one caller-zeroed slab, partial sums combined with f32 atomics, then pssr_unpack_conv_wgrad.   */
typedef struct pssr_wgrad_desc {
    int32_t dtype;
    int32_t n, h, w;
    const void* dy; int32_t dy_cstride, dy_coff, dy_blk, cout;   /* cout*elemsize % 16 == 0       */
    const void* in; int32_t in_cstride, in_coff, in_blk, cin_pad; /* cin_pad % 16 == 0            */
    int32_t taps;
    int32_t prologue; const float* pro_scale; const float* pro_shift;
    float* dw;                                                   /* [max(dw_parts,1)][cout][taps][cin_pad] */
    int32_t dw_parts;
} pssr_wgrad_desc;

int pssr_conv2d_wgrad(const pssr_wgrad_desc* desc, pssr_stream_t stream);
/* number of partial slabs this shape is split into (> 0), or a negative PSSR_ERR_*; pointers in `desc` are ignored */
int pssr_conv2d_wgrad_parts(const pssr_wgrad_desc* desc);


/* ---------------------------------------------------------------------------------------------
 * Per-channel and pointwise kernels around the convolutions (all HBM-bound).
 * NHWC tensor slices are passed as (pointer, channel stride, channel offset); C % 4 == 0.
 */

/* (statistic buffer of PSSR_STAT_ROWS rows, see there) stats[0:c] += sum, stats[c:2c] += sum of squares of (x*pre_scale + pre_shift) over N,H,W of an
 * NCHW f32 tensor: batch statistics of ResUNet.norm on "x/128-1" (pssr/models/resunet.py:66-68). */
int pssr_channel_stats_nchw(const float* x, int n, int c, int64_t hw, float pre_scale, float pre_shift,
                            double* stats, pssr_stream_t stream);

/* nn.BatchNorm2d training-mode bookkeeping (pssr/models/_blocks.py:31; torch defaults eps=1e-5,
 * momentum=.1): from [sum, sumsq] -> scale=gamma*invstd, shift=beta-mean*scale, mean, invstd and the
 * running_mean / running_var update (unbiased variance).  running_* may both be NULL. */
int pssr_bn_finalize(const double* stats, double count, const float* gamma, const float* beta, float eps,
                     float momentum, float* running_mean, float* running_var, float* scale, float* shift,
                     float* mean, float* invstd, int c, pssr_stream_t stream);
/* eval mode: scale/shift from the running statistics */
int pssr_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean,
                        const float* running_var, float eps, float* scale, float* shift, int c,
                        pssr_stream_t stream);
/* a = relu(scale * y + shift) in the storage type (16-bit, power-of-two channel count): the activated input of the next convolution of a
 * ResBlock (pssr/models/_blocks.py:26-41, nn.BatchNorm2d + nn.ReLU) written out once per layer, bit-identical to what the convolution
 * loaders' BatchNorm+ReLU prologue stages, so that pssr_conv2d_wgrad can read it without a prologue (LDS-DMA kernel). */
int pssr_bn_relu_apply(const void* y, int y_cs, int y_co, const float* scale, const float* shift, void* a, int a_cs,
                       int a_co, int64_t npix, int c, int dtype, pssr_stream_t stream);
/* BatchNorm backward: with stats = [sum g, sum g*xhat] the input gradient is A*g + B*y + C per channel;
 * also emits dgamma = sum g*xhat and dbeta = sum g (either may be NULL). */
int pssr_bn_bwd_coefs(const double* stats, double count, const float* gamma, const float* mean,
                      const float* invstd, float* coef_a, float* coef_b, float* coef_c, float* dgamma,
                      float* dbeta, int c, pssr_stream_t stream);
int pssr_bn_bwd_apply(const void* g, int g_cs, int g_co, const void* y, int y_cs, int y_co,
                      const float* coef_a, const float* coef_b, const float* coef_c,
                      void* dy, int dy_cs, int dy_co, int64_t npix, int c, int dtype, pssr_stream_t stream);

/* Input stage of ResUNet.forward (resunet.py:66-70) fused with the im2col of the 3x3 neighbourhood:
 * xcol[n,y,x, ch*9+tap] = ((x[n,ch,y+ky-1,x+kx-1]*pre_scale+pre_shift)*scale[ch]+shift[ch]), zero
 * outside the image, channels [9c, xc) zero.  The first conv, the first respass and the input
 * channel of Reconstruction.pre then run as flat-K 1x1 convolutions over xcol. */
int pssr_input_im2col(const float* x_nchw, void* xcol, int n, int c, int h, int w, int xc,
                      float pre_scale, float pre_shift, const float* scale, const float* shift,
                      int dtype, pssr_stream_t stream);
/* backward of the above for the parameters of ResUNet.norm: folds d(xcol) (two optional sources)
 * onto the normalised input and accumulates stats = [sum dx0, sum dx0*xhat0] per input channel. */
int pssr_input_norm_bwd(const void* dxcol_a, const void* dxcol_b, int xc, const float* x_nchw,
                        float pre_scale, float pre_shift, const float* mean, const float* invstd,
                        int n, int c, int h, int w, double* stats, int dtype, pssr_stream_t stream);

/* F.max_pool2d(x, 2) (resunet.py:76) and its gradient; the gradient goes to the first maximum of
 * each window and is added to `dskip` (the skip-connection gradient of the same tensor, may be NULL). */
/* Same with a third, optional gradient source: the patchify stem of RDNet (pssr_input_patchify below).  Any of
 * dxcol_a / dxcol_b / dpatch may be NULL (not all three). */
int pssr_input_norm_bwd2(const void* dxcol_a, const void* dxcol_b, int xc, const void* dpatch, int pc, int patch,
                         const float* x_nchw, float pre_scale, float pre_shift, const float* mean, const float* invstd,
                         int n, int c, int h, int w, double* stats, int dtype, pssr_stream_t stream);

int pssr_maxpool2(const void* in, int in_cs, int in_co, void* out, int out_cs, int out_co,
                  int n, int h, int w, int c, int dtype, pssr_stream_t stream);
int pssr_maxpool2_bwd(const void* act, int act_cs, int act_co, const void* dpool, int dp_cs, int dp_co,
                      const void* dskip, int ds_cs, int ds_co, void* dout, int do_cs, int do_co,
                      int n, int h, int w, int c, int dtype, pssr_stream_t stream);

/* F.pixel_shuffle(x, r) (resunet.py:82) written straight into a channel slice of the concat buffer
 * (torch.cat at resunet.py:84 is never materialised separately); inverse=1 is the gradient. */
int pssr_pixel_shuffle(const void* lo, int lo_cs, int lo_co, void* hi, int hi_cs, int hi_co,
                       int n, int h, int w, int c_hi, int r, int inverse, int dtype, pssr_stream_t stream);

/* backward of "relu(bn(y) + r)" (ResBlock tail, _blocks.py:40): dz = dout*(out>0) and
 * stats += [sum dz, sum dz*xhat(y)] for the BatchNorm in front of the addition. */
int pssr_relu_bwd_stats(const void* dout, int do_cs, int do_co, const void* out, int o_cs, int o_co,
                        const void* y, int y_cs, int y_co, const float* mean, const float* invstd,
                        void* dz, int dz_cs, int dz_co, double* stats, int64_t npix, int c, int dtype,
                        pssr_stream_t stream);

/* The same with the gradient of the block output formed in the loader instead of read from a tensor (16-bit storage, c a power of two;
 * PSSR_ERR_UNSUPPORTED otherwise -- the caller then runs the separate kernels):
 *   _pool:      d(out) = dskip + route(dpool): the block output feeds F.max_pool2d(x, 2) (resunet.py:76, first maximum in row-major
 *               window order takes the gradient, as torch) and the decoder's skip connection (resunet.py:84); h, w even
 *   _unshuffle: d(out)[n, y, x, 4 ch + 2 i + j] = dhi[n, 2 y + i, 2 x + j, ch]: the block output went through F.pixel_shuffle(x, 2)
 *               (resunet.py:82) into the first c / 4 channels of the next level's concat buffer; c >= 32
 * dz is bit for bit what pssr_maxpool2_bwd / pssr_pixel_shuffle(inverse) followed by pssr_relu_bwd_stats write. */
int pssr_relu_bwd_stats_pool(const void* dpool, int dp_cs, int dp_co, const void* dskip, int ds_cs, int ds_co,
                             const void* out, int o_cs, int o_co, const void* y, int y_cs, int y_co,
                             const float* mean, const float* invstd, void* dz, int dz_cs, int dz_co, double* stats,
                             int n, int h, int w, int c, int dtype, pssr_stream_t stream);
int pssr_relu_bwd_stats_unshuffle(const void* dhi, int dh_cs, int dh_co, const void* out, int o_cs, int o_co,
                                  const void* y, int y_cs, int y_co, const float* mean, const float* invstd,
                                  void* dz, int dz_cs, int dz_co, double* stats, int n, int h, int w, int c, int dtype,
                                  pssr_stream_t stream);

/* out[row][c] += sum over pixels (bias gradients); out is a statistic buffer of PSSR_STAT_ROWS x c doubles */
int pssr_channel_sum_nhwc(const void* x, int cs, int co, int64_t npix, int c, double* out, int dtype,
                          pssr_stream_t stream);
/* f32 NCHW -> NHWC in the compute dtype, scaled, channels [c, out_cs) zero (gradient of the output) */
int pssr_nchw_to_nhwc(const float* in, void* out, int n, int c, int64_t hw, int out_cs, float scale,
                      int dtype, pssr_stream_t stream);
/* np.clip(x, 0, 255).astype(np.uint8): truncation toward zero (pssr/predict.py:245-246) */
int pssr_clip_u8(const float* in, uint8_t* out, int64_t n, pssr_stream_t stream);
/* out[i] (+)= sum over `stripes` copies in[k*n + i] */
int pssr_f64_to_f32(const double* in, float* out, int n, int accumulate, int stripes, pssr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * SSIM / MS-SSIM + Gaussian-L1 loss (pssr/util.py:10-52; pytorch_msssim 1.0.0 algorithm) on f32
 * NCHW planes [planes = N*C][h][w].  `win_host` is a HOST array of k (odd, <= 33) filter taps.
 * One level forward: sums[plane*2+0] += sum of the cs map, sums[plane*2+1] += sum of the ssim map
 * over the (h-k+1)x(w-k+1) valid region; optional l1_sum += sum_q |x-y|(q) * S(q), S = zero-padded
 * window mass (the mean over the padded G (*) |x-y| map of pssr/util.py:50 without materialising it). */
int pssr_ssim_level_fwd(const float* x, const float* y, int planes, int h, int w, const float* win_host,
                        int k, float c1, float c2, double* sums, double* l1_sum, pssr_stream_t stream);
/* F.avg_pool2d(kernel 2, padding = size % 2) between MS-SSIM levels */
int pssr_avgpool2_planes(const float* in, float* out, int planes, int h, int w, pssr_stream_t stream);
/* loss value and the per-plane, per-level upstream weights of the map elements (device side, no
 * host sync): ms=1 -> prod_l relu(v_l)^w_l with v_l = cs mean (ssim mean at the last level);
 * ms=0 -> plain SSIM mean.  loss = mix*(1-mean) + (1-mix)*l1 (l1_sum may be NULL when mix == 1). */
int pssr_msssim_weights(const double* sums, int levels, int planes, const double* nvalid,
                        const float* level_weights, int ms, float mix, const double* l1_sum,
                        double l1_numel, const float* grad_out, float* loss_out, float* wts,
                        float* l1_coef, pssr_stream_t stream);
/* gradient of one level wrt x: transposed Gaussian filtering of the three adjoint maps, plus the
 * avg-pool gradient from the coarser level (dcoarse, may be NULL) and the L1 term (l1_coef, device
 * scalar, may be NULL). */
int pssr_ssim_level_bwd(const float* x, const float* y, int planes, int h, int w, const float* win_host,
                        int k, float c1, float c2, const float* wts, int use_ssim, const float* dcoarse,
                        int hc, int wc, const float* l1_coef, float* dx, pssr_stream_t stream);

/* The same pair with the per-position derivatives kept between the passes (training; 11-tap window only): the forward also stores
 * `adj` = [planes][3][h][w] f32 -- d(cs or ssim map)/d(mu_x, E[x^2], E[xy]) at every valid position, per unit of upstream weight
 * (use_ssim: the last MS-SSIM level / plain SSIM) -- and the backward filters those three maps instead of recomputing the five
 * forward maps on a 20-pixel-wider halo first (78 k instead of 295 k multiply-adds per 32 x 32 tile).  Same values as the pair above
 * up to the rounding of one reassociated product. */
int pssr_ssim_level_fwd_adj(const float* x, const float* y, float in_div, int planes, int h, int w, const float* win_host, int k,
                            float c1, float c2, int use_ssim, double* sums, double* l1_sum, int stripes, int64_t stripe_stride,
                            float* adj, pssr_stream_t stream);
/* `sums` / `l1_sum` of pssr_ssim_level_fwd_adj are 2 x `stripes` copies `stripe_stride` doubles apart (a workgroup adds the two exact
 * pieces of each of its sums -- see PSSR_STAT_ROWS -- to copy s and copy stripes + s:
 * a 512^2 x 32 level ends with 8192 workgroups); pssr_msssim_weights_striped folds them in a fixed order into `folded`
 * ([levels * planes * 2 + 1] doubles) before doing what pssr_msssim_weights does.  It folds for every stripes >= 1: with one stripe
 * the two pieces of a sum still lie stripe_stride apart (pssr_msssim_weights, which does not fold, is for sums that
 * pssr_ssim_level_fwd wrote, or pssr_ssim_level_fwd_adj with stripes = 1 and stripe_stride = 0).
 * The L1 term's border mass S(q) is summed from the taps as they are indexed, which is the zero-padded window mass only for a
 * symmetric window (win[t] == win[k-1-t]); the SSIM maps and their gradient take any window (a correlation, as F.conv2d). */
int pssr_msssim_weights_striped(const double* sums, int stripes, int64_t stripe_stride, double* folded, int levels, int planes,
                                const double* nvalid, const float* level_weights, int ms, float mix, const double* l1_sum,
                                double l1_numel, const float* grad_out, float* loss_out, float* wts, float* l1_coef,
                                pssr_stream_t stream);
int pssr_ssim_level_bwd_adj(const float* x, const float* y, float in_div, const float* adj, int planes, int h, int w,
                            const float* win_host, int k, const float* wts, const float* dcoarse, int hc, int wc,
                            const float* l1_coef, float* dx, pssr_stream_t stream);
/* in_div (1 = none): the pair works on x / in_div and y / in_div (as torch evaluates `hr_hat / 255` of pssr/train.py:101: a
 * multiplication by the f32 reciprocal)
 * without those tensors existing, and dx is the gradient wrt the UNdivided x; pssr_avgpool2_planes_div makes the next level's inputs
 * from the undivided level-0 maps the same way. */
int pssr_avgpool2_planes_div(const float* in, float in_div, float* out, int planes, int h, int w, pssr_stream_t stream);
/* both pyramids of the loss (prediction and target) in one launch */
int pssr_avgpool2_pair_div(const float* x, const float* y, float in_div, float* xo, float* yo, int planes, int h, int w,
                           pssr_stream_t stream);

/* torch.optim.AdamW step (decoupled weight decay) over flat f32 buffers; `step` is 1-based.  p, g, m and v must be 16-byte
 * aligned when n >= 4 (all three entry points; pssr_amp_check asks it of g for every n): PSSR_ERR_ARG otherwise, nothing is launched. */
int pssr_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                    float beta2, float eps, float weight_decay, int64_t step, float grad_scale,
                    pssr_stream_t stream);
/* hipGraph-safe variant: `state` is a device int64[2] = {step, lr as f32 bits}; the call increments the
 * step on the stream and the update kernel reads both from memory (nothing is frozen at capture). */
int pssr_adamw_step_dev(float* p, const float* g, float* m, float* v, int64_t n, int64_t* state,
                        float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                        pssr_stream_t stream);
/* Dynamic loss scaling without the host (fp16 storage, BASELINE config 4; the reference trains in fp32: no upstream counterpart;
 * policy = torch.amp.GradScaler's).  `amp` is a device int32[4]: [0] loss scale (f32 bits) -- the caller multiplies the loss by it --,
 * [1] good steps in a row, [2] steps skipped, [3] a gradient of the current step is not finite.
 *   pssr_amp_check       sets amp[3] when any of the n gradients is inf / NaN.
 *   pssr_adamw_step_amp  pssr_adamw_step_dev with the gradients divided by the scale; when amp[3] is set neither the step count nor a
 *                        parameter moves; afterwards the scale is multiplied by `backoff` (skipped step) or, every `interval` good
 *                        steps, by `growth`, and amp[3] is cleared.  Everything in stream order: a whole fp16 step replays as a graph. */
int pssr_amp_check(const float* g, int64_t n, int32_t* amp, pssr_stream_t stream);
int pssr_adamw_step_amp(float* p, const float* g, float* m, float* v, int64_t n, int64_t* state,
                        float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                        int32_t* amp, float growth, float backoff, int interval, pssr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Pair generation / crappifiers (pssr/data.py:471-495, pssr/crappifiers.py).
 */
/* PIL.Image.resize(BILINEAR) of uint8 planes [planes][H][W] -> [planes][h][w], bit-exact with Pillow's
 * two-pass 22-bit fixed-point resampler (pssr/data.py:483).  `tmp` holds [planes][H][w] bytes. */
int pssr_bilinear_down_u8(const uint8_t* hr, uint8_t* tmp, uint8_t* lr, int planes, int H, int W,
                          int h, int w, pssr_stream_t stream);
int pssr_u8_to_f32(const uint8_t* in, float* out, int64_t n, pssr_stream_t stream);
/* flags: 1 = clip to [0,255] (MultiCrappifier, crappifiers.py:41-42); 2 = np.round (half-to-even) then
 * clip (data.py:487).  Noise comes from Philox4x32-10 keyed by (seed, tile_offset + tile) with the pixel
 * index as counter, so results do not depend on batching or on the number of GPUs.
 * AdditiveGaussian (crappifiers.py:62-64): out = in + N(gain, sigma), sigma = max(N(intensity, spread), 0)
 * per tile; `noise` (f64, may be NULL) injects a pre-drawn field instead (exact-parity tests). */
int pssr_crappify_gaussian(const float* in, float* out, int tiles, int64_t per_tile, float intensity,
                           float gain, float spread, uint64_t seed, uint64_t tile_offset,
                           const double* noise, int flags, const uint64_t* tile_counter,
                           pssr_stream_t stream);
/* Poisson (crappifiers.py:81-86): out = x*(1-i) + Poisson(max(x,0))*i + gain */
int pssr_crappify_poisson(const float* in, float* out, int tiles, int64_t per_tile, float intensity,
                          float gain, float spread, uint64_t seed, uint64_t tile_offset, int flags,
                          const uint64_t* tile_counter, pssr_stream_t stream);
/* The same mix with the Poisson samples handed in (f64 [n], e.g. numpy's legacy-stream draws of the reference run): numpy's
 * arithmetic of pssr/crappifiers.py:81-86 exactly (x*(1-i) in float32, y*i and the sums in float64), then flags (pssr/data.py:487).
 * For exact-parity tests, like `noise` of pssr_crappify_gaussian; `intensity` / `gain` are the Python floats, undrawn. */
int pssr_crappify_poisson_samples(const float* in, const double* samples, float* out, int64_t n, double intensity,
                                  double gain, int flags, pssr_stream_t stream);
/* `tile_counter` (device, may be NULL) is added to tile_offset inside the kernel, so a captured hipGraph
 * draws fresh noise on every replay; pssr_counter_add advances it on the stream. */
int pssr_counter_add(uint64_t* counter, uint64_t inc, pssr_stream_t stream);
/* Blur (crappifiers.py:122-124): per-plane separable Gaussian, edge replicate, radius int(4*sigma+.5) */
int pssr_gaussian_blur(const float* in, float* tmp, float* out, int planes, int h, int w, float sigma,
                       float gain, int flags, pssr_stream_t stream);

/* SaltPepper (pssr/crappifiers.py:88-105): clip(x + gain, 0, 255), then `amount` (a fraction, per-tile max(N(amount, spread), 0)) of
 * the pixels becomes 255 or 0 with equal probability; Philox stream as the other noises; flags as pssr_crappify_gaussian. */
int pssr_crappify_saltpepper(const float* in, float* out, int tiles, int64_t per_tile, float amount, float gain, float spread,
                             uint64_t seed, uint64_t tile_offset, int flags, const uint64_t* tile_counter, pssr_stream_t stream);
/* Blur(spread > 0) (pssr/crappifiers.py:107-124): every tile of planes_per_tile frames is blurred with its own
 * sigma = max(N(sigma, spread), 0) drawn from the tile's Philox stream (sigma <= 0: the tile is only offset by gain). */
int pssr_gaussian_blur_tiles(const float* in, float* tmp, float* out, int tiles, int planes_per_tile, int h, int w, float sigma,
                             float spread, float gain, uint64_t seed, uint64_t tile_offset, int flags, const uint64_t* tile_counter,
                             pssr_stream_t stream);
/* Geometry of _gen_pair (pssr/data.py:471-482) for a batch of uint8 stacks resident in HBM: centred square crop to at most
 * `res`, np.pad(mode="reflect") up to res at the bottom / right, np.rot90 in the image plane when rot != 0, np.flip along
 * flip_axis (0 frames, 1 rows, 2 columns, 3 rows and columns, -1 none).  The random draws (rot, flip_axis) stay on the host in the reference's
 * order; out is uint8 [n_items][c][res][res]. */
typedef struct pssr_gather_item { const uint8_t* src; int sh, sw, rot, flip_axis; } pssr_gather_item;
int pssr_gen_pair_geometry_u8(const pssr_gather_item* items_dev, int n_items, uint8_t* out, int c, int res, pssr_stream_t stream);
/* Sliding windows of image sheets resident in HBM (pssr/data.py:629-660 `_sliding_window` / `_slice_image`, then the rot90 / flip of
 * `_gen_pair`): out[i][f] = sheet[frame0 + f][y0 : y0 + res, x0 : x0 + res] of sheets_dev[items_dev[i].sheet], np.rot90 in the
 * image plane when rot != 0, np.flip along flip_axis (as pssr_gather_item).  Sheets are uint8 [frames][h][w], contiguous, of any
 * size each; both tables live on the device; out is uint8 [n_items][c][res][res].  Windows are always whole: an item whose sheet
 * index, frame range [frame0, frame0 + c) or window leaves its sheet is written as zeros and reads nothing.  n_items <= 65535.
 * 16-byte stores when res % 16 == 0 and out is 16-byte aligned (sheet rows may be misaligned); byte accesses otherwise. */
typedef struct pssr_sheet_desc { const uint8_t* base; int frames, h, w, reserved; } pssr_sheet_desc;      /* 24 bytes */
typedef struct pssr_window_item { int sheet, frame0, y0, x0, rot, flip_axis; } pssr_window_item;           /* 24 bytes */
int pssr_gather_windows_u8(const pssr_sheet_desc* sheets_dev, int n_sheets, const pssr_window_item* items_dev, int n_items,
                           uint8_t* out, int c, int res, pssr_stream_t stream);

/* Collage rows of predict_collage (pssr/predict.py:85-142; `_collage_preds` / `_image_stack`, pssr/predict.py:213-243): for each of
 * n_images images one row of n_panels (1..3) panels of h x w pixels side by side in a uint8 canvas resident in HBM,
 *   canvas[(row0 + i) * h + y][p * w + x] = panel_p(i)[yi_p[y]][xi_p[x]],
 * canvas rows canvas_pitch >= n_panels * w bytes apart; the caller provides (row0 + n_images) * h of them.  `panels` is a HOST array
 * (it travels as a kernel argument).  A panel is a strided view: `src` points at pixel (0, 0) of image 0 (it already selects channel,
 * frame and crop), image i lies image_stride elements further, rows row_pitch elements apart; src_h x src_w is what may be read.
 * Pixels are uint8, or (is_f32) float32 turned into fminf(fmaxf(v, 0), 255) truncated toward zero as pssr_clip_u8 does.  yi / xi:
 * device int32 tables of h / w source indices (PIL.Image.resize(NEAREST): pssr/predict.py:228), both NULL = the identity.  An index
 * outside [0, src_h) / [0, src_w) writes 0 for that byte and reads nothing.  n_images <= 65535.  16-byte stores when w % 16 == 0 and
 * canvas and canvas_pitch are 16-byte aligned (16-byte loads for identity panels whose source rows are); byte accesses otherwise. */
typedef struct pssr_collage_panel {
    const void* src; int64_t image_stride; int32_t row_pitch, src_h, src_w, is_f32; const int32_t* yi; const int32_t* xi;
} pssr_collage_panel;                                                                                       /* 48 bytes */
int pssr_collage_rows_u8(const pssr_collage_panel* panels, int n_panels, uint8_t* canvas, int64_t canvas_pitch, int row0, int n_images,
                         int h, int w, pssr_stream_t stream);

/* Shifted-window attention of SwinIR (pssr/models/swinir.py:345-385 SwinTransformerBlock.forward, :563-594 WindowAttention.forward)
 * on the un-rolled, un-windowed token tensor.  qkv [B, H, W, 3C] contiguous, channel which * C + head * hd + d (which = 0 q, 1 k,
 * 2 v; hd = C / heads): the qkv Linear applied per token.  out [B, H, W, C], channel head * hd + d, original token order, dtype of
 * qkv.  lse [B, heads, H, W] float32: the log-sum-exp of every query row.  Per (window, head):
 *   S = (q * scale) k^T + bias_table[rel(i, j)] + mask(i, j),  P = softmax_j S,  O = P v,
 * bias_table [(2 ws - 1)^2, heads] float32, rel(i, j) = (ri - rj + ws - 1) (2 ws - 1) + (ci - cj + ws - 1).  The cyclic shift
 * (-shift, -shift), the window partition (row-major tokens inside a window), its reverse and the shift back are addressing; the mask
 * of calculate_mask is computed from the coordinates: -100.0f is added where the regions of the two tokens differ and shift > 0.
 * Takes 1 <= ws <= 8, H % ws == W % ws == 0, 0 <= shift < ws, C % heads == 0, hd <= 32, dtype PSSR_F32 or PSSR_BF16 (S, the softmax,
 * all sums and lse in float32 for both); PSSR_ERR_ARG otherwise.  16-byte loads when hd * sizeof(element) is a multiple of 16 and the
 * tensors are 16-byte aligned, element loads otherwise.
 * Backward: P is recomputed from q, k and lse.  dqkv [B, H, W, 3C] (dtype of qkv) is written in full; dbias_table
 * [(2 ws - 1)^2, heads] float32 is written (not accumulated): per-workgroup sums go to `workspace`
 * (pssr_window_attn_workspace_bytes(...) bytes, 4-byte aligned) and a second launch adds them in a fixed order -- no atomics, the same
 * bits on every run. */
int64_t pssr_window_attn_workspace_bytes(int B, int H, int W, int heads, int ws);        /* negative = PSSR_ERR_ARG */
int pssr_window_attn_fwd(const void* qkv, const float* bias_table, void* out, float* lse, int B, int H, int W, int C, int heads, int ws,
                         int shift, float scale, int dtype, pssr_stream_t stream);
int pssr_window_attn_bwd(const void* qkv, const float* bias_table, const float* lse, const void* dout, void* dqkv, float* dbias_table,
                         void* workspace, int64_t workspace_bytes, int B, int H, int W, int C, int heads, int ws, int shift, float scale,
                         int dtype, pssr_stream_t stream);


/* ---------------------------------------------------------------------------------------------
 * Atrous / PSP-pooling model variants (pssr/models/_blocks.py:43-92 ResBlockA, PSP_Pooling).
 * A dilated 3x3 convolution (Conv2d(kernel_size=3, padding="same", dilation=d), _blocks.py:55) = pssr_im2col_dil + the 1x1
 * kernels of pssr_conv2d / pssr_conv2d_wgrad over K = 9 * cp (weights packed with mode 4; mode 5 for the input gradient) +
 * pssr_col2im_dil.  Tensors are NHWC slices (pointer, channel stride, channel offset) in the compute dtype.
 */
/* out[n, y, x, ci] = x_nchw * pre_scale + pre_shift (ci < c), 0 for c <= ci < out_cs: the network input "x / 128 - 1"
 * (resunet.py:66) of the atrous models, which have no input BatchNorm (resunet.py:50) */
int pssr_input_plain(const float* x_nchw, void* out, int n, int c, int h, int w, int out_cs, float pre_scale, float pre_shift,
                     int dtype, pssr_stream_t stream);
/* col[pixel][t * cp + ci] = act(in[pixel + ((t / 3 - 1) * dil, (t % 3 - 1) * dil)][ci]), zero outside the image and for
 * c <= ci < cp; act = relu(v * scale[ci] + shift[ci]) rounded to the compute dtype (the pre-activation BatchNorm + ReLU of
 * ResBlockA, _blocks.py:52-55) or the identity when scale == shift == NULL.  col: [n][h][w][9 * cp]. */
int pssr_im2col_dil(const void* in, int in_cs, int in_co, int c, const float* scale, const float* shift, void* col, int cp,
                    int n, int h, int w, int dil, int dtype, pssr_stream_t stream);
/* Gradient of the above: out[pixel][ci] = sum_t dcol[pixel - off_t][t * cp + ci].  With y != NULL the ReLU mask of the
 * pre-activation (y * scale + shift > 0) is applied; with stats != NULL also stats[stripe][0:c] += sum g,
 * stats[stripe][c:2c] += sum g * (y - mean) * invstd (f64 statistic buffer of PSSR_STAT_ROWS rows, caller-zeroed): the inputs of
 * pssr_bn_bwd_coefs for the BatchNorm in front of the ReLU. */
int pssr_col2im_dil(const void* dcol, int cp, void* out, int out_cs, int out_co, int c, int n, int h, int w, int dil,
                    const void* y, int y_cs, int y_co, const float* scale, const float* shift, const float* mean,
                    const float* invstd, double* stats, int dtype, pssr_stream_t stream);
/* stats[stripe][0:c] += sum x, stats[stripe][c:2c] += sum x^2 over the pixels of an NHWC slice: batch statistics of a
 * BatchNorm that normalises an existing tensor (the first BatchNorm of every ResBlockA branch, the BatchNorms of PSP_Pooling) */
int pssr_channel_stats_nhwc(const void* x, int cs, int co, int c, int64_t npix, double* stats, int dtype, pssr_stream_t stream);
/* out = sum of n_in (1..8) NHWC slices, then ReLU if relu != 0: "relu(sum(branches) + respass)" (_blocks.py:67).  ins / in_cs /
 * in_co are HOST arrays. */
int pssr_sum_relu(const void* const* ins, const int* in_cs, const int* in_co, int n_in, void* out, int out_cs, int out_co,
                  int64_t npix, int c, int relu, int dtype, pssr_stream_t stream);
/* dz = dout where out > 0 else 0 (gradient of a ReLU from its output) */
int pssr_relu_mask(const void* dout, int do_cs, int do_co, const void* out, int o_cs, int o_co, void* dz, int dz_cs, int dz_co,
                   int64_t npix, int c, int dtype, pssr_stream_t stream);
/* out = relu(x * scale[c] + shift[c]): F.relu(BatchNorm(x)) of PSP_Pooling (_blocks.py:88,91) */
int pssr_affine_relu(const void* x, int cs, int co, const float* scale, const float* shift, void* out, int out_cs, int out_co,
                     int64_t npix, int c, int dtype, pssr_stream_t stream);
/* F.max_pool2d(x, kernel_size=k) (_blocks.py:87; floor mode: out is [n][h / k][w / k][c]) and its gradient (to the first
 * maximum of each window in row-major order, zero for pixels outside every window) */
int pssr_maxpool_k(const void* in, int in_cs, int in_co, void* out, int out_cs, int out_co, int n, int h, int w, int c, int k,
                   int dtype, pssr_stream_t stream);
int pssr_maxpool_k_bwd(const void* act, int act_cs, int act_co, const void* dpool, int dp_cs, int dp_co, void* dx, int dx_cs,
                       int dx_co, int n, int h, int w, int c, int k, int dtype, pssr_stream_t stream);
/* F.interpolate(x, size=(h, w), mode="bilinear") (align_corners=False, _blocks.py:87) from [n][hs][ws][c] and its gradient */
int pssr_bilinear_up(const void* in, int in_cs, int in_co, void* out, int out_cs, int out_co, int n, int hs, int ws, int h, int w,
                     int c, int dtype, pssr_stream_t stream);
int pssr_bilinear_up_bwd(const void* dout, int do_cs, int do_co, void* din, int di_cs, int di_co, int n, int hs, int ws, int h,
                         int w, int c, int dtype, pssr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * RDNet encoder of RDResUNet (pssr/models/_rdnet.py, pssr/models/rdresunet.py:84).  The 1x1 convolutions of its
 * blocks and transitions run on pssr_conv2d / pssr_conv2d_wgrad (taps = 1; PSSR_PRO_GELU / PSSR_EPI_DGRAD_GELU fuse
 * nn.GELU); the kernels below are the HBM-bound remainder.  torch.cat of the dense features (_rdnet.py:132-138,
 * 169-170) is elided: every op reads / writes a channel slice (pointer, channel stride, channel offset).
 */
/* PatchifyStem input (_rdnet.py:110-111 seen as a 1x1 conv over patches): xpatch[n, y/ps, x/ps, ci*ps*ps + (y%ps)*ps + x%ps]
 * = (x*pre_scale + pre_shift)*scale[ci] + shift[ci]  (input scaling + input BatchNorm, rdresunet.py:105-107); `pc` =
 * channel stride (>= c*ps*ps, multiple of 16, rest zero).  Pack the stem weight with mode 2. */
int pssr_input_patchify(const float* x_nchw, void* xpatch, int n, int c, int h, int w, int ps, int pc,
                        float pre_scale, float pre_shift, const float* scale, const float* shift, int dtype,
                        pssr_stream_t stream);
/* Depthwise 7x7 conv, stride 1, zero padding 3 (nn.Conv2d(C, C, groups=C, kernel_size=7, padding=3), _rdnet.py:182,197).
 * pssr_dwconv7_pack: torch weight [C,1,7,7] f32 -> [49][C] f32 (flip = 1: rotated by 180 degrees, for the input gradient).
 * pssr_dwconv7: out (+)= bias + conv(in, packed)  (accumulate = 1 adds into `out`: the gradient of a dense-stage input
 * that several blocks read).  Weight gradient, dw[C][49] += sum_pixels dy * shifted x, in two forms:
 * pssr_dwconv7_wgrad (any w) adds every workgroup's partial sums to dw with f32 atomics, so the order of the additions and
 * the last bits of the result vary from run to run (one kernel for w % 8 != 0, a row-segment kernel for w % 8 == 0);
 * pssr_dwconv7_wgrad_ws (w % 8 == 0 only) uses no atomics -- the row-segment kernel writes one [C][49] slab per workgroup
 * into `workspace` (pssr_dwconv7_wgrad_workspace_bytes) and a second kernel adds the slabs to dw in a fixed order:
 * reproducible bit for bit, and not bound by the L2 atomic rate (2.7 M atomics on 21 k addresses cost ~150 us whatever
 * the map size).  Both add to what dw holds (the caller zeroes it or keeps a running gradient). */
int pssr_dwconv7_pack(const float* w, float* packed, int c, int flip, pssr_stream_t stream);
/* pssr_dwconv7_pack of up to PSSR_DWPACK_BATCH_MAX weights by one launch (every block's forward and 180-degree-rotated copy: the
 * depthwise weights of pssr/models/rdnet.py:71-73 change once per optimizer step). */
#define PSSR_DWPACK_BATCH_MAX 48
typedef struct pssr_dwpack_batch {
    const float* w[PSSR_DWPACK_BATCH_MAX];
    float* packed[PSSR_DWPACK_BATCH_MAX];
    int32_t c[PSSR_DWPACK_BATCH_MAX];
    int32_t flip[PSSR_DWPACK_BATCH_MAX];
} pssr_dwpack_batch;
int pssr_dwconv7_pack_batch(const pssr_dwpack_batch* items, int n_items, pssr_stream_t stream);
int pssr_dwconv7(const void* in, int in_cs, int in_co, const float* w_packed, const float* bias, void* out, int out_cs,
                 int out_co, int n, int h, int w, int c, int accumulate, int dtype, pssr_stream_t stream);
int pssr_dwconv7_wgrad(const void* dy, int dy_cs, int dy_co, const void* x, int x_cs, int x_co, float* dw, int n, int h,
                       int w, int c, int dtype, pssr_stream_t stream);
int64_t pssr_dwconv7_wgrad_workspace_bytes(int n, int h, int w, int c);
int pssr_dwconv7_wgrad_ws(const void* dy, int dy_cs, int dy_co, const void* x, int x_cs, int x_co, float* dw, int n, int h,
                          int w, int c, int dtype, void* workspace, int64_t workspace_bytes, pssr_stream_t stream);
/* timm LayerNorm2d (_rdnet.py:60,112,183,198): layer norm over the C channels of every pixel, eps inside the sqrt, affine.
 * Channels [c, c_pad) of the output are written as zeros (K padding of the following 1x1 conv).  s2d = 1 writes the
 * 2x2 space-to-depth layout out[n, y/2, x/2, ((y&1)*2 + (x&1))*c_pad + ch], which makes the stride-2 transition conv
 * (_rdnet.py:56-62) a 1x1 conv over 4*c_pad channels (weights packed with mode 4).  mean / rstd: f32 [n*h*w], kept for
 * the backward pass (NULL in inference).
 * Backward: dx (+)= rstd*(g*gamma - mean_c(g*gamma) - xhat*mean_c(g*gamma*xhat)); stats[stripe][0..C) += sum g*xhat
 * (dgamma), stats[stripe][C..2C) += sum g (dbeta), f64 statistic buffer of PSSR_STAT_ROWS rows, caller-zeroed. */
int pssr_layernorm2d_fwd(const void* in, int in_cs, int in_co, const float* gamma, const float* beta, float eps, void* out,
                         int out_cs, int out_co, int s2d, int c_pad, int n, int h, int w, int c, float* mean, float* rstd,
                         int dtype, pssr_stream_t stream);
int pssr_layernorm2d_bwd(const void* g, int g_cs, int g_co, int s2d, int c_pad, const void* x, int x_cs, int x_co,
                         const float* gamma, const float* mean, const float* rstd, void* dx, int dx_cs, int dx_co,
                         int accumulate, int n, int h, int w, int c, double* stats, int dtype, pssr_stream_t stream);
/* out[img][c] += scale * sum_{pixels of img} a*b (b may be NULL: plain sum): the spatial mean of timm's
 * EffectiveSEModule (x.mean((2,3))) and the per-image reductions of its backward.  One workgroup per (image, 32 channels) sums all the
 * image's pixels in a fixed order: the same bits on every run, nothing but `out` written. */
int pssr_image_channel_dot(const void* a, int a_cs, int a_co, const void* b, int b_cs, int b_co, int n, int hw, int c,
                           float scale, float* out, int dtype, pssr_stream_t stream);
/* Entry points of the earlier version that met through a workspace: the workspace size is now 0 and `workspace` is ignored. */
int64_t pssr_image_channel_dot_workspace_bytes(int n, int hw, int c);
int pssr_image_channel_dot_ws(const void* a, int a_cs, int a_co, const void* b, int b_cs, int b_co, int n, int hw, int c,
                              float scale, float* out, int dtype, void* workspace, int64_t workspace_bytes, pssr_stream_t stream);
/* EffectiveSEModule gate: u = fc(s) (1x1 conv on the [N, C] means), gate = hard_sigmoid(u) = relu6(u + 3)/6. */
int pssr_ese_gate(const float* s_mean, const float* w_fc, const float* b_fc, int n, int c, float* u, float* gate,
                  pssr_stream_t stream);
/* out[p, c] = t[p, c] * gate[img][c] * gamma[c] + add[img][c]  (gate / add may be NULL): ESE gating and the layer
 * scale of DenseBlock.forward (_rdnet.py:173-174) written at the block's channel offset of the stage buffer; with
 * `add` it is also the backward of both. */
int pssr_scale_nc(const void* t, int t_cs, int t_co, const float* gate, const float* gamma, const float* add, void* out,
                  int out_cs, int out_co, int n, int hw, int c, int dtype, pssr_stream_t stream);
/* Backward of gate + layer scale on the [N, C] side tensors, A[n][c] = sum_pixels dout*t (pssr_image_channel_dot):
 * dgamma, d fc.bias, d fc.weight and add[n][c] = (1/hw) * W^T du, the per-image term of dt.  gate == NULL: plain
 * layer scale (dgamma = sum_n A only). */
int pssr_ese_bwd(const float* A, const float* gate, const float* u, const float* gamma, const float* s_mean,
                 const float* w_fc, int n, int c, int hw, float* du, float* dgamma, float* db_fc, float* dw_fc, float* add,
                 pssr_stream_t stream);

/* Second half of PSSR_EPI_HEADQ / PSSR_FLAG_HEADQ: out_f32_nchw[n][0][Y][X] = (bias + sum over the 9 taps (ky, kx) of
 * q[tap] at high-resolution pixel (Y + ky - 1, X + kx - 1), zero outside the image) * out_scale + out_shift, high-resolution pixel
 * (4 y + i, 4 x + j) being sub-pixel 4 i + j of low-resolution pixel (y, x)  (F.pixel_shuffle + Reconstruction.conv, _blocks.py:17;
 * "x * 128 + 128", resunet.py:94).  h, w: the LOW-resolution size. */
int pssr_head_q_gather(const float* q, const float* bias, float* out_nchw, int n, int h, int w,
                       float out_scale, float out_shift, pssr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Reconstruction.conv (pssr/models/_blocks.py:11,17 + "x*128+128", pssr/models/resunet.py:95) for C_out = 1..3: dedicated
 * streaming kernels (csrc/head_conv.hip) for the conv that reads the largest tensor of the network; bf16 storage only.
 * `act` is the NHWC activation in blocked pixel order (log2 r = blk, see pssr_conv_desc), `g` the incoming f32 NCHW
 * gradient of the network output (scaled by g_scale = the output scale, 128).
 *   fwd:   out_nchw = (conv3x3(act, w) + bias) * out_scale + out_shift
 *   dgrad: dact = (act > 0) * conv3x3_transposed(g * g_scale, w)        (ReLU of Reconstruction.pre fused)
 *   wgrad: dw_oihw += sum_pixels (g * g_scale) (x) shifted act            (f32 atomics into the caller-zeroed gradient)
 */
int pssr_head_conv_fwd(const void* act, int act_cs, int act_co, int blk, const float* w_oihw, const float* bias,
                       float* out_nchw, int n, int h, int w, int cin, int cout, float out_scale, float out_shift,
                       int dtype, pssr_stream_t stream);
int pssr_head_conv_dgrad(const float* g_nchw, float g_scale, const float* w_oihw, const void* act, int act_cs, int act_co,
                         void* dact, int d_cs, int d_co, int blk, int n, int h, int w, int cin, int cout, int dtype,
                         pssr_stream_t stream);
int pssr_head_conv_wgrad(const float* g_nchw, float g_scale, const void* act, int act_cs, int act_co, int blk,
                         float* dw_oihw, int n, int h, int w, int cin, int cout, int dtype, pssr_stream_t stream);
/* dgrad and wgrad in ONE pass over the activation (each tile is read once and used as ReLU mask, as the dW operand and for
 * the optional bias sums): dact and dw_oihw as above (blk <= 2); bias_sum (or NULL) is a caller-zeroed f32
 * [4^blk * cin] that receives sum_pixels dact per (sub-pixel, channel) = per channel of the blocked NHWC tensor viewed at
 * low resolution, i.e. the bias gradient of the pixel-shuffle convolution in front (Reconstruction.pre). */
int pssr_head_conv_bwd(const float* g_nchw, float g_scale, const float* w_oihw, const void* act, int act_cs, int act_co,
                       void* dact, int d_cs, int d_co, int blk, float* dw_oihw, float* bias_sum, int n, int h, int w, int cin,
                       int cout, int dtype, pssr_stream_t stream);

/* The same with order-independent sums (bit-reproducible training): dw_rows [PSSR_STAT_ROWS][cout * cin * 9] and bias_rows (or NULL)
 * [PSSR_STAT_ROWS][4^blk * cin], caller-zeroed f64 statistic buffers; fold them with pssr_f64_to_f32(rows = PSSR_STAT_ROWS). */
int pssr_head_conv_bwd_rows(const float* g_nchw, float g_scale, const float* w_oihw, const void* act, int act_cs, int act_co,
                            void* dact, int d_cs, int d_co, int blk, double* dw_rows, double* bias_rows, int n, int h, int w,
                            int cin, int cout, int dtype, pssr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Backward of the flat-K (im2col) source of a wide convolution in ONE pass over its output gradient (csrc/pre_xcol_bwd.hip;
 * Reconstruction.pre's input-image source, pssr/models/_blocks.py:10,16): for dy [npix][cout], x [npix][kx] and dx [npix][kx] in 16-bit
 * storage (channel strides / offsets in elements) and the f32 weight window W1[k][j] = w[n_perm[k] * w_row + w_off + j]
 * (j < nk <= kx, zero beyond; n_perm NULL: identity), rounded to storage as the packed weights are,
 *   dx[p][j] = sum_k dy[p][k] W1[k][j]   (rounded to storage)      dw[k][j] = sum_p dy[p][k] x[p][j]   (f32 [cout][kx]; feed it to
 *   pssr_unpack_conv_wgrad_parts as one part with k_pad = kx, which applies n_perm and the channel window of the OIHW gradient).
 * Every workgroup stores one partial slab of dw into `slabs` (f32 [parts][cout][kx], parts = pssr_flatk_bwd_pair_parts(npix)) and a
 * second launch sums the slabs in a fixed order: no floating-point atomics, the result is bit-reproducible.
 * pssr_flatk_bwd_pair_supported: bf16 / f16, cout a multiple of 64 up to 1024, kx = 16. */
int pssr_flatk_bwd_pair_supported(int dtype, int cout, int kx);
int pssr_flatk_bwd_pair_parts(int64_t npix);
int pssr_flatk_bwd_pair(const void* dy, int dy_cs, int dy_co, int cout, const void* x, int x_cs, int x_co, void* dx, int dx_cs,
                        int dx_co, int kx, const float* w, int w_row, int w_off, int nk, const int32_t* n_perm, float* slabs,
                        int parts, float* dw, int64_t npix, int dtype, pssr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Whole-sheet prediction on the device (BASELINE config 5).
 * pssr_sliding_tiles_u8: tiles [ntile][c][size][size] f32 = the row-major sliding windows tile0 .. tile0+ntile-1 of a uint8 sheet
 *   [c][h][w] (pssr/data.py:629-638 `_sliding_window` + `_tensor_ready`; stride = size - overlap; remainders dropped).
 * pssr_patch_tiles_u8: sheet [c][n_rows*step+overlap][n_cols*step+overlap] u8 = overlap-averaged stitching of u8 tiles
 *   [n_rows*n_cols][c][size][size] with `margin` pixels trimmed on inner edges, then the uint8 cast (truncation):
 *   pssr/util.py:116-137 `_patch_images` + pssr/util.py:101.  step = size - overlap (all in output pixels).
 */
int pssr_sliding_tiles_u8(const uint8_t* sheet, float* tiles, int c, int h, int w, int size, int stride, int tile0, int ntile,
                          pssr_stream_t stream);
int pssr_patch_tiles_u8(const uint8_t* tiles, uint8_t* sheet, int c, int n_rows, int n_cols, int size, int overlap, int margin,
                        pssr_stream_t stream);
/* The same two steps for a frame stack and for sheets that do not fit the tile grid (predict_sheet's n_frames / slide / cover).
 * pssr_stack_tiles_u8: tiles [ntile][m][size][size] f32 cut from a uint8 stack [frames][h][w].  Tiles are numbered slice-major over
 *   a grid of tiles_y x tiles_x windows per frame slice: for g = tile0 + i, k = g / (tiles_y*tiles_x), t = g % (tiles_y*tiles_x),
 *   ty = t / tiles_x, tx = t % tiles_x and
 *     tiles[i][f][y][x] = (float) stack[k*frame_step + f][fold(ty*stride + y, h)][fold(tx*stride + x, w)],
 *   where fold(i, n) = (j = i mod 2(n-1)) < n ? j : 2(n-1) - j is the source index of np.pad(mode="reflect"): a grid that reaches past
 *   the bottom or the right edge reads the sheet extended by reflection, and no extended copy exists.  Every slice touched must lie
 *   inside the stack (k*frame_step + m <= frames), and an axis the grid leaves needs at least 2 pixels.  With m = frames,
 *   frame_step anything, one slice and a grid inside the sheet this is pssr_sliding_tiles_u8.
 * pssr_patch_stack_u8: out [n_slices][c][out_h][out_w] u8 = the top-left out_h x out_w pixels of pssr_patch_tiles_u8's sheet for each of
 *   n_slices tile sets [n_slices*n_rows*n_cols][c][size][size] (slice-major, as above), in one launch;
 *   1 <= out_h <= n_rows*step+overlap and 1 <= out_w <= n_cols*step+overlap.  Pixels outside the crop are not computed.
 */
int pssr_stack_tiles_u8(const uint8_t* stack, float* tiles, int frames, int h, int w, int m, int frame_step, int size, int stride,
                        int tiles_y, int tiles_x, int tile0, int ntile, pssr_stream_t stream);
int pssr_patch_stack_u8(const uint8_t* tiles, uint8_t* out, int n_slices, int c, int n_rows, int n_cols, int size, int overlap,
                        int margin, int out_h, int out_w, pssr_stream_t stream);
/* predict_sheet's blend / ensemble path: the dihedral self-ensemble and weighted stitching, all in integers.
 * Member d = 0 .. ensemble-1 (ensemble in {1, 2, 4, 8}) of a square plane a is T_d(a) = rot90(d & 4 ? a[..., ::-1] : a, d & 3) in numpy's
 * terms, U_d its inverse.  Items are numbered g = tile * ensemble + d, tile slice-major as in pssr_stack_tiles_u8.
 * pssr_dihedral_tiles_u8: tiles [nitem][m][size][size] f32 = items item0 .. item0 + nitem - 1: pssr_stack_tiles_u8's window of tile
 *   g / ensemble (same reflection, same limits), every frame plane turned by T_(g % ensemble).  ensemble = 1 is pssr_stack_tiles_u8.
 * pssr_clip_u8_dihedral: out [nitem][c][size][size] u8 = pssr_clip_u8's value of in (f32, same layout), plane (i, ch) stored through U_d with
 *   d = (item0 + i) % ensemble: item0 selects the member phase only, both pointers are the batch's.  ensemble = 1 is pssr_clip_u8.
 * pssr_blend_stack_u8: out [n_slices][c][out_h][out_w] u8 from tiles [n_slices*n_rows*n_cols*ensemble][c][size][size] u8 (item order).  With
 *   T = max(overlap - 2 margin, 0) + 1 a tile that is first / last of its grid row or column weighs local coordinate l on that axis by
 *     w1(l) = 0 if (!first && l < margin) || (!last && l >= size - margin), else min(T, first ? T : l - margin + 1, last ? T : size - margin - l)
 *   (blend = 1, "linear"; blend = 0, "average": every non-zero w1 is 1), w(ly, lx) = w1_y(ly) * w1_x(lx), and
 *     out = floor(sum_tiles w * sum_d tiles[..] / (ensemble * sum_tiles w)), 0 where no tile covers the pixel.
 *   Integer arithmetic throughout, no atomics: the same bits on every run.  blend = 0, ensemble = 1 is pssr_patch_stack_u8. */
int pssr_dihedral_tiles_u8(const uint8_t* stack, float* tiles, int frames, int h, int w, int m, int frame_step, int size, int stride,
                           int tiles_y, int tiles_x, int ensemble, int item0, int nitem, pssr_stream_t stream);
int pssr_clip_u8_dihedral(const float* in, uint8_t* out, int nitem, int c, int size, int ensemble, int item0, pssr_stream_t stream);
int pssr_blend_stack_u8(const uint8_t* tiles, uint8_t* out, int n_slices, int c, int n_rows, int n_cols, int size, int overlap,
                        int margin, int out_h, int out_w, int blend, int ensemble, pssr_stream_t stream);
/* The self-ensemble of a batch of square items (predict_images' / test_metrics' ensemble) and the per-pixel spread of the members, in integers.
 * pssr_dihedral_batch_u8 / pssr_dihedral_batch_f32: out [n*ensemble][m][size][size] f32 from in [n][m][size][size] (u8 / f32, contiguous): item
 *   i*ensemble + d = T_d(in[i]), every frame plane turned.  ensemble = 1 is a conversion / a copy.
 * pssr_ensemble_reduce_u8: in [n*ensemble][c][size][size] f32 (that member order) -> mean, spread [n][c][size][size] u8.  With
 *   q[i][d] = U_d(pssr_clip_u8's value of in[i*ensemble + d]) (clip to [0, 255], truncation, NaN gives 0):
 *     mean[i] = floor(sum_d q[i][d] / ensemble),   spread[i] = max_d q[i][d] - min_d q[i][d].
 *   spread may be null (not written).  mean is pssr_clip_u8_dihedral + pssr_blend_stack_u8 of a one-tile sheet without overlap, bit for bit;
 *   ensemble = 1 is pssr_clip_u8 and a zero spread.  The members are never stored: 4*ensemble bytes read, 1 - 2 written per output pixel.
 * pssr_spread_stack_u8: out [n_slices][c][out_h][out_w] u8 from pssr_blend_stack_u8's tiles: max - min of tiles[tile*ensemble + d] over every
 *   member d and every tile that covers the pixel with w1_y * w1_x != 0 (the support is the same for both blends); 0 where no tile does.
 *   Same argument checks as pssr_blend_stack_u8, the crop included.
 * Integer sums, min and max in registers: no atomics, no floating-point accumulation, the same bits on every run. */
int pssr_dihedral_batch_u8(const uint8_t* in, float* out, int n, int m, int size, int ensemble, pssr_stream_t stream);
int pssr_dihedral_batch_f32(const float* in, float* out, int n, int m, int size, int ensemble, pssr_stream_t stream);
int pssr_ensemble_reduce_u8(const float* in, uint8_t* mean, uint8_t* spread, int n, int c, int size, int ensemble, pssr_stream_t stream);
int pssr_spread_stack_u8(const uint8_t* tiles, uint8_t* out, int n_slices, int c, int n_rows, int n_cols, int size, int overlap,
                         int margin, int out_h, int out_w, int ensemble, pssr_stream_t stream);


/* ---------------------------------------------------------------------------------------------
 * normalize_preds (pssr/util.py:139-191) for uint8 image pairs of equal size resident in HBM: percentile window
 * of the ground truth, mean removal, covariance amplitude of the prediction, rescaling to the ground truth's intensity, clip
 * and uint8 cast -- bit-exact with the reference's numpy float32 / float64 arithmetic (float32 percentile lerp and pairwise
 * summation reproduced; see csrc/metrics.hip).  Images are [n_images][pixels_per_image]; workspace of
 * n_images * pssr_normalize_preds_workspace_bytes(pixels_per_image) bytes. */
int64_t pssr_normalize_preds_workspace_bytes(int64_t pixels_per_image);
int pssr_normalize_preds_u8(const uint8_t* hr, const uint8_t* hr_hat, uint8_t* hr_norm, uint8_t* hr_hat_norm, int n_images,
                            int64_t pixels_per_image, float pmin, float pmax, void* workspace, pssr_stream_t stream);
/* The same for a prediction [n_images][h][w] whose size differs from the ground truth's [n_images][H][W] (pssr/util.py:176-179): the
 * covariance amplitude is taken between the ground truth and skimage.transform.resize(prediction, (H, W)) -- order-1 interpolation at
 * (i + 0.5) * in / out - 0.5, mirror boundary, Gaussian pre-filter sigma = (in / out - 1) / 2 along shrinking axes (scikit-image
 * >= 0.19, i.e. scipy.ndimage.zoom(grid_mode=True) + gaussian_filter; restated and checked against scipy in oracle/metrics_ref.py;
 * scikit-image itself is absent: parity unpinned).  Outputs keep their own sizes, as upstream.  Workspace of
 * pssr_normalize_preds_resized_workspace_bytes(...) bytes. */
int64_t pssr_normalize_preds_resized_workspace_bytes(int n_images, int H, int W, int h, int w);
int pssr_normalize_preds_resized_u8(const uint8_t* hr, int H, int W, const uint8_t* hr_hat, int h, int w, uint8_t* hr_norm,
                                    uint8_t* hr_hat_norm, int n_images, float pmin, float pmax, void* workspace,
                                    pssr_stream_t stream);

/* Per-image restoration metrics of uint8 image pairs [n_images][h][w] resident in HBM, as pssr/predict.py:193-203 computes them
 * through skimage.metrics (peak_signal_noise_ratio, structural_similarity with data_range 255: uniform 7x7 window, K1 .01,
 * K2 .03, sample covariance, mean over the interior).  out[i] = { sum of squared differences (exact integer in a double),
 * mean SSIM }: mse = out[0] / (h w 255^2), psnr = 10 log10(255^2 h w / out[0]).  h, w >= 7 (skimage raises below that too).
 * workspace: pssr_image_metrics_workspace_bytes(n_images, h, w) bytes.  Reproducible bit for bit (fixed summation order). */
int64_t pssr_image_metrics_workspace_bytes(int n_images, int h, int w);
int pssr_image_metrics_u8(const uint8_t* hr, const uint8_t* hr_hat, double* out, int n_images, int h, int w, void* workspace,
                          pssr_stream_t stream);

/* Consistency of a prediction with its own low-resolution input (pssr2_amd.util.consistency_map; csrc/consistency.hip): the
 * resolution-scaled error of the super-resolution microscopy literature, for which no ground truth is needed.  Per plane pair
 * Y [s*h][s*w] (the uint8 prediction) and L [h][w] (the uint8 LR input), s an integer in 1 .. 16, n = h w:
 *   1. D = PIL.Image.resize(Y, (w, h), BILINEAR) bit for bit: pssr_bilinear_down_u8's two-pass 22-bit fixed-point resampler with the
 *      uint8 rounding between the passes (one copy of the tap arithmetic: csrc/pil_taps.h).
 *   2. Sd = sum D, Sl = sum L, Sdd = sum D^2, Sdl = sum D L, Sll = sum L^2: exact unsigned 64-bit integers over the plane.
 *   3. (host, from the integers) num = n Sdl - Sd Sl, den = n Sdd - Sd^2, denl = n Sll - Sl^2; fit "affine": alpha = num / den,
 *      beta = (Sl - alpha Sd) / n (den == 0: alpha = 0, beta = Sl / n); fit "identity": alpha = 1, beta = 0;
 *      rsp = num / sqrt(den denl) if den > 0 and denl > 0 else 0, the Pearson correlation of D and L.
 *   4. (host) P[v] = min(max(round_half_even(256 (alpha v + beta)), -65536), 131071), v = 0 .. 255, int32: the fitted expected LR
 *      value in 1/256 grey levels.
 *   5. e = |256 L - P[D]|; map = min(255, (e + 128) >> 8) u8 [h][w]; sse = sum e^2, an exact unsigned 64-bit integer (e < 2^18, so
 *      up to 2^28 pixels per plane; larger planes are PSSR_ERR_ARG); rse = sqrt(sse / n) / 256 grey levels.
 * pssr_reduce_moments_u8: steps 1 and 2 in one fused pass.  y [planes][s*h][s*w], l and d [planes][h][w], sums [planes][5] in the order
 *   of step 2.  Every byte of y is read from HBM about once (plus a halo of s rows and columns per 32 x 32 outputs); the horizontally
 *   reduced intermediate stays in LDS.  d equals pssr_bilinear_down_u8(y), bit for bit.
 * pssr_consistency_map_u8: step 5.  d, l and map [planes][pixels], lut [planes][256] (step 4), sse [planes].
 * Both validate before anything is launched (null pointers, planes, sizes, s outside 1 .. 16, an axis of y of 2^30 or more, more than
 * 2^28 pixels per plane): PSSR_ERR_ARG.  Integer sums through per-workgroup 64-bit partials in the workspace and a second small launch:
 * no atomics, no fence, no floating-point accumulation, the same bits on every run.  Workspaces of
 * pssr_reduce_moments_workspace_bytes / pssr_consistency_map_workspace_bytes bytes (0 for arguments the entry point rejects). */
int64_t pssr_reduce_moments_workspace_bytes(int planes, int h, int w, int s);
int pssr_reduce_moments_u8(const uint8_t* y, const uint8_t* l, uint8_t* d, uint64_t* sums, int planes, int h, int w, int s,
                           void* workspace, pssr_stream_t stream);
int64_t pssr_consistency_map_workspace_bytes(int planes, int64_t pixels);
int pssr_consistency_map_u8(const uint8_t* d, const uint8_t* l, const int32_t* lut, uint8_t* map, uint64_t* sse, int planes,
                            int64_t pixels, void* workspace, pssr_stream_t stream);

/* Registration of real (HR, LR) pairs: an exhaustive search over integer shifts (pssr2_amd.util.register_pairs; csrc/register.hip).
 * Real pairs are two acquisitions, and stage drift puts a few HR pixels between them; everything downstream (the noise-profile
 * objective, test_metrics, train_crappifier) assumes the same field of view pixel for pixel.  After the definitions everything is
 * integer arithmetic.
 * Inputs, per plane pair: H uint8 [s*h][s*w] (the HR side), L uint8 [h][w] (the LR side), s an integer in 1 .. 16, a search radius R in
 * HR pixels, 0 .. 32, giving T = (2R+1)^2 shifts t = (ty, tx), ty, tx in [-R, R]; the row index of t is (ty + R) (2R + 1) + (tx + R).
 *   1. Interior taps.  For an integer s, Pillow's BILINEAR reduction by s uses the same 2 s fixed-point coefficients k[0 .. 2s) (22-bit,
 *      csrc/pil_taps.h, evaluated for an interior index; not restated) for every interior output x, starting at input index
 *      s x - floor(s / 2).  For s = 1 they are the identity.
 *   2. Margin.  m = 1 + ceil(R / s) LR pixels; h' = h - 2m and w' = w - 2m must both be >= 1, otherwise PSSR_ERR_ARG.  With this m no
 *      candidate ever touches a border tap or leaves H.
 *   3. Reduced window per shift.  D_t[y][x], 0 <= y < h', 0 <= x < w', is the two-pass reduction of H sampled at HR origin
 *      (s (y + m) + ty, s (x + m) + tx): horizontal pass first, then vertical, clip8 (the rounding to uint8) after each pass, as in
 *      pssr_bilinear_down_u8.  Equivalently: filter H densely at every HR position and sample that map at stride s with offset t.
 *      Consequence: D_(0,0) == pssr_bilinear_down_u8(H)[m : h - m, m : w - m], bit for bit.
 *   4. Sums.  Lc = L[m : h - m, m : w - m].  Per plane and shift: Sd = sum D_t, Sdd = sum D_t^2, Sdl = sum D_t Lc; per plane:
 *      Sl = sum Lc, Sll = sum Lc^2.  All exact unsigned 64-bit integers.  Limits: s h, s w < 2^30 and h w <= 2^28.
 *   5. Choice (host, Python ints).  An item's planes pool: their sums add, and n = C h' w'.  num_t = n Sdl - Sd Sl,
 *      den_t = n Sdd - Sd^2, denl = n Sll - Sl^2.  The score is the signed squared Pearson correlation num_t |num_t| / (den_t denl), taken
 *      as 0 when den_t = 0 or denl = 0; scores are compared by cross-multiplying integers, never in floating point.  The chosen shift
 *      maximises the score; ties go to the smaller ty^2 + tx^2, then the smaller ty, then the smaller tx (a constant pair therefore
 *      chooses (0, 0)).  The reported score is the float num / sqrt(den denl) of the chosen shift.
 *   6. Aligned pair.  lr_out = L[m : h - m, m : w - m], hr_out = H[s m + ty : s (h - m) + ty, s m + tx : s (w - m) + tx].
 * pssr_register_shifts_u8: steps 1 - 4 in one fused pass.  hr [planes][s*h][s*w], lr [planes][h][w], sums [planes][3T + 2]: T triples
 *   (Sd, Sdd, Sdl) in row-index order, then Sl, Sll.  Every byte of hr is read from HBM about once; the dense filtered map lives in LDS.
 * pssr_crop_shift_u8: step 6.  out[p] = in[p][y0 : y0 + ho, x0 : x0 + wo] for in [planes][H][W], out [planes][ho][wo] and a device table
 *   origins [planes][2] of (y0, x0), with 16-byte accesses where alignment allows.  The table's values are the caller's contract
 *   (0 <= y0 <= H - ho, 0 <= x0 <= W - wo), as lut is for pssr_consistency_map_u8; pssr2_amd.ops.crop_shift_u8 checks them.
 * Both validate on the host before anything is launched (null pointers, planes, sizes, s outside 1 .. 16, radius outside 0 .. 32,
 * h' or w' < 1, the limits of step 4, a window larger than its plane): PSSR_ERR_ARG with a message.  Integer sums through per-workgroup
 * 64-bit partials in the workspace and a second small launch: no atomics, no fence, no floating-point accumulation, the same bits on
 * every run.  Workspace of pssr_register_shifts_workspace_bytes bytes (0 for arguments the entry point rejects). */
int64_t pssr_register_shifts_workspace_bytes(int planes, int h, int w, int s, int radius);
int pssr_register_shifts_u8(const uint8_t* hr, const uint8_t* lr, uint64_t* sums, int planes, int h, int w, int s, int radius,
                            void* workspace, pssr_stream_t stream);
int pssr_crop_shift_u8(const uint8_t* in, uint8_t* out, const int32_t* origins, int planes, int H, int W, int ho, int wo,
                       pssr_stream_t stream);

/* Estimate of the resolution-scaling function (RSF): an exhaustive search over candidate blurs (pssr2_amd.util.estimate_rsf,
 * consistency_map(rsf=...); csrc/rsf.hip).  The resolution-scaled error of the literature is defined after a Gaussian has been fitted
 * between the sharp image and the measured one; the consistency block above stops at Pillow's bilinear reduction.  For every candidate
 * sigma the best intensity fit L ~ alpha D_sigma + beta has the residual denl (1 - rho^2) / n, so the best sigma has the largest signed
 * squared Pearson correlation: the score of the registration block, over blurs instead of shifts.  After the tap table everything is
 * integer arithmetic.
 * Inputs, per plane pair: Y uint8 [s*h][s*w] (the sharp side), L uint8 [h][w] (the measured side), s an integer in 1 .. 16, a radius R in
 * HR pixels, 0 .. 32, K candidates, 1 .. 64.
 *   1. Tap table.  taps int32 [K][NT], NT = 2 s + 2 R, made on the host; it is the caller's contract, as the FRC tables and lut are
 *      (pssr2_amd.ops.rsf_taps makes it, ops.rsf_moments_u8 checks it).  Every row is non-negative; a row of sigma > 0 sums to exactly 2^22, the row of
 *      sigma = 0 to whatever Pillow's interior taps sum to (2^22 + e, |e| <= 6: e = 1 at s = 3, 0 at s = 1, 2, 4, 8, 16; Pillow rounds
 *      each tap on its own, and this row must stay Pillow's bit for bit).  For the candidates sigma_k: rad_k = 0 for sigma_k = 0, else ceil(3 sigma_k); R = max rad_k unless a larger one is given.  The row of
 *      sigma_k = 0 is the 2 s interior taps of the registration block (step 1 there) at columns R .. R + 2 s, zeros elsewhere.  For
 *      sigma_k > 0: the float64 Gaussian g[i] = exp(-i^2 / (2 sigma^2)), |i| <= rad_k, normalised to sum 1; convolved with the interior
 *      taps divided by 2^22 (2 s + 2 rad_k values c[n] = sum_i g[i] t[n - i]); rounded as floor(c 2^22 + 1/2); the difference of their
 *      sum to 2^22 added to the first largest tap; placed at columns R - rad_k .. R + rad_k + 2 s, zeros elsewhere.  The Gaussian's
 *      sum and every c[n] are correctly rounded sums of float64 terms (math.fsum), so the table does not depend on an order of addition.
 *   2. Margin.  m = 1 + ceil(R / s) LR pixels; h' = h - 2m and w' = w - 2m must both be >= 1, otherwise PSSR_ERR_ARG.  No candidate
 *      touches a border tap or leaves Y.
 *   3. Blurred reduction per candidate.  Horizontal pass first: T_k[r][x] = clip8(2^21 + sum_j taps[k][j] Y[r][s (x + m) - floor(s/2) - R + j]),
 *      0 <= x < w', j < NT; then the vertical pass, the same on the columns of T_k: D_k[y][x] = clip8(2^21 + sum_j taps[k][j]
 *      T_k[s (y + m) - floor(s/2) - R + j][x]), 0 <= y < h'.  clip8(v) = min(max(v >> 22, 0), 255), as in pssr_bilinear_down_u8.
 *      Consequence: with the row of sigma = 0, D == pssr_bilinear_down_u8(Y)[m : h - m, m : w - m] bit for bit, whatever R.
 *   4. Sums.  Lc = L[m : h - m, m : w - m].  Per plane and candidate: Sd = sum D_k, Sdd = sum D_k^2, Sdl = sum D_k Lc; per plane:
 *      Sl = sum Lc, Sll = sum Lc^2.  All exact unsigned 64-bit integers.  Limits: s h, s w < 2^30 and h w <= 2^28.
 *   5. Choice (host, Python ints).  The pooled planes add their sums, n = their pixels.  num_k = n Sdl - Sd Sl, den_k = n Sdd - Sd^2,
 *      denl = n Sll - Sl^2.  The score is num_k |num_k| / (den_k denl), taken as 0 when den_k = 0 or denl = 0; scores are compared by
 *      cross-multiplying integers.  The largest wins, ties go to the smaller k (a constant pair therefore chooses candidate 0).  The
 *      reported correlation is the float num / sqrt(den denl).
 * pssr_rsf_moments_u8: steps 2 - 4 in one fused pass.  y [planes][s*h][s*w], l [planes][h][w], taps [K][NT] (device), sums
 *   [planes][3K + 2]: K triples (Sd, Sdd, Sdl), then Sl, Sll -- the layout of pssr_register_shifts_u8 with T = K.  Every byte of y is read
 *   from HBM about once for all K candidates; T_k and D_k never leave LDS; a row of the table costs the taps between its first and last
 *   non-zero column only.
 * pssr_rsf_reduce_u8: d[p] = D_sel[p], uint8 [planes][h'][w'], for a device table sel [planes] of candidate indices.  Its values are the
 *   caller's contract (0 <= sel[p] < K; pssr2_amd.ops.rsf_reduce_u8 checks them); no row outside the table is read either way.
 * pssr_rsf_block: the side B of the square blocks of outputs a workgroup owns at (s, radius), 0 for an s or a radius out of range.
 * Both kernels' entry points validate on the host before anything is launched (null pointers, planes, sizes, s outside 1 .. 16, K outside
 * 1 .. 64, radius outside 0 .. 32, h' or w' < 1, the limits of step 4): PSSR_ERR_ARG with a message.  Integer sums through per-workgroup
 * 64-bit partials in the workspace and a second small launch: no atomics, no fence, no floating point, the same bits on every run.
 * Workspace of pssr_rsf_moments_workspace_bytes bytes (0 for arguments the entry point rejects). */
int pssr_rsf_block(int s, int radius);
int64_t pssr_rsf_moments_workspace_bytes(int planes, int h, int w, int s, int K, int radius);
int pssr_rsf_moments_u8(const uint8_t* y, const uint8_t* l, const int32_t* taps, uint64_t* sums, int planes, int h, int w, int s, int K,
                        int radius, void* workspace, pssr_stream_t stream);
int pssr_rsf_reduce_u8(const uint8_t* y, const int32_t* taps, const int32_t* sel, uint8_t* d, int planes, int h, int w, int s, int K,
                       int radius, pssr_stream_t stream);

/* Fourier ring correlation (FRC): down to which detail size two images of one field agree (pssr2_amd.util.frc; csrc/frc.hip) -- a
 * prediction against its ground truth, or two predictions of independent acquisitions.  The correlation of the two spectra, ring by ring
 * in spatial frequency, read off where it falls through a threshold (1/7 by convention).
 * Inputs: two uint8 plane stacks A, B [planes][H][W] and an even block side n, 16 <= n <= 1024, n <= min(H, W).  Each plane is tiled into
 * nby x nbx = (H / n) x (W / n) blocks at stride n (integer division); the grid of blocks is centred: its origin is
 * ((H - nby n) / 2, (W - nbx n) / 2), integer division again.  R = n / 2.
 *   1. Tables.  w[x] = sin^2(pi (x + 1/2) / n) (window "hann") or 1 (window "none").  Ct[x][k] = w[x] cos(2 pi ((x k) mod n) / n),
 *      St[x][k] = - w[x] sin(2 pi ((x k) mod n) / n), x, k = 0 .. n - 1, the product reduced mod n in integers before the angle is formed;
 *      evaluated in float64 on the host, rounded once to float32, row-major [n][n].  The tables are the caller's contract, as lut is for
 *      pssr_consistency_map_u8 (pssr2_amd.ops.frc_tables makes them); the kernels never evaluate a sine.
 *   2. Transform.  For a block a: Fa[ky][kx] = sum_y sum_x (Ct + i St)[y][ky] a[y][x] (Ct + i St)[x][kx], the DFT of the block times the
 *      separable window, in float32 (sum over x first, then over y, each an ascending chain of fused multiply-adds: the order is fixed).
 *      Fb likewise.
 *   3. Rings.  fy = ky if ky <= n / 2 else ky - n; q = fy^2 + kx^2; r = (isqrt(4 q) + 1) / 2 in integers, that is floor(sqrt(q) + 1/2).
 *      Rings 0 .. R are kept, r > R is dropped.
 *   4. Sums.  Per plane, block and ring three float64 sums over the full spectrum, kx in [0, n) with fx signed like fy:
 *      Sab = sum Re(Fa conj Fb), Saa = sum |Fa|^2, Sbb = sum |Fb|^2.  The kernel visits kx <= n / 2 and doubles the columns 0 < kx < n / 2,
 *      which is the same sum (the blocks are real).  The products are formed in float32, the sums across coefficients in float64.
 *   5. Curve and resolution (host, Python floats, from the sums).  An item's planes and blocks pool their sums ring by ring.  With
 *      smooth = k >= 0, ring r >= 1 takes the sums of rings max(1, r - k) .. min(R, r + k); ring 0 is never pooled into another ring.
 *      frc[r] = Sab / sqrt(Saa Sbb), or 0 where Saa Sbb <= 0.  The crossing is the first r >= 1 with frc[r] < threshold:
 *      r* = (r - 1) + (frc[r-1] - threshold) / (frc[r-1] - frc[r]) (r* = 1 where ring 0 itself lies below the threshold),
 *      resolution = pixel_size n / r* (infinite for r* = 0), crossed = true.  No ring below the threshold: resolution = 2 pixel_size,
 *      the sampling limit, crossed = false.
 * pssr_frc_rings_u8: steps 2 - 4.  a, b [planes][H][W], ct, st [n][n] (step 1), sums [planes][nby nbx][n / 2 + 1][3] in the order
 *   Sab, Saa, Sbb.  Any even n in range (500 as well as 512): the transform is two matrix products against the tables on the f32-input
 *   MFMA.  A row pass leaves T = a (Ct + i St)[:, 0 .. n/2] of both images in the workspace; a column pass forms 64 x 64 tiles of Fa and Fb
 *   in registers and reduces them to ring sums; F never leaves the compute unit.  A third small launch adds the tiles' partial sums in
 *   tile order.  No atomics, no fence: the same bits on every run.
 * Both validate on the host before anything is launched (null pointers, planes, sizes, n odd or outside 16 .. 1024 or larger than
 * the plane, more than 2^24 blocks): PSSR_ERR_ARG with a message.  Workspace of pssr_frc_workspace_bytes bytes (0 for arguments the entry
 * point rejects; at most about 256 MB: blocks are worked off in chunks). */
int64_t pssr_frc_workspace_bytes(int planes, int H, int W, int n);
int pssr_frc_rings_u8(const uint8_t* a, const uint8_t* b, const float* ct, const float* st, double* sums, int planes, int H, int W, int n,
                      void* workspace, pssr_stream_t stream);

/* Resolution of one image by decorrelation analysis (pssr2_amd.util.decorr; csrc/frc.hip): the figure FRC gives for a pair, from a single
 * image, with no threshold and no calibration (Descloux, Grussmayer, Radenovic, Nature Methods 16, 2019).  The spectrum F is correlated
 * with its own normalised self F / |F| inside a disc of radius r; that correlation, d(r), rises while the disc gathers signal and falls
 * once it gathers noise alone, and the position of its peak is the cut-off.  High-pass filtering the image first moves the peak outwards
 * as far as the signal reaches; the largest peak position over a family of filters is the resolution.  Because |F / |F|| = 1 and a radial
 * filter is one weight per ring, every curve of the family follows from two sums per ring, sum |F| and sum |F|^2, of one transform.
 * Inputs: a uint8 stack A [planes][H][W] and an even block side n, 16 <= n <= 1024, n <= min(H, W); blocks, the centred grid, the tables
 * Ct, St (step 1 of the FRC block above, the caller's contract) and the ring index r = (isqrt(4 q) + 1) / 2, rings 0 .. R = n / 2 kept,
 * are FRC's.  On the device:
 *   1. Mean.  S = sum of the block's n^2 bytes, an exact integer (at most 2^20 x 255).  m = float32(S / n^2), the quotient taken in double
 *      and rounded once to float32.  c[y][x] = float32(a[y][x]) - m, one float32 subtraction.  A constant block is exactly zero.  The mean
 *      is the block's own, not the plane's.  (Without it the window leaks the mean into rings 1 - 2 and every curve peaks there.)
 *   2. Spectrum and sums.  F = W^T c W, W = Ct + i St, in float32 exactly as step 2 of FRC (x first, then y, ascending chains of fused
 *      multiply-adds).  With fr = Re F and fi = Im F as they leave the accumulators: p = fmaf(fr, fr, fi * fi) (the product fi * fi rounded,
 *      then one fused multiply-add) is |F|^2 and sqrtf(p), correctly rounded, is |F|; both float32.  Per plane, block and ring r two
 *      float64 sums over the full spectrum: A[r] = sum |F| and P[r] = sum |F|^2.  The kernel visits kx <= n / 2 and doubles (exactly, in
 *      float32) the columns 0 < kx < n / 2.  Layout [planes][nby nbx][R + 1][2], A first.
 * On the host (pssr2_amd.util._decorr_resolve, Python floats, no device), with pop[r] the number of coefficients of the full spectrum in
 * ring r (counted from the ring index, kx signed like ky), A[r] and P[r] the pooled sums and B the number of block spectra pooled:
 *   3. Pooling.  An item's planes and blocks add their sums ring by ring (pool "item"), or every block stands alone (pool "block": the
 *      planes of an item still pool per block position).  M(r) = B sum_{rho = 1 .. r} pop[rho].  Ring 0 never enters.
 *   4. Curve.  For ring weights g[rho]: d_g(r) = sum_{rho = 1 .. r} g[rho] A[rho] / sqrt(sum_{rho = 1 .. R} g[rho]^2 P[rho] . M(r)),
 *      r = 1 .. R; 0 where the denominator is 0; d_g(0) = 0.  The unfiltered curve has g = 1.  (It is the Pearson-like correlation
 *      sum Re(G conj(N_r)) / sqrt(sum |G|^2 sum |N_r|^2) of the weighted spectrum G = g F over rings 1 .. R with N_r = F / |F| inside rings 1 .. r.)
 *   5. Peak rule.  For e = R down to 2: i = the first index of the maximum of d[1 .. e]; if i == e, go on; if d[i] - min(d[i .. e]) >= 5e-4
 *      the peak is ring i with amplitude d[i]; otherwise go on.  No e succeeds: no peak.  Refinement: p = i + (d[i-1] - d[i+1]) /
 *      (2 (d[i-1] - 2 d[i] + d[i+1])) where that second difference is negative, else p = i (d[0] = 0 serves for i = 1).
 *   6. Filter family.  Ng filters, 0 .. 64 (default 10).  s_0 = min(2 R / i0, R) with i0 the unfiltered peak's ring, s_0 = R without one;
 *      s_j = s_0 (0.15 / s_0)^(j / (Ng - 1)), j = 0 .. Ng - 1 (s_0 alone for Ng = 1).  g_j[rho] = 1 - exp(-2 s_j^2 (rho / R)^2): the
 *      Gaussian high-pass I - I * G evaluated at the ring's own radius.
 *   7. Result.  p* = the largest refined position among the peaks of the Ng + 1 curves (the first such curve on a tie);
 *      resolution = pixel_size n / p*, found = true.  No curve has a peak: found = false, resolution = 2 pixel_size, as FRC without a
 *      crossing.
 * pssr_decorr_rings_u8: steps 1 - 2.  a [planes][H][W], ct, st [n][n], sums [planes][nby nbx][n / 2 + 1][2].  The kernels are FRC's with one
 *   image per block: a small launch leaves the block means in the workspace, the row pass stages float(a) - m (zeros past the block) and
 *   leaves T = c (Ct + i St)[:, 0 .. n/2], [2][n][K] floats per block; the column pass forms 64 x 64 tiles of F in registers, p and sqrtf(p)
 *   per lane, and reduces them ring by ring in float64; the fold adds the tiles' rows in tile order.  F never goes to memory.  No atomics,
 *   no fence: the same bits on every run.
 * Both validate on the host before anything is launched (null pointers, planes, sizes, n odd or outside 16 .. 1024 or larger than the
 * plane, more than 2^24 blocks, workspace_bytes below pssr_decorr_workspace_bytes): PSSR_ERR_ARG with a message.
 * pssr_decorr_workspace_bytes is 0 for arguments the entry point rejects and at most about 256 MB: blocks are worked off in chunks. */
int64_t pssr_decorr_workspace_bytes(int planes, int H, int W, int n);
int pssr_decorr_rings_u8(const uint8_t* a, const float* ct, const float* st, double* sums, int planes, int H, int W, int n, void* workspace,
                         int64_t workspace_bytes, pssr_stream_t stream);

/* Directional resolution: sectorial FRC and decorrelation analysis (pssr2_amd.util.frc_sectors, decorr_sectors; csrc/frc.hip).  A ring
 * pools every direction, and a point-scanning microscope is not isotropic: its fast axis (along a line) and its slow axis (line to line)
 * differ in bandwidth.  Here every ring is cut into S sectors of the direction of the frequency vector, 1 <= S <= 16, and the sums of FRC
 * (three) and of decorrelation analysis (two) are kept per (ring, sector) cell.  Blocks, the centred grid, windows, tables, the transform,
 * the ring index, the doubling of the columns 0 < kx < n / 2 and the float32 / float64 split are exactly those of pssr_frc_rings_u8 and
 * pssr_decorr_rings_u8 above; only the cell that a coefficient's products are added to differs.
 *   S1. Boundary vectors (the caller's contract, made once on the host, int32 [S] each; pssr2_amd.ops.frc_sector_bounds makes them; the
 *       kernels evaluate no sine).  For j = 0 .. S - 1: beta_j = (j + 1/2) pi / S, bx[j] = rint(2^20 cos beta_j),
 *       by[j] = rint(2^20 sin beta_j).
 *   S2. Sector of a coefficient, exact in integers like the ring index.  A kept coefficient is (ky, kx) with kx <= n / 2 and
 *       fy = ky if ky <= n / 2 else ky - n.  Its upper-half-plane representative is (gx, gy) = (kx, fy) if fy >= 0, else (-kx, -fy).
 *       sector = #{ j : bx[j] gy - by[j] gx >= 0 } mod S; |g| <= 512, so a product stays below 2^30.  A coefficient with kx > n / 2 has the
 *       sector of its Hermitian mirror ((n - ky) mod n, n - kx), so doubling the columns 0 < kx < n / 2 stays valid sector by sector.
 *       Sector s is centred on the direction s pi / S of the frequency vector: sector 0 holds frequencies along x (detail along a scan
 *       line), and for even S sector S / 2 holds frequencies along y.  Ties: the origin falls into sector 0 (all S products are 0, and
 *       S mod S = 0); at S = 2 the diagonal gy = gx goes to sector 1 and gy = -gx to sector 0.  At S = 1 every coefficient is in sector 0.
 *   S3. Sums.  The three sums of step 4 of FRC, or the two of step 2 of decorrelation analysis, per plane, block, ring and sector, float64:
 *       [planes][nby nbx][R + 1][S][3] and [planes][nby nbx][R + 1][S][2].  Every cell is one float64 chain: the rows of a 64 x 64 tile of
 *       the spectrum in row order and kx order within a row, then the tiles in tile order -- so two calls give equal bits, and S = 1 gives
 *       exactly the bits of pssr_frc_rings_u8 and pssr_decorr_rings_u8.
 *   S4. Populations (host).  pop[r][s] = the number of coefficients of the full spectrum (kx in [0, n), the mirror rule of S2) in the cell;
 *       pssr2_amd.ops.frc_sector_pop.  Rings >= 1 have empty cells once S is large against the ring's few coefficients (6 cells at S = 8,
 *       32 - 33 at S = 16).
 *   S5. FRC per sector (host, pssr2_amd.util._frc_resolve_sector): step 5 of FRC on the sector's sums, with a rule for empty cells.  With
 *       smooth = k the cell (r, s), r >= 1, pools the sums and the populations of the cells (max(1, r - k) .. min(R, r + k), s).  A cell
 *       whose pooled population is 0 has the curve value NaN and is skipped: the crossing search walks the populated rings r >= 1 of the
 *       sector in ascending order, and at the first one below the threshold, with r_prev the populated ring before it (ring 0 counts) and
 *       c the curve, r* = r_prev + (c[r_prev] - t) / (c[r_prev] - c[r]) (r - r_prev); r* = 1 where ring 0 lies below the threshold too, or where
 *       no populated ring comes before (ring 0, the origin alone, is populated in sector 0 only).  No crossing: resolution = 2 pixel_size,
 *       crossed = false.
 *   S6. Decorrelation analysis per sector (host): steps 3 - 7 on the sector's two sums with M(r) = B sum_{rho = 1 .. r} pop[rho][s].
 *       Empty cells add nothing to either sum and need no rule.
 * pssr_frc_sectors_u8, pssr_decorr_sectors_u8: the row pass of the unsectored call, and a column pass whose reduction bins by (ring,
 *   sector): the thread that owns ring r walks the ring's run of each row of the tile as before and follows the sector with a pointer into
 *   the boundary vectors (the vectors with a non-negative product are a prefix of the list); the cell's chain continues in the thread's own
 *   slot of the tile's partial row, [R + 1][S][3 or 2] float64.  No atomics, no fence.  Partial rows are S times those of the unsectored
 *   call, and the chunk of blocks shrinks so that a chunk stays inside about 256 MB.
 * Both validate on the host before anything is launched (the checks of the unsectored calls; S outside 1 .. 16; null bx or by;
 * workspace_bytes below the _workspace_bytes figure): PSSR_ERR_ARG with a message.  The _workspace_bytes functions return 0 for arguments
 * that the entry point rejects. */
int64_t pssr_frc_sectors_workspace_bytes(int planes, int H, int W, int n, int S);
int pssr_frc_sectors_u8(const uint8_t* a, const uint8_t* b, const float* ct, const float* st, const int32_t* bx, const int32_t* by, double* sums,
                        int planes, int H, int W, int n, int S, void* workspace, int64_t workspace_bytes, pssr_stream_t stream);
int64_t pssr_decorr_sectors_workspace_bytes(int planes, int H, int W, int n, int S);
int pssr_decorr_sectors_u8(const uint8_t* a, const float* ct, const float* st, const int32_t* bx, const int32_t* by, double* sums, int planes,
                           int H, int W, int n, int S, void* workspace, int64_t workspace_bytes, pssr_stream_t stream);

/* The noise model of a pair, measured: level-conditional moments (pssr2_amd.util.estimate_noise; csrc/levels.hip).  Let D be the reduced
 * (and, if wanted, RSF-blurred) HR image and L = clip8(rint(D (1 - i) + i Poisson(D) + g + N(0, sigma_n))), the crappifier family of this
 * package.  On every grey level v far from the clipping ends E[L | D = v] = v + g and Var[L | D = v] = i^2 v + sigma_n^2: a
 * photon-transfer curve, binned by the signal the pair already contains.  The slope of the variance against the level is i^2, its
 * intercept sigma_n^2 (plus the 1/12 of the rounding, which is not taken off), the mean residual is g, and pixels at exactly 0 or 255 on
 * levels where noise cannot reach them are salt and pepper.
 * Inputs: two uint8 stacks D, L [planes][per_plane], per_plane 1 .. 2^28.
 *   1. Table (device).  Per plane and level v = 0 .. 255, over the pixels with D = v: n = their number, S1 = sum L, S2 = sum L^2,
 *      n0 = #{L = 0}, n255 = #{L = 255}.  Exact unsigned 64-bit integers, layout [planes][256][5] in that order.
 *   2. Pooling (device, int64 adds).  The planes of an item add their tables (pool "item"), or every plane of every item (pool "all").
 *   3. Fit (host, pssr2_amd.util._noise_fit, Python ints and floats, from one [256][5] table, with min_count >= 2 and guard > 0).
 *      Saturated pixels are taken off: n' = n - n0 - n255, S1' = S1 - 255 n255, S2' = S2 - 255^2 n255.
 *      pepper = sum_{v >= 128} n0[v] / sum_{v >= 128} n[v], salt = sum_{v < 128} n255[v] / sum_{v < 128} n[v], each 0 for an empty
 *      denominator; amount = pepper + salt, or twice the one side when the other has no pixels.
 *      Level v is used when n' >= min_count (and n' >= 2) and, with mean_v = S1' / n', var_v = (S2' - S1'^2 / n') / (n' - 1) and
 *      sd = sqrt(var_v): mean_v - guard sd > 0 and mean_v + guard sd < 255.
 *      Two weighted least-squares lines over the used levels, weights n', in the centred form sum w (v - vbar)(y - ybar) / sum w (v - vbar)^2:
 *      var_v ~ slope v + intercept and mean_v ~ alpha v + beta.  With fewer than two distinct used levels slope = 0, intercept = the
 *      weighted mean variance, alpha = 1, beta = the weighted mean of mean_v - v.  With none everything is 0 and found = false.
 *      gain = sum n' (mean_v - v) / sum n', poisson = sqrt(max(slope, 0)), gaussian = sqrt(max(intercept, 0)), saltpepper = 100 amount.
 * pssr_level_moments_u8: step 1.  Per-wave private LDS tables, integer LDS adds, a flush into 64-bit registers every 2^14 pixels, one
 *   row of 1280 64-bit partial sums per workgroup and plane in the workspace, and a second small launch that adds the rows: no global
 *   atomics, no fence, no floating point, the same bits on every run.  Planes may start at any address.
 * It validates on the host before anything is launched (null pointers, planes < 1, per_plane outside 1 .. 2^28, workspace_bytes below
 * pssr_level_moments_workspace_bytes): PSSR_ERR_ARG with a message.  pssr_level_moments_workspace_bytes is 0 for arguments the entry
 * point rejects. */
int64_t pssr_level_moments_workspace_bytes(int planes, int64_t per_plane);
int pssr_level_moments_u8(const uint8_t* d, const uint8_t* l, uint64_t* table, int planes, int64_t per_plane, void* workspace,
                          int64_t workspace_bytes, pssr_stream_t stream);

/* Several small f32 device-to-device copies in one launch (host struct passed by value to the kernel): the hand-written
 * backward pass moves side results (dbeta doubling as a bias gradient, centre taps, ...) into the flat gradient buffer the
 * all-reduce and AdamW read (the reference leaves this to autograd's .grad accumulation). */
#define PSSR_COPY_BATCH_MAX 16
typedef struct pssr_copy_batch {
    float* dst[PSSR_COPY_BATCH_MAX];
    const float* src[PSSR_COPY_BATCH_MAX];
    int64_t n[PSSR_COPY_BATCH_MAX];
} pssr_copy_batch;
int pssr_copy_f32_batch(const pssr_copy_batch* items, int n_items, pssr_stream_t stream);
/* Several pssr_f64_to_f32 folds (striped f64 statistic rows [stripes][n] -> f32 [n], optionally accumulated) by one launch: the
 * bias / LayerNorm / layer-scale gradient sums of a backward pass (RDNet has ~115 per step) are parameter gradients nobody reads
 * before the pass ends, so the engine queues them and folds 16 at a time. */
typedef struct pssr_fold_batch {
    float* dst[PSSR_COPY_BATCH_MAX];
    const double* src[PSSR_COPY_BATCH_MAX];
    int32_t n[PSSR_COPY_BATCH_MAX];
    int32_t accumulate[PSSR_COPY_BATCH_MAX];
} pssr_fold_batch;
int pssr_f64_to_f32_batch(const pssr_fold_batch* items, int n_items, int stripes, pssr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * GradHist soft histogram (pssr/models/_blocks.py:94-112) and the crappifier loss around it (pssr/train.py:388-402), for
 * train_crappifier (pssr/train.py:168-322).  Per image over its n = C*H*W f32 values: bins centred at
 * c_k = lo + (hi - lo) / bins * (k + 1/2), s_k(x) = sigmoid(sigma (x - c_k)), s_{-1} = 1.  Reproducible bit for bit (no atomics);
 * the work skipped and what it can drop are bounded in csrc/hist.hip's header comment.  Non-finite values follow torch: a NaN x
 * makes its image's histogram row NaN and its dx NaN (0 where PSSR_HIST_CLAMP cut a NaN xa); x = -inf adds 1 to bin 0, x = +inf
 * adds nothing, both have dx = 0.
 */
#define PSSR_HIST_CLAMP 1          /* clamp the first operand to [0, 255] on load (and mask its gradient: torch.clamp, inclusive) */
#define PSSR_HIST_ACCUMULATE 2     /* pssr_gradhist_bwd adds into dx */
#define PSSR_HIST_MAX_BINS 8192    /* both kernels take 1 .. 8192 bins (the backward keeps its bins' gradients in LDS) */
int64_t pssr_gradhist_workspace_bytes(int batch, int64_t n, int bins);
/* h0[b, j] = sum_i (s_{j-1}(x_i) - s_j(x_i)), x = a0 - b0 (b0 may be NULL: x = a0; PSSR_HIST_CLAMP clamps a0); the optional second pair
 * (a1, b1) -> h1 in the same launch.  [batch, bins] outputs; workspace: pssr_gradhist_workspace_bytes bytes. */
int pssr_gradhist_fwd(const float* a0, const float* b0, const float* a1, const float* b1, float* h0, float* h1, float* workspace,
                      int64_t workspace_bytes, int batch, int64_t n, int bins, float lo, float hi, float sigma, int flags,
                      pssr_stream_t stream);
/* dx_i = sigma sum_k s_k (1 - s_k) (G[k+1] [k+1 < bins] - G[k]) with x = xa - xb as in the forward and
 * G = (g - g_ref) * g_scale * dev_scale[0] (g_ref, dev_scale optional): the fused crappifier loss forms
 * dL/dh = 2 (p - t) / (B bins W^2) * P * dL on the device. */
int pssr_gradhist_bwd(const float* xa, const float* xb, const float* g, const float* g_ref, const float* dev_scale, float g_scale,
                      float* dx, int batch, int64_t n, int bins, float lo, float hi, float sigma, int flags, pssr_stream_t stream);
/* pred = clamp?(lr_hat) - ds_hr, target = lr - ds_hr (pssr/train.py:390-391; flags: PSSR_HIST_CLAMP = pssr/train.py:238-239) */
int pssr_crappifier_profiles(const float* lr_hat, const float* lr, const float* ds_hr, float* pred, float* target, int64_t n, int flags,
                             pssr_stream_t stream);
/* dst = src[:, :, ::stride, ::stride] of [planes, h_in, w_in] into a dense [planes, ceil(h_in/stride), ceil(w_in/stride)] (pssr/train.py:233) */
int pssr_subsample_f32(const float* src, float* dst, int64_t planes, int h_in, int w_in, int stride, pssr_stream_t stream);
/* D = sum (pred_hist - target_hist)^2 * dist_scale over m values (F.mse_loss / W^2 with dist_scale = 1 / (m W^2)), P = ssim_loss[0]:
 * out = [D * P, D, P] (pssr/train.py:397-401) */
int pssr_crappifier_loss_combine(const float* pred_hist, const float* target_hist, int64_t m, const float* ssim_loss, float dist_scale,
                                 float* out, pssr_stream_t stream);
/* backward of D * P: out = [D * grad_out, P * grad_out] from parts = [L, D, P] */
int pssr_crappifier_loss_bwd_scalars(const float* parts, const float* grad_out, float* out, pssr_stream_t stream);
/* y = min(max(x, lo), hi), NaN kept (in place when y == x): nn.utils.clip_grad_value_ over a flat gradient buffer (pssr/train.py:244) */
int pssr_clamp_f32(const float* x, float* y, int64_t n, float lo, float hi, pssr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Noise-profile statistics of approximate_crappifier's objective (pssr/train.py:348-386), csrc/profile.hip.
 * Per image over its per_image = C*H*W values: v = a - b in f32 (pssr/train.py:372-373), b the reduced HR (uint8), a the crappified
 * image (f32, not rounded, not clipped) or the real LR (uint8);
 *   hist[image][k], k = 0 .. 510 = np.histogram(v, np.arange(-256, 256)) (pssr/train.py:375-377): -256 + k <= v < -255 + k, the last
 *     bin also v == 255; values below -256, above 255, NaN and +-inf are counted nowhere;
 *   sum[image] = sum of every v in f64 (pssr/train.py:382 takes the mean over the whole image).
 * Counts are exact; the sums are added in a fixed order: bit-identical from run to run.  workspace:
 * pssr_noise_profile_workspace_bytes(images, per_image) bytes (0 when every image is one workgroup's; NULL is accepted then).
 */
#define PSSR_PROFILE_BINS 511
int64_t pssr_noise_profile_workspace_bytes(int images, int64_t per_image);
int pssr_noise_profile_f32(const float* a, const uint8_t* b, int32_t* hist, double* sum, int images, int64_t per_image, void* workspace,
                           int64_t workspace_bytes, pssr_stream_t stream);
int pssr_noise_profile_u8(const uint8_t* a, const uint8_t* b, int32_t* hist, double* sum, int images, int64_t per_image, void* workspace,
                          int64_t workspace_bytes, pssr_stream_t stream);
/* loss[i] = mean_k((t_k - p_k)^2) / width^2 + |target_sum[i] / per_image - pred_sum[i] / per_image| (pssr/train.py:381-384; the first
 * term from an exact integer sum and the reference's two f64 divisions: bit for bit), terms (or NULL) [images][2] = the two terms,
 * mean[0] = mean over images (pssr/train.py:386), all f64.  per_image <= 2^25. */
int pssr_noise_profile_loss(const int32_t* pred_hist, const double* pred_sum, const int32_t* target_hist, const double* target_sum,
                            int images, int64_t per_image, int width, double* loss, double* terms, double* mean, pssr_stream_t stream);

/* Scan phase of a bidirectional point scanner (pssr2_amd.crappifiers.ScanPhase, pssr2_amd.util.estimate_scan_phase /
 * correct_scan_phase; csrc/scanline.hip, csrc/crappify.hip, csrc/shift_rows.h).  Every second line of a resonant or bidirectional scan
 * is acquired on the way back, and a timing error moves all odd rows sideways against the even ones, usually by a fraction of a pixel
 * to 3 pixels.  One definition of "row y moved by d / 256 pixels" serves the crappifier, the estimate and the correction.
 *   D1. Row resampling.  X a plane [H][W], d[y] an int32 per row in 1/256 pixel, |d| <= 256 * 64 (an entry beyond it is clamped).  The
 *       content of row y moves right by d[y] / 256, edge replicated:
 *         p = 256 x - d[y],  i = p >> 8 (floor),  f = p & 255,  a = X[y][clamp(i, 0, W-1)],  b = X[y][clamp(i+1, 0, W-1)]
 *       uint8:    out = ((256 - f) a + f b + 128) >> 8.
 *       float32:  v = ((256 - f) a + f b) / 256 in float64 (both products and the division are exact and the sum rounds once, so a
 *                 contraction cannot move it), then + gain, then the finish(flags) of every crappifier stage (bit 1: rint, half to even;
 *                 bits 0 or 1: clip to [0, 255]), then float32.
 *       On integer-valued input with gain = 0 and flags 0 the two agree up to the + 128 >> 8 rounding.
 *   D2. The crappifier's row table, for tile t (the global index: tile_offset + the device tile_counter + the batch index, as in the
 *       other stages), frame c and row y, from the Philox stream of (seed, t):
 *         phi_t = intensity, or intensity + spread N(draw(seed, t, ~0, 7)) when spread > 0 -- NOT clamped at 0, the sign is the direction;
 *         j     = jitter N(draw(seed, t, c H + y, 11)) when jitter > 0, else 0;
 *         d     = rint(256 (phi_t (y & 1) + j)), clamped to +-256 * 64.
 *   D3. Row sums.  X uint8 [planes][H][W], a radius R of 0 .. 16, T = 2R + 1; H >= 3, W >= T, H W <= 2^28.  For every interior row
 *       y in 1 .. H-2, every column x in R .. W-R-1 and every k in -R .. R:  O_k = X[y][x + k],  E = X[y-1][x] + X[y+1][x].
 *       One output row holds 3T + 2 exact unsigned 64-bit integers: (sum O_k, sum O_k^2, sum O_k E) for k = -R .. R, then sum E, sum E^2:
 *       the layout of pssr_register_shifts_u8, per row.  The output is [planes][H-2][3T+2].
 *   D4. The estimate (host, Python ints).  The rows of a pool (a plane, the planes of an item, or everything) add: odd rows add at k, even
 *       interior rows at -k (an even row sits unmoved between two moved ones); n = the number of (row, column) pairs.  With D = O_k, L = E:
 *       num_k = n Sdl - Sd Sl, den_k = n Sdd - Sd^2, denl = n Sll - Sl^2.  The score of k is the signed squared Pearson correlation
 *       num_k |num_k| / (den_k denl), 0 where a variance is 0; candidates are compared by cross-multiplying integers; ties go to the
 *       smaller |k|, then to the smaller k.  Sub-pixel step with the float correlations r-, r0, r+ at k-1, k, k+1: if |k| < R and
 *       c = r- - 2 r0 + r+ < 0 then delta = 0.5 (r- - r+) / c clipped to +-0.5, else 0; phase = k + delta.
 *   D5. The correction: D1 (uint8) on the odd rows with d = -floor(256 phase + 0.5), d = 0 on the even rows.
 * pssr_line_moments_u8: D3 in one launch for all planes, integers only, every output slot written by one thread: no atomics, no fence, no
 *   floating point, no workspace, the same bits on every run.
 * pssr_shift_rows_u8 / pssr_shift_rows_f32: D1 for in, out [planes][H][W] (not in place) and a device table [planes][H], with 16-byte
 *   stores where the rows are whole aligned pieces.  Nothing outside a row is read whatever the table holds.
 * pssr_scan_rows_table: D2, table [tiles][frames][h]; tile_counter (or NULL) is a device uint64 added to tile_offset in the kernel.
 * All four validate on the host before anything is launched (null pointers, planes or sizes < 1, H < 3, W < 2R + 1, R outside 0 .. 16,
 * H W > 2^28, flags outside 0 .. 3, negative spread or jitter, in == out): PSSR_ERR_ARG with a message. */
int pssr_line_moments_u8(const uint8_t* x, uint64_t* sums, int planes, int H, int W, int radius, pssr_stream_t stream);
int pssr_shift_rows_u8(const uint8_t* in, uint8_t* out, const int32_t* table, int planes, int H, int W, pssr_stream_t stream);
int pssr_shift_rows_f32(const float* in, float* out, const int32_t* table, int planes, int H, int W, float gain, int flags,
                        pssr_stream_t stream);
int pssr_scan_rows_table(int32_t* table, int tiles, int frames, int h, float intensity, float spread, float jitter, uint64_t seed,
                         uint64_t tile_offset, const uint64_t* tile_counter, pssr_stream_t stream);

/* Classical baselines: the model-free rows of a super-resolution table, the LR image enlarged and the LR image denoised and then
 * enlarged (pssr2_amd.util.upsample / nlm_denoise, pssr2_amd.baselines.Baseline; csrc/baseline.hip, csrc/pil_taps.h).  Both are defined
 * in integers, so that a device result is compared with ==.
 *   B1. Enlargement: Pillow's 8-bit Image.resize with BILINEAR or BICUBIC, bit for bit.  X a uint8 plane [h][w], r an integer 1 .. 8,
 *       the output is [h r][w r].  filter 0 = bilinear (triangle, support S = 1), 1 = bicubic (Keys, A = -0.5, S = 2):
 *         f(a) = ((A + 2) a - (A + 3)) a^2 + 1 for |a| < 1,  (((a - 5) a + 8) a - 4) A for |a| < 2,  else 0.
 *       The taps of output index xx of an axis in -> out are Pillow's precompute_coeffs + normalize_coeffs_8bpc, in double, in Pillow's
 *       operation order and without fused multiply-adds:
 *         scale = in / out,  filterscale = max(scale, 1),  support = S filterscale,  center = (xx + 0.5) scale,
 *         xmin = max((int)(center - support + 0.5), 0),  xmax = min((int)(center + support + 0.5), in),  n = xmax - xmin,
 *         w[x] = f((x + xmin - center + 0.5) / filterscale),  x < n;  w[x] /= sum w (added in the order of x);
 *         k[x] = (int)(0.5 + w[x] 2^22) for w[x] >= 0, (int)(-0.5 + w[x] 2^22) below 0   (PRECISION_BITS = 22).
 *       Two passes, as Pillow runs them: along x into a uint8 intermediate [h][w r],  mid = clip8((sum_x k[x] X[xmin + x] + 2^21) >> 22)
 *       (arithmetic shift, then clipped to 0 .. 255); then along y from that intermediate by the same rule.  The rounding and clipping
 *       between the passes is part of the definition: bicubic overshoot clips in both.
 *   B2. Non-local means (Buades et al.) in integers.  X a uint8 plane [H][W]; patch radius p in 1 .. 3, P = 2p + 1; search radius s in
 *       1 .. 10; strength h in grey levels, 0.5 <= h <= 255; noise level sigma >= 0.  The host turns the last two into three integers:
 *         bias = rint(2 P^2 sigma^2);  qshift = the largest of 0 .. 31 with rint(32 2^qshift / (P^2 h^2)) <= 1023;  qmul = that value
 *         (qmul < 1: no such h is representable, an error).
 *       For the output pixel (y, x) and every offset (dy, dx) in [-s, s]^2 whose centre (y + dy, x + dx) lies inside the plane (the others
 *       are skipped, not clamped), with cy / cx clamping a coordinate into the plane on its own:
 *         ssd  = sum over (py, px) in [-p, p]^2 of (X[cy(y + py)][cx(x + px)] - X[cy(y + dy + py)][cx(x + dx + px)])^2
 *         q    = min((max(ssd - bias, 0) qmul) >> qshift, 255),   wgt = LUT[q],   v = X[y + dy][x + dx]
 *         LUT[q] = rint(16383 exp(-(q + 0.5) / 32)) for q < 255, LUT[255] = 0: a fixed table of the library (pssr_nlm_lut); h enters only
 *         through qmul and qshift.
 *       out = (sum wgt v + (sum wgt >> 1)) / sum wgt (integer division).  The centre candidate has ssd = 0, so sum wgt >= LUT[0] > 0.
 *       Everything fits uint32: ssd <= 49 255^2 < 2^22, ssd qmul < 2^32, 441 16383 255 + 441 16383 / 2 < 2^32 (static_asserts of
 *       csrc/baseline.hip).
 * pssr_nlm_u8: B2 for x, out [planes][H][W] in one launch; pssr_upsample_u8: B1 for x [planes][h][w] -> out [planes][h r][w r] in one
 *   launch, both passes fused, the intermediate in LDS.  No floating point beyond B1's taps, no atomics, no workspace: the same bits on
 *   every run.  16-byte stores where the output rows are whole aligned pieces.
 * pssr_nlm_lut: copies LUT to a host table of 256 int32.
 * All validate on the host before anything is launched (null pointers, planes or sizes < 1, p outside 1 .. 3, s outside 1 .. 10, r
 * outside 1 .. 8, an unknown filter, qmul outside 1 .. 1023, qshift outside 0 .. 31, bias < 0, more than 2^28 input or output pixels per
 * plane, x == out): PSSR_ERR_ARG with a message. */
int pssr_nlm_lut(int32_t* table);
int pssr_nlm_u8(const uint8_t* x, uint8_t* out, int planes, int H, int W, int p, int s, int qmul, int qshift, int bias,
                pssr_stream_t stream);
int pssr_upsample_u8(const uint8_t* x, uint8_t* out, int planes, int h, int w, int r, int filter, pssr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PSSR_MI355_H */
