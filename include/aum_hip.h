/*
 * aum_hip.h -- C ABI of libaum_hip.so: the MI355X (gfx950) implementation of the native boundary that
 * kaistmm/Audio-Mamba-AuM reaches through two un-vendored CUDA wheels.
 *
 * Reference interfaces replaced (paths relative to the reference repo):
 *   selective_scan_cuda.fwd / .bwd            call sites vim-mamba_ssm/mamba_ssm/ops/selective_scan_interface.py:37,
 *                                             62-65, 213-215, 247-251, 354-356, 389-393, 499-505, 541-552
 *   causal_conv1d_cuda.causal_conv1d_fwd/_bwd call sites selective_scan_interface.py:177, 239, 281-283, 318, 380,
 *                                             425-427, 463, 532, 594-596 (arithmetic: modules/mamba_simple.py:272)
 *   Triton _layer_norm_fwd_1pass_kernel / _layer_norm_bwd_kernel (fused residual-add + RMSNorm)
 *                                             vim-mamba_ssm/mamba_ssm/ops/triton/layernorm.py:123-177, 293-377
 *
 * Conventions (same as the reference's extension ABI, SURVEY.md 8b "Conventions"):
 *   - every pointer is a DEVICE pointer; nothing is allocated, freed or synchronised inside the library;
 *     every call only enqueues kernels on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *   - activation tensors (u, delta, z, B, C, x, dout, ...) share one element type `dtype`;
 *     A, D, delta_bias, conv weights/bias, norm weights and every parameter gradient are fp32;
 *   - the time axis is always unit-stride; batch / channel strides are explicit, in ELEMENTS;
 *   - return value 0 on success, a negative AUM_E_* code on invalid arguments (no exceptions cross the ABI).
 */
#ifndef AUM_HIP_H
#define AUM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AUM_ABI_VERSION 13  /* 2: x_ck (chunk-entry state checkpoint) appended to the two scan argument structs;
                               3: x_lane (lane-entry state checkpoint of the L = 513 row kernels) appended after it;
                               4: aug / noise (per-clip augmentation in the log-mel kernel's epilogue) appended to AumFbankArgs;
                               5: aum_frontend_tokens_fwd (waveform -> token sequence in one launch);
                               6: aum_sum_rows (fixed-order sum of partial results);
                               7: aum_scan_tm_fwd / _bwd (time-serial selective scan on token-major activations);
                               8: aum_conv1d_tm_fwd / _bwd (the causal conv on token-major activations);
                               9: aum_gemm_tn (the dense in_proj / out_proj GEMMs on token-major activations); aum_dtproj_tm_fwd, aum_xdt_tm_fwd; aum_scan_tm_ckpt_rows
                                  (packed 16-bit state checkpoints of the token-major scan for 16-bit activations);
                               10: aum_gemm_wgrad (weight gradients of the projections), aum_scan_tm_seg_fwd / _bwd (time segments: long rows at a small
                                  batch), aum_causal_conv1d_update / aum_selective_state_update (streaming inference);
                               11: aum_sum_rows_multi (several partial sets summed in one launch);
                               12: experiment switches and entry points removed from the boundary (AUM_GEMM_STAGGERED / _PERSISTENT / _NO_COUNTED_WAIT /
                                   _NO_PREFETCH / _W4 / _RING, aum_gemm_tn_sk, aum_gemm_tn_sk_workspace_bytes, aum_scan_tm_bwd_matrix_sums); AUM_GEMM_PACED;
                                   aum_sum_rows / aum_sum_rows_multi take any float address as destination;
                               13: aum_cast_bank (the 16-bit copies -- and transposes -- of a group of fp32 master weights in one launch);
                                   aum_rmsnorm_bwd_partial_rows (the vectorised norm backward leaves an eighth of the partial rows);
                                   additions without a version step (no existing struct or entry point changes): aum_stft_logmel_fwd, aum_spec_time_warp
                                   (the EPIC-Sounds frontend); AUM_SCAN_DELTA_ACTIVATED (token-major scans) and, appended to AumXdtArgs, delta_bias /
                                   flags (AUM_XDT_DELTA_SOFTPLUS) -- zero / NULL keeps the previous behaviour; aum_xdt_tm_bwd also takes
                                   (ncols, rank) = (56, 24) and aum_gemm_wgrad k in {24, 56} (AuM-Small: shapes that were AUM_E_UNSUPPORTED);
                                   aum_stream_park / AumParkArgs (streaming sessions to a blob and back in one launch);
                                   aum_rmsnorm_drop_fwd / _bwd / AumNormDropArgs (stochastic depth inside the add + RMSNorm);
                                   aum_rmsnorm_pool_fwd / _bwd / AumNormPoolArgs, aum_rmsnorm_pool_partial_rows (add + RMSNorm + mean over a
                                   sample's tokens: the head of a cls-free model) */

enum { AUM_F32 = 0, AUM_BF16 = 1, AUM_F16 = 2 };

enum {
    AUM_OK = 0,
    AUM_E_NULL = -1,        /* a required pointer is NULL */
    AUM_E_SHAPE = -2,       /* non-positive or unsupported size */
    AUM_E_DTYPE = -3,       /* unknown dtype enum */
    AUM_E_UNSUPPORTED = -4, /* combination not implemented (e.g. dstate > 256) */
    AUM_E_WORKSPACE = -5,   /* workspace missing or too small */
    AUM_E_LAUNCH = -6       /* hipLaunchKernel reported an error */
};

/* flags */
#define AUM_SCAN_SOFTPLUS 1u /* delta = softplus(delta + delta_bias)  (delta_softplus=True)                     */
#define AUM_SCAN_REVERSE 2u  /* run the recurrence from t=len-1 down to 0 (replaces the .flip([-1]) copies of   */
                             /* selective_scan_interface.py:503-507,547-561 and mamba_simple.py:229-246)        */
#define AUM_SCAN_GENERIC 4u  /* force the generic single-wave kernels (any dstate <= 256); default: 8-wave workgroup */
#define AUM_SCAN_ROWPAIR 8u  /* debug / A-B: keep the general row-pair kernels where a specialised one would run (one-row backward for
                                 512 + tail rows, chunked kernels for rows of 512*m + 1 steps, forward and backward) */
                             /* kernels when dstate <= 16                                                        */
#define AUM_SCAN_ACCUMULATE 16u /* long rows (the chunked kernels; anything else: AUM_E_UNSUPPORTED): add to out (forward) / du, ddelta, dz
                                  (backward) instead of overwriting them -- the second direction of a bidirectional layer lands on
                                  the first one's tensors, replacing the element-wise sums of selective_scan_interface.py:507,554-559 */
#define AUM_SCAN_DELTA_ACTIVATED 32u /* token-major scans (aum_scan_tm_* and their time-segment forms), 16-bit activations with z only (else
                                  AUM_E_UNSUPPORTED): delta already holds softplus(raw + delta_bias) (aum_xdt_tm_fwd with AUM_XDT_DELTA_SOFTPLUS).
                                  Replaces AUM_SCAN_SOFTPLUS (either may be set with it).  Forward: delta is used as it is; delta_bias is not read.
                                  Backward: delta_bias is not read; ddelta and ddelta_bias remain the gradients with respect to RAW and the bias
                                  (ddelta = d delta * sigmoid(raw + delta_bias), sigmoid formed as 1 - exp(-delta)), and ddelta_bias is written
                                  whenever the pointer is not NULL */
#define AUM_CONV_SILU 1u
#define AUM_CONV_REVERSE 2u  /* anti-causal: y[l] = act(b + sum_w W[w] x[l+(W-1)-w])                            */
#define AUM_CONV_GENERIC 4u  /* force the any-width kernel (default: the vectorised width-4 kernel when width == 4)  */
/* aum_gemm_tn picks its kernel by the length of the K loop (the paced-store kernel from k = 448 on, else one workgroup per tile); these name one: */
#define AUM_GEMM_LOCKSTEP 1u        /* one workgroup per 256 x 256 tile, one barrier per K-step */
#define AUM_GEMM_PIPELINED 32u      /* one workgroup per tile, fragment reads of the next half K-step under the current half's MFMAs */
#define AUM_GEMM_PACED 256u         /* one workgroup per CU walking a tile list as one stream of K-steps (hand-placed schedule, AGPR accumulators); a tile's
                                       stores leave under the next tile's first K-steps; k >= 448 (else AUM_E_UNSUPPORTED) */
#define AUM_NORM_PRENORM 1u  /* also return residual_out                                                        */
#define AUM_NORM_GENERIC 2u  /* force the any-cols kernel (default: register-cached vector kernel, cols <= 2048)  */

/*
 * Selective scan forward (selective_scan_cuda.fwd).
 *   u, delta, z, out, out_pre : (batch, dim, len)        B, C : (batch, dstate, len)   [the G=1 (B,1,N,L) case]
 *   A, A_b : (dim, dstate) fp32    D, delta_bias : (dim) fp32 or NULL     last_state : (batch, dim, dstate) fp32 or NULL
 * A_b != NULL selects the direction-fused bidirectional form of BiMambaInnerFn.forward
 * (selective_scan_interface.py:499-507): out = scan(A, forward) + scan(A_b, time-reversed), inputs read once, no flip
 * copies.  z == NULL: no gate.  out_pre (optional) receives the pre-gate value y + D*u summed over directions (what
 * the reference saves as `out` / `out_f`,`out_b` for the backward's dz).
 * workspace: unused by the forward (kept for ABI symmetry).
 * x_ck (optional, output): the `x` checkpoint tensor of selective_scan_cuda.fwd in this library's chunking -- the state
 * entering every 512-step chunk in scan order, (batch, dim, len/512, dstate) fp32.  Only rows the chunked kernels take
 * (aum_selective_scan_ckpt_bytes(...) > 0, one direction, neither AUM_SCAN_GENERIC nor AUM_SCAN_ROWPAIR) have one;
 * passing it for any other call is AUM_E_UNSUPPORTED.  Handed to the backward it replaces the backward's own pre-pass.
 */
typedef struct AumScanFwdArgs {
    const void *u, *delta, *z, *B, *C;
    const float *A, *A_b, *D, *delta_bias;
    void *out, *out_pre;
    float *last_state;
    void *workspace;
    int64_t workspace_bytes;
    int64_t u_bs, u_ds;         /* batch / channel strides of u (elements) */
    int64_t delta_bs, delta_ds; /* ... of delta */
    int64_t z_bs, z_ds;
    int64_t B_bs, B_ns;         /* batch / state strides of B */
    int64_t C_bs, C_ns;
    int64_t out_bs, out_ds;     /* strides of out and out_pre */
    int32_t batch, dim, len, dstate;
    int32_t dtype;
    uint32_t flags;
    float *x_ck;                /* ABI 2 */
    float *x_lane;              /* ABI 3 (optional, output): see aum_selective_scan_lane_ckpt_bytes */
} AumScanFwdArgs;

/*
 * Selective scan backward (selective_scan_cuda.bwd).  dout is the gradient of `out`.
 *   du, ddelta, dz : (batch, dim, len) in `dtype` (written; dz only when z != NULL)
 *   dA, dA_b : (dim, dstate); dD, ddelta_bias : (dim); dB, dC : (batch, dstate, len) -- all fp32, ACCUMULATED INTO
 *   (the caller zero-fills them; the fused bidirectional call adds both directions, selective_scan_interface.py:554-559).
 * out_pre is the tensor saved by the forward (required when z != NULL; it feeds dz).
 * workspace (required; size from aum_selective_scan_workspace_bytes(..., backward=1)): per-workgroup dB/dC partial
 * tiles and per-batch dA/dD/ddelta_bias partials that a second kernel of the same call reduces -- the backward issues
 * no global atomics.
 * The gradient is the mathematically complete one (autograd of bimamba_inner_ref), see DESIGN.md "dz".
 */
typedef struct AumScanBwdArgs {
    const void *u, *delta, *z, *B, *C, *dout, *out_pre;
    const float *A, *A_b, *D, *delta_bias;
    void *du, *ddelta, *dz;
    float *dA, *dA_b, *dB, *dC, *dD, *ddelta_bias;
    void *workspace;
    int64_t workspace_bytes;
    int64_t u_bs, u_ds, delta_bs, delta_ds, z_bs, z_ds, B_bs, B_ns, C_bs, C_ns;
    int64_t dout_bs, dout_ds, out_bs, out_ds; /* out_* = strides of out_pre */
    int64_t du_bs, du_ds, ddelta_bs, ddelta_ds, dz_bs, dz_ds;
    int64_t dB_bs, dB_ns, dC_bs, dC_ns;
    int32_t batch, dim, len, dstate;
    int32_t dtype;
    uint32_t flags;
    const float *x_ck;          /* ABI 2: the forward's checkpoint of the same call shape and direction, or NULL */
    const float *x_lane;        /* ABI 3: the forward's lane-entry checkpoint of the same call (shape, direction mode), or NULL */
} AumScanBwdArgs;

int aum_selective_scan_fwd(const AumScanFwdArgs* args, void* stream);
int aum_selective_scan_bwd(const AumScanBwdArgs* args, void* stream);
/* longest `len` handled in one pass per row (no workspace needed, direction fusion available) */
int aum_scan_max_single_pass_len(void);
int64_t aum_selective_scan_workspace_bytes(int32_t batch, int32_t dim, int32_t len, int32_t dstate, int32_t bidirectional,
                                           int32_t backward);
/* bytes of the x_ck checkpoint for this shape (one direction), 0 when the shape has none */
int64_t aum_selective_scan_ckpt_bytes(int32_t batch, int32_t dim, int32_t len, int32_t dstate);
/*
 * x_lane: the second form of the `x` tensor selective_scan_cuda.fwd returns for its backward (SSI:37-45), at the granularity
 * this library's L = 513 row kernels want it: the state entering every lane's 8-step block, per (row, direction, state) --
 * (batch, dim, directions, dstate, 64) fp32, directions = 2 for the fused bidirectional call.  Rows the row kernels take
 * (len == 513, dstate <= 16, neither AUM_SCAN_GENERIC nor AUM_SCAN_ROWPAIR) have one; bytes = 0 otherwise, and passing x_lane for
 * such a call is AUM_E_UNSUPPORTED.  Handed to the backward of the same call it replaces the recomputation of the forward scan
 * (the backward without it runs the previous-generation kernels).
 */
int64_t aum_selective_scan_lane_ckpt_bytes(int32_t batch, int32_t dim, int32_t len, int32_t dstate, int32_t bidirectional);

/*
 * Depthwise causal conv1d + bias + SiLU (causal_conv1d_cuda.causal_conv1d_fwd / _bwd).
 *   x, y, dy, dx : (batch, dim, len) in `dtype`;  weight : (dim, width) fp32;  bias : (dim) fp32 or NULL
 *   dweight (dim, width), dbias (dim): fp32, accumulated into (caller zero-fills).
 */
typedef struct AumConvArgs {
    const void *x, *dy;  /* dy: backward only */
    const float *weight, *bias;
    void *y;             /* forward: output.  backward: unused */
    void *dx;            /* backward */
    float *dweight, *dbias;
    int64_t x_bs, x_ds, y_bs, y_ds, dy_bs, dy_ds, dx_bs, dx_ds;
    int32_t batch, dim, len, width;
    int32_t dtype;
    uint32_t flags;
} AumConvArgs;

int aum_causal_conv1d_fwd(const AumConvArgs* args, void* stream);
int aum_causal_conv1d_bwd(const AumConvArgs* args, void* stream);

/*
 * Fused residual-add + RMSNorm (rms_norm_fn -> LayerNormFn, layernorm.py:380-478).
 *   x (rows, cols) in x_dtype; residual (rows, cols) in res_dtype or NULL; weight (cols) fp32;
 *   y (rows, cols) in y_dtype; residual_out (rows, cols) in res_dtype or NULL; rstd (rows) fp32.
 * backward: dy (rows, cols) in y_dtype; dresidual_out in res_dtype or NULL; x = the saved residual_out (or the input x
 * when no residual stream exists) in res_dtype; writes dx in x_dtype, dresidual_in (res_dtype, optional, receives the same
 * values as dx), and per-workgroup partial sums dweight_partial (n_partials, cols) fp32 that the caller reduces
 * (layernorm.py:333-372 does the same); n_partials = aum_rmsnorm_bwd_partial_rows(rows, cols, flags): the rows the caller allocates, and
 * every one of them holds a sum after the call.
 */
typedef struct AumNormArgs {
    const void *x, *residual, *dy, *dresidual_out;
    const float *weight, *rstd_in;
    void *y, *residual_out, *dx, *dresidual_in;
    float *rstd_out, *dweight_partial;
    int64_t row_stride_x, row_stride_res, row_stride_y, row_stride_res_out;
    int64_t row_stride_dy, row_stride_dres_out, row_stride_dx, row_stride_dres_in;
    float eps;
    int32_t rows, cols;
    int32_t x_dtype, res_dtype, y_dtype;
    uint32_t flags;
} AumNormArgs;

int aum_rmsnorm_fwd(const AumNormArgs* args, void* stream);
int aum_rmsnorm_bwd(const AumNormArgs* args, void* stream);
/* the grid-side bound: the waves the backward runs, min(rows, 4096), each with its own partial sum.  NOT the size of dweight_partial. */
int aum_rmsnorm_bwd_partials(int32_t rows);
/* ABI 13: THE number of dweight_partial rows the caller must allocate for aum_rmsnorm_bwd / aum_rmsnorm_drop_bwd with these rows, cols and
 * flags; the kernels write exactly these rows and nothing behind them.  Derived from the bound above: one row per wave for the any-cols
 * kernels (cols > 2048 or AUM_NORM_GENERIC), ceil(aum_rmsnorm_bwd_partials(rows) / 8) for the vectorised kernels, which add eight waves'
 * sums inside the workgroup, in wave order. */
int aum_rmsnorm_bwd_partial_rows(int32_t rows, int32_t cols, uint32_t flags);

/*
 * Stochastic depth in the fused add + RMSNorm (timm DropPath on the x operand, MM:90 / MM:650): row r of x is multiplied by
 * row_scale[r / rows_per_scale] -- 0 for a dropped sample, 1 / keep for a kept one -- on its way into the add.  The same kernels, limits
 * and dweight_partial rows as aum_rmsnorm_fwd / _bwd (aum_rmsnorm_bwd_partials / _partial_rows); an all-ones row_scale gives their bits.
 *   base                 the arguments of the unscaled pair, with these differences:
 *   row_scale            (rows / rows_per_scale) fp32, one factor per sample; rows % rows_per_scale == 0 (else AUM_E_SHAPE)
 *   forward              residual and residual_out are required.  residual_out = fma(s, x, residual) in fp32 (no 16-bit rounding of s or of
 *                        s * x), rounded once to res_dtype; rstd and y follow from it.  s == 0: residual_out = residual and the row of x
 *                        is NOT READ -- a NaN or inf in a dropped sample's x does not reach the residual stream
 *   backward             dresidual_in is required and is always a buffer of its own: dresidual_in = g, dx = s * g rounded once to x_dtype
 *                        (s == 0: +0), where g is what aum_rmsnorm_bwd writes as dx.  dweight_partial as in aum_rmsnorm_bwd
 * AUM_E_NULL: row_scale, residual / residual_out (forward) or dresidual_in (backward) is NULL -- nothing is written.  reserved: 0 (anything else: AUM_E_UNSUPPORTED).
 */
typedef struct AumNormDropArgs {
    AumNormArgs base;
    const float* row_scale;
    int32_t rows_per_scale;
    int32_t reserved;
} AumNormDropArgs;

int aum_rmsnorm_drop_fwd(const AumNormDropArgs* args, void* stream);
int aum_rmsnorm_drop_bwd(const AumNormDropArgs* args, void* stream);

/*
 * Fused add + RMSNorm + mean over a sample's tokens (the head of a cls-free model, final_pool_type 'mean': MM:649-669).  Row r belongs to
 * sample r / rows_per_sample.  The normalised rows are never stored: forward moves x and residual once, backward has no (rows, cols) dy.
 *   base      the arguments of aum_rmsnorm_fwd / _bwd with these differences: x_dtype is AUM_BF16 or AUM_F16, res_dtype AUM_F32, flags 0,
 *             cols % 8 == 0 and cols <= 2048 (anything else: AUM_E_UNSUPPORTED); y, dy and dresidual_out are not used and must be NULL
 *   forward   per row z = x + residual, rstd and y = z * rstd * weight rounded to x_dtype exactly as aum_rmsnorm_fwd computes them;
 *             pooled[s][c] = (sum over the sample's rows of the ROUNDED y) / rows_per_sample, added in fp32 in a fixed order (a wave's 4
 *             consecutive rows in row order, the 8 waves of a 32-row chunk in wave order, the chunks in chunk order) and rounded once to
 *             x_dtype: a sample's result depends on neither the batch size, its neighbours nor the run.  residual (required), weight;
 *             residual_out and rstd_out are optional, BOTH or NEITHER (aum_rmsnorm_fwd's bits; the backward needs them)
 *   pooled    (rows / rows_per_sample, cols) x_dtype, row stride row_stride_pooled elements
 *   pool_partial   fp32 workspace of rows / rows_per_sample * aum_rmsnorm_pool_partial_rows(rows_per_sample) contiguous rows of cols, every
 *             one written; needed only where that count is above 1 (a sample of more than 32 rows: a second launch adds its chunks)
 *   backward  dpooled (rows / rows_per_sample, cols) x_dtype; g[s] = dpooled[s] / rows_per_sample (fp32 division) rounded to x_dtype; every
 *             row of sample s gets the dx (x_dtype) and dresidual_in (fp32, required) that aum_rmsnorm_bwd writes for dy = g[s], bit for
 *             bit; x = the saved residual_out, rstd_in.  dweight_partial: aum_rmsnorm_bwd_partial_rows(rows, cols, 0) rows, as there
 * AUM_E_NULL: a required pointer is NULL;  AUM_E_SHAPE: rows_per_sample < 1 or rows % rows_per_sample != 0;  reserved: 0 (else
 * AUM_E_UNSUPPORTED).  A refused call writes nothing.
 */
typedef struct AumNormPoolArgs {
    AumNormArgs base;
    void* pooled;
    const void* dpooled;
    float* pool_partial;
    int64_t row_stride_pooled, row_stride_dpooled;
    int32_t rows_per_sample;
    int32_t reserved;
} AumNormPoolArgs;

int aum_rmsnorm_pool_fwd(const AumNormPoolArgs* args, void* stream);
int aum_rmsnorm_pool_bwd(const AumNormPoolArgs* args, void* stream);
/* the 32-row chunks of a sample: ceil(rows_per_sample / 32) (0 for rows_per_sample < 1); pool_partial holds that many rows per sample */
int aum_rmsnorm_pool_partial_rows(int32_t rows_per_sample);

/*
 * Log-mel filterbank frontend (replaces torchaudio.compliance.kaldi.fbank + pad + normalise on the CPU DataLoader
 * workers, src/dataloader.py:134-147, 220-221).
 *   wave : (batch, n_samples) fp32, already mean-removed (dataloader.py:101);  out : (batch, target_length, num_mel) fp32
 *   window (win), twiddle (padded/2 complex pairs exp(-2 pi i k / padded)), mel_start_f / mel_count_f (num_mel, small
 *   integers stored as fp32), mel_w (num_mel, mel_wstride): tables built by the host (aum/frontend.py).
 *   frames >= num_frames are written as the reference's zero padding after normalisation.
 */
typedef struct AumFbankArgs {
    const float *wave, *window, *twiddle, *mel_start_f, *mel_count_f, *mel_w;
    float *out;
    int64_t wave_bs, out_bs;
    int32_t batch, n_samples, win, shift, padded, num_frames, target_length, num_mel, mel_wstride;
    float preemph, norm_mean, norm_inv2std, log_floor;
    /* ABI 4, both optional.  aug: (batch, AUM_FBANK_AUG) fp32 per-clip table applied in the kernel's store (the training-time
     * chain of src/dataloader.py:139-145, 206-228 without extra passes over the spectrogram):
     *   [0] frames of this clip (ragged batches: frames >= it are the reference's zero padding; < 0: use num_frames)
     *   [1],[2] frequency band [lo, hi) and [3],[4] time band [lo, hi) set to 0 BEFORE normalisation (SpecAug; empty when lo >= hi)
     *   [5] roll along time (torch.roll shift, applied last)   [6] noise amplitude: out += noise[b][t][m] * amp, before the roll
     * noise: (batch, target_length, num_mel) fp32 uniform numbers from the caller's generator, or NULL (no noise). */
    const float *aug, *noise;
} AumFbankArgs;
#define AUM_FBANK_AUG 8
int aum_fbank_fwd(const AumFbankArgs* args, void* stream);

/*
 * Waveform -> token sequence in one launch (ABI 5): the log-mel frontend above, the 16 x 16 patch embedding, its bias, the
 * position rows and the cls row, i.e. src/dataloader.py:134-147, 206-228 -> src/models/mamba_models.py:509-541 with
 * src/utilities/tokenization.py:278-310 (FlexiPatchEmbed, kernel = stride = 16) -- without the spectrogram or an im2col copy
 * of it in HBM.
 *   fbank   : as for aum_fbank_fwd (aug / noise included); .out is ignored.  Needs padded == 512, num_mel == 128 and
 *             target_length % 64 == 0 (AUM_E_UNSUPPORTED otherwise: call aum_fbank_fwd and a GEMM instead).
 *   weight  : (dim, 256) in `dtype` (bf16 / f16) = the conv weight (dim, 1, 16, 16) flattened: k = 16 * mel_row + frame
 *   bias    : (dim) fp32      pos : (n_patches, dim) fp32, row f_block * n_t + t_block (pos_embed rows 1 ..)
 *   cls_row : (dim) fp32 = cls_token + pos_embed row 0, written as token `cls_pos` of every clip; NULL = no cls row
 *   tokens  : (batch, n_patches + (cls_row != NULL), dim) in `out_dtype`, batch stride tokens_bs elements:
 *             round16(patch . weight + bias) + pos   (the 16-bit conv output of the autocast reference, then the fp32 add)
 *   patches : optional (batch * n_patches, 256) in `dtype`, rows in f_block * n_t + t_block order: the GEMM's input, saved
 *             for the weight gradient.
 *   flags   : AUM_FRONTEND_TIME_MAJOR = patch tokens in time-major order (transpose_token_sequence, MM:545-566).
 */
typedef struct AumFrontendArgs {
    AumFbankArgs fbank;
    const void *weight;
    const float *bias, *pos, *cls_row;
    void *tokens, *patches;
    int64_t tokens_bs;
    int32_t dim, cls_pos, dtype, out_dtype;
    uint32_t flags;
} AumFrontendArgs;
#define AUM_FRONTEND_TIME_MAJOR 1u
int aum_frontend_tokens_fwd(const AumFrontendArgs* args, void* stream);

/*
 * Streaming log-mel (no version step: an addition): the NEW frames of several sessions whose PCM arrives in hops of any size.  A Kaldi
 * snip_edges frame t depends on samples [t * shift, t * shift + win) and nothing else, so every frame is computed by the arithmetic of
 * aum_fbank_fwd's wave-per-frame kernel on the session's virtual stream [its carried tail ; its hop] and is bit-identical to the same row
 * of aum_fbank_fwd on the whole clip, however the sample stream was cut.
 *   fbank       : the table, normalisation and pre-emphasis fields of AumFbankArgs (window .. mel_w, win, shift, padded, num_mel, mel_wstride,
 *                 preemph, norm_mean, norm_inv2std, log_floor).  aug and noise must be NULL and padded must be 512 (AUM_E_UNSUPPORTED).
 *                 .wave = (total_samples) fp32, the sessions' new samples behind one another (may be NULL when total_samples == 0);
 *                 .out = (total_frames, num_mel) fp32, the sessions' new frames behind one another (may be NULL when total_frames == 0);
 *                 batch, n_samples, num_frames, target_length, wave_bs, out_bs are not read.
 *   cu_samples  : (nseq + 1) int32, session i's hop is wave[cu_samples[i] .. cu_samples[i + 1])
 *   cu_frames   : (nseq + 1) int32, session i's frames are rows [cu_frames[i], cu_frames[i + 1]) of out; a session with no new frame is legal
 *   tail_len    : (nseq) int32, samples session i holds in its pool row, 0 <= tail_len < cap
 *   idx         : (nseq) int32 pool row of session i, distinct; NULL: session i owns row i
 *   first_frame : (nseq) int32 clip index of session i's first new frame; n_real : (nseq) int32, frames with clip index >= n_real[i] are
 *                 written as the normalised zero-padding row (the end of a clip); a negative entry means no limit
 *   tails       : (nrows, cap) fp32 pool of carried samples, cap == win + 15 * shift (what a session holds at most before a whole column of
 *                 16 frames is covered; 2800 at 16 kHz) and cap <= 2816
 * Frame j of session i reads the virtual stream at [j * shift, j * shift + win), every load masked and clamped to [0, tail_len + m_i).
 * Tail rule: behind the frames, row idx[i] holds the last tail_len + m_i - consumed_i samples of the virtual stream, where
 * consumed_i = min(shift * frames_i, tail_len + m_i) (0 when no frame was produced: the hop is appended).  The update is a SECOND launch
 * enqueued on the same stream behind the frame launch (one workgroup per session reads its whole new tail into registers, a workgroup
 * barrier, then writes it), so it cannot race with the frame waves that read the old tail, nor with itself.  Rows of sessions that are
 * not in the call are not touched.  A session whose operands are out of range (row outside the pool, lengths outside the buffers) is
 * skipped by both launches.  The caller keeps tail_len on the host (aum_hip.wave_map checks frames_i against the samples there are).
 */
typedef struct AumFbankStreamArgs {
    AumFbankArgs fbank;
    const int32_t *cu_samples, *cu_frames, *tail_len, *idx, *first_frame, *n_real;
    float *tails;
    int32_t total_samples, total_frames, nseq, nrows, cap, reserved;
} AumFbankStreamArgs;
int aum_fbank_stream_fwd(const AumFbankStreamArgs* args, void* stream);

/*
 * The skinny projections around the scan on CHANNEL-MAJOR activations (token t = b*len + l contiguous):
 *   conv_out / delta / ddelta / dconv : [dim][ntok]     x_dbl / dx_dbl : [dt_rank + 2*dstate][ntok], rows = dt | B | C
 * 16-bit activations only (AUM_BF16 / AUM_F16, fp32 accumulation on the MFMA units); weights in the same dtype.
 * Limits: dim % 64 == 0, dt_rank <= 64, dt_rank + 2*dstate <= 80, ntok * 80 < 2^31; otherwise AUM_E_UNSUPPORTED and the
 * caller uses its library GEMMs.
 *
 * aum_proj_fwd       replaces SSI:467-468 (F.linear x_proj, delta_proj matmul) and the B/C slicing + transposes of
 *                    SSI:471-493:   act = conv_out (in), w_x [dt_rank+2*dstate][dim], w_dt [dim][dt_rank],
 *                    x_dbl (out), out_act = delta (out, no bias / softplus: the scan applies them).
 * aum_proj_bwd_data  replaces SSI:570-574 (dB/dC scatter into dx_dbl), SSI:587 and SSI:590:
 *                    act = ddelta (in), w_dt = W_dt^T [dt_rank][dim], w_x = W_x^T [dim][dt_rank+2*dstate],
 *                    dB/dC fp32 (batch, dstate, len) with element strides, x_dbl = dx_dbl (out),
 *                    out_act = dconv, ACCUMULATED in place on top of the scan's du.
 */
typedef struct AumProjArgs {
    const void *act, *w_x, *w_dt;
    void *x_dbl, *out_act;
    const float *dB, *dC;
    int64_t dB_bs, dB_ns, dC_bs, dC_ns;
    int64_t ntok;
    int32_t dim, dt_rank, dstate, len, dtype;
    int32_t w_ld;   /* row pitch (elements, multiple of 8) of the matrix whose rows run along the SHORT k dimension:
                       forward: w_dt [dim][w_ld >= dt_rank]; backward: w_x = W_x^T [dim][w_ld >= dt_rank + 2*dstate].
                       Pad columns are never multiplied in (the other operand is zero there) but must be readable. */
} AumProjArgs;
int aum_proj_fwd(const AumProjArgs* args, void* stream);
int aum_proj_bwd_data(const AumProjArgs* args, void* stream);
/*
 * aum_proj_bwd_weight  replaces SSI:586 and SSI:589: partial[s][...] = sum over the s-th token range of
 *                    x[e][t] * y[r][t]  (x: [dim][ntok] 16-bit, y: [nrows][ntok] 16-bit, nrows <= 80), written as
 *                    [dim][nrows] (transpose_out = 0) or [nrows][dim] (transpose_out = 1) fp32 per split; the caller
 *                    sums the nsplit partials.  nsplit = aum_proj_bwd_weight_splits(dim, ntok).
 */
typedef struct AumProjWArgs {
    const void *x, *y;
    float* out;                 /* [nsplit][dim * nrows] */
    int64_t ntok;
    int32_t dim, nrows, nsplit, transpose_out, dtype;
} AumProjWArgs;
int aum_proj_bwd_weight(const AumProjWArgs* args, void* stream);
int aum_proj_bwd_weight_splits(int32_t dim, int64_t ntok);

/*
 * Selective scan on TOKEN-MAJOR activations, time-serial (ABI 7).  Same arithmetic as aum_selective_scan_fwd/_bwd
 * (selective_scan_cuda.fwd / .bwd, SSI:37, 62-65, 499-507, 541-561; oracle selective_scan_ref SSI:86-152), different division of the
 * work: a wavefront owns 64 CHANNELS of one batch entry and walks the sequence step by step with the 16 states of every channel in
 * registers; B_t / C_t are wave-uniform and come through the scalar cache.  No associative scan, no LDS tiles, any length.
 *   u, delta, z, out, out_pre, dout, du, ddelta, dz : element (b, t, e) at  b * X_bs + t * X_ts + e   (channels contiguous -- the
 *       natural output of F.linear; z / dz may be the second half of an xz row: pass the offset pointer and X_ts = 2 * dim)
 *   B, C : element (b, t, n) at  b * X_bs + t * X_ts + n, same dtype; rows 4-byte aligned (even strides / offsets for 16-bit dtypes)
 *   A, A_b : (dim, dstate) fp32;  D, delta_bias : (dim) fp32 or NULL
 * A_b != NULL: both directions in one launch (BiMambaInnerFn, SSI:499-507): out = gate * (y_fwd + y_rev + 2 D u); the two
 * direction waves of a channel group meet in the middle of the sequence and exchange their halves through `out`.
 * AUM_SCAN_REVERSE (A_b == NULL): the recurrence runs from t = len-1 down to 0.
 * ckpt (optional, forward output / backward input): the state entering every AUM_SCAN_TM_CK-step block in scan order,
 *   (directions, batch, nck, rows, dim) dwords with nck = aum_scan_tm_nck(len) and rows = aum_scan_tm_ckpt_rows(dtype) -- the `x` tensor
 *   of selective_scan_cuda.fwd at this kernel's granularity: the dstate states as fp32 for fp32 activations, dstate / 2 rows of PAIRS in the
 *   activations' own 16-bit type (states 2j, 2j+1 in one dword) for 16-bit activations (ABI 9; the entry state of an 8-step block rounded to the precision of the block's
 *   own inputs: half the checkpoint traffic of the training forward, which is HBM-bound on it).  A buffer sized for dstate rows is always
 *   large enough; forward and backward of one call must see the same dtype.  The backward requires it.
 * Limits: dstate == 16, dim % 64 == 0, len * X_ts * sizeof(element) < 2^31 for every tensor; otherwise AUM_E_UNSUPPORTED (callers
 * use aum_selective_scan_*).
 */
#define AUM_SCAN_TM_CK 8
typedef struct AumScanTmFwdArgs {
    const void *u, *delta, *z, *B, *C;
    const float *A, *A_b, *D, *delta_bias;
    void *out, *out_pre;
    float *ckpt;
    int64_t u_bs, u_ts, delta_bs, delta_ts, z_bs, z_ts, B_bs, B_ts, C_bs, C_ts, out_bs, out_ts, pre_bs, pre_ts;
    int32_t batch, dim, len, dstate;
    int32_t dtype;
    uint32_t flags;
} AumScanTmFwdArgs;
int aum_scan_tm_fwd(const AumScanTmFwdArgs* args, void* stream);
int32_t aum_scan_tm_nck(int32_t len);
int32_t aum_scan_tm_ckpt_rows(int32_t dtype);

/*
 * Backward of the above.  du, ddelta, dz in `dtype` (written).  dBC: (batch, len, 2 * dstate) fp32 = dB | dC per token, written
 * (the sum over the channel-group partials the kernel leaves in `workspace`).  dA, dA_b (dim, dstate), dD, ddelta_bias (dim): fp32,
 * written.  out_pre: the pre-gate sum saved by the forward (required with z).  workspace: aum_scan_tm_workspace_bytes(...) bytes.
 */
typedef struct AumScanTmBwdArgs {
    const void *u, *delta, *z, *B, *C, *dout, *out_pre;
    const float *A, *A_b, *D, *delta_bias;
    const float *ckpt;
    void *du, *ddelta, *dz;
    float *dA, *dA_b, *dBC, *dD, *ddelta_bias;
    void *workspace;
    int64_t workspace_bytes;
    int64_t u_bs, u_ts, delta_bs, delta_ts, z_bs, z_ts, B_bs, B_ts, C_bs, C_ts, dout_bs, dout_ts, pre_bs, pre_ts;
    int64_t du_bs, du_ts, ddelta_bs, ddelta_ts, dz_bs, dz_ts;
    int32_t batch, dim, len, dstate;
    int32_t dtype;
    uint32_t flags;
    /* ABI 10, optional (NULL: not written): dA .* A and dA_b .* A_b, (dim, dstate) fp32 -- the gradient with respect to A_log when
       A = -exp(A_log) (mamba_simple.py:190, 204), written by the same partial-sum launch that writes dA / dA_b */
    float *dA_xA, *dA_b_xA;
} AumScanTmBwdArgs;
int aum_scan_tm_bwd(const AumScanTmBwdArgs* args, void* stream);
int64_t aum_scan_tm_workspace_bytes(int32_t batch, int32_t dim, int32_t len, int32_t dstate, int32_t bidirectional);

/*
 * The same two operators on rows cut into TIME SEGMENTS (ABI 10): long rows at a small batch -- the reference's long-form setting
 * (B = 8, L = 4097: SURVEY section 8 config 5) is 384 (batch entry, channel group, direction) waves on 1024 SIMDs, each a 4097-step
 * serial chain.  The recurrence x_t = a_t x_{t-1} + b_t is affine in the state, so every direction is cut into `segments` ranges of
 * steps that run as waves of their own: a carry pass leaves each range's exit state from a zero entry and the product of its decays,
 * every range then starts from the composition of the carries before it (selective_scan_fn's results: SSI:86-152 restated on
 * ranges; nothing is approximated -- the sums are re-associated in fp32).  The backward cuts the adjoint recurrence the same way.
 *   segments: 2 .. AUM_SCAN_TM_MAX_SEGMENTS; ranges are ceil(len / segments) steps rounded up to a multiple of AUM_SCAN_TM_CK.
 *   carry: aum_scan_tm_seg_carry_bytes(...) bytes of scratch (forward); the backward keeps its carries in its workspace, which is
 *   aum_scan_tm_seg_workspace_bytes(...) bytes.  ckpt has the unsegmented layout: the two forms of the forward may be mixed with the
 *   two forms of the backward.  Everything else as aum_scan_tm_fwd / aum_scan_tm_bwd (base).
 */
#define AUM_SCAN_TM_MAX_SEGMENTS 32
typedef struct AumScanTmSegFwdArgs {
    AumScanTmFwdArgs base;
    float* carry;
    int64_t carry_bytes;
    int32_t segments;
    int32_t reserved;
} AumScanTmSegFwdArgs;
typedef struct AumScanTmSegBwdArgs {
    AumScanTmBwdArgs base;
    int32_t segments;
    int32_t reserved;
} AumScanTmSegBwdArgs;
int aum_scan_tm_seg_fwd(const AumScanTmSegFwdArgs* args, void* stream);
int aum_scan_tm_seg_bwd(const AumScanTmSegBwdArgs* args, void* stream);
int64_t aum_scan_tm_seg_carry_bytes(int32_t batch, int32_t dim, int32_t len, int32_t dstate, int32_t bidirectional, int32_t segments);
int64_t aum_scan_tm_seg_workspace_bytes(int32_t batch, int32_t dim, int32_t len, int32_t dstate, int32_t bidirectional, int32_t segments);

/*
 * aum_scan_tm_fwd with STATE IN and STATE OUT (additive; inference only): the one-direction, forward-time scan entered with a carried
 * state and leaving the state behind the row's last step -- the prefill of a streaming session (Mamba.forward with inference_params at
 * seqlen_offset == 0, MS:268-271, 300-302 restated on token-major rows), continued by aum_scan_tm_chunk / aum_stream_block_tm on the same
 * cache row.
 *   base:      as aum_scan_tm_fwd (both delta forms, with and without z, fp32 / bf16 / fp16).  A_b, ckpt, out_pre must be NULL and
 *              AUM_SCAN_REVERSE clear: AUM_E_UNSUPPORTED otherwise (no backward exists for this entry point).
 *   state_in:  (batch, dim, dstate) fp32 contiguous, 16-byte aligned, or NULL = a zero entry state: `out` is then bit for bit what
 *              aum_scan_tm_fwd (segments == 1) / aum_scan_tm_seg_fwd (the same segments) writes.
 *   state_out: the same shape, or NULL; the states behind step len - 1, exact fp32.  May be state_in (advance in place).
 *   segments:  1 = uncut; 2 .. AUM_SCAN_TM_MAX_SEGMENTS = time ranges as aum_scan_tm_seg_fwd, carry = aum_scan_tm_seg_carry_bytes(batch,
 *              dim, len, dstate, 0, segments) bytes of scratch.  Uncut, advancing by T1 + T2 steps in one call and by T1, then T2 gives
 *              bit-identical out and state_out; the segmented form re-associates the recurrence at the range boundaries.
 */
typedef struct AumScanTmFwdStateArgs {
    AumScanTmFwdArgs base;
    const float* state_in;
    float* state_out;
    float* carry;
    int64_t carry_bytes;
    int32_t segments;
    int32_t reserved;
} AumScanTmFwdStateArgs;
int aum_scan_tm_fwd_state(const AumScanTmFwdStateArgs* args, void* stream);

/*
 * Depthwise causal conv1d (+ SiLU) on TOKEN-MAJOR activations (ABI 8): the same operator as aum_causal_conv1d_fwd / _bwd
 * (MS:272 causal_conv1d_fn; SSI:463 forward and SSI:594-596 backward call sites) for tensors laid out (batch, len, dim) with the
 * channel contiguous -- the layout of the in_proj output rows [x | z] and of the time-serial scan's operands, so x / dx may be the
 * first half of a (batch, len, 2 dim) tensor (strides in ELEMENTS: *_bs batch, *_ts token; channel stride 1).
 *   x, y, dy, dx in `dtype`; weight (dim, width) fp32, width <= 4; bias (dim) fp32 or NULL; flags: AUM_CONV_SILU, AUM_CONV_REVERSE.
 *   backward: dx written; dw_part [nparts][dim][width] (the weight's layout) and db_part [nparts][dim] (NULL without bias) fp32 are per-wave partial sums
 *   (nparts = aum_conv1d_tm_nparts(batch, len)) that the caller adds up in a fixed order (aum_sum_rows): no atomics.
 * Limits: dim % (16 / sizeof(dtype)) == 0, 16-byte aligned pointers (weight and bias included) and row strides.
 */
typedef struct AumConvTmArgs {
    const void *x, *dy;      /* dy: backward only */
    const float *weight, *bias;
    void *y;                 /* forward */
    void *dx;                /* backward */
    float *dw_part, *db_part;
    int64_t x_bs, x_ts, y_bs, y_ts, dy_bs, dy_ts, dx_bs, dx_ts;
    int32_t batch, dim, len, width;
    int32_t dtype;
    uint32_t flags;
} AumConvTmArgs;
int aum_conv1d_tm_fwd(const AumConvTmArgs* args, void* stream);
int aum_conv1d_tm_bwd(const AumConvTmArgs* args, void* stream);
int32_t aum_conv1d_tm_nparts(int32_t batch, int32_t len);

/*
 * Dense projection GEMM on token-major activations (ABI 9): the in_proj / out_proj matrix products of the Mamba block and their
 * data gradients, which the reference leaves to cuBLAS through F.linear (vim-mamba_ssm/mamba_ssm/modules/mamba_simple.py:185-189;
 * selective_scan_interface.py:517 out_proj forward, :540 its data gradient; the in_proj data gradient is autograd's).
 *   c[m][n] = sum over k of a[m][k] * b[n][k]      ("TN": both operands K-contiguous; fp32 accumulation, one rounding at the store)
 *   a: (m, k) row pitch lda;  b: (n, k) row pitch ldb;  c: (m, n) row pitch ldc -- pitches in ELEMENTS, all three tensors `dtype`
 *   (AUM_BF16 or AUM_F16; AUM_F32: AUM_E_DTYPE).  m is arbitrary (the token count); n % 256 == 0 and k % 64 == 0 (the model widths
 *   768 / 1536 / 3072; else AUM_E_UNSUPPORTED); pointers 16-byte aligned, pitches % 8 == 0, every tensor below 2 GiB per 256-row block
 *   (32-bit buffer offsets).  forward: a = activations, b = the weight as nn.Linear stores it; data gradient: a = d out, b = the weight's transpose.
 */
typedef struct AumGemmArgs {
    const void *a, *b;
    void *c;
    int32_t m, n, k;
    int32_t lda, ldb, ldc;
    int32_t dtype;
    uint32_t flags;
} AumGemmArgs;
int aum_gemm_tn(const AumGemmArgs* args, void* stream);

/*
 * Weight-gradient GEMM of the in / out projections on token-major operands (ABI 10; autograd of mamba_simple.py:185-189 and
 * selective_scan_interface.py:563: d W = d out^T . input):
 *   part[s][n][k] = sum over the tokens t of split s of  y[t][n] * x[t][k]          s = 0 .. splits - 1
 *   y: (t, n) rows of pitch ldy (the output gradient);  x: (t, k) rows of pitch ldx (the layer's input) -- pitches in ELEMENTS, both `dtype`
 *   (AUM_BF16 / AUM_F16; else AUM_E_DTYPE);  part: (splits, n, k) fp32, contiguous: the caller sums the splits in a fixed order (aum_sum_rows).
 *   Split s takes tokens [s c, min(t, (s + 1) c)) with c = ceil(ceil(t / splits) / 64) * 64 (a split may be empty: its tile is zero).
 *   n % 256 == 0, k % 256 == 0 or k in {48, 80, 24, 56} (the skinny operands of the dt_proj / x_proj weight gradients, SSI:586, 589, of AuM-Base and AuM-Small), splits <= 64, pitches % 8 == 0, 16-byte aligned pointers, c * pitch * 2 < 2 GiB (else AUM_E_UNSUPPORTED: callers
 *   use a library GEMM).  fp32 accumulation; no atomics: the result is bitwise repeatable.
 */
typedef struct AumGemmWArgs {
    const void *y, *x;
    float* part;
    int64_t t;
    int64_t ldy, ldx;
    int32_t n, k, splits;
    int32_t dtype;
} AumGemmWArgs;
int aum_gemm_wgrad(const AumGemmWArgs* args, void* stream);

/*
 * dt projection of the token-major block (ABI 9): delta = x_dbl[:, :dt_rank] . dt_proj.weight^T (selective_scan_interface.py:468 without
 * its transposes; the bias and the softplus stay in the scan, as in the reference).
 *   x: (ntok, >= rank) rows of pitch ldx, the first `rank` columns are read (x_dbl: the dt block sits in front of B and C);
 *   w: (dim, rank) rows of pitch ldw (dt_proj.weight as nn.Linear stores it);  out: (ntok, dim) rows of pitch ldo.  Pitches in ELEMENTS, all
 *   three tensors `dtype` (AUM_BF16 / AUM_F16; else AUM_E_DTYPE); dim % 32 == 0, rank % 8 == 0, rank <= 64, pitches % 8 == 0, 16-byte
 *   aligned pointers (else AUM_E_UNSUPPORTED: callers use a library GEMM).  fp32 accumulation, one rounding at the store.
 */
typedef struct AumDtProjArgs {
    const void *x, *w;
    void *out;
    int64_t ntok;
    int32_t dim, rank;
    int32_t ldx, ldw, ldo;
    int32_t dtype;
} AumDtProjArgs;
int aum_dtproj_tm_fwd(const AumDtProjArgs* args, void* stream);

/*
 * x_proj and dt_proj of the token-major block in one pass over conv_out (ABI 9; selective_scan_interface.py:467-468 without their
 * transposes): x_dbl = u . x_proj.weight^T, delta = x_dbl[:, :rank] . dt_proj.weight^T.  flags = 0 (delta_bias NULL): delta is that
 * product and the scan adds the bias and applies the softplus, as in the reference.  flags = AUM_XDT_DELTA_SOFTPLUS: delta =
 * softplus(product + delta_bias) formed on the fp32 accumulators (the scans' softplus, SSI:106-107) and rounded once -- what a token-major
 * scan with AUM_SCAN_DELTA_ACTIVATED reads; delta_bias: (dim) fp32, 16-byte aligned, or NULL (no bias).
 *   u: (ntok, dim) rows of pitch ldu (conv_out);  wx: (ncols, dim) pitch ldwx;  wdt: (dim, rank) pitch ldwdt;
 *   x_dbl (out): (ntok, ncols) pitch ldx;  delta (out): (ntok, dim) pitch ldd.  Pitches in ELEMENTS, all tensors `dtype` (AUM_BF16 / AUM_F16).
 *   Built for ncols == 80, 56 (dt_rank + 2 d_state of AuM-Base / AuM-Small) or 48 (AuM-Tiny's 12 + 32 padded by the caller to [dt 12 | 4 zero | B | C], rank 16), dim % 128 == 0, dim <= 1536, rank % 8 == 0, rank <= 64, pitches % 8 == 0,
 *   16-byte aligned pointers; anything else AUM_E_UNSUPPORTED (callers use a GEMM for x_dbl and aum_dtproj_tm_fwd).  delta is computed from
 *   the ROUNDED x_dbl, as the two separate products do.
 */
typedef struct AumXdtArgs {
    const void *u, *wx, *wdt;
    void *x_dbl, *delta;
    int64_t ntok;
    int32_t dim, rank, ncols;
    int32_t ldu, ldwx, ldwdt, ldx, ldd;
    int32_t dtype;
    const float* delta_bias;    /* AUM_XDT_DELTA_SOFTPLUS only (else NULL) */
    uint32_t flags;
} AumXdtArgs;
#define AUM_XDT_DELTA_SOFTPLUS 1u
int aum_xdt_tm_fwd(const AumXdtArgs* args, void* stream);

/*
 * The token-parallel pieces of the x_proj / dt_proj gradients in one pass (ABI 10; selective_scan_interface.py:570-574, :587, :590):
 *   dx_dbl[:, :rank] = ddelta . dt_proj.weight  (rounded to `dtype`),  dx_dbl[:, rank:] = dB | dC (the scan backward's fp32 rows),
 *   du += dx_dbl . x_proj.weight  (in place).
 *   ddelta: (ntok, dim) pitch ldd;  dbc: (ntok, ncols - rank) fp32 pitch lddbc;  wdt_t: dt_proj.weight TRANSPOSED, (rank, dim) pitch ldwdt;
 *   wx_t: x_proj.weight TRANSPOSED, (dim, ncols) pitch ldwx;  du (in / out): (ntok, dim) pitch ldu;  dx_dbl (out): (ntok, ncols) pitch ldx.
 *   Built for (ncols, rank) == (80, 48) (AuM-Base) or (56, 24) (AuM-Small) -- no other pair, not (80, 24) or (56, 48) --, dim % 256 == 0, dim <= 1536, pitches % 8 == 0 (lddbc % 4 == 0), 16-byte aligned pointers;
 *   anything else AUM_E_UNSUPPORTED (callers use the three library calls).
 */
typedef struct AumXdtBwdArgs {
    const void *ddelta;
    const float *dbc;
    const void *wdt_t, *wx_t;
    void *du, *dx_dbl;
    int64_t ntok;
    int32_t dim, rank, ncols;
    int32_t ldd, lddbc, ldwdt, ldwx, ldu, ldx;
    int32_t dtype;
} AumXdtBwdArgs;
int aum_xdt_tm_bwd(const AumXdtBwdArgs* args, void* stream);

/*
 * Streaming inference, one token per call (ABI 10; mamba_simple.py:313-358 `Mamba.step`).  The caches are fp32, contiguous, updated in place.
 *
 * aum_causal_conv1d_update -- `causal_conv1d_update(x, conv_state, weight, bias, activation)` of the causal_conv1d wheel (call site
 *   mamba_simple.py:328-334; arithmetic = the fallback at :322-327): conv_state (batch, dim, width) <- (conv_state[..., 1:], x);
 *   out (batch, dim) = act(sum_k conv_state[..., k] * weight[dim][k] + bias).  x / out: `dtype`, contiguous; weight (dim, width), bias (dim) fp32;
 *   flags: AUM_CONV_SILU.  width <= 8.
 * aum_selective_state_update -- `selective_state_update(state, x, dt, A, B, C, D, z, dt_bias, dt_softplus)` (ops/triton/selective_state_update.py:
 *   157-192, call site mamba_simple.py:352-354): dt' = softplus?(dt + dt_bias); state (batch, dim, dstate) <- exp(dt' A) state + dt' x B;
 *   out (batch, dim) = (<state, C> + D x) * silu(z).  x, dt, z, out (batch, dim) and B, C (batch, dstate): `dtype`, contiguous; A (dim, dstate),
 *   D, dt_bias (dim) fp32 (D, dt_bias, z may be NULL);  flags: AUM_SCAN_SOFTPLUS.  dstate <= 256.
 */
typedef struct AumConvUpdateArgs {
    const void* x;
    float* conv_state;
    const float *weight, *bias;
    void* out;
    int32_t batch, dim, width;
    int32_t dtype;
    uint32_t flags;
} AumConvUpdateArgs;
int aum_causal_conv1d_update(const AumConvUpdateArgs* args, void* stream);
typedef struct AumStateUpdateArgs {
    float* state;
    const void *x, *dt, *z, *B, *C;
    const float *A, *D, *dt_bias;
    void* out;
    int32_t batch, dim, dstate;
    int32_t dtype;
    uint32_t flags;
} AumStateUpdateArgs;
int aum_selective_state_update(const AumStateUpdateArgs* args, void* stream);

/*
 * Streaming inference, T >= 1 tokens per call from carried caches (additive to ABI 13; `Mamba.step_chunk`).  Token-major activations:
 * element (b, t, e) at  b * X_bs + t * X_ts + e  (strides in ELEMENTS, channel stride 1 -- x / u and z may be the two halves of an in_proj
 * output row with X_ts = 2 * dim), `dtype` fp32 / bf16 / fp16.  The caches are fp32, contiguous, updated in place, in the layouts of
 * aum_causal_conv1d_update / aum_selective_state_update; the arithmetic is fp32.  Inference only (no backward).
 * Both results are independent of how a token stream is cut into calls: advancing by T1 + T2 tokens in one call or by T1, then T2 gives
 * bit-identical outputs and caches.
 *
 * aum_conv1d_tm_chunk -- `len` successive aum_causal_conv1d_update calls in one launch: y[t] = act(bias + sum_k weight[k] * win_t[k]) with the
 *   window sliding over (conv_state, x[0..t]); on exit conv_state (batch, dim, width) holds the last `width` inputs (for len < width old
 *   entries survive, shifted).  x, y (batch, len, dim), y != x; weight (dim, width) fp32, width <= 4; bias (dim) fp32 or NULL; flags:
 *   AUM_CONV_SILU.  Limits as aum_conv1d_tm_fwd: dim % (16 / sizeof(dtype)) == 0, 16-byte aligned x, y, weight, bias and row strides.
 * aum_scan_tm_chunk -- `len` successive aum_selective_state_update calls in one launch: d = softplus?(delta + delta_bias);
 *   state (batch, dim, dstate) <- exp(d A) state + d u B_t;  out_t = (<state, C_t> + D u) * silu(z).  u, delta, z, out (batch, len, dim);
 *   B, C (batch, len, dstate) in `dtype` (column blocks of the x_dbl rows, read in place); A (dim, dstate), D, delta_bias (dim) fp32
 *   (D, delta_bias, z may be NULL).  flags: AUM_SCAN_SOFTPLUS, or AUM_SCAN_DELTA_ACTIVATED when delta already holds
 *   softplus(raw + delta_bias) (what aum_xdt_tm_fwd writes with AUM_XDT_DELTA_SOFTPLUS; delta_bias is then ignored) -- either form for
 *   every dtype, with or without z.  Limits as aum_scan_tm_fwd: dstate == 16, dim % 64 == 0, 16-byte aligned state; otherwise
 *   AUM_E_UNSUPPORTED (callers use the per-token kernels).
 */
typedef struct AumConvTmChunkArgs {
    const void* x;
    float* conv_state;
    const float *weight, *bias;
    void* y;
    int64_t x_bs, x_ts, y_bs, y_ts;
    int32_t batch, dim, len, width;
    int32_t dtype;
    uint32_t flags;
} AumConvTmChunkArgs;
int aum_conv1d_tm_chunk(const AumConvTmChunkArgs* args, void* stream);
typedef struct AumScanTmChunkArgs {
    const void *u, *delta, *z, *B, *C;
    const float *A, *D, *delta_bias;
    float* state;
    void* out;
    int64_t u_bs, u_ts, delta_bs, delta_ts, z_bs, z_ts, B_bs, B_ts, C_bs, C_ts, out_bs, out_ts;
    int32_t batch, dim, len, dstate;
    int32_t dtype;
    uint32_t flags;
} AumScanTmChunkArgs;
int aum_scan_tm_chunk(const AumScanTmChunkArgs* args, void* stream);

/*
 * The same two operators on PACKED SESSIONS (additive to ABI 13; `Mamba.step_chunk(..., seq_map=)`): the new rows of `nseq` streaming
 * sessions, each at its own position and with its own number of rows, behind one another in one token stream, and a pool of `nrows`
 * cache rows of which every session owns one.  Activations are packed: element (row, e) at  row * X_ts + e  (no batch stride), `total`
 * rows in all.  cu_seqlens: device int32[nseq + 1], cu_seqlens[0] == 0, non-decreasing, cu_seqlens[nseq] <= total -- sequence i owns rows
 * [cu_seqlens[i], cu_seqlens[i + 1]).  state_indices: device int32[nseq], the cache row of sequence i, or NULL (sequence i uses row i).
 * conv_state (nrows, dim, width) / state (nrows, dim, dstate): the pool, fp32 contiguous; rows that no sequence names are not touched.
 *
 * For every sequence i with cache row r = state_indices[i] the outputs and cache row r are BIT FOR BIT what aum_conv1d_tm_chunk /
 * aum_scan_tm_chunk give at batch 1 on those rows and that cache row (the kernels share one step routine).  So the partition property
 * extends to packing: a session's results depend neither on which other sessions share the call, nor on its place in the pack, nor on
 * its cache row.  An empty sequence is a no-op.  A sequence whose index is outside [0, nrows), or whose cu_seqlens pair is not inside
 * [0, total], is a no-op too: nothing is read or written for it, and nothing is reported (no device-side assert).  Two sequences naming
 * one cache row in one call: undefined results for that row (callers refuse it on the host).  Every other field, flag and limit is that of the fixed-batch
 * entry point; the 32-bit byte-cursor limit applies to `total` rows (the launcher cannot see the per-sequence lengths).
 * nseq >= 1, nrows >= 1, total >= 1; cu_seqlens non-NULL; cu_seqlens and state_indices 4-byte aligned.
 */
typedef struct AumConvTmChunkVarArgs {
    const void* x;
    float* conv_state;
    const float *weight, *bias;
    void* y;
    const int32_t *cu_seqlens, *state_indices;
    int64_t x_ts, y_ts;
    int32_t total, nseq, nrows, dim, width;
    int32_t dtype;
    uint32_t flags;
} AumConvTmChunkVarArgs;
#define AUM_CONV_PEEK_LAST 8u    /* aum_conv1d_tm_chunk_var only: conv_state is written as after len - 1 rows (see AUM_STREAM_PEEK_LAST) */
int aum_conv1d_tm_chunk_var(const AumConvTmChunkVarArgs* args, void* stream);
typedef struct AumScanTmChunkVarArgs {
    const void *u, *delta, *z, *B, *C;
    const float *A, *D, *delta_bias;
    float* state;
    void* out;
    const int32_t *cu_seqlens, *state_indices;
    int64_t u_ts, delta_ts, z_ts, B_ts, C_ts, out_ts;
    int32_t total, nseq, nrows, dim, dstate;
    int32_t dtype;
    uint32_t flags;
} AumScanTmChunkVarArgs;
#define AUM_SCAN_PEEK_LAST 64u   /* aum_scan_tm_chunk_var only: state is written as after len - 1 rows (see AUM_STREAM_PEEK_LAST) */
int aum_scan_tm_chunk_var(const AumScanTmChunkVarArgs* args, void* stream);

/*
 * PEEK ROWS EVERY P ROWS (additive to ABI 13; `Mamba.step_chunk(..., peek_every=)`, `AudioMamba.stream_timeline`): the packed entry
 * points above with an uncommitted row behind every P = peek_every >= 1 committed rows -- the cls row behind every time column of a
 * clip, "what would the logits be if the clip ended now" after each column, all in one pass.
 *   Within every sequence, row j (0-based, counted from the sequence's first row IN THIS CALL) is a peek row iff (j + 1) % (P + 1) == 0.
 *   A peek row is computed and stored like any other row (conv: from the window of the last committed inputs plus its own input; scan:
 *   one step from the current state, then the gate) and neither shifts the window nor updates the state: on exit the cache row holds what
 *   the committed rows alone produce.  A length that is not a multiple of P + 1 is fine (the trailing rows are committed rows); a
 *   sequence shorter than P + 1 has no peek row.
 *   Per sequence, y and the cache row are BIT FOR BIT what aum_*_tm_chunk_var gives when the sequence is cut into groups of P + 1 rows,
 *   called with AUM_*_PEEK_LAST on one full group after the other and once more, without the flag, on the trailing partial group (the
 *   kernels run the same step routine; whether a row commits depends on its index only).
 *   `base`: every field, flag, dtype and limit of aum_conv1d_tm_chunk_var / aum_scan_tm_chunk_var, the no-op rules for empty sequences
 *   and for out-of-range rows or pairs, and the 32-bit cursor limit on `total`.  Refused with nothing touched: peek_every < 1
 *   (AUM_E_SHAPE); base.flags carrying AUM_CONV_PEEK_LAST / AUM_SCAN_PEEK_LAST (AUM_E_UNSUPPORTED).  reserved: 0.
 */
typedef struct AumConvTmChunkPeeksArgs { AumConvTmChunkVarArgs base; int32_t peek_every; int32_t reserved; } AumConvTmChunkPeeksArgs;
typedef struct AumScanTmChunkPeeksArgs { AumScanTmChunkVarArgs base; int32_t peek_every; int32_t reserved; } AumScanTmChunkPeeksArgs;
int aum_conv1d_tm_chunk_peeks(const AumConvTmChunkPeeksArgs* args, void* stream);
int aum_scan_tm_chunk_peeks(const AumScanTmChunkPeeksArgs* args, void* stream);

/*
 * TIMELINE TRAINING (additive to ABI 13; `Mamba.forward(..., peek_every=)`, `AudioMamba.forward_timeline`): the two peek-row operators
 * above as differentiable operations on packed sequences that START A CLIP -- every sequence enters with a zero conv window and a zero
 * state, nothing is carried out, and there is no pool (base.state / base.conv_state, base.state_indices and base.nrows are not read).
 * Row rule as above: row j of a sequence (0-based) is a peek row iff (j + 1) % (P + 1) == 0, P = peek_every >= 1, else a committed row.
 * Gradients into an entry state are not provided.  `base` keeps every other field, dtype, stride rule and limit of the *_chunk_var entry
 * points (cu_seqlens, total, nseq, the 32-bit cursor limit on `total`); an empty sequence is a no-op, and so is a cu_seqlens pair outside
 * [0, total]: none of its rows and none of its partial rows is touched.  No atomics: every result is bitwise repeatable and a sequence's
 * results do not depend on its neighbours or on its place in the pack.  The conv's training forward is aum_conv1d_tm_chunk_peeks itself on
 * a zeroed pool.
 *
 * Scan, per channel e and state n, h the state in front of row t (zero in front of row 0):
 *     dl = delta_t + delta_bias, through softplus with AUM_SCAN_SOFTPLUS (with AUM_SCAN_DELTA_ACTIVATED delta_t is taken as it is);
 *     a = exp(dl A[e,n]);  hn = a h + dl u_t B_t[n];  y_t = sum_n hn C_t[n] + D[e] u_t;  out_t = y_t z_t sigmoid(z_t) (y_t without z);
 *     h <- hn behind a committed row; h stays behind a peek row.
 *   aum_scan_tm_peeks_fwd_ckpt -- the forward.  `out` is BIT FOR BIT that of aum_scan_tm_chunk_peeks on a zeroed pool (the same step
 *     routine); in addition the fp32 state in front of rows 0, 8, 16, ... of every sequence is stored to `ckpt`, which the backward reads:
 *     aum_scan_tm_peeks_ckpt_bytes(total, nseq, dim, dstate) bytes = (total / 8 + nseq) slots of (dim, dstate) fp32, 16-byte aligned.
 *   aum_scan_tm_peeks_bwd -- the adjoint.  base.out is dout (read).  Rows walked downward, g = dL/dh behind row t, zero behind the last row:
 *     dy = dout_t z sigmoid(z);  dz_t = dout_t y_t d/dz[z sigmoid(z)];  dhn[n] = C_t[n] dy + (committed ? g[n] : 0);
 *     dC_t[n] = sum_e hn dy;  dB_t[n] = sum_e dhn dl u_t;  du_t = D dy + dl sum_n dhn B_t[n];  ddl = sum_n dhn (A a h + u_t B_t[n]);
 *     dA[e,n] += dhn dl a h;  dD[e] += dy u_t;  g[n] <- a dhn[n] + (committed ? 0 : g[n]).
 *     ddelta_t is ddl in RAW space as aum_scan_tm_bwd returns it: times 1 - exp(-dl) (the softplus derivative) with AUM_SCAN_SOFTPLUS or
 *     AUM_SCAN_DELTA_ACTIVATED; ddelta_bias[e] += ddelta_t.  du, ddelta, dz: (total, dim) in `dtype`, row strides du_ts / ddelta_ts / dz_ts
 *     (dz NULL without z).  The sums over channels and sequences are left as fp32 PARTIAL ROWS in `workspace`
 *     (aum_scan_tm_peeks_bwd_workspace_bytes(total, nseq, dim, dstate) bytes, 16-byte aligned), in this order:
 *         dBC_part [dim / 64][total][2 dstate]   (dB | dC of a token, one row per 64-channel group)
 *         dA_part  [nseq][dim][dstate],  dD_part [nseq][dim],  dbias_part [nseq][dim]   (one row per sequence)
 *     which the caller adds over the first axis with aum_sum_rows (a fixed order).  The rows of an empty sequence are not written: the
 *     caller zeroes the per-sequence parts first.
 *
 * Conv (width <= 4, weight (dim, width) and bias (dim) fp32, AUM_CONV_SILU):  pre_j = bias + sum_k w[k] win_j[k], win_j = the last
 * width - 1 COMMITTED inputs in front of row j (zeros in front of the sequence) followed by x_j;  y_j = silu?(pre_j).
 *   aum_conv1d_tm_peeks_bwd -- dpre_j = dy_j act'(pre_j) (pre_j recomputed, as aum_conv1d_tm_bwd does); dx of each row in win_j gains
 *     w[k] dpre_j; dw[e,k] += dpre_j win_j[k]; db[e] += dpre_j.  dx (total, dim) in `dtype`, dx != x, dx != dy; the sums over sequences are
 *     left in `workspace` (aum_conv1d_tm_peeks_bwd_workspace_bytes(nseq, dim, width) bytes, 16-byte aligned) as dw_part [nseq][dim][width],
 *     db_part [nseq][dim], to be added with aum_sum_rows; the caller zeroes them first.
 *
 * Refused with nothing touched: peek_every < 1 (AUM_E_SHAPE); AUM_SCAN_PEEK_LAST / AUM_CONV_PEEK_LAST or any flag the forward entry points
 * do not take (AUM_E_UNSUPPORTED); ckpt_bytes / workspace_bytes below the sizes above (AUM_E_WORKSPACE); the 32-bit cursor limit, which
 * here also covers a sequence's checkpoints and the partial rows (AUM_E_UNSUPPORTED).  reserved: 0.
 */
typedef struct AumScanTmPeeksFwdArgs {
    AumScanTmChunkVarArgs base;
    float* ckpt;
    int64_t ckpt_bytes;
    int32_t peek_every, reserved;
} AumScanTmPeeksFwdArgs;
typedef struct AumScanTmPeeksBwdArgs {
    AumScanTmChunkVarArgs base;         /* base.out: dout */
    const float* ckpt;
    void *du, *ddelta, *dz;
    float* workspace;
    int64_t ckpt_bytes, workspace_bytes, du_ts, ddelta_ts, dz_ts;
    int32_t peek_every, reserved;
} AumScanTmPeeksBwdArgs;
typedef struct AumConvTmPeeksBwdArgs {
    const void *x, *dy;
    const float *weight, *bias;
    void* dx;
    float* workspace;
    const int32_t* cu_seqlens;
    int64_t workspace_bytes, x_ts, dy_ts, dx_ts;
    int32_t total, nseq, dim, width;
    int32_t dtype;
    uint32_t flags;
    int32_t peek_every, reserved;
} AumConvTmPeeksBwdArgs;
int64_t aum_scan_tm_peeks_ckpt_bytes(int32_t total, int32_t nseq, int32_t dim, int32_t dstate);
int64_t aum_scan_tm_peeks_bwd_workspace_bytes(int32_t total, int32_t nseq, int32_t dim, int32_t dstate);
int64_t aum_conv1d_tm_peeks_bwd_workspace_bytes(int32_t nseq, int32_t dim, int32_t width);
int aum_scan_tm_peeks_fwd_ckpt(const AumScanTmPeeksFwdArgs* args, void* stream);
int aum_scan_tm_peeks_bwd(const AumScanTmPeeksBwdArgs* args, void* stream);
int aum_conv1d_tm_peeks_bwd(const AumConvTmPeeksBwdArgs* args, void* stream);

/*
 * The recurrent middle of the causal block on packed sessions in ONE launch (additive to ABI 13; `Mamba.step_chunk` through
 * aum_hip.stream_block): from the x half of the in_proj rows to the gated scan output,
 *     xc = silu(conv(x) from conv_state);  x_dbl = xc . wx^T;  delta = softplus(x_dbl[:, :rank] . wdt^T + delta_bias);
 *     y  = scan(xc, delta, A, B = x_dbl[:, rank : rank + 16], C = x_dbl[:, rank + 16 : rank + 32], D, z) from state
 * with y, conv_state and state BIT FOR BIT what the three launches  aum_conv1d_tm_chunk_var (AUM_CONV_SILU)  ->  aum_xdt_tm_fwd
 * (AUM_XDT_DELTA_SOFTPLUS)  ->  aum_scan_tm_chunk_var (AUM_SCAN_DELTA_ACTIVATED)  give on the same operands (the kernels share the step
 * routines), so the partition and packing properties above carry over.  One workgroup per session takes its rows through the three
 * phases; no workgroup waits for another.
 *   x, z: (total, dim) packed rows of pitch x_ts / z_ts ELEMENTS (the halves of the in_proj rows), `dtype` AUM_BF16 / AUM_F16;  y (out):
 *   (total, dim) pitch y_ts, y != x.  conv_state (nrows, dim, width) / state (nrows, dim, dstate): the fp32 pools, the named rows advanced
 *   in place.  conv_weight (dim, width), conv_bias (dim) or NULL, A (dim, dstate), D (dim) or NULL, delta_bias (dim) or NULL: fp32, 16-byte
 *   aligned;  wx (ncols, dim) pitch ldwx, wdt (dim, rank) pitch ldwdt in `dtype`.  cu_seqlens, state_indices, total, nseq, nrows: as for
 *   aum_*_tm_chunk_var, with the same no-op rule (an empty sequence, a row outside the pool, a pair outside [0, total]).  max_len: the
 *   longest session of the call as the host knows it, <= aum_stream_block_max_len() (128); a session longer than max_len is a no-op.
 *   scratch: aum_stream_block_scratch_bytes(total, dim, ncols) bytes, 16-byte aligned -- xc, delta and x_dbl of the call; a session's
 *   workgroup touches the rows of its own session only.
 *   Built for width == 4, dstate == 16 and the shapes of aum_xdt_tm_fwd (dim % 128 == 0, dim <= 1536, ncols 80, 56 or 48, rank % 8 == 0,
 *   rank <= 64, rank + 32 <= ncols, pitches % 8 == 0, 16-byte aligned pointers); anything else returns the error the three entry points
 *   would (AUM_E_DTYPE for fp32 activations, AUM_E_UNSUPPORTED, ...) and callers use the three launches.
 *   flags: AUM_STREAM_NO_COMMIT -- the caches are read and not written (the stores that close the conv and the scan are skipped, nothing
 *   else changes): the logits of a session "if the clip ended now" without copying its caches.
 *   AUM_STREAM_PEEK_LAST (additive to ABI 13) -- the LAST row of every session is a PEEK ROW: it is computed exactly like any other row
 *   (conv from the window, x/dt projections, scan step from the state, gate) and its y is stored, but conv_state and state are written
 *   as they stand after the session's first len - 1 rows.  A cls row that rides behind a session's new tokens sees the state the tokens
 *   produced, and the next call does not see the cls row: "push, then read" in one pass.  Rows 0 .. len - 1 all produce output; for
 *   len == 1 nothing of the session's cache row is written; the no-op rules are unchanged; max_len counts the peek row (128 rows = 127
 *   tokens and the peek).  With AUM_STREAM_NO_COMMIT nothing is written, as without the peek.  Per session, y and both cache rows are BIT
 *   FOR BIT a call without the flag on rows 0 .. len - 2 followed by an AUM_STREAM_NO_COMMIT call on row len - 1 alone (the peek row
 *   runs the same step routine from the same fp32 window and state).  The same rule as two flags of the packed entry points:
 *   AUM_CONV_PEEK_LAST for aum_conv1d_tm_chunk_var and AUM_SCAN_PEEK_LAST for aum_scan_tm_chunk_var (any dtype, any of their other
 *   flags); the three launches with the two flags are bit for bit the one launch with AUM_STREAM_PEEK_LAST.  The fixed-batch entry points
 *   refuse them (AUM_E_UNSUPPORTED).
 */
typedef struct AumStreamBlockArgs {
    const void *x, *z;
    float *conv_state, *state;
    const float *conv_weight, *conv_bias;
    const void *wx, *wdt;
    const float *A, *D, *delta_bias;
    void *y, *scratch;
    const int32_t *cu_seqlens, *state_indices;
    int64_t x_ts, z_ts, y_ts, scratch_bytes;
    int32_t total, nseq, nrows, max_len;
    int32_t dim, width, dstate, rank, ncols, ldwx, ldwdt;
    int32_t dtype;
    uint32_t flags;
} AumStreamBlockArgs;
#define AUM_STREAM_NO_COMMIT 1u
#define AUM_STREAM_PEEK_LAST 2u  /* the last row of every session is computed and stored, the caches close one row early */
int aum_stream_block_tm(const AumStreamBlockArgs* args, void* stream);
int64_t aum_stream_block_scratch_bytes(int32_t total, int32_t dim, int32_t ncols);
int32_t aum_stream_block_max_len(void);

/*
 * PACKED PREFILL (additive to ABI 13; `Mamba.prefill_chunk(..., seq_map=)`): the BACKLOGS of `nseq` streaming sessions in one pass -- the
 * time-parallel conv and the state in / state out scan of the offline forward on packed rows, each session entered with and leaving its
 * own row of the pools.  Packed operands, cu_seqlens, state_indices, total, nseq, nrows and the no-op rule (an empty session, a row
 * outside the pool, a pair outside [0, total]): as for aum_*_tm_chunk_var.  max_len: the longest session of the call as the host knows
 * it (>= 1); a session longer than max_len is a no-op.  Two sessions naming one cache row: undefined results for that row.
 *
 * aum_conv1d_tm_prefill_var -- y[t] = act(bias + sum_k weight[k] * in[t - (width - 1) + k]) over (the session's window, its rows): the
 *   steps of aum_conv1d_tm_fwd, one wave per (session, chunk of at most 64 rows, channel block).  The rows before a session's first row
 *   are conv_state[row, :, 1:], read as fp32 (no rounding, no copy); afterwards conv_state[row] holds the session's last `width` inputs
 *   (fewer rows than `width`: the old entries shift, as under aum_conv1d_tm_chunk).  x (total, dim) pitch x_ts, y (total, dim) pitch
 *   y_ts, y != x; every other field, flag (AUM_CONV_SILU) and limit as aum_conv1d_tm_chunk_var.  Per session, y and the window are bit for bit
 *   what aum_conv1d_tm_fwd gives at batch 1 on the rows [window ; session] when the window's values are exact in `dtype`: the conv is
 *   not recurrent and a step is the same multiply-adds in the same order wherever the chunk boundaries fall.
 * aum_scan_tm_fwd_state_var -- aum_scan_tm_fwd_state per session: rows [cu_seqlens[i], cu_seqlens[i + 1]) from state row
 *   state_indices[i] of state (nrows, dim, 16) fp32, advanced in place.  Forward time, both delta forms (AUM_SCAN_SOFTPLUS /
 *   AUM_SCAN_DELTA_ACTIVATED), with and without z, fp32 / bf16 / fp16; limits of aum_scan_tm_fwd_state on the packed rows (16-byte rows
 *   of u, delta, z, out; 4-byte aligned B / C rows; the 32-bit byte cursor applies to `total` rows).
 *   range_len == 0: uncut, one wave per (session, 64 channels); per session bit for bit aum_scan_tm_fwd_state (segments == 1) at batch 1.
 *   range_len > 0 (a multiple of AUM_SCAN_TM_CK): every session is cut into ranges of range_len steps, nranges = ceil(max_len /
 *   range_len) <= AUM_SCAN_TM_MAX_SEGMENTS, a carry launch and a main launch as aum_scan_tm_fwd_state with segments; carry:
 *   aum_scan_tm_fwd_state_var_carry_bytes(nseq, dim, dstate, nranges) bytes of scratch.  Ranges past a session's end are empty.  A
 *   session's results are bit for bit aum_scan_tm_fwd_state(segments = ceil(len / range_len)) at batch 1 where that call's ranges are
 *   range_len steps too; elsewhere they differ by the re-association at the range boundaries.
 */
typedef struct AumConvTmPrefillVarArgs {
    const void* x;
    float* conv_state;
    const float *weight, *bias;
    void* y;
    const int32_t *cu_seqlens, *state_indices;
    int64_t x_ts, y_ts;
    int32_t total, nseq, nrows, dim, width;
    int32_t dtype;
    uint32_t flags;
    int32_t max_len;
} AumConvTmPrefillVarArgs;
int aum_conv1d_tm_prefill_var(const AumConvTmPrefillVarArgs* args, void* stream);
typedef struct AumScanTmFwdStateVarArgs {
    const void *u, *delta, *z, *B, *C;
    const float *A, *D, *delta_bias;
    float* state;
    void* out;
    const int32_t *cu_seqlens, *state_indices;
    int64_t u_ts, delta_ts, z_ts, B_ts, C_ts, out_ts;
    int32_t total, nseq, nrows, dim, dstate;
    int32_t dtype;
    uint32_t flags;
    int32_t range_len, max_len, reserved;
    float* carry;
    int64_t carry_bytes;
} AumScanTmFwdStateVarArgs;
int aum_scan_tm_fwd_state_var(const AumScanTmFwdStateVarArgs* args, void* stream);
int64_t aum_scan_tm_fwd_state_var_carry_bytes(int32_t nseq, int32_t dim, int32_t dstate, int32_t nranges);

/* Self-tests and calibration (used by tests/ and bench.py; not part of the reference's surface). */
int aum_abi_version(void);
/* runs wave_scan_affine<rev> on 64 (P,S) pairs: in/out are device arrays of 128 floats (P[0..63], S[0..63]) */
int aum_selftest_wave_scan(const float* in, float* out, int rev, void* stream);
/* runs wave_sum32 (transposing butterfly sum over the 64 lanes) on 32 x 64 values in[k][lane]; out[lane] = the total of value
 * 2 * (lane & 15) + ((lane >> 4) & 1); out[64 + lane] = wave_sum16 of values 0..15; out[128 + lane] / out[192 + lane] = the matrix-pipe
 * sums (terms rounded to bf16, round 4) of values 0..15 / 16..31: the total of value 4 * (lane >> 4) + bit3(lane) + 2 * bit2(lane) of
 * the tile.  out: 256 floats */
int aum_selftest_wave_sum32(const float* in, float* out, void* stream);
/* float4 streaming copy, the measured-HBM-roofline denominator of SURVEY.md 8(d) */
int aum_hbm_copy(const void* src, void* dst, int64_t bytes, void* stream);

/*
 * dst[b][i] = sum over o of src[b][o][i] in fp32 (ABI 6; batch = 1 for a plain sum, > 1 for the first stage of a two-stage sum): the fixed-order sum of the per-workgroup partial results that
 * aum_rmsnorm_bwd (dweight_partial) and aum_proj_bwd_weight (out) leave to the caller, and of split-K GEMM partial products
 * (SSI:563, 586, 589; the reference leaves the same kind of sum to torch: LN:333-372).  src: (batch, outer, inner) contiguous in
 * src_dtype (AUM_F32 / AUM_BF16 / AUM_F16), dst: (batch, inner) fp32.  inner % 8 == 0; src 16-byte aligned, dst any float address (round 6: a parameter
 * gradient's view inside a DistributedDataParallel bucket may sit behind an odd-sized parameter).
 */
int aum_sum_rows(const void* src, float* dst, int64_t batch, int64_t outer, int64_t inner, int32_t src_dtype, void* stream);

/*
 * ABI 11: up to AUM_SUM_MAX_JOBS independent fixed-order sums of fp32 partial results in ONE launch -- a layer's backward leaves five partial sets behind
 * (the out_proj weight-gradient splits and the two skinny partial sets of aum_gemm_wgrad, SSI:563, 586, 589; the conv weight and bias partials of
 * aum_conv1d_tm_bwd), and a 5 us launch per set is 5 us of the step.  Job q:  dst[i] = sum over o < outer of src[o][i],  i < inner  -- each job with
 * the row grouping aum_sum_rows (batch = 1) picks for it, i.e. the same additions in the same order as a launch of its own: bitwise the same result.  tr_cols > 0: the summed (inner / tr_cols, tr_cols) matrix is stored transposed, dst
 * (tr_cols, inner / tr_cols) -- the x_proj weight gradient leaves aum_gemm_wgrad as (dim, R + 2N) and the parameter is (R + 2N, dim).
 * 1 <= njobs <= AUM_SUM_MAX_JOBS, inner % 8 == 0, inner % tr_cols == 0; src 16-byte aligned, dst any float address; `jobs` is read on the host during the call.
 */
#define AUM_SUM_MAX_JOBS 8
typedef struct AumSumJob {
    const float* src;       /* (outer, inner) contiguous */
    float* dst;             /* (inner), or (tr_cols, inner / tr_cols) */
    int64_t outer, inner;
    int32_t tr_cols;
    int32_t reserved;
} AumSumJob;
int aum_sum_rows_multi(const AumSumJob* jobs, int32_t njobs, void* stream);

/* The 16-bit working copies of fp32 master weights (ABI 13).  Replaces: torch.autocast's per-call cast of F.linear's weight operand (the
 * reference's in_proj / x_proj / dt_proj / out_proj under --mixed_precision, MS:185-189, SSI:467-468, 517) -- hoisted to one launch per
 * group of equally shaped matrices at the top of a forward (ssi.step_cache).
 *   src     DEVICE array of n addresses, each an fp32 (rows, cols) contiguous matrix
 *   bank    (n, rows, cols) in `dtype` (AUM_BF16 / AUM_F16), round-to-nearest-even (what Tensor.to() does)
 *   bank_t  (n, cols, rows): the transposes, or NULL
 * rows % 8 == 0, cols % 4 == 0; bank / bank_t 16-byte aligned. */
int aum_cast_bank(const uint64_t* src, int32_t n, int32_t rows, int32_t cols, void* bank, void* bank_t, int32_t dtype, void* stream);

/*
 * Parking streaming sessions (no version step: an addition).  A session of a pool is one row of every pool tensor -- per layer the conv
 * window and the scan state, and the sample tail of a raw-audio stream.  ONE launch copies those rows of n_sessions sessions into one
 * record per session of a byte blob (flags 0), or the records back into rows of a pool (AUM_PARK_RESTORE): the same pool or another one
 * of the same layout, any rows.  The bytes are moved as they are; nothing is converted.
 *   base[t], row_stride[t], row_bytes[t]   pool tensor t < n_tensors: row r is the row_bytes[t] bytes at base[t] + r * row_stride[t]
 *   blob_off[t]                            where tensor t's row sits inside a record; the ranges [blob_off[t], blob_off[t] + row_bytes[t])
 *                                          ascend with t, do not overlap and end inside blob_stride
 *   rows                                   (n_sessions) int32 in DEVICE memory: the pool row of session i, >= 0 and distinct.  That the rows
 *                                          exist in every pool tensor is the caller's check (aum_hip.stream_park makes it on the host); a
 *                                          negative entry is skipped
 *   blob, blob_stride                      record i is the blob_stride bytes at blob + i * blob_stride.  AUM_PARK_RESTORE also takes
 *                                          blob_stride == 0: every session is restored from the one record at `blob`
 * Workgroups of 256 lanes over (session, tensor, 4 KiB chunk of the row), 16 bytes per lane; the tail of a row is guarded by row_bytes.
 * Only the named rows' row_bytes and the records' [blob_off, blob_off + row_bytes) ranges are read or written: the bytes between the rows
 * of a strided pool tensor and between or behind the ranges of a record keep what they hold.
 * AUM_E_NULL: args, rows, blob or a base is NULL.  AUM_E_UNSUPPORTED: n_tensors outside [1, AUM_PARK_MAX_TENSORS], n_sessions < 1, an
 * unknown flag, a base, blob, stride, row size or offset that is not a multiple of 16 (rows: of 4), row_bytes < 16, row_stride < row_bytes,
 * ranges of a record that overlap, descend or pass blob_stride, or more than 2^31 - 1 workgroups.
 */
#define AUM_PARK_MAX_TENSORS 64
#define AUM_PARK_RESTORE 1u
typedef struct AumParkArgs {
    void*   base[AUM_PARK_MAX_TENSORS];
    int64_t row_stride[AUM_PARK_MAX_TENSORS]; /* bytes */
    int64_t row_bytes[AUM_PARK_MAX_TENSORS];  /* bytes copied per row, multiple of 16 */
    int64_t blob_off[AUM_PARK_MAX_TENSORS];   /* byte offset of tensor t's row inside a session's record, multiple of 16 */
    const int32_t* rows;    /* (n_sessions) pool rows, device memory */
    void*   blob;           /* (n_sessions, blob_stride) bytes */
    int64_t blob_stride;
    int32_t n_tensors, n_sessions;
    uint32_t flags;         /* AUM_PARK_RESTORE: blob -> pool; 0: pool -> blob */
} AumParkArgs;
int aum_stream_park(const AumParkArgs* args, void* stream);

/*
 * A HOP THROUGH ALL BLOCKS IN ONE CALL (no version step: an addition; `AudioMamba.stream_stack`, aum_hip.stream_layers).  What is left of
 * a streaming hop around aum_stream_block_tm is the add + RMSNorm, the two skinny projections and the host between them; here a block is
 * three launches that a C loop enqueues back to back:
 *     aum_stream_in_tm   residual_out = hidden (+ residual_in)   fp32
 *                        normed       = rmsnorm(residual_out) * norm_weight, rounded to `dtype`   (bit for bit aum_rmsnorm_fwd: its row routine)
 *                        xz           = normed . w_in^T
 *     aum_stream_block_tm on xz's halves (the existing kernel, the existing arguments)
 *     aum_stream_out_tm  out = y . w_out^T
 * Both projections: every output element is ONE round-to-nearest-even of an fp32 accumulation of exact 16-bit products, on the matrix
 * pipe (v_mfma_f32_16x16x32), the weights as the A operand and 16 token rows as the B operand: an MFMA column is one token, and the
 * order of the K loop (four waves take the K-steps of 32 round robin, their four partial sums are added in wave order) depends on
 * nothing but K.  A row's bits therefore do not depend on total, on the row's place in the pack or on its neighbours.
 * A workgroup owns 32 (in) / 16 (out) output columns, keeps their weights in registers and walks the rows in tiles of 16; the norm
 * prologue is recomputed by every workgroup (the rows come from L2), workgroup 0 alone writes residual_out.  No workgroup waits for
 * another: no grid sync, no flags, no atomics, no partial sums through memory.
 *   hidden (total, d_model) pitch hidden_ts, xz (total, 2 dim) pitch xz_ts, y (total, dim) pitch y_ts, out (total, d_model) pitch out_ts,
 *   w_in (2 dim, d_model) pitch ldw, w_out (d_model, dim) pitch ldw: `dtype` AUM_BF16 / AUM_F16 (AUM_F32: AUM_E_DTYPE), K contiguous.
 *   residual_in (total, d_model) fp32 contiguous or NULL; residual_out the same, never NULL and NOT residual_in (other workgroups still
 *   read residual_in while it is written: AUM_E_UNSUPPORTED).  norm_weight (d_model) fp32.
 *   Built for (d_model, dim) = (192, 384), (384, 768), (768, 1536), any total >= 1; pointers 16-byte aligned, pitches % 8 == 0 and not
 *   below the row, total * pitch * 2 < 2^31; anything else AUM_E_UNSUPPORTED.
 */
typedef struct AumStreamInArgs {
    const void* hidden;
    const float *residual_in, *norm_weight;
    const void* w_in;
    float* residual_out;
    void* xz;
    int64_t hidden_ts, xz_ts;
    int32_t total, d_model, dim, ldw, dtype;
    float eps;
} AumStreamInArgs;
typedef struct AumStreamOutArgs {
    const void *y, *w_out;
    void* out;
    int64_t y_ts, out_ts;
    int32_t total, d_model, dim, ldw, dtype, reserved;
} AumStreamOutArgs;
int aum_stream_in_tm(const AumStreamInArgs* args, void* stream);
int aum_stream_out_tm(const AumStreamOutArgs* args, void* stream);
/*
 * aum_stream_layers: `depth` blocks on the packed rows of a hop, 3 * depth launches on the one stream.
 *   layers      HOST array of depth records of DEVICE pointers (read during the call only): norm_weight (d_model) fp32, w_in, w_out as
 *               above (pitches d_model / dim), conv_weight .. delta_bias and the pools conv_state (nrows, dim, 4) / state (nrows, dim, 16)
 *               as AumStreamBlockArgs names them (conv_bias, D, delta_bias may be NULL), wx pitch ldwx, wdt pitch ldwdt
 *   hidden      (total, d_model) pitch hidden_ts: the rows that enter block 0;  residual_in: fp32 (total, d_model) or NULL
 *   hidden_out  (total, d_model) contiguous, residual_out fp32 the same: what the last block leaves (residual_out != residual_in)
 *   cu_seqlens, state_indices, total, nseq, nrows, max_len, flags (AUM_STREAM_NO_COMMIT, AUM_STREAM_PEEK_LAST): aum_stream_block_tm's
 *   workspace   aum_stream_layers_scratch_bytes(total, d_model, dim, ncols) bytes, 16-byte aligned: xz, y, two hidden buffers, two fp32
 *               residual buffers (a block reads one and writes the other) and aum_stream_block_tm's scratch, every offset a multiple of 16
 * EVERY operand of EVERY layer is checked before the first launch (the checks of the three entry points on the arguments the loop will
 * hand them): a refused call returns its code and has written nothing.  Given the same xz the middle launch's y and pool rows are bit for
 * bit aum_stream_block_tm's, and the whole call is bit for bit the loop of the three entry points.
 */
typedef struct AumStreamLayer {
    const float* norm_weight;
    const void* w_in;
    const float *conv_weight, *conv_bias;
    const void *wx, *wdt;
    const float *A, *D, *delta_bias;
    const void* w_out;
    float *conv_state, *state;
} AumStreamLayer;
typedef struct AumStreamLayersArgs {
    const AumStreamLayer* layers;
    const void* hidden;
    const float* residual_in;
    void* hidden_out;
    float* residual_out;
    void* workspace;
    const int32_t *cu_seqlens, *state_indices;
    int64_t hidden_ts, workspace_bytes;
    int32_t depth, total, nseq, nrows, max_len;
    int32_t d_model, dim, rank, ncols, ldwx, ldwdt;
    int32_t dtype;
    uint32_t flags;
    float eps;
} AumStreamLayersArgs;
int aum_stream_layers(const AumStreamLayersArgs* args, void* stream);
int64_t aum_stream_layers_scratch_bytes(int32_t total, int32_t d_model, int32_t dim, int32_t ncols);

/*
 * EPIC-Sounds log-mel frontend (an addition to ABI 13; replaces librosa.stft + filters.mel + log on the CPU DataLoader workers of the reference,
 * src/epic_sounds/epic_data/audio_loader_epicsounds.py:94-156).  Per clip b and output frame t < target_length:
 *   frames  = 1 + n_valid[b] / hop   (librosa center=True: the clip is zero-padded by n_fft / 2 on both sides);  frame t >= frames is a copy of
 *             frame frames - 1 (np.pad 'edge'), frames past target_length are dropped
 *   frame f = samples f * hop - n_fft / 2 + (n_fft - win) / 2 + j, j < win, times window[j] (zero outside [0, n_valid[b]))
 *   out[b][t][m] = log(sum_c mel_w[m][c] * |X[mel_start[m] + c]| + eps),   X = the n_fft-point DFT of the frame (magnitude, not power)
 *   wave        (batch, n_samples) fp32, batch stride wave_bs elements;  n_valid (batch) int32, 0 <= n_valid[b] <= n_samples
 *   window      (win) fp32;  twiddle (n_fft / 2 complex pairs exp(-2 pi i k / n_fft));  mel_start_f / mel_count_f (num_mel, small integers
 *               stored as fp32), mel_w (num_mel, mel_wstride): the sparse HTK filterbank built by the host (aum/epic.py)
 *   out         (batch, target_length, num_mel) fp32, batch stride out_bs elements
 * n_fft a power of two, 256 <= n_fft <= AUM_STFT_MAX_FFT; 0 < win <= n_fft; hop > 0.
 */
#define AUM_STFT_MAX_FFT 2048
typedef struct AumStftArgs {
    const float *wave, *window, *twiddle, *mel_start_f, *mel_count_f, *mel_w;
    const int32_t* n_valid;
    float* out;
    int64_t wave_bs, out_bs;
    int32_t batch, n_samples, win, hop, n_fft, num_mel, mel_wstride, target_length;
    float eps;
    int32_t reserved;
} AumStftArgs;
int aum_stft_logmel_fwd(const AumStftArgs* args, void* stream);

/*
 * SpecAugment time warp of the EPIC-Sounds recipe (an addition to ABI 13; spec_augment.py:346-360 -> sparse_image_warp / dense_image_warp,
 * :6-42, 199-345), out of place.  The reference warps the (num_mel, frames) image with a one-centre polyharmonic spline (order 2) whose
 * frequency flow is exactly 0; per clip its time flow is
 *   r(y, x)    = (xn - 2 (y cy + x cx)) + yn                      (the reference's squared distance: xn sums the squares of EVERY grid point)
 *   flow(y, x) = 0.5 r log(max(r, 1e-10)) w + ((y v0 + x v1) + v2),   y = mel bin, x = frame
 * and out[y][x] is the bilinear sample of in at (y, x - flow) with dense_image_warp's clamping (floor in [0, size - 2], weight in [0, 1]).
 *   in / out (batch, frames, num_mel) fp32 (frame-major, the layout of aum_stft_logmel_fwd), batch strides in_bs / out_bs; in != out
 *   table    (batch, AUM_TIME_WARP_COLS) fp32 per clip: [cy, cx, w, v0, v1, v2, xn, yn], solved on the host (aum/epic.py)
 * frames >= 2, num_mel >= 2, frames * num_mel >= 64.
 */
#define AUM_TIME_WARP_COLS 8
typedef struct AumTimeWarpArgs {
    const float *in, *table;
    float* out;
    int64_t in_bs, out_bs;
    int32_t batch, frames, num_mel, reserved;
} AumTimeWarpArgs;
int aum_spec_time_warp(const AumTimeWarpArgs* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AUM_HIP_H */
