/* C ABI of libfourm_hip.so — the MI355X (gfx950) kernels behind the 4M training hot path.
 *
 * The upstream project (apple/ml-4m) is pure PyTorch and has no FFI of its own; every entry point
 * below therefore names the chain of upstream torch ops it replaces (file:line under
 * /root/reference).  INTEGRATION.md shows the ctypes binding a maintainer would add upstream.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless stated otherwise; the caller owns all memory,
 *     including workspaces; no function allocates, frees or synchronises;
 *   - `stream` is a hipStream_t (pass torch.cuda.current_stream().cuda_stream), 0 = null stream;
 *   - bf16 buffers are raw uint16 bit patterns; leading dimensions (ld*) are in ELEMENTS;
 *   - return value: 0 = launched, <0 = rejected (-1 bad argument, -2 launch failure); the reason is
 *     available from fm_last_error() (thread-local, valid until the next call on that thread);
 *   - functions are re-entrant; one host thread per device is the intended use.
 */
#ifndef FOURM_HIP_H
#define FOURM_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FM_ABI_VERSION 11
int fm_abi_version(void);
const char* fm_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * GEMM (bf16 operands, fp32 accumulate on the MFMA matrix cores)
 * ---------------------------------------------------------------------------------------------- */
enum fm_epilogue {
    FM_EPI_BF16 = 0,     /* out(bf16)  = bf16(acc + bias)                                            */
    FM_EPI_GELU = 1,     /* out(bf16)  = gelu(bf16(acc + bias)); out2(bf16, optional) = pre-activation */
    FM_EPI_RESIDUAL = 2, /* out(f32)   = res(f32) + bf16(acc + bias)      (out may alias res)         */
    FM_EPI_SWIGLU = 3,   /* W -> g, W2 -> u: out(bf16)[m][h] = silu(g)*u; out2(bf16, optional)[m][h] = g, [m][Hp+h] = u */
    FM_EPI_F32 = 4,      /* out(f32)   = acc + bias (+ res(f32) when given; no rounding)              */
    FM_EPI_TANH = 5,     /* out(bf16)  = tanh(bf16(acc + bias))                                       */
    FM_EPI_SWIGLU_BWD = 6, /* acc = d(silu(g)*u); res(bf16,(M,2*Hp)) = g|u saved by FM_EPI_SWIGLU;
                              out(bf16,(M,2*Hp)) = dg | du.  Columns [roundup4(N), Hp) of each half are not written */
    FM_EPI_GELU_BWD = 7, /* acc = d(gelu(pre)); res(bf16) = pre saved by FM_EPI_GELU; out(bf16) = d(pre) */
    FM_EPI_QUICK_GELU = 8, /* CLIP's QuickGELU: pre = bf16(acc + bias); out(bf16) = pre / (1 + exp(-1.702 pre)); out2(bf16, optional) = pre.
                             Accepted wherever FM_EPI_GELU is (same kernels, same dispatch) and by the few-row kernel; large |pre| gives
                             +-0 or pre, never NaN */
    FM_EPI_RELU = 9,      /* out(bf16) = max(bf16(acc + bias), 0).  Implicit convolutions (conv_*) only, never split over K; dense launches are
                             refused.  fm_gemm_f32 takes it too: out(f32) = max(acc + bias, 0) */
    FM_EPI_RELU_BWD = 10  /* acc = d(relu(pre)); res(bf16, row stride ldr) = the ReLU output saved by FM_EPI_RELU (or any rows whose sign is
                             the mask); out(bf16) = res > 0 ? bf16(acc) : 0.  No bias.  Implicit convolutions only; refused by fm_gemm_f32 */
};

typedef struct fm_gemm_group {  /* one entry per row segment (modality) in grouped mode */
    const void* W;              /* NT: weight-like operand of this group; TN: unused               */
    void* out;                  /* TN: fp32 accumulator of this group;    NT: unused               */
    int32_t N, K, ldw, pad_;
} fm_gemm_group;

/* out[m][n] = sum_k X[m][k] * W[n][k]  (+ epilogue).
 * Replaces nn.Linear forward under bf16 autocast — fourm/models/fm_utils.py:116-126,137-144,155-157,
 * 190-194 — and, with a transposed weight shadow, its input gradient.
 * K % 64 == 0 (zero padded), ldw/ldx % 8 == 0, ldo % 4 == 0 and ldo >= roundup4(N): a lane stores 4
 * consecutive features, so for N % 4 != 0 the columns [N, roundup4(N)) of out receive don't-care values
 * (FM_EPI_SWIGLU writes zeros there instead).
 * Grouped mode (groups != NULL): rows of X are segmented in FM_SEG_ROWS-row tiles, tile_group[tile] selects
 * the group (or -1 = skip); W/N/K/ldw come from the group record, max_N bounds the launch and K (an upper bound
 * of the groups' K, 0 = unknown) picks the tile configuration. */
typedef struct fm_gemm_nt_args {
    const void* W; const void* W2; const void* X;
    void* out; void* out2; const void* res; const void* bias; const void* bias2;
    int32_t M, N, K, ldw, ldx, ldo, ldo2, ldr, Hp, epilogue;
    const fm_gemm_group* groups; const int32_t* tile_group; int32_t max_N;
    /* fixed_tiling (ABI 9; dense launches, no conv_*): != 0 pins the launch to ONE kernel and tile configuration (128 x 128 tiles, K-step 32,
     * no split over K, no few-row kernel) whatever M, N and K are, so that a row of out depends on that row of X alone, bit for bit, however
     * many rows the call has.  The instance-mask tokenizer runs on it: an instance's tokens and mask must not depend on the batch it came in. */
    int32_t fixed_tiling;
    /* Row range in DEVICE memory (ABI 7; both or neither, NULL = rows [0, M)): the launch covers rows [*row0_dev, *row0_dev +
     * roundup(*m_dev, FM_SEG_ROWS)) of X / out - one modality head's segment as fm_segment_rows laid it out (seg_start[h], seg_count[h];
     * pad rows zero) - with M an upper bound.  One dense launch per head then replaces the grouped launch without a host read of the
     * row counts (FourM.forward_logits, fm.py:521-545).  FM_EPI_BF16 without bias, ldo % 64 == 0, out 128-byte aligned, N % 8 == 0,
     * K % 64 == 0; other arguments are rejected. */
    const int32_t* m_dev; const int32_t* row0_dev;
    /* Scratch for split-K (ABI 8; optional, NULL = never split): a dense FM_EPI_BF16 launch whose output has too few tiles for the chip
     * (small M x N, long K: the convolutions of the DiVAE UNet at its coarse levels) is cut into up to 16 K-slices that write fp32 partial
     * tiles here (slices x M x roundup4(N) x 4 bytes are needed; a smaller buffer means fewer slices or none), followed by one reduction
     * pass (sum of the slices + bias -> bf16).  The buffer is dead when the call's work has run; calls on one stream may share it. */
    void* splitk_ws; int64_t splitk_ws_bytes;
    /* Implicit 3 x 3 convolution (ABI 8; conv_C = 0: off).  X is then a bf16 feature map in rows, (B, conv_H >> conv_up, conv_W >> conv_up, conv_C)
     * with row stride ldx, read at (y >> conv_up, x >> conv_up) (conv_up = 1: the nearest x2 up-sampling in front of the convolution); the launch
     * computes out[(b, oy, ox)][n] = sum over tap, c of in[b][oy stride + tap / 3 - 1][ox stride + tap % 3 - 1][c] W[n][tap conv_C + c] (zero
     * padding) on a (conv_Ho, conv_Wo) output grid: M = B conv_Ho conv_Wo, K = 9 conv_C, conv_C % 64 == 0, conv_stride 1 | 2 - exactly
     * fm_unet_im2col + the plain launch (bit-identical), without writing the 9 x expanded rows.  FM_EPI_BF16 (may be split over K like any
     * small launch) or FM_EPI_F32, dense, no residual / second output; FM_EPI_RELU (bias allowed) and FM_EPI_RELU_BWD (res = the bf16
     * mask rows, ldr % 4 == 0, ldr >= roundup4(N), res / out 8-byte aligned, no bias), neither ever split over K. */
    int32_t conv_C, conv_H, conv_W, conv_Ho, conv_Wo, conv_stride, conv_up, conv_pad_;
} fm_gemm_nt_args;
int fm_gemm_nt(const fm_gemm_nt_args* args, void* stream);
/* tile configuration of fm_gemm_nt, for A/B measurements (table in csrc/gemm.hip): low byte 0-8 = fixed
 * configuration, 9 = automatic (default); +256 = raise the wave priority around the MFMA clusters;
 * bits 16-19 / 20-23 (when non-zero) = the configurations "automatic" picks for K < 1536 / K >= 1536 (and reading
 * epilogues); bits 24-27 (when non-zero) = its choice for the SwiGLU epilogue. */
void fm_set_gemm_nt_config(int cfg);
int fm_get_gemm_nt_config(void);
/* Compute units the persistent GEMM grids leave free (default 0; env FOURM_RESERVED_CUS): set by the data-parallel wrapper so that
 * RCCL's kernels find CUs while a gradient bucket is exchanged under the backward GEMMs (upstream: DDP overlap, run_training_4m.py:512). */
void fm_set_reserved_cus(int n);
int fm_get_reserved_cus(void);

/* out[n][k] += sum_r A[r][n] * B[r][k]   (fp32 atomic accumulation, reduction split over blocks).
 * Replaces the weight-gradient matmul autograd runs for nn.Linear (dW = dY^T X).
 * Any R >= 1: reduction rows >= R are masked inside the kernel (A / B need no padding rows); lda/ldb % 8 == 0; a_cols/b_cols = number of
 * readable columns of A/B (0 = lda/ldb).  splits <= 0 picks a split count; force_tr: -1 = library
 * default, 0 = 2-byte LDS gathers, 1 = ds_read_b64_tr_b16 transpose reads.
 * Grouped mode: group g reduces rows [seg_start[g], seg_start[g] + roundup64(seg_count[g])) into
 * groups[g].out with N = groups[g].N. */
typedef struct fm_gemm_tn_args {
    const void* A; const void* B; void* out;
    int32_t R, N, K, lda, ldb, ldo, a_cols, b_cols, splits, force_tr;
    const fm_gemm_group* groups; const int32_t* seg_start; const int32_t* seg_count;
    int32_t n_groups, max_N, max_R, pad_;
} fm_gemm_tn_args;
int fm_gemm_tn(const fm_gemm_tn_args* args, void* stream);
/* A list of dense weight-gradient GEMMs in ONE launch (all dW of a transformer layer: fourm/models/fm_utils.py Block /
 * DecoderBlock backward as autograd runs it, one addmm per nn.Linear): job i does out_i[n][k] += sum_{r<R_i} A_i[r][n] * B_i[r][k]
 * with fm_gemm_tn's operand rules.  The tiles of all jobs share one grid of one workgroup per CU: whole-row reductions while a
 * full round of tiles remains, one main + tail cut of the last partial round (csrc/gemm.hip, gemm_tn_multi_kernel).
 * n_jobs <= FM_TN_MAX_JOBS; the job array is read on the host at call time. */
#define FM_TN_MAX_JOBS 16
typedef struct fm_gemm_tn_job {
    const void* A; const void* B; void* out;
    int32_t R, N, K, lda, ldb, ldo, a_cols, b_cols;
} fm_gemm_tn_job;
int fm_gemm_tn_multi(const fm_gemm_tn_job* jobs, int n_jobs, void* stream);
/* tile schedule of fm_gemm_tn (table in csrc/gemm.hip): 0 = K-step 32, two workgroups per CU; 1 = K-step 64,
 * one workgroup per CU, ping-pong schedule (half the workgroups -> half the atomic epilogue traffic); 3 = as 1, and
 * fm_gemm_tn_multi falls back from its 256 x 256 tiles to 128 x 256. */
void fm_set_gemm_tn_config(int cfg);
int fm_get_gemm_tn_config(void);
void fm_set_tn_transpose_read(int on);
int fm_get_tn_transpose_read(void);

/* ------------------------------------------------------------------------------------------------
 * LayerNorm (eps inside the sqrt, fp32 statistics) — F.layer_norm as used by
 * fourm/models/fm_utils.py:93-108 (and nn.LayerNorm in the *_gelu factories, fm.py:853).
 * x: f32 (R, D); y: bf16 (default) or f32; b may be NULL; mean/rstd (R) f32 optional outputs.
 * row_map (optional): y row r is written to row row_map[r] (skipped when negative).
 * D % 4 == 0, D <= 2048. */
int fm_layernorm_fwd(const void* x, int ldx, const void* w, const void* b, void* y, int ldy, int y_is_f32,
                     void* mean, void* rstd, const int32_t* row_map, int R, int D, float eps, void* stream);
/* The same with the residual add in front: row = x + delta (delta: bf16 (R, D), the output of the Linear that precedes the norm,
 * fm_utils.py:332-333, 363-365); the sum is also written to x_out (f32, the new residual stream; may not alias x). */
int fm_layernorm_fwd_res(const void* x, int ldx, const void* delta, int ldd, void* x_out, int ldxo, const void* w, const void* b,
                         void* y, int ldy, int y_is_f32, void* mean, void* rstd, const int32_t* row_map, int R, int D, float eps,
                         void* stream);
/* dx(f32) = dres + LN'(dy);  dw += sum_r dy*xhat;  db += sum_r dy  (fp32 atomics; dw/db may be NULL).
 * dy: bf16, read at row dy_row_map[r] when a map is given (negative = zero gradient).
 * dres (optional, may alias dx) is the residual-stream gradient flowing around the norm.
 * dx_bf16 (optional) receives a bf16 copy of dx (operand of the next GEMM). */
int fm_layernorm_bwd(const void* dy, int lddy, const int32_t* dy_row_map, const void* x, int ldx, const void* w,
                     const void* mean, const void* rstd, const void* dres, void* dx, int lddx, void* dx_bf16,
                     int lddxbf, void* dw, void* db, int R, int D, void* stream);
/* The same for a bias-free norm whose bf16 output h = bf16(xhat * w) (R, D; what fm_layernorm_fwd wrote, kept for the weight-gradient
 * GEMM of the Linear it feeds) is still in memory: xhat = h / w is rebuilt from the 2-byte h instead of the 4-byte x (14 instead of
 * 16 bytes per element; xhat carries h's bf16 rounding, relative 2^-9).  x is read only for 4-column chunks holding a weight of
 * magnitude < 1e-20.  No row map, no bias gradient. */
int fm_layernorm_bwd_h(const void* dy, int lddy, const void* h, int ldh, const void* x, int ldx, const void* w,
                       const void* mean, const void* rstd, const void* dres, void* dx, int lddx, void* dx_bf16,
                       int lddxbf, void* dw, int R, int D, void* stream);

/* Per-head LayerNorm of q / k for qk_norm models (NormAttention / NormCrossAttention q_norm, k_norm:
 * fourm/models/fm_utils.py:235-236,244-245,279-280,290-291).  x, y: bf16 rows of H heads x 64 contiguous features
 * (row stride ldx / ldy, e.g. the q or k column block of the fused qkv buffer); w, b: f32 (64) (b may be NULL);
 * stats: f32 (R*H, 2) = (mean, rstd) kept for the backward.  fp32 arithmetic, bf16 result (autocast). */
int fm_headnorm_fwd(const void* x, int ldx, const void* w, const void* b, void* y, int ldy, void* stats, int R, int H, float eps,
                    void* stream);
/* dx (bf16) = LayerNorm backward of dy w.r.t. the head vectors; dw / db (f32 (64), may be NULL) are accumulated. */
int fm_headnorm_bwd(const void* dy, int lddy, const void* x, int ldx, const void* w, const void* stats, void* dx, int lddx, void* dw,
                    void* db, int R, int H, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Masked multi-head attention, head_dim 64 — fourm/models/fm_utils.py:160-180 (Attention) and
 * :197-219 (CrossAttention).  Element (b, t, h, d) of Q lives at Q[(b*Nq + t)*ldq + h*64 + d]
 * (K, V with Nk; O, dO, dQ like Q; dK, dV like K), so q/k/v can alias one fused qkv buffer.
 * A blocked score is replaced by -finfo(bf16).max (upstream semantics: fully blocked rows attend
 * uniformly).  stat_m / stat_l: (B, H, Nq) f32 row max and row sum, written by fwd, read by bwd. */
enum fm_mask_kind {
    FM_MASK_NONE = 0,
    FM_MASK_KEYPAD = 1,   /* kpad (B, Nk) uint8, 1 = blocked                  — fm.py:388                   */
    FM_MASK_DECODER = 2,  /* k >= cs[b][q] (or k > q if causal)  ||  modq[b][q] != modk[b][k] — fm.py:440-475 */
    FM_MASK_DENSE = 3     /* dense (B, Nq, Nk) uint8, 1 = blocked                                            */
};
typedef struct fm_attn_args {
    const void* Q; const void* K; const void* V; void* O;
    void* stat_m; void* stat_l;
    int32_t ldq, ldk, ldv, ldo;
    int32_t B, H, Nq, Nk, head_dim, mask_kind;
    float scale; int32_t causal;
    const void* kpad; const int32_t* cs; const int16_t* modq; const int16_t* modk; const void* dense;
    /* backward only */
    const void* dO; void* dQ; void* dK; void* dV;
    int32_t lddo, lddq, lddk, lddv;
    int32_t force_tr;         /* -1 = library default, 0 = 2-byte LDS gathers, 1 = transpose reads */
    int32_t kv_batch_rows;    /* forward only: rows between two samples in K / V (0 = Nk).  A K/V cache of capacity T holds sample b's
                                 keys at rows [b*T, b*T + Nk): incremental decoding attends to the Nk filled rows without copying */
    int32_t zero_attn;        /* allow_zero_attn (fm_utils.py:28-30, :171-172): softmax over the scores AND one extra zero logit whose
                                 probability is dropped (p_k = e^{s_k} / (1 + sum_j e^{s_j})): a query may attend to nothing */
} fm_attn_args;
int fm_attn_fwd(const fm_attn_args* args, void* stream);
int fm_attn_bwd(const fm_attn_args* args, void* stream);   /* any Nq, Nk (single pass up to 512 rows, 256-row chunks above) */
void fm_set_attn_transpose_read(int on);
int fm_get_attn_transpose_read(void);

/* Single-query attention of one cached decoder layer (csrc/attn_decode.hip): the whole attention step of incremental decoding in
 * one launch, for every trunk variant - NormAttention / NormCrossAttention (fm_utils.py:222-261) included.
 * One query row per sample, head_dim 64, head h in columns [64h, 64h + 64).  q: (B) rows of stride ldq; k, v: views of row strides
 * ldk / ldv whose sample b starts at row b * kv_batch_rows (0 = Nk, the fm_attn_args convention) - e.g. the k and v column blocks
 * of a (B, T, 3 D) q | k | v cache; the first Nk rows of a sample are attended to, nothing else of k / v is read.  is_f32 selects
 * fp32 instead of bf16 elements for q, k, v and o alike.
 * Head norm (q_w != NULL; q_w, q_b, k_w, k_b: f32 (64), the biases may be NULL): LayerNorm over the 64 features of a head with eps.
 *   q is normalised on chip and never written back.  k_new_row >= 0: the key in row k_new_row of every sample is normalised (k_w
 *   required), WRITTEN BACK in place in the storage type and used as that stored (rounded) value - the cache then holds normalised
 *   keys and later tokens read them as they are.  k_new_row < 0: every key is taken as already normalised (cross-attention over
 *   context keys normalised once).  The statistics and the affine map are evaluated in double and rounded once, so the stored key is
 *   the correctly rounded LayerNorm also where x - mean cancels.  Without q_w no byte of k is written, whatever k_new_row says.
 * Scores scale * q.k_j in fp32 (64 fused multiply-adds in feature order); kpad (optional): (B, Nk) uint8, 1 = blocked: the score is
 *   REPLACED by -finfo(bf16).max (-finfo(float32).max with is_f32) as in fm_attn_fwd / fm_attn_f32_fwd, so a fully blocked sample
 *   attends uniformly.  Softmax in fp32, or softmax1 with zero_attn (fm_attn_args.zero_attn).  o = sum_j p_j v_j in fp32, rounded once.
 * One workgroup per (sample, head); workgroups share nothing; the result is bit-reproducible.
 * Refused (-1): null q / k / v / o; B, H < 1; Nk < 1 or > FM_ATTN_DECODE_MAX_NK; kv_batch_rows < Nk with B > 1; k_new_row >= Nk; a norm
 * on k_new_row without k_w; a row stride below 64 H; k / v not 16-byte aligned or ldk / ldv not a multiple of 16 bytes; q / o / the
 * norm vectors not aligned to their element. */
#define FM_ATTN_DECODE_MAX_NK 8192
typedef struct fm_attn_decode_args {
    const void* q; void* k; const void* v; void* o;
    const void* q_w; const void* q_b; const void* k_w; const void* k_b;
    const void* kpad;
    int32_t ldq, ldk, ldv, ldo;
    int32_t B, H, Nk, kv_batch_rows, k_new_row, is_f32, zero_attn, pad_;
    float scale, eps;
} fm_attn_decode_args;
int fm_attn_decode(const fm_attn_decode_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Token selection + embedding  (encoder: fm.py:245-277,338-390 + encoder_embeddings.py forward()s;
 * decoder: fm.py:279-336,392-438 + decoder_embeddings.py forward_embed()s)
 * ---------------------------------------------------------------------------------------------- */
#define FM_MAX_MODS 24
enum fm_mod_kind {
    FM_KIND_TOK = 0,      /* grid of discrete tokens      (ImageToken{En,De}coderEmbedding)   */
    FM_KIND_PATCH = 1,    /* raw pixels, patch projection (ImageEncoderEmbedding)             */
    FM_KIND_SEQ = 2,      /* token sequence               (Sequence{En,De}coderEmbedding)     */
    FM_KIND_SEQ_EMB = 3   /* dense-embedding sequence     (SequenceEmbEncoderEmbedding)       */
};
typedef struct fm_mod_desc {
    const void* ids;       /* TOK/SEQ: int64 or int32 ids; PATCH: f32 pixels (C,H,W); SEQ_EMB: f32 (n_pos, orig_dim) */
    const void* mask;      /* uint8 (B, mask_stride): input_mask (encoder) / target_mask (decoder), 1 = masked        */
    const void* dam;       /* int32 (B, mask_stride): decoder_attention_mask (decoder only)                           */
    const void* table;     /* f32 (vocab, D) token_emb.weight                                                         */
    const void* pos;       /* f32 (pos_rows, D) pos_emb                                                               */
    const void* mod_emb;   /* f32 (D)                                                                                 */
    const void* proj_bias; /* SEQ_EMB: f32 (D) emb_proj.bias                                                          */
    int32_t L;             /* positions contributed to the concatenation (decoder sequences: tensor_len - 1)         */
    int32_t kind, ids_are_i64, mod_id;
    int32_t max_len;       /* decoder sequences: position ids >= max_len collapse to 0 (decoder_embeddings.py:128)   */
    int32_t shifted;       /* decoder sequences: input j, target j+1, mask[j] | mask[j+1]   (fm.py:309-319)           */
    int32_t mask_stride, id_stride;   /* elements per sample in mask/dam resp. ids                                    */
    int32_t patch, channels, grid_w, orig_dim;
    int32_t head_index;    /* decoder: index of this modality's head (stable, independent of the shuffled order)    */
    int32_t pad_;
} fm_mod_desc;

typedef struct fm_select_desc {
    fm_mod_desc mods[FM_MAX_MODS];   /* in concatenation order */
    int32_t n_mods, batch, dim, n_keep, n_reg, total_len, is_decoder;
    int32_t raw;             /* 0: select n_keep positions (stable partition), masked slots zeroed — forward_mask_encoder/decoder;
                                1: every position in place, nothing zeroed — cat_encoder_tensors / cat_decoder_tensors (fm.py:245-336);
                                2: as 1 for ONE modality's own forward() / forward_embed() (decoder grid tokens embed their ids) */
    const void* reg_tokens;  /* f32 (n_reg, D)                      */
    const void* mask_token;  /* f32 (D), decoder                    */
    /* outputs, Nt = n_reg + n_keep rows per sample */
    void* tokens;       /* f32 (B, Nt, D)  gathered token rows (zero where masked)                 */
    void* emb;          /* f32 (B, Nt, D)  pos_emb + mod_emb (zero where masked)                   */
    void* x0;           /* f32 (B, Nt, D)  optional: tokens + emb                                  */
    void* out_mask;     /* uint8 (B, Nt)   1 = masked slot                                         */
    void* out_mod;      /* int16 (B, Nt)   modality id, -1 where masked / register                 */
    void* slot_mod;     /* int32 (B, Nt)   index into mods[] (-1 masked, -2 register)              */
    void* slot_src;     /* int32 (B, Nt)   token id (TOK/SEQ) or position inside the modality      */
    void* slot_pos;     /* int32 (B, Nt)   pos_emb row used                                        */
    void* target_ids;   /* int64 (B, Nt)   decoder                                                 */
    void* out_cs;       /* int32 (B, Nt)   decoder: cumsum of the kept decoder_attention_mask      */
    void* out_mod_pre;  /* int16 (B, Nt)   decoder: modality id *before* pads are set to -1        */
    void* out_mod_index;/* int32 (B, Nt)   decoder: head index, -1 where masked                    */
    void* patch_rows;   /* bf16 (B*Nt, patch_ld)  optional: pixels of the kept PATCH slots, zero elsewhere  */
    void* seqemb_rows;  /* bf16 (B*Nt, seqemb_ld) optional: embeddings of the kept SEQ_EMB slots            */
    int32_t patch_ld, seqemb_ld;
    int32_t rows_f32;   /* 1: patch_rows / seqemb_rows are f32 (fp32 verification path)                     */
    int32_t pad2_;
} fm_select_desc;
/* Limits (refused with -1 otherwise): 1 <= n_mods <= FM_MAX_MODS; dim % 4 == 0; total_len = sum of the L, at most 8192 concatenated
 * positions per sample; n_keep <= total_len and at most 1024 kept slots (8192 in the raw views, which need n_keep == total_len and
 * n_reg == 0); patch_ld % 4 == seqemb_ld % 4 == 0.  Register rows carry zero patch_rows / seqemb_rows like every other non-dense slot. */
int fm_select_embed(const fm_select_desc* desc, void* stream);

typedef struct fm_embed_bwd_mod {
    void* d_table;      /* f32 (vocab, D) or NULL */
    void* d_pos;        /* f32 (pos_rows, D) for learned position embeddings, NULL for fixed sin-cos */
    void* d_mod_emb;    /* f32 (D) */
    void* d_proj_bias;  /* SEQ_EMB: f32 (D) */
    int32_t kind, has_padding_idx, padding_idx, pad_;
} fm_embed_bwd_mod;
typedef struct fm_embed_bwd_desc {
    fm_embed_bwd_mod mods[FM_MAX_MODS];
    const void* dx;          /* f32 (B, Nt, lddx): gradient w.r.t. tokens + emb */
    const void* slot_mod; const void* slot_src; const void* slot_pos;
    void* d_mask_token;      /* decoder */
    void* d_reg_tokens;      /* encoder, (n_reg, D) */
    int32_t n_mods, batch, dim, Nt, lddx, is_decoder;
} fm_embed_bwd_desc;
/* Accumulates (fp32 atomics) into every non-NULL gradient buffer; NULL ones are skipped.  Limits (refused with -1 otherwise):
 * 1 <= n_mods <= FM_MAX_MODS; dim % 4 == 0 and dim <= 2048; lddx % 4 == 0; the per-modality column sums live in LDS, so
 * (n_mods + 1) * dim * 4 bytes must not exceed 150 KB (24 modalities at dim 2048 do). */
int fm_embed_bwd(const fm_embed_bwd_desc* desc, void* stream);

/* dense (B, M, M) uint8 mask from the compressed form (FourM.adapt_decoder_attention_mask, fm.py:440-475) */
int fm_dense_decoder_mask(const int32_t* cs, const int16_t* mod, void* out, int B, int M, int causal, int use_cs,
                          int use_sep, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Heads: segment rows by modality, cross-entropy  (fm.py:573-637)
 * ---------------------------------------------------------------------------------------------- */
enum fm_loss_type { FM_LOSS_MOD = 0, FM_LOSS_TOKEN = 1 };
#define FM_SEG_ROWS 256   /* row alignment of the per-modality segments = the row tile of the grouped GEMMs */
/* Buckets rows 0..R-1 by head_of_row (-1 = no head) into FM_SEG_ROWS-aligned segments of a padded row
 * space of Rp rows (Rp % FM_SEG_ROWS == 0, Rp >= roundup(R) + FM_SEG_ROWS*(n_heads-1)).  perm[pr] = source row or
 * -1; row_to_padded[r] = padded row or -1; tile_group[pr/FM_SEG_ROWS] = head or -1. */
int fm_segment_rows(const int32_t* head_of_row, int R, int n_heads, int32_t* seg_start, int32_t* seg_count,
                    int32_t* perm, int32_t* row_to_padded, int32_t* tile_group, int Rp, void* stream);
int fm_gather_rows(const void* src, int ld_src, const int32_t* perm, void* dst, int ld_dst, int Rp, int D, void* stream);
/* logits: bf16 (Rp, ldl) produced by the grouped fm_gemm_nt (16-byte aligned, ldl % 8 == 0).
 * write_grad == 0 (forward): one streaming pass; writes row_loss (Rp), row_lse (Rp), head_loss (n_heads) and
 *   total_loss (1), all f32.
 * write_grad == 1 (backward): the logits are replaced in place by d(total)/d(logits) * grad_scale[0] (bf16; pad
 *   rows and the columns up to roundup64(vocab) zeroed) using the row_lse of the forward call. */
int fm_cross_entropy(void* logits, int ldl, const int32_t* perm, const int32_t* tile_group, const int64_t* target_ids,
                     const int32_t* vocab, const int32_t* seg_start, const int32_t* seg_count, const void* grad_scale,
                     int loss_type, int n_heads, int Rp, int max_vocab, void* row_loss, void* row_lse, void* head_loss,
                     void* total_loss, int write_grad, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Element-wise / reductions
 * ---------------------------------------------------------------------------------------------- */
/* fm_swiglu_bwd: Hp and the leading dims multiples of 8, buffers 16-byte aligned (16-byte accesses). */
int fm_swiglu_bwd(const void* da, int ldda, const void* gu, int ldgu, void* dgu, int lddgu, int R, int H, int Hp, void* stream);
int fm_gelu_bwd(const void* dh, int lddh, const void* pre, int ldp, void* dpre, int lddp, int R, int H, int Hp, void* stream);
/* One launch refreshing many bf16 weight shadows from their fp32 masters (what autocast's per-call weight
 * casts amount to, fm_utils.py Linear layers under torch.autocast).  Job i covers the 64x64 tiles
 * [tile_start_i, tile_start_{i+1}) of its (rows, cols) source, tiles_i = ceil(rows/64)*ceil(cols/64);
 * transpose == 0: dst[r][c] = bf16(src[r][c]);  transpose == 1: dst[c][r] = bf16(src[r][c]).
 * col_scale (optional, fp32[cols]): the source is multiplied by col_scale[c] first - a LayerNorm weight folded into the Linear
 * that consumes the normalised rows (DecoderBlock.context_norm -> cross_attn.kv, fm_utils.py:364: every decoder block normalises
 * the SAME context, so x_hat is computed once and gamma_l lives in the weight image).  dst_f32 != 0: fp32 destination (the
 * fp32 verification mode keeps the same launch sequence).
 * Destination padding is not written.  descs: DEVICE pointer, sorted by tile_start (first = 0). */
typedef struct fm_shadow_desc {
    const void* src; void* dst;
    int32_t ld_src, ld_dst, rows, cols, transpose, tile_start;
    const void* col_scale;
    int32_t dst_f32, reserved;
} fm_shadow_desc;
int fm_shadow_refresh(const fm_shadow_desc* descs, int n_descs, int total_tiles, void* stream);
/* Gradient of a folded LayerNorm weight (see col_scale above).  With W' = W diag(gamma) used in the forward and
 * dWp = dL/dW' (rows x cols, fp32, leading dimension ld_dwp) produced by the ordinary weight-gradient GEMM:
 *     gW[r][c]  += dWp[r][c] * gamma[c]                (dL/dW,     accumulated like every gradient)
 *     ggamma[c] += sum_r dWp[r][c] * W[r][c]           (dL/dgamma, fp32 atomics)
 * W, gW: contiguous (rows x cols) fp32.  Job table passed by value (graph-capturable, no upload). */
#define FM_FOLD_MAX_JOBS 48
typedef struct fm_fold_grad_job {
    const void* dWp; const void* W; const void* gamma; void* gW; void* ggamma;
    int32_t rows, cols, ld_dwp, reserved;
} fm_fold_grad_job;
int fm_fold_colscale_grad(const fm_fold_grad_job* jobs, int n_jobs, void* stream);

/* bf16 weight shadows: dst[r][c] = src[r][c], columns [cols, ld_dst) zero /
 * dst[c][r] = src[r][c], columns [rows, dst_cols) zero (dst_cols <= ld_dst) */
int fm_cast_pad(const void* src, int ld_src, void* dst, int ld_dst, int rows, int cols, void* stream);
int fm_transpose_cast_pad(const void* src, int ld_src, void* dst, int ld_dst, int dst_cols, int rows, int cols, void* stream);
int fm_colsum(const void* dy, int ldy, void* db, int R, int N, void* stream);            /* db[n] += sum_r dy[r][n] */
int fm_f32_to_bf16(const void* src, void* dst, int64_t n, void* stream);
/* dst(f32)[i] = scale * src(bf16)[i]: unpacks a gradient bucket that travelled in bf16 (optional wire format of the exchange) */
int fm_bf16_to_f32_scaled(const void* src, void* dst, int64_t n, float scale, void* stream);
/* out = x + delta over n contiguous elements (x, out f32; delta bf16): the residual add of fm_utils.py:332-333 on its own */
int fm_add_bf16_f32(const void* x, const void* delta, void* out, int64_t n, void* stream);
/* Stochastic depth (DropPath, fourm/models/fm_utils.py:64-87): x[r][:] *= scale[r / rows_per_sample] in place on a bf16 (R, N) tile of
 * row stride ld (scale f32 per sample = mask / keep_prob).  The forward scales a residual branch's output, the backward the bf16
 * gradient copy that enters the branch.  N, ld multiples of 8. */
int fm_scale_rows_bf16(void* x, int ld, const void* scale, int rows_per_sample, int R, int N, void* stream);

/* Dense front end of FourMViT (fourm/models/fm_vit.py), csrc/vit_embed.hip.
 * fm_vit_patch_rows: pixels f32 (B, C, H, W) -> rows (B * (H/P) * (W/P), ld): EVERY patch of every image, patches in row-major grid
 *   order, feature f = (py * P + px) * C + c (upstream's 'b d (nh ph) (nw pw) -> b (nh nw) (ph pw d)').  Rows are bf16 (round to nearest
 *   even), or f32 copies with rows_f32 (verification mode).  Columns [P*P*C, ld) are written as zero (the K padding of the projection
 *   GEMM); rows past B * (H/P) * (W/P) are not touched.  A workgroup owns a strip of horizontally adjacent patches: whole image-row
 *   segments are read contiguously, transposed through LDS and stored 16 bytes per lane.
 *   Refused (-1): H or W not a multiple of P, ld not a multiple of 8 or smaller than P*P*C, P*P*C > 8192, null pointers, pixels or rows
 *   not 16-byte aligned.
 * fm_vit_emb_rows: x[(b * Np + n)][:] = pos[n][:] + mod_emb[:] (all f32; x of row stride ldx): the embedding rows the projection GEMM
 *   adds onto in place (FM_EPI_RESIDUAL with res == out).  D and ldx multiples of 4, pointers 16-byte aligned.
 * fm_vit_colsum: db[n] += sum_r dy[r][n] for f32 dy (R, N) of row stride ldy and f32 db: every column summed in double in a fixed order and
 *   rounded once (deterministic; the bias gradient of encoder_norm from the head's fp32 gradient).  ws: scratch of at least
 *   min(64, ceil(R / 32)) * N * 8 bytes, 8-byte aligned. */
int fm_vit_patch_rows(const void* pixels, void* rows, int ld, int B, int C, int H, int W, int P, int rows_f32, void* stream);
int fm_vit_emb_rows(const void* pos, const void* mod_emb, void* x, int ldx, int B, int Np, int D, void* stream);
int fm_vit_colsum(const void* dy, int ldy, void* db, int R, int N, void* ws, int64_t ws_bytes, void* stream);

/* Front end of CLIP's VisionTransformer (fourm/utils/clip/model.py:229-237: cat(class_embedding, conv1 patches) + positional_embedding,
 * then ln_pre), csrc/clip.hip.  patches: the (B * G, D) output rows of the bias-free conv1-as-GEMM, row stride ldp, bf16 or (patches_f32)
 * f32; cls (D), pos ((G + 1, D), contiguous), w / b (ln_pre, D): f32.  out: the f32 residual stream (B * (G + 1), D), row stride ldo:
 *   out[b (G + 1)]         = LN(cls + pos[0])
 *   out[b (G + 1) + 1 + g] = LN(patches[b G + g] + pos[1 + g])
 * One pass, one wavefront per row, the row in registers, fp32 statistics (eps inside the sqrt), 16-byte accesses (8 bytes for bf16 rows).
 * Rows of patches past B * G are not read, rows of out past B * (G + 1) and columns past D are not written.
 * Refused (-1): null pointers (b may be NULL: no bias), B, G or D not positive, D not a multiple of 4 or > 2048, ldp / ldo smaller than D
 * or not multiples of 4, pointers not 16-byte aligned, more than 2^31 - 1 output rows. */
int fm_clip_embed_ln(const void* patches, int ldp, int patches_f32, const void* cls, const void* pos, const void* w, const void* b,
                     void* out, int ldo, int B, int G, int D, float eps, void* stream);

/* Backward of a FROZEN CLIP tower, for the perceptual loss of tokenizer training (upstream fourm/vq/percept_losses/timm_perceptual_loss.py:89-109:
 * features of the reconstruction and of the image after some blocks, compared token by token).  csrc/clip.hip, csrc/elementwise.hip.
 *
 * fm_feat_distance: pred / tgt f32 (B * T, ld) feature rows of one tap.  Per sample b the value of this tap,
 *       FM_FEAT_COSINE: (1 - mean_t cos(p_t, t_t)) / B,  cos = <p, t> / (max(|p|, 1e-8) max(|t|, 1e-8))      (F.cosine_similarity)
 *       FM_FEAT_L1:     (mean_t sum_d |p^_d - t^_d|) / B,  x^ = x / max(|x|, 1e-12)                          (F.normalize + l1_loss)
 *   is ADDED to loss[b] (f32 (B,); the 1 / B is upstream's own division of the per-sample vector by the batch size), and its gradient
 *   with respect to pred is written to dpred f32 (B * T, lddp) (sign(0) = 0; below the clamp the norm is a constant, as in torch).
 *   One workgroup per sample: a wavefront reduces a token over D, keeps its tokens' sum in token order, the 16 partial sums are added
 *   in wave order - no atomics, the same bits on every run.  tgt receives no gradient.
 *   Refused (-1): null pointers, B, T or D not positive, D not a multiple of 4 or > 2048, a leading dimension below D or not a multiple
 *   of 4, pointers not 16-byte aligned, a mode other than the two.
 * fm_quick_gelu_bwd / fm_quick_gelu_bwd_f32: a = u sigmoid(1.702 u) -> dpre = da s (1 + 1.702 u (1 - s)), s = sigmoid(1.702 u), u the saved
 *   pre-activation.  Signatures and layout rules of fm_gelu_bwd (bf16: Hp and the leading dims multiples of 4, columns [H, Hp) written
 *   as zero) and fm_gelu_bwd_f32 (columns past H untouched).
 * fm_clip_embed_ln_bwd: the adjoint of fm_clip_embed_ln with respect to the patch rows.  dy f32 (B * (G + 1), lddy): gradient of the
 *   normalised stream rows.  Each pre-norm patch row is rebuilt from patches + pos, its statistics recomputed, and
 *   d_patches[b * G + g] = rstd (dy w - mean(dy w) - x_hat mean(dy w x_hat)) written as bf16 or f32 rows (as patches_f32 says, row
 *   stride lddp); the class rows are skipped.  Refusals as fm_clip_embed_ln.
 * fm_tap_add: g[r] += row_scale[r / rows_per_sample] * dtap[r] on f32 (R, D) tiles (row_scale f32 per sample, or NULL: 1; product and sum
 *   rounded separately), then g_bf[r] = bf16(g[r]) unless g_bf is NULL: a tap's gradient enters the stream gradient in front of the block
 *   below it.  D, ldg, ldt, ldgb multiples of 4, g / dtap 16-byte and g_bf 8-byte aligned. */
enum { FM_FEAT_COSINE = 0, FM_FEAT_L1 = 1 };
int fm_feat_distance(const void* pred, int ldp, const void* tgt, int ldt, int B, int T, int D, int mode, void* loss, void* dpred, int lddp,
                     void* stream);
int fm_quick_gelu_bwd(const void* da, int ldda, const void* pre, int ldp, void* dpre, int lddp, int R, int H, int Hp, void* stream);
int fm_quick_gelu_bwd_f32(const void* da, int ldda, const void* pre, int ldp, void* dpre, int lddp, int R, int H, void* stream);
int fm_clip_embed_ln_bwd(const void* dy, int lddy, const void* patches, int ldp, int patches_f32, const void* pos, const void* w,
                         void* d_patches, int lddp, int B, int G, int D, float eps, void* stream);
int fm_tap_add(void* g, int ldg, void* g_bf, int ldgb, const void* dtap, int ldt, const void* row_scale, int rows_per_sample, int R, int D,
               void* stream);

/* LPIPS perceptual loss (upstream fourm/vq/percept_losses/lpips.py:96-109, :112-177): a FROZEN VGG16 feature stack tapped after relu1_2,
 * relu2_2, relu3_3, relu4_3 and relu5_3, forward and the backward down to the pixels (never a dW).  csrc/lpips.hip.  Feature maps are rows
 * (B * H * W, C) ("NHWC"), bf16 or (is_f32 != 0) f32; the 12 convolutions behind the stem are fm_gemm_nt(conv_*) with FM_EPI_RELU, their
 * input gradients the same launch on the dgrad weight image with FM_EPI_RELU_BWD (fp32 mode: fm_unet_im2col_f32 + fm_gemm_f32).
 * Fixed summation orders and no atomics throughout: two runs give the same bits.
 *
 * fm_lpips_stem: ScalingLayer + conv1_1 (3 -> 64, 3 x 3, padding 1) + bias + ReLU.  img f32 (B, 3, H, W) contiguous; mul / add f32 (3): the
 *   ScalingLayer as ONE fp32 multiply-add, s = fma(x, mul[c], add[c]) (mul = 1 / scale, add = -shift / scale); w f32 (64, 27) = conv.weight
 *   (k = c 9 + ky 3 + kx), bias f32 (64).  The zero padding is applied to s: a tap outside the image contributes 0, not add[c].
 *   is_f32 == 0: s, w and bias are rounded to bf16, the 27 products are added in fp32 in k order, out(bf16) = max(bf16(acc + bias), 0);
 *   is_f32 != 0: nothing is rounded, out(f32) = max(acc + bias, 0).  out rows (B * H * W, ldo >= 64), ldo % 8 == 0, 16-byte aligned.
 * fm_lpips_stem_bwd: the adjoint.  d: the MASKED gradient of conv1_1's pre-activation, rows (B * H * W, ldd) bf16 or f32;
 *   dimg[b][c][y][x] = ((sum over ky, kx, then n = 0..63, of d[b][y + 1 - ky][x + 1 - kx][n] w[n][c][ky][kx]) * mul[c]) * row_scale[b]
 *   f32 (B, 3, H, W), every element written once; row_scale f32 (B) = the incoming d / d loss[b] (the whole backward is linear per sample,
 *   so it is applied once, here), or NULL: 1.  is_f32 == 0 rounds w to bf16 as the forward does.  ldd % 8 == 0, 16-byte aligned d.
 * fm_maxpool2x2_nhwc: y[b][oy][ox][c] = max of the 2 x 2 window of x (B, H, W, C) -> (B, H / 2, W / 2, C); H, W even, C % 8 == 0,
 *   ldx / ldy % 8 == 0 and >= C, 16-byte aligned rows.
 * fm_lpips_distance: pred / tgt rows (B * P, C) of one tap, w f32 (C) = the tap's 1 x 1 lin weights.  Per pixel p^ = p / (|p| + 1e-10), t^
 *   likewise (upstream's normalize_tensor); loss[b] += (sum over the pixels of sum_c w_c (p^_c - t^_c)^2) / P, all in fp32.  dpred (f32 rows
 *   (B * P, lddp), or NULL: the no-grad pass) receives d loss[b] / d p = g / (|p| + eps) - p <g, p> / ((|p| + eps)^2 |p|) with
 *   g_c = 2 w_c (p^_c - t^_c) / P.  Where |p| = 0 the second term, which divides by the norm, is taken as 0 (torch's autograd yields NaN
 *   there; the ReLU mask of the tap layer zeroes that pixel's gradient anyway, p = 0 meaning every channel is masked).
 *   One workgroup per (sample, chunk of FM_LPIPS_CHUNK pixels) writes its partial sum to scratch (f32, B * ceil(P / FM_LPIPS_CHUNK) values,
 *   caller-owned); a second launch adds a sample's partial sums in chunk order onto loss[b].  C % 4 == 0, C <= 512, ldp / ldt / lddp % 4 == 0
 *   and >= C, 16-byte aligned pointers.
 * fm_lpips_tap_bwd: the gradient of a layer's pre-activation from what arrives at its ReLU output, rows (B * H * W, C):
 *     d = [act > 0] (din + dtap + (this position is the FIRST maximum of its 2 x 2 window in scan order (0,0),(0,1),(1,0),(1,1) ? dpool : 0))
 *   act: the saved ReLU output; din (same type as d, may alias d: the in-place mask), dtap (f32 rows from fm_lpips_distance) and dpool
 *   (rows (B * H/2 * W/2, C) of d's type: the gradient of the max-pool's output; H, W even) are each optional (NULL).  The first-maximum rule
 *   is torch's max_pool2d backward; bf16 activations tie often.  Sum in fp32 in the order written, one rounding to d's type.  C % 4 == 0,
 *   leading dimensions % 4 == 0 and >= C, 16-byte (f32) / 8-byte (bf16) aligned pointers.
 * Refused (-1) without touching any output: null pointers where one is required, non-positive sizes, the alignment rules above. */
#define FM_LPIPS_CHUNK 64
int fm_lpips_stem(const void* img, const void* mul, const void* add, const void* w, const void* bias, void* out, int ldo, int is_f32, int B, int H,
                  int W, void* stream);
int fm_lpips_stem_bwd(const void* d, int ldd, int is_f32, const void* w, const void* mul, const void* row_scale, void* dimg, int B, int H, int W,
                      void* stream);
int fm_maxpool2x2_nhwc(const void* x, int ldx, void* y, int ldy, int is_f32, int B, int H, int W, int C, void* stream);
int fm_lpips_distance(const void* pred, int ldp, const void* tgt, int ldt, int is_f32, const void* w, int B, int P, int C, void* loss, void* dpred,
                      int lddp, void* scratch, void* stream);
int fm_lpips_tap_bwd(const void* act, int lda, const void* din, int ldi, const void* dtap, int ldt, const void* dpool, int ldp, void* d, int ldd,
                     int is_f32, int B, int H, int W, int C, void* stream);

/* Low-rank adapters (LoRAWrapper, fourm/models/lora_utils.py:44-81: y = linear(x) + scale * lora_up(lora_down(x))), csrc/lora.hip.
 * P = x down^T (fp32 accumulation over K), y += scale * P up^T in place (fp32 sum, rounded once to y's type), P written to p_out.
 * x: (R, K) row stride ldx; y: (R, N) row stride ldy; x_f32 / y_f32 select fp32 instead of bf16 elements (bf16 x with fp32 y is
 * built, fp32 x with bf16 y is not).  down, up: fp32, addressed through element strides: down(j, k) = down[j * down_sr + k * down_sk],
 * up(n, j) = up[n * up_sn + j * up_sr] - an nn.Linear pair passes (K, 1) and (r, 1).  The backward's dX += scale * (dY up) down is the
 * same call with the roles exchanged: x = dY, "down" = up read as (1, r), "up" = down read as (1, K), y = dX, and p_out receives
 * Q = dY up.  p_out: f32 (R, r) contiguous.  Rows >= R and columns >= K / N of x and y are neither read as values nor written.
 * Refused (-1): null pointers, r < 1 or r > 64, R, K, N < 1, ldx / ldy not a multiple of 4 or smaller than K / N, x / y not aligned
 * to 4 elements. */
int fm_lora_apply(const void* x, int ldx, const void* down, int64_t down_sr, int64_t down_sk, const void* up, int64_t up_sn, int64_t up_sr,
                  void* y, int ldy, float scale, void* p_out, int R, int K, int N, int r, int x_f32, int y_f32, void* stream);
/* out(c, j) (+)= scale * sum_{row < R} a[row][c] * b[row][j], out(c, j) = out[c * out_sn + j * out_sr] fp32: the adapters' gradients.
 * a: (R, n) bf16 (fp32 with a_f32) of row stride lda; b: f32 (R, r) contiguous.  d(lora_up) = scale dY^T P is (a, b) = (dY, P) with
 * strides (r, 1); d(lora_down) = scale Q^T x is (a, b) = (x, Q) with strides (1, K).  accumulate == 0 overwrites.  Rows >= R are
 * never read.  The row ranges of different workgroups meet in fp32 atomics: the sum order, and so the last bits, vary from run to run.
 * Refused (-1): null pointers, r < 1 or r > 64, R, n < 1, lda not a multiple of 4 or smaller than n, a not aligned to 4 elements. */
int fm_lora_grad(const void* a, int lda, const void* b, void* out, int64_t out_sn, int64_t out_sr, float scale, int accumulate,
                 int R, int n, int r, int a_f32, void* stream);

/* torch.optim.AdamW update on a contiguous fp32 range (fourm/utils/optim_factory.py:239-240);
 * grad_mult: optional device scalar multiplied into the gradient (clipping).
 * hyper: optional DEVICE float[4] = {lr, weight_decay, 1 - beta1^step, sqrt(1 - beta2^step)} that overrides the scalar arguments:
 * a launch captured in a hipGraph keeps following the schedule (the host refreshes those 16 bytes before each replay).
 * sumsq: optional device scalar that receives += sum g^2 of the RAW gradients of this range (round 5: with no clipping the gradient norm of
 * NativeScaler / get_grad_norm_ rides on the update's own pass over the gradients instead of a separate 4 B/param read). */
int fm_adamw(void* p, const void* g, void* m, void* v, int64_t n, float lr, float beta1, float beta2, float eps,
             float weight_decay, int64_t step, const void* grad_mult, const void* hyper, void* sumsq, void* stream);
/* AdamW on weight MATRICES with their plain bf16 shadow (the W operand of y = x W^T) rewritten in the same streaming pass: the
 * update already reads and writes every master weight, the bf16 copy costs 2 B/param on top instead of a separate 6 B/param pass.
 * One launch walks a device table of jobs in tiles of FM_ADAMW_CHUNK (8192) consecutive elements; job i owns tiles
 * [tile_start_i, tile_start_{i+1}); p, g, m, v: contiguous fp32 (rows, cols); dst_plain (optional): bf16 [r][c], row stride ld_plain.
 * dst_t / ld_t are reserved (transposed shadows are refreshed by fm_shadow_refresh).  All jobs of a launch share the
 * hyper-parameters and the step count.  Same arithmetic as fm_adamw. */
#define FM_ADAMW_CHUNK 8192
typedef struct fm_adamw_job {
    void* p; const void* g; void* m; void* v; void* dst_plain; void* dst_t;
    int32_t rows, cols, ld_plain, ld_t, tile_start, pad_;
} fm_adamw_job;
int fm_adamw_shadow(const fm_adamw_job* jobs, int n_jobs, int total_tiles, float lr, float beta1, float beta2, float eps,
                    float weight_decay, int64_t step, const void* grad_mult, const void* hyper, void* sumsq, void* stream);
int fm_sumsq(const void* x, int64_t n, void* out, void* stream);                         /* out[0] += sum x^2 */
int fm_clip_coef(const void* sumsq, float max_norm, void* norm_out, void* coef_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Generation step: token sampling + MaskGIT commit (csrc/sample.hip) — GenerationSampler.top_k_top_p_filtering / sample_tokens /
 * select_tokens_batched and the scatter updates of maskgit_step_batched, fourm/models/generate.py:332-420,650-661.
 * One workgroup per logits row: temperature (0 = argmax), top_k (0 = off; entries strictly below the k-th largest logit are
 * dropped), top_p (0 or 1 = off; an entry survives iff the temperature-1 probability mass of strictly larger logits is <= top_p),
 * then one multinomial draw by inverse CDF in index order from uniforms[row] in [0, 1).  Deterministic: fixed-polynomial exp with
 * separately rounded fp32 operations, integer radix selects, a fixed summation tree (oracle/sample_oracle.py is bit-identical).
 * out_ids: int64 (R); out_prob: f32 (R) = probability of the drawn token after filtering at the sampling temperature. */
int fm_sample_tokens(const void* logits, int ld, int logits_are_f32, int R, int V, float temperature, int top_k, float top_p,
                     const void* uniforms, void* out_ids, void* out_prob, void* stream);
/* Per sample b: the num_select entries of prob (B, N) with the largest value (ties: lower index first), in that order, go to
 * top_idx (B, num_select) and are committed: tensor[b][mod_pos[b][i]] = samples[b][i] (int64 or int32 tensor of row length L),
 * input_mask[b][pos] = 0, target_mask[b][pos] = 1 (bool / uint8). */
/* Classifier-free guidance on logits (generate.py:684, :718): out = base + weight * (cond - uncond) in fp32, one rounding per operation;
 * base = uncond (accumulate == 0) or the current out (accumulate != 0: further weighted conditions).  uncond / cond: bf16 or f32 (R, V)
 * with row strides ldu / ldc; out: f32 (R, ldo). */
int fm_guidance_combine(const void* uncond, int ldu, int uncond_is_f32, const void* cond, int ldc, int cond_is_f32, float weight,
                        void* out, int ldo, int R, int V, int accumulate, void* stream);
int fm_maskgit_commit(const void* prob, const void* samples, const int32_t* mod_pos, int B, int N, int num_select, void* tensor,
                      int tensor_is_i64, int L, void* input_mask, void* target_mask, int32_t* top_idx, void* stream);

/* ------------------------------------------------------------------------------------------------
 * fp32 VERIFICATION path (csrc/fp32_verify.hip): the floating-point kernels above once more with fp32 activations and weights
 * and no bf16 rounding, so that the launch sequence of the engine can be checked against the upstream fp32 model at fp32
 * tolerances.  Plain kernels, not the hot path.  Same conventions; every activation pointer is f32.
 * ---------------------------------------------------------------------------------------------- */
/* out[m][n] (+)= sum_k X[m*sxm + k*sxk] * W[n*swn + k*swk]  + epilogue (fm_epilogue without the *_BWD forms; no rounding).
 * Fully strided operands: NT (sxk = swk = 1), dX = dY W (swn = 1, swk = ldw) and dW = dY^T X (sxm = swn = 1, accumulate = 1)
 * are one kernel.  Grouped NT: groups + tile_group + seg_rows as in fm_gemm_nt (groups[g].W f32).  Grouped TN: groups[g].out /
 * .N with seg_start / seg_count (device), max_N = largest group N, n_groups; reduces rows [seg_start[g], + seg_count[g]).
 * accumulate = 1 (out += result) only with FM_EPI_F32 / FM_EPI_BF16; GELU / TANH / RESIDUAL / SWIGLU with accumulate are refused
 * (-1, fm_last_error).  Kernel choice: NT operands (sxk = swk = 1, no groups, not SWIGLU) with sxm % 4 == swn % 4 == 0 and 16-byte aligned X / W
 * run on the fp32 matrix cores, everything else on an LDS-tiled FMA kernel; both give the same results within fp32 rounding. */
typedef struct fm_gemm_f32_args {
    const void* X; const void* W; const void* W2; void* out; void* out2; const void* res; const void* bias; const void* bias2;
    int64_t sxm, sxk, swn, swk;
    int32_t M, N, K, ldo, ldo2, ldr, Hp, epilogue, accumulate, max_N, seg_rows, n_groups;
    const fm_gemm_group* groups; const int32_t* tile_group; const int32_t* seg_start; const int32_t* seg_count;
} fm_gemm_f32_args;
int fm_gemm_f32(const fm_gemm_f32_args* args, void* stream);
/* fm_attn_args with f32 Q / K / V / O (/ dO, dQ, dK, dV); blocked scores are replaced by -finfo(float32).max; stat_m / stat_l
 * unused by the forward.  The backward ACCUMULATES into dK and dV (the caller zeroes them).  Backward without stat_m / stat_l: every query's
 * contribution to dK / dV arrives by an fp32 atomic (the sum's order, and with it the last bits, vary from run to run).  With both given
 * ((B, H, Nq) f32 each, used as SCRATCH: row max and 1 / row sum) and O holding the forward's output: dQ as before, then dK / dV by a second
 * launch in which one wavefront per key row adds the queries in order - no atomics, the same bits on every run. */
int fm_attn_f32_fwd(const fm_attn_args* args, void* stream);
int fm_attn_f32_bwd(const fm_attn_args* args, void* stream);
/* fm_layernorm_bwd_f32 (dw, db) and fm_colsum_f32 (db) ACCUMULATE column sums over the rows in a fixed order (64 columns per workgroup, 16 row
 * groups added in group order; no atomics): two runs give the same bits. */
int fm_layernorm_bwd_f32(const void* dy, int lddy, const int32_t* dy_row_map, const void* x, int ldx, const void* w, const void* mean,
                         const void* rstd, const void* dres, void* dx, int lddx, void* dx2, int lddx2, void* dw, void* db, int R, int D,
                         void* stream);
int fm_headnorm_f32_fwd(const void* x, int ldx, const void* w, const void* b, void* y, int ldy, void* stats, int R, int H, float eps, void* stream);
int fm_headnorm_f32_bwd(const void* dy, int lddy, const void* x, int ldx, const void* w, const void* stats, void* dx, int lddx, void* dw, void* db,
                        int R, int H, void* stream);
int fm_swiglu_bwd_f32(const void* da, int ldda, const void* gu, int ldgu, void* dgu, int lddgu, int R, int H, int Hp, void* stream);
int fm_gelu_bwd_f32(const void* dh, int lddh, const void* pre, int ldp, void* dpre, int lddp, int R, int H, void* stream);
int fm_colsum_f32(const void* dy, int ldy, void* db, int R, int N, void* stream);
int fm_cross_entropy_f32(void* logits, int ldl, const int32_t* perm, const int32_t* tile_group, const int64_t* target_ids,
                         const int32_t* vocab, const int32_t* seg_start, const int32_t* seg_count, const void* grad_scale, int loss_type,
                         int n_heads, int padded_rows, int max_vocab, void* row_loss, void* row_lse, void* head_loss, void* total_loss,
                         int write_grad, void* stream);

/* ------------------------------------------------------------------------------------------------
 * fp32 compute mode of the diffusion detokenizer (csrc/unet_f32.hip): the non-GEMM kernels of csrc/unet.hip (declared further down) once
 * more with f32 feature maps and no bf16 rounding - compute_precision = "fp32" on PatchedUNetCondCat / DiVAE.  Same semantics, index rules
 * and conventions as their bf16 counterparts; every activation pointer is f32, every convolution and Linear of this mode is fm_gemm_f32 (a
 * 3 x 3 convolution behind the im2col below).  Plain kernels, not the hot path; fixed summation orders (bit-reproducible).
 * ---------------------------------------------------------------------------------------------- */
/* The bf16 im2col with f32 rows: same arguments and index rules (two sources, ksize 1 | 3, stride 1 | 2, up1, the fp32 nearest rule
 * min(floor(fp32(i) * fp32(n_in) / fp32(n_out)), n_in - 1) for src2).  C1, C2, ld1, ld2, ldo and kpad are multiples of 4 (no 64-column
 * padding in this mode); columns [ksize^2 (C1 + C2), kpad) are zeroed, nothing is written at or beyond column kpad. */
int fm_unet_im2col_f32(const void* src1, int ld1, int C1, const void* src2, int ld2, int C2, int H2, int W2, void* out, int ldo, int kpad,
                       int B, int H, int W, int ksize, int stride, int up1, void* stream);
/* y = [silu] GroupNorm_groups(x + add[b][c]) * w + b over f32 rows (B, HW, C), f32 result: two-pass statistics per (sample, group) - the
 * mean, then the squared deviations about it - in a fixed order.  add f32 (B, >= C) with row stride ld_add, or NULL.  Any C that is a
 * multiple of groups, C <= 1024; needs no scratch. */
int fm_groupnorm_nhwc_f32(const void* x, int ldx, const void* add, int ld_add, const void* w, const void* b, void* y, int ldy, int B, int HW, int C,
                          int groups, float eps, int silu, void* stream);
/* QKVAttentionLegacy on f32 qkv rows (B * T, ld): per head [q | k | v] of ch channels, q and k each scaled by ch^-1/4, fp32 softmax;
 * out f32 (B * T, ldo).  ch % 4 == 0, ld % 4 == 0, (ch + T) * 4 bytes <= 60 KB of LDS. */
int fm_unet_attention_f32(const void* qkv, int ld, void* out, int ldo, int B, int T, int heads, int ch, void* stream);
int fm_add_f32(const void* a, int lda, const void* b, int ldb, void* out, int ldo, int64_t rows, int C, void* stream);   /* out = a + b, f32 rows with row strides */
int fm_silu_f32(const void* x, void* y, int64_t n, void* stream);                                                        /* y = x * sigmoid(x), f32 to f32 */
/* out[b] = [cos(t_b f_i) | sin(t_b f_i)], f_i = exp(-ln(max_period) i / (dim / 2)); t f32 (B), out f32 (B, ldo)   (nn.py:120-140) */
int fm_timestep_embedding_f32(const void* t, void* out, int ldo, int B, int dim, float max_period, void* stream);
/* Backward of this mode (csrc/unet_f32_bwd.hip): what training the UNet on a frozen encoder needs besides fm_gemm_f32 (dX = dY W and dW = dY^T X
 * through its strides).  Fixed summation orders, no atomics, every output element written once: two runs agree bit for bit.
 * fm_unet_col2im_f32: the adjoint of fm_unet_im2col_f32 with respect to src1 for ksize 3 (C2 = 0), stride 1 | 2, up1 0 | 1, (H, W) the forward's
 *   logical grid: dsrc[(b, sy, sx)][c] (+)= sum of the col entries the forward filled from that pixel, taps in a fixed order (<= 9, <= 36 with up1).
 *   col f32 (B * Ho * Wo, ldc >= 9 C); dsrc f32 (B * (H >> up1) * (W >> up1), ld >= C); accumulate = 1 adds to dsrc; nothing is written outside
 *   columns [0, C).  C, ld, ldc multiples of 4, 16-byte aligned pointers. */
int fm_unet_col2im_f32(const void* col, int ldc, void* dsrc, int ld, int C, int B, int H, int W, int ksize, int stride, int up1, int accumulate, void* stream);
/* Backward of fm_groupnorm_nhwc_f32: the two-pass statistics of x + add[b][c] are recomputed as the forward computes them, with silu the
 * pre-activation is rebuilt and silu' applied.  dx f32 (B * HW, lddx); dadd[b][c] = sum_HW dx (f32 (B, ld_dadd), or NULL); dw[c], db[c] (f32 (C),
 * either may be NULL) are OVERWRITTEN with the sums over (B, HW): per-sample partial sums in scratch (2 * B * C floats; NULL allowed when dw and
 * db are), combined over the samples in order.  Same shape contract as the forward. */
int fm_groupnorm_nhwc_bwd_f32(const void* dy, int lddy, const void* x, int ldx, const void* add, int ld_add, const void* w, const void* b, void* dx, int lddx,
                              void* dw, void* db, void* dadd, int ld_dadd, void* scratch, int B, int HW, int C, int groups, float eps, int silu, void* stream);
/* Backward of fm_unet_attention_f32: the probabilities are recomputed from qkv with the forward's arithmetic; dout f32 (B * T, lddo) is the
 * gradient of its output, dqkv f32 (B * T, lddqkv) receives [dq | dk | dv] per head, every element written exactly once (one workgroup per
 * query writes dq, one per key dk and dv).  scratch: 3 * B * heads * T floats (row max, row sum, sum_s P dP).  The forward's limits; lddo % 4 == 0
 * and a 16-byte aligned dout as well. */
int fm_unet_attention_bwd_f32(const void* qkv, int ld, const void* dout, int lddo, void* dqkv, int lddqkv, void* scratch, int B, int T, int heads, int ch,
                              void* stream);
int fm_silu_bwd_f32(const void* dy, const void* x, void* dx, int64_t n, void* stream);      /* dx = dy s (1 + x (1 - s)), s = sigmoid(x), n contiguous f32 */

/* ------------------------------------------------------------------------------------------------
 * VQ tokenizer front end (fourm/vq/vqvae.py:302-331)
 * ---------------------------------------------------------------------------------------------- */
/* out[(b*G + g)][c*P*P + py*P + px] (bf16, row stride ld_out, pad zero) <- img (B, C, H, W) f32: the operand
 * of the patch-projection GEMM that replaces Conv2d(k = s = P)  (vq/models/vit_models.py:402-405,482) */
int fm_vq_patchify(const void* img, void* out, int ld_out, int B, int C, int H, int W, int P, void* stream);
int fm_l2norm_rows(const void* x, int ldx, void* y, int ldy, int R, int D, void* stream);   /* F.normalize(p=2, dim=-1) */
/* Cosine-similarity nearest code (quantize_lucid.py:394-407): tokens[r] = argmax_c <zn[r], En[c]> with the
 * first maximum winning; quant (optional, f32 (B, D, tokens_per_image)) = embed[tokens].  z: f32 (R, ldz),
 * l2-normalised in-kernel when normalize_latents; codes_normalized / embed: f32 (K, D).  D == 32.
 * ws_val / ws_idx: (R, splits) f32 / int32 scratch. */
int fm_vq_assign(const void* z, int ldz, const void* codes_normalized, const void* embed, int K, int D, int R,
                 int tokens_per_image, int normalize_latents, void* ws_val, void* ws_idx, int splits, int64_t* tokens,
                 void* quant, void* stream);
/* The same search for any latent width (SAM-instance tokenizer: latent_dim 1024; replaces l2norm(z) @ l2norm(embed).T, argmax and
 * embed[ind] of CosineSimCodebook.forward, quantize_lucid.py:388-407, without the (R, K) score matrix).  z: f32 (R, ldz), always
 * l2-normalised in-kernel; codes_normalized / embed: f32 (K, D) contiguous; z and codes_normalized 16-byte aligned.  Exact fp32
 * scores (v_mfma_f32_32x32x2_f32: one fmaf chain over d), lowest index on equal scores.  D % 4 == 0, 8 <= D <= 4096, ldz % 4 == 0.
 * ws_val / ws_idx: (R, code_tiles) f32 / int32 scratch, code_tiles = ceil(K / FM_VQ_WIDE_TILE).  tokens, quant: as fm_vq_assign. */
#define FM_VQ_WIDE_TILE 128
int fm_vq_assign_wide(const void* z, int ldz, const void* codes_normalized, const void* embed, int K, int D, int R,
                      int tokens_per_image, void* ws_val, void* ws_idx, int code_tiles, int64_t* tokens, void* quant, void* stream);
/* Memcodes code search (multi-head inner-product codebook of the pose / global-feature tokenizers; replaces the eval branch of
 * Memcodes.forward, quantize_memcodes.py:84-109: logits = einsum(q, k), argmax, one_hot, einsum(attn, v), without the (R, K) score matrix).
 * z: f32 (R, ldz), head h reads columns [h d, (h + 1) d); keys, values: f32 (H, K, d) contiguous (to_k / to_v applied to the codes); row
 * r = b tokens_per_image + g.  tokens[(b H + h) tokens_per_image + g] = lowest index of the largest fp32 score <z_h, keys[h][j]> (exact fp32,
 * one fmaf chain over d per score; NO normalisation; upstream's d^-0.5 factor on the query is left out: a positive scale cannot change an
 * arg-max).  quant (optional): f32 (B, H d, tokens_per_image), quant[b][h d + c][g] = values[h][token][c].  d % 4 == 0, 8 <= d <= 4096,
 * H, K, R >= 1, ldz % 4 == 0, ldz >= H d, z and keys 16-byte aligned, at most 65535 heads and 65535 row tiles of FM_VQ_WIDE_TILE rows.
 * ws_val / ws_idx: (H, R, code_tiles) f32 / int32 scratch, code_tiles = ceil(K / FM_VQ_WIDE_TILE). */
int fm_memcodes_assign(const void* z, int ldz, const void* keys, const void* values, int K, int d, int H, int R,
                       int tokens_per_image, void* ws_val, void* ws_idx, int code_tiles, int64_t* tokens, void* quant, void* stream);
/* Codebook training statistics (CosineSimCodebook.forward, training branch, quantize_lucid.py:409-419): bins[k] = number of
 * latents assigned to code k, sums[k][:] = sum of those latents after L2 normalisation.  z: f32 (R, ldz); tokens: int64 (R);
 * bins f32 (K), sums f32 (K, D): zeroed here, accumulated with fp32 atomics.  With a synchronised codebook the caller all-reduces
 * bins and sums over the ranks between the two calls (:411, :419).  D <= 64. */
int fm_vq_code_stats(const void* z, int ldz, const int64_t* tokens, int R, int D, int K, void* bins, void* sums, void* stream);
/* EMA update (quantize_lucid.py:413, :421-425): cluster_size = cluster_size * decay + bins * (1 - decay);
 * embed = embed * decay + target * (1 - decay), target = l2norm(sums / bins) where bins > 0, l2norm(embed) elsewhere. */
int fm_vq_ema_update(const void* bins, const void* sums, void* embed, void* cluster_size, int K, int D, float decay, void* stream);
/* Euclidean codebook (EuclideanCodebook, quantize_lucid.py:181-301; VectorQuantize(use_cosine_sim=False), i.e. norm_codes=False):
 *   fm_vq_code_bias:   bias[k] = -|embed[k]|^2 / 2;
 *   fm_vq_assign_bias: fm_vq_assign with the score of code c starting at code_bias[c] (NULL: 0): with `codes` = embed (not normalised),
 *       normalize_latents = 0 and that bias the arg-max is the nearest code in Euclidean distance (:272-280);
 *   fm_vq_code_stats_raw: fm_vq_code_stats on the latents as they are (no L2 normalisation; :283-289);
 *   fm_vq_ema_update_euclid: cluster_size and embed_avg EMAs, then embed = embed_avg / Laplace-smoothed cluster size (:286-296).
 *       total_scratch: one DEVICE float (zeroed here). */
int fm_vq_code_bias(const void* embed, int K, int D, void* bias, void* stream);
int fm_vq_assign_bias(const void* z, int ldz, const void* codes, const void* code_bias, const void* embed, int K, int D, int R,
                      int tokens_per_image, int normalize_latents, void* ws_val, void* ws_idx, int splits, int64_t* tokens,
                      void* quant, void* stream);
int fm_vq_code_stats_raw(const void* z, int ldz, const int64_t* tokens, int R, int D, int K, void* bins, void* sums, void* stream);
int fm_vq_ema_update_euclid(const void* bins, const void* sums, void* embed, void* embed_avg, void* cluster_size, void* total_scratch,
                            int K, int D, float decay, float eps, void* stream);

/* Tokenizer training path (fourm/vq/vqvae.py:454-481 VQVAE, vq/models/vit_models.py:504-648 ViTDecoder,
 * vq/quantizers/quantize_lucid.py:533-541).
 *   fm_vq_unpatchify: rows f32 (B * G, ld_rows) with features ordered (c, py, px) -> img f32 (B, C, H, W)  (the rearrange behind
 *       ViTDecoder.out_proj, vit_models.py:640-643; the inverse of fm_vq_patchify)
 *   fm_vq_latent_grad: the quantizer's backward and commitment value.  z f32 (R, ldz) latents, tokens (R), embed f32 (K, D);
 *       dquant f32 (R, ld_dquant) or NULL: gradient w.r.t. the quantised rows (straight-through estimator);  grad_loss: DEVICE f32
 *       scalar d(objective)/d(code_loss) or NULL;  dz (optional) = dquant + grad_loss * w * 2 (z - embed[token]) / (R D);
 *       commit_value (optional, f32 scalar the caller zeroed) += w * mean((z - embed[token])^2).  D <= 64.
 *   fm_tanh_bwd_f32: dx = dy * (1 - t * t) on f32 (R, N) tiles of row stride ld (Mlp with act_layer = Tanh, vit_models.py:494-496)
 *   fm_embed_rows_f32: out[r] = table[idx[r]] (f32 rows; F.embedding) */
int fm_vq_unpatchify(const void* rows, int ld_rows, void* img, int B, int C, int H, int W, int P, void* stream);
/* One ConvNeXt block of ViTDecoder(out_conv=True) (vit_models.py:298-335; two of them follow the unpatchify, :655-657) in one launch:
 *   y = x + gamma * pwconv2(GELU(pwconv1(LayerNorm_C(dwconv7x7(x)))))
 * replaces Conv2d(C, C, 7, padding=3, groups=C) -> permute -> LayerNorm(C) -> Linear(C, 4C) -> GELU (erf) -> Linear(4C, C) -> gamma * . ->
 * permute -> residual add.  x, y: f32 (B, C, H, W), y != x;  dw_weight (C, 1, 7, 7), dw_bias (C), ln_weight / ln_bias (C),
 * pw1_weight (4C, C), pw1_bias (4C), pw2_weight (C, 4C), pw2_bias (C), gamma (C): f32.  1 <= C <= FM_CONVNEXT_MAX_C. */
#define FM_CONVNEXT_MAX_C 4
int fm_convnext_block(const void* x, void* y, const void* dw_weight, const void* dw_bias, const void* ln_weight, const void* ln_bias,
                      const void* pw1_weight, const void* pw1_bias, const void* pw2_weight, const void* pw2_bias, const void* gamma,
                      int B, int C, int H, int W, float eps, void* stream);
int fm_vq_latent_grad(const void* z, int ldz, const void* embed, const int64_t* tokens, const void* dquant, int ld_dquant, const void* grad_loss,
                      float commitment_weight, void* dz, int ld_dz, void* commit_value, int R, int D, void* stream);
int fm_tanh_bwd_f32(const void* dy, const void* t, void* dx, int R, int N, int ld, void* stream);
int fm_embed_rows_f32(const void* table, const int64_t* idx, void* out, int ld_out, int R, int D, void* stream);
/* fp32 products on the bf16 matrix cores: out (R, ldo >= 3 K) bf16 = [hi | hi | lo] of x f32 (R, K) (weight_order = 0: the activation
 * operand) or [hi | lo | hi] (weight_order = 1: the weight operand), hi = bf16(x), lo = bf16(x - hi); apply_tanh: x <- tanh(x) first.
 * ONE bf16 NT GEMM over the 3 K columns then accumulates hi hi + hi lo + lo hi in fp32: error within 3 * 2^-16 of sum |x| |w|, measured
 * <= 2.2e-6 of it (the tokenizer's fp32 tail at inference, vit_models.py:494-496). */
int fm_split3_bf16(const void* x, int ldx, void* out, int ldo, int R, int K, int weight_order, int apply_tanh, void* stream);
/* Input variants of the tokenizer (VQ.prepare_input, vq/vqvae.py:269-286) folded into the patch gather: fm_vq_patchify with
 *   labels != NULL: class maps int64 (B, H, W) embedded by cls_emb f32 (n_labels, C) (semantic segmentation, n_labels; img unused);
 *   scale / shift: DEVICE float[C] (or both NULL): value = scale[c] * v + shift[c] (undo_std: 2 * denormalize(x) - 1).
 * fm_vq_cls_emb_bwd: d cls_emb[label] += the bf16 gradient of the patch rows (B * G, ld), fp32 atomics (the embedding's backward).
 * fm_vq_latent_grad_normalized: fm_vq_latent_grad for norm_latents = True (quantize_lucid.py:525-527): x = l2norm(z) enters the
 *   commitment term, dz carries the backward of the normalisation. */
int fm_vq_patchify_ex(const void* img, const int64_t* labels, const void* cls_emb, const void* scale, const void* shift, void* out, int ld_out,
                      int B, int C, int H, int W, int P, void* stream);
int fm_vq_cls_emb_bwd(const void* d_patches, int ld, const int64_t* labels, void* d_cls_emb, int B, int C, int H, int W, int P, void* stream);
int fm_vq_latent_grad_normalized(const void* z, int ldz, const void* embed, const int64_t* tokens, const void* dquant, int ld_dquant, const void* grad_loss,
                                 float commitment_weight, void* dz, int ld_dz, void* commit_value, int R, int D, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Data side: input / target masks of an image-like modality (UnifiedMasking.image_mask, fourm/data/masking.py:237-266)
 * noise: f32 (B, L) uniform draws (the caller's RNG); input_budget / target_budget: int32 (B) (target_budget NULL = "None":
 * every non-input position is a target).  With ids = stable argsort(noise[b]):  input_mask[b][i] = ids[i] >= input_budget[b],
 * target_mask[b][i] = !(input_budget <= ids[i] < input_budget + target_budget)  (uint8, 1 = masked out), and
 * decoder_attention_mask (int32) = 0 except the number of targets at the first target position.  L <= 4096. */
int fm_image_mask(const void* noise, const int32_t* input_budget, const int32_t* target_budget, int B, int L, void* input_mask,
                  void* target_mask, int32_t* decoder_attention_mask, void* stream);

/* Compact host-to-device batch format: uint8 pixels, uint16 ids and bit-packed masks cross PCIe, the mod_dict tensors
 * the model takes are rebuilt on the device.
 *   fm_unpack_image_u8: (B, H, W, C) uint8 -> (B, C, H, W) f32 = ((x / 255) - mean[c]) / std[c]  (to_tensor + normalize,
 *       fourm/data/modality_transforms.py:215-218; mean / std are HOST arrays of C floats; bit-identical to the float pipeline)
 *   fm_unpack_ids_u16: n uint16 -> int64
 *   fm_unpack_mask_bits: row b = ceil(L / 8) bytes, bit (i & 7) of byte (i >> 3) -> uint8 / bool (B, L)
 *   fm_decoder_attention_from_target: image-like modalities' decoder_attention_mask (target count at the first target position,
 *       fourm/data/masking.py:262-264) from the unpacked target_mask (1 = masked out) */
int fm_unpack_image_u8(const void* src, void* dst, int B, int H, int W, int C, const float* mean, const float* stdv, void* stream);
int fm_unpack_ids_u16(const void* src, int64_t* dst, int64_t n, void* stream);
int fm_unpack_mask_bits(const void* bits, void* dst, int B, int L, void* stream);
int fm_decoder_attention_from_target(const void* target_mask, int32_t* decoder_attention_mask, int B, int L, void* stream);

/* Token budgets of a batch (UnifiedMasking.input_token_budget / target_token_budget, fourm/data/masking.py:181-234), one sample per
 * thread.  The caller draws:  main_draws f32 (B, T, M) - the Dirichlet sample of try t;  extra_draws f32 (B, T, E, M) - the
 * sample_n(diff) draws of try t (the first diff = n - sum(floor(p * n)) rows are used, E >= M covers every case).
 *   budget = floor(p * n) + bincount(argmax(extra[:diff])), clamped to max_tokens[m]; the first try with budget >= min_tokens everywhere is
 *   taken, else the last one (tries (B), optional: the number of tries consumed; T + 1 = none fitted).
 * Target budgets: pass input_budget int32 (B, M) and is_img uint8 (M): the clamp becomes max(min_tokens, max_tokens - input_budget) for
 * image-like modalities (:218-219).  Input budgets: input_budget = NULL.  M <= 64. */
int fm_token_budgets(const void* main_draws, const void* extra_draws, const int32_t* num_tokens, const int32_t* min_tokens,
                     const int32_t* max_tokens, const void* is_img, const int32_t* input_budget, int B, int T, int E, int M,
                     int32_t* budget, int32_t* tries, void* stream);

/* Span masking of sequence modalities (fourm/data/masking.py: sequence_mask :345-445 after tokenisation, sequence_token_mask :268-343,
 * sequence_emb_mask_span :448-516; simple_span_masking :58-91, chunk_span_masking :94-127), one wave per sample.
 *   ids (B, ld_ids) int32 with len (B): the token ids upstream has after tokenising and appending [EOS] (vocab_offset is added, :286);
 *   unit (B, ld_ids) or NULL: index of the chunk a token belongs to (chunk_span_masking: one mask decision per chunk, truncation by whole
 *     chunks; chunks must be non-empty);  NULL = one decision per token (truncation to max_tokens tokens);
 *   noise f32 (B, T, ld_noise): row t = the torch.rand vector of try t, indexed by token (or chunk);  keep_prob f64 (B): the first keep
 *     probability (sample_uniform / 1.0 / random.choice), multiplied by 0.9 per retry while the input is over its budget (:405-408); a unit
 *     is kept iff noise <= (float)keep_prob;  after T tries everything is masked (the limit keep_prob -> 0);
 *   input_budget (B);  target_budget (B) or NULL (= None; an entry < 0 = None for that sample);  r_choice (B) or NULL: the integer that
 *     replaces np.random.randint (taken modulo its argument, :425);  sentinel_ids[k] = sentinel_to_id[k].
 * Outputs, each (B, 2 * (max_tokens + 1)): tensor int32 (pad_id where empty), input_mask / target_mask uint8 (1 = masked out),
 * decoder_attention_mask int32;  tries (B) optional: draws consumed (T + 1 = they ran out: everything masked), -1 = more spans than sentinel ids (upstream raises KeyError).
 * Embedding mode (emb != NULL; sequence_emb_mask_span): emb f32 (B, emb_rows, emb_dim) with len (B); ids / unit / tensor / target_budget
 * unused; outputs are (B, max_tokens): input_mask, target_mask (all 1), decoder_attention_mask (all 0), src int32 (the source row of every
 * position, -1 = zero row) and emb_out f32 (B, max_tokens, emb_dim). */
typedef struct fm_span_mask_args {
    const int32_t* ids; const int32_t* len; const int32_t* unit; const void* noise; const double* keep_prob; const int32_t* r_choice;
    const int32_t* input_budget; const int32_t* target_budget; const int32_t* sentinel_ids;
    const void* emb; void* emb_out; int32_t* src;
    int32_t* tensor; void* input_mask; void* target_mask; int32_t* decoder_attention_mask; int32_t* tries;
    int32_t B, ld_ids, T, ld_noise, n_sentinels, max_tokens, vocab_offset, pad_id, emb_rows, emb_dim;
} fm_span_mask_args;
int fm_span_mask(const fm_span_mask_args* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Diffusion detokenizer (DiVAE decoder), inference (csrc/unet.hip).  Feature maps are rows (B * H * W, C) bf16 ("NHWC"): a 1 x 1
 * convolution is fm_gemm_nt on the rows; a 3 x 3 convolution is fm_unet_im2col + fm_gemm_nt with K = 9 C.
 * Replaces fourm/vq/models/unet/unet.py (ResBlock :163-274, AttentionBlock :277-322, QKVAttentionLegacy :345-374, Upsample /
 * Downsample :103-160, PatchedUNetCondCat :693-744), nn.py:23-25 / :120-140, and the element-wise half of
 * fourm/vq/scheduling/scheduling_{ddim,ddpm}.py (step, _threshold_sample).
 * ---------------------------------------------------------------------------------------------- */
/* out[(b, oy, ox)][tap * (C1 + C2) + c] (bf16, row stride ldo; columns [ksize^2 (C1 + C2), kpad) zero) <- the ksize x ksize neighbourhood
 * (padding ksize / 2, stride 1 | 2) of the channel concatenation [src1 | src2] on an (H, W) grid: src1 (B, H >> up1, W >> up1, C1) is read
 * at (y >> up1, x >> up1) (up1 = 1: the nearest x2 up-sampling of Upsample), src2 (B, H2, W2, C2) at (y H2 / H, x W2 / W) (nearest: the skip
 * tensor of an output block, or the conditioning under a finer grid); src2 = NULL, C2 = 0: one source.  ksize = 1: the plain concatenation.
 * The weight operand of the GEMM behind it is conv.weight.permute(0, 2, 3, 1).reshape(Cout, ksize^2 (C1 + C2)). */
int fm_unet_im2col(const void* src1, int ld1, int C1, const void* src2, int ld2, int C2, int H2, int W2, void* out, int ldo, int kpad,
                   int B, int H, int W, int ksize, int stride, int up1, void* stream);
/* y = [silu] GroupNorm_groups(x + add[b][c]) * w + b over rows (B, HW, C): fp32 statistics per (sample, group) over HW x C / groups
 * values (two passes), fp32 arithmetic, bf16 result (GroupNorm32, nn.py:23-25; ``add`` f32 (B, >= C) with row stride ld_add, or NULL: the
 * timestep embedding a ResBlock adds in front of out_layers, unet.py:270).  stats: f32 scratch of B * groups * 2 * (ceil(HW / 32) + 1) values (per-chunk partial sums,
 * added in a fixed order: the result is bit-reproducible).  C <= 1024. */
int fm_groupnorm_nhwc(const void* x, int ldx, const void* add, int ld_add, const void* w, const void* b, void* y, int ldy, void* stats, int B, int HW,
                      int C, int groups, float eps, int silu, void* stream);
int fm_add_bf16(const void* a, int lda, const void* b, int ldb, void* out, int ldo, int64_t rows, int C, void* stream);   /* out = a + b, bf16 rows */
int fm_silu_f32_to_bf16(const void* x, void* y, int64_t n, void* stream);                                                 /* y = bf16(x * sigmoid(x)) */
/* out[b] = [cos(t_b f_i) | sin(t_b f_i)], f_i = exp(-ln(max_period) i / (dim / 2)); t f32 (B), out bf16 (B, ldo)   (nn.py:120-140) */
int fm_timestep_embedding(const void* t, void* out, int ldo, int B, int dim, float max_period, void* stream);
/* Spatial self-attention of AttentionBlock with QKVAttentionLegacy: qkv bf16 (B * T, ld) whose columns are, per head, [q | k | v] of ch
 * channels each; weights = softmax_fp32(q k^T / sqrt(ch)); out bf16 (B * T, ldo) with a head's ch channels side by side. */
int fm_unet_attention(const void* qkv, int ld, void* out, int ldo, int B, int T, int heads, int ch, void* stream);
/* Scheduler step, element-wise (f32, n = B * per_sample values):
 *   fm_diffusion_x0:    x0 = c0 * sample + c1 * model_output                     (v-prediction: c0 = sqrt(a_t), c1 = -sqrt(1 - a_t); ...)
 *   fm_quantile_abs:    out[b] = torch.quantile(|x[b]|, q) (linear interpolation) - radix select, one workgroup per sample
 *   fm_diffusion_step:  x0' = quantile ? clamp(x0, -s, s) / s with s = clamp(quantile[b], 1, sample_max_value)   (_threshold_sample)
 *                           : clip_range > 0 ? clamp(x0, -clip_range, clip_range) : x0;
 *                       out = k0 * x0' + k1 * sample + k2 * model_output + k3 * noise   (noise may be NULL);  x0_out (optional) = x0' */
int fm_diffusion_x0(const void* sample, const void* model_output, float c0, float c1, void* x0, int64_t n, void* stream);
int fm_quantile_abs(const void* x, int B, int64_t n, float q, void* out, void* stream);
int fm_diffusion_step(const void* x0, const void* quantile, float sample_max_value, float clip_range, const void* sample, const void* model_output,
                      const void* noise, float k0, float k1, float k2, float k3, void* out, void* x0_out, int B, int64_t per_sample, void* stream);

/* Tokenizer training objective (csrc/train_objective.hip): what a tokenizer training step does besides VQVAE.forward / backward and the
 * perceptual losses.  fp32 throughout; compiled without fused multiply-adds.  No floating-point atomics: every reduction is per-workgroup
 * partial sums in caller-owned scratch, added in a fixed order - two calls on the same inputs give the same bits.  No input value is ever
 * used as an index without a range check.
 *
 * fm_reconst_loss: upstream's compute_reconst_loss (run_training_vqvae.py:961-1003).  x f32 (B, C, HW) contiguous; target of the same shape,
 *   except FM_LOSS_CE_INDEX: int64 class indices (B, HW), x holding C = K class scores per pixel.  loss[0] = the scalar loss; grad (f32, x's
 *   shape, or NULL) = d loss / d x, written in the same launch that writes the loss partials.  scratch: fm_reconst_loss_scratch(...) f32
 *   values (that function returns the count, or -1).  Two launches (main, fixed-order sum); the index cross-entropy counts its valid pixels
 *   first (integer atomics), two launches more.
 *     MSE / L1 / SMOOTH_L1 (beta = 1): mean over all elements; d |d| / d d = 0 at d = 0.
 *     CE_INDEX: F.cross_entropy over the strided class axis, ignore_index = -100, mean over the pixels whose label is not -100 (none: nan).
 *       A label outside [0, K) other than -100 makes that pixel's loss and gradient NaN.
 *     BCE: s = sigmoid(x); F.cross_entropy of the 2 C "logits" [s, 1 - s] against the probabilities q = [t, 1 - t] per pixel (a softmax over
 *       probabilities, upstream's formulation; sum q = C): d / d z_k = (C p_k - q_k) / (B HW), chained through both occurrences of s_c.
 *     COSINE: 1 - mean over (b, c) of the cosine similarity along HW;  COSINE_1D: 1 - mean over (b, hw) of the similarity along C.
 *       cos = <x, t> / (max(|x|, 1e-8) max(|t|, 1e-8)); d cos / d x = t / (|x|' |t|') - cos x / (|x|' |x|), the second term 0 where |x| = 0.
 * fm_scale_f32: x[i] *= scale[0] (scale: one f32 in DEVICE memory) - the loss's backward; nothing is read or written when scale[0] is exactly 1.
 * fm_mask_out_samples: upstream's mask_out_samples (:857-878).  clean f32 (B, C, HW), valid uint8 / bool (B, HW), out f32 (B, C + 1, HW):
 *   where valid is 0 clean is overwritten IN PLACE with mask_value; out = [clean after that | valid * 2 - 1].
 * fm_ema_update: ModelEma.update (fourm/utils/timm/model_ema.py:70-81) over a job list in ONE launch: for every element of every job
 *   ema = fadd(fmul(ema, decay), fmul(one_minus_decay, model)), each operation rounded to fp32 separately (torch's three kernels).  jobs: a
 *   DEVICE array of n_jobs fm_ema_job sorted by first_chunk, job i covering workgroups [first_chunk, first_chunk + ceil(n / FM_EMA_CHUNK));
 *   chunks = their total.  Pointers 4-byte aligned (16-byte aligned pairs take 16-byte accesses).
 * fm_diffusion_pair: noisy = fadd(fmul(sa, clean), fmul(ss, noise)) and, unless velocity is NULL, velocity = fsub(fmul(sa, noise),
 *   fmul(ss, clean)) with sa = sqrt_alpha[timesteps[b]], ss = sqrt_sigma[timesteps[b]] gathered on the device (tables f32 (T), timesteps
 *   int64 (B)): the schedulers' add_noise / get_velocity, clean and noise read once.  A timestep outside [0, T) yields NaN.  B <= 65535.
 * fm_token_usage: counts[w] (int32) = the number of distinct values in tokens[w * window, (w + 1) * window), tokens int16 / int32 / int64
 *   (elem_size 2 / 4 / 8) in [0, K), K <= FM_TOKEN_USAGE_MAX_K: a K-bit bitmap in LDS per window (integer atomicOr), then its population
 *   count.  bad[0] (int32) = the number of tokens outside [0, K); they are not counted.
 * Refused (-1) without touching any output: null pointers where one is required, non-positive sizes, misaligned pointers, the limits above. */
enum { FM_LOSS_MSE = 0, FM_LOSS_L1 = 1, FM_LOSS_SMOOTH_L1 = 2, FM_LOSS_CE_INDEX = 3, FM_LOSS_BCE = 4, FM_LOSS_COSINE = 5, FM_LOSS_COSINE_1D = 6 };
#define FM_RECONST_CHUNK 4096
#define FM_EMA_CHUNK 4096
#define FM_TOKEN_USAGE_MAX_K (1 << 20)
typedef struct fm_ema_job {
    void* ema;
    const void* model;
    int64_t n;
    int64_t first_chunk;
} fm_ema_job;
int fm_reconst_loss_scratch(int mode, int B, int C, int64_t HW);
int fm_reconst_loss(const void* x, const void* target, int mode, int B, int C, int64_t HW, void* grad, void* scratch, void* loss, void* stream);
int fm_scale_f32(void* x, const void* scale, int64_t n, void* stream);
int fm_mask_out_samples(void* clean, const void* valid, float mask_value, void* out, int B, int C, int64_t HW, void* stream);
int fm_ema_update(const void* jobs, int n_jobs, int64_t chunks, float decay, float one_minus_decay, void* stream);
int fm_diffusion_pair(const void* clean, const void* noise, const void* timesteps, const void* sqrt_alpha, const void* sqrt_sigma, int T, void* noisy,
                      void* velocity, int B, int64_t per_sample, void* stream);
int fm_token_usage(const void* tokens, int elem_size, int64_t n_windows, int64_t window, int K, void* counts, void* bad, void* stream);

/* Tokenizer validation metrics (csrc/metrics.hip): the image metrics of upstream's eval_metrics (run_training_vqvae.py:1427-1632) - MSE, MAE,
 * PSNR, MS-SSIM, IoU - and the token histogram.  Images are f32 (B, C, H, W) contiguous; only the first C_use channels of each sample are read,
 * in place (prediction and target may have different channel counts).  transform is applied in the loads:
 *     FM_METRIC_RAW: the values as they are;  FM_METRIC_DENORM: (v + 1) * 0.5 on both images, one fp32 add and an exact halving (upstream's
 *     denormalize, TF.normalize with mean -1 and std 2);  FM_METRIC_SIGMOID_PRED: 1 / (1 + exp(-v)) on the prediction, the target raw.
 * Per-element arithmetic is fp32, compiled without fused multiply-adds; every sum over elements, window positions and tiles is carried in double
 * and added in a fixed order (per thread, shuffle tree, wavefronts, per-workgroup partials in caller-owned scratch, a second launch over the
 * partials in index order).  No floating-point atomics: two calls on the same inputs give the same bits.  Integer atomics only where the order
 * cannot matter (the IoU counts, the histogram).  No input value is used as an index without a range check.
 *
 * fm_metric_sums: with p, t the converted prediction and target and d = p - t rounded once,  sums[0] += sum d * d,  sums[1] += sum |d|  (f64
 *   accumulators in device memory, each term formed in fp32),  counts[3] += B C_use HW  (counts: int64 (5) in device memory).  With iou != 0
 *   also counts[0] += tp, counts[1] += fp, counts[2] += fn, counts[4] += the number of targets that are neither 0 nor 1, where the prediction
 *   is positive when min(max(p, 0), 1) > threshold and the target when t == 1.  scratch: fm_metric_sums_scratch doubles (that function returns
 *   the count, or -1).  Workgroup w takes elements [w, w + 1) FM_METRIC_CHUNK of the B C_use HW in (b, c, hw) order, whatever Cp and Ct are.
 * fm_ssim_scale: SSIM of one scale with a separable window of ksize taps (f32 (ksize) in device memory; ksize odd, <= FM_SSIM_MAX_KERNEL) over
 *   the valid positions only, (H - ksize + 1) (W - ksize + 1) per channel:  mu_x = sum g_i g_j x,  var_x = sum g_i g_j x^2 - mu_x^2,  cov = sum
 *   g_i g_j x y - mu_x mu_y,  cs = (2 cov + c2) / (var_x + var_y + c2),  ssim = (2 mu_x mu_y + c1) / (mu_x^2 + mu_y^2 + c1) * cs.  ssim[b] and
 *   cs[b] (f64 (B) in device memory) = the means over channels and positions of image b.  One workgroup per (plane, FM_SSIM_TILE^2 positions):
 *   the haloed tile of both images in LDS, the five moments filtered along the rows, then the columns.  scratch: fm_ssim_scale_scratch doubles.
 * fm_avgpool2x2_pair: xo, yo f32 (B, C_use, H / 2, W / 2) = the 2 x 2 mean with stride 2 of the converted first C_use channels of x and y,
 *   ((a + b) + (c + d)) * 0.25; an odd last row or column is dropped (F.avg_pool2d).  The next scale reads xo, yo with FM_METRIC_RAW.
 * fm_token_histogram: hist[v] += the number of tokens equal to v (hist: int64 (K) in device memory, zeroed by the caller; tokens int16 / int32 /
 *   int64 by elem_size 2 / 4 / 8); bad[0] (int32) = the number of tokens outside [0, K), which are not counted.
 * Refused (-1) before anything is written: null or misaligned pointers, non-positive sizes, C_use above a channel count, an unknown transform,
 *   a window that is even, longer than FM_SSIM_MAX_KERNEL or longer than the image. */
enum { FM_METRIC_RAW = 0, FM_METRIC_DENORM = 1, FM_METRIC_SIGMOID_PRED = 2 };
#define FM_METRIC_CHUNK 4096
#define FM_SSIM_TILE 32
#define FM_SSIM_MAX_KERNEL 11
int fm_metric_sums_scratch(int B, int C_use, int64_t HW);
int fm_metric_sums(const void* pred, const void* target, int B, int Cp, int Ct, int C_use, int64_t HW, int transform, int iou, float threshold,
                   void* scratch, void* sums, void* counts, void* stream);
int fm_ssim_scale_scratch(int B, int C_use, int H, int W, int ksize);
int fm_ssim_scale(const void* x, const void* y, int B, int Cx, int Cy, int C_use, int H, int W, int transform, const void* window, int ksize, float c1,
                  float c2, void* scratch, void* ssim, void* cs, void* stream);
int fm_avgpool2x2_pair(const void* x, const void* y, int B, int Cx, int Cy, int C_use, int H, int W, int transform, void* xo, void* yo, void* stream);
int fm_token_histogram(const void* tokens, int elem_size, int64_t n, int K, void* hist, void* bad, void* stream);

/* Image resize (csrc/resize.hip): F.interpolate with a given size and align_corners = False, as upstream's tokenizer trainer uses it
 * (run_training_vqvae.py prepare_inputs :881-958; the Resize of the CLIP loss's percept_transform) - bilinear, antialiased bilinear and
 * nearest - with the adjoint of the two bilinear modes.  fp32 planes (planes = B C, H, W) contiguous.  Both bilinear modes are separable:
 * one axis is a table (start[o], count[o], weights[o][taps]) per output index o, output o = sum_k weights[o][k] * input[start[o] + k].
 *
 * fm_resize_axis_table: HOST function, no GPU call.  Fills the table of one axis into caller-owned HOST arrays (any of them may be NULL):
 *   start, count int32 (n_out); weights f32 (n_out, taps) = the weights computed in double and rounded once, rows padded with zeros;
 *   weights_f64 the same before rounding; t_start, t_count int32 (n_in) = the transposed description: input i is read by exactly the outputs
 *   [t_start[i], t_start[i] + t_count[i]) (contiguous because start and start + count do not decrease; t_count[i] = 0 where no output reads
 *   i, and t_start does not decrease either).  Returns taps = max count (call once with NULLs to size the weights), or -1.  With scale =
 *   n_in / n_out in double:
 *     FM_RESIZE_BILINEAR:    s = max(scale (o + 0.5) - 0.5, 0), i0 = min(floor(s), n_in - 1), i1 = min(i0 + 1, n_in - 1), weights 1 - (s - i0), s - i0;
 *     FM_RESIZE_BILINEAR_AA: support = max(scale, 1), inv = min(1 / scale, 1), c = scale (o + 0.5), xmin = max(int(c - support + 0.5), 0),
 *                            xsize = min(int(c + support + 0.5), n_in) - xmin, w_j = max(0, 1 - |(j + xmin - c + 0.5) inv|) / their sum;
 *     FM_RESIZE_NEAREST:     i = min(floorf(fp32(o) * (fp32(n_in) / fp32(n_out))), n_in - 1), one tap of weight 1.
 *   Taps of weight zero at either end of a window are dropped (i0 = i1 becomes one tap of weight 1), so every stored tap inside count is
 *   non-zero.  Windows wider than FM_RESIZE_MAX_TAPS and sizes above 2^24 are refused.
 * fm_resize_bilinear_fwd: y[p] = a_c R(x[p]) + b_c, c = p mod C, one fused multiply-add on the filtered value; scale (a) and shift (b) are
 *   f32 (C) in device memory or NULL (both or neither; NULL = identity).  Tables in DEVICE memory, as fm_resize_axis_table made them for
 *   (H_in, H_out) and (W_in, W_out).  One launch: a workgroup owns a tile of outputs, stages the tile's input window and table rows in LDS,
 *   filters along the rows into LDS, then along the columns.  The tile (at most 32 x 32) is the largest whose window fits 64 KiB of LDS.
 * fm_resize_bilinear_bwd: dx[p] = a_c R^T(dy[p]) as a gather over the transposed tables: a workgroup owns a tile of INPUT pixels, stages the
 *   window of dy that reads them (tiles of at most 64 x 64), and every input pixel sums its covering outputs in index order.  One launch, no
 *   atomics.
 * fm_resize_nearest: y[p][oh][ow] = x[p][index_h[oh]][index_w[ow]] for elements of elem_size 4 (f32) or 8 (int64 class maps); index_h, index_w
 *   int32 (H_out), (W_out) in device memory (the start array of FM_RESIZE_NEAREST), clamped into the image.
 * Two calls on the same inputs give the same bits.  Refused (-1) before any launch: null or misaligned pointers, non-positive sizes, taps
 * outside [1, FM_RESIZE_MAX_TAPS], a geometry whose smallest tile does not fit the LDS.  The kernels never index by a table entry they have not
 * range-checked: a tile whose table rows are inconsistent with the sizes is filled with NaN. */
enum { FM_RESIZE_BILINEAR = 0, FM_RESIZE_BILINEAR_AA = 1, FM_RESIZE_NEAREST = 2 };
#define FM_RESIZE_MAX_TAPS 64
int fm_resize_axis_table(int n_in, int n_out, int mode, int32_t* start, int32_t* count, float* weights, double* weights_f64, int32_t* t_start,
                         int32_t* t_count);
int fm_resize_bilinear_fwd(const void* x, void* y, int planes, int H_in, int W_in, int H_out, int W_out, const void* start_h, const void* count_h,
                           const void* weights_h, int taps_h, const void* start_w, const void* count_w, const void* weights_w, int taps_w,
                           const void* scale, const void* shift, int C, void* stream);
int fm_resize_bilinear_bwd(const void* dy, void* dx, int planes, int H_in, int W_in, int H_out, int W_out, const void* start_h, const void* count_h,
                           const void* weights_h, int taps_h, const void* t_start_h, const void* t_count_h, const void* start_w,
                           const void* count_w, const void* weights_w, int taps_w, const void* t_start_w, const void* t_count_w,
                           const void* scale, int C, void* stream);
int fm_resize_nearest(const void* x, void* y, int elem_size, int planes, int H_in, int W_in, int H_out, int W_out, const void* index_h,
                      const void* index_w, void* stream);

/* Pillow-exact crops (csrc/pil_resize.hip): the data stage of upstream's save_vq_tokens.py - PIL.Image.crop + Image.resize + horizontal flip
 * of 8-bit images - byte for byte.  Source: uint8 (H, W, C), 1 <= C <= 4.  One crop: (top, left, h, w, flip) inside the image, target S x S.
 * Result: np.asarray(img.crop((left, top, left + w, top + h)).resize((S, S), resample)), then the flip.
 *
 * Filter modes (FM_PIL_BILINEAR, support 1; FM_PIL_BICUBIC, support 2), one axis of length n (the crop's) to S, everything in double, in this
 * order, without fused multiply-add:  scale = n / S, fs = max(scale, 1), support = filter_support * fs;  per output o: center = (o + 0.5) *
 * scale, xmin = max(int(center - support + 0.5), 0), xmax = min(int(center + support + 0.5), n), taps x = 0 .. xmax - xmin - 1 with k[x] =
 * filter((x + xmin - center + 0.5) * (1 / fs)), ww = their sum in tap order, k[x] /= ww where ww != 0, and the integer coefficient
 * int(0.5 + k * 2^22) for k >= 0, int(-0.5 + k * 2^22) for k < 0 (C truncation).  bilinear(x) = 1 - |x| below 1;  bicubic(x), a = -0.5:
 * ((a + 2)|x| - (a + 3)) * |x| * |x| + 1 below 1, (((|x| - 5)|x| + 8)|x| - 4) * a below 2, else 0.  A pass computes acc = 2^21 + sum pixel *
 * coef in int32 and out = clamp(acc >> 22, 0, 255) (arithmetic shift).  The horizontal pass runs first, over the crop's rows, into a uint8
 * intermediate (h, S, C) - that rounding is part of the contract - then the vertical pass.  A pass whose size does not change is the
 * identity (its table is the single coefficient 2^22).
 * FM_PIL_NEAREST: Pillow's affine scaler: a = n / S in double, xo = a * 0.5, per output idx = int(xo), then xo += a (repeated addition; the
 * closed form int((o + 0.5) * a) is NOT the same table).
 * Flip, after the resize: columns reversed; channels in invert_mask (bit c) become 255 - v (channel 0 of surface normals).
 * Four-channel images are four plain 8-bit planes (CMYK, RGBX); the premultiplication Pillow wraps around RGBA / LA resizes is not applied.
 * Both entry points were ADDED without raising FM_ABI_VERSION (it stays 11: nothing that existed changed its meaning); a caller that needs
 * them checks for the symbols, not for the version.
 *
 * fm_pil_axis_table: HOST function, no GPU call.  Fills start, count int32 (n_out) and coef int32 (n_out, taps), rows padded with zeros, for
 *   one axis and filter (NULLs allowed); returns taps = the largest count (call once with NULLs to size coef), or -1.  FM_PIL_NEAREST and
 *   n_in = n_out give one tap per output: start = the index, count = 1, coef = 2^22.  Windows above FM_PIL_MAX_TAPS are refused.
 * fm_pil_crop_resize: n_jobs crops in two launches (rows, then columns).  jobs_dev: the DEVICE copy of jobs_host (8-byte aligned); the host
 *   copy is validated completely before the first launch.  src: packed uint8 images (src_bytes);  tables: packed int32 axis tables
 *   (table_words), the table of one axis laid out start (S) | count (S) | coef (S, taps);  scratch: caller-owned uint8 (scratch_bytes) for
 *   the intermediates.  Outputs (any may be NULL, not all): out_u8 uint8 (n_slots, S, S, C);  out_f32 f32 (n_slots, C, S, S) = lut[c][v],
 *   lut f32 (C, 256) in device memory;  out_i64 int64 (n_slots, S, S), C = 1 only.  Job i owns workgroups [blk_rows, blk_rows + ceil(h S /
 *   256)) of the first launch and [blk_cols, blk_cols + ceil(S S / 256)) of the second, both prefix sums over the jobs in order.
 * Refused (-1) before any launch: a box that leaves its image, an image, table, intermediate or slot outside its buffer, first workgroups
 * that are not the prefix sums, a launch of 2^24 workgroups or more, C outside 1 .. 4, out_i64 with C != 1, out_f32 without lut.  The kernels use a table entry as an index only
 * after checking it against the crop (a pixel whose table row is inconsistent is written as 0).  Two calls give the same bytes. */
enum { FM_PIL_NEAREST = 0, FM_PIL_BILINEAR = 1, FM_PIL_BICUBIC = 2 };
#define FM_PIL_MAX_TAPS 1024
typedef struct fm_pil_crop_job {
    int64_t src_off;  /* byte offset of the source image in src */
    int64_t mid_off;  /* byte offset of this crop's (h, S, C) intermediate in scratch */
    int64_t out_slot; /* index of the crop in the outputs */
    int64_t blk_rows; /* first workgroup of the rows launch */
    int64_t blk_cols; /* first workgroup of the columns launch */
    int32_t H;        /* source size */
    int32_t W;
    int32_t top;      /* the box */
    int32_t left;
    int32_t h;
    int32_t w;
    int32_t flip;     /* 0 or 1 */
    int32_t tab_w;    /* int32-word offset in tables of the table w -> S (rows launch) */
    int32_t tab_h;    /* the same of h -> S (columns launch) */
    int32_t taps_w;   /* row lengths of their coef arrays */
    int32_t taps_h;
    int32_t pad_;
} fm_pil_crop_job;
int fm_pil_axis_table(int n_in, int n_out, int filter, int32_t* start, int32_t* count, int32_t* coef);
int fm_pil_crop_resize(const fm_pil_crop_job* jobs_host, const void* jobs_dev, int n_jobs, const void* src, int64_t src_bytes, const void* tables,
                       int64_t table_words, void* scratch, int64_t scratch_bytes, int C, int S, int invert_mask, const void* lut, void* out_u8,
                       void* out_f32, void* out_i64, int64_t n_slots, void* stream);

/* Pillow-exact 16-bit depth crops (csrc/pil_resize16.hip): PIL.Image.crop + Image.resize + horizontal flip of mode "I;16" images (16-bit
 * depth PNGs) - byte for byte - and upstream's DepthTransform.truncated_depth_standardization on the result.  Source: uint16 (H, W).
 * Result of one crop (top, left, h, w, flip), target S x S: np.asarray(img.crop((left, top, left + w, top + h)).resize((S, S), resample)),
 * then the flip.
 *
 * Pillow resamples "I;16" through ImagingResampleHorizontal/Vertical_16bpc, not the 8-bit integer path: the coefficients are the normalised
 * DOUBLES of the section above - exactly what fm_pil_axis_table computes before it quantises to 2^22 (k = filter((x + xmin - center + 0.5) *
 * ss), ww summed left to right, k / ww where ww != 0).  One output sample of a pass that resamples: ss = 0.0; for each tap in order ss +=
 * (double)in[x] * k[x], the product and the sum rounded separately (NO fused multiply-add, on the device either); r = (int)(ss < 0 ? ss -
 * 0.5 : ss + 0.5); low byte = clip8(r % 256) with C's remainder sign, high byte = clip8(r >> 8), clip8 the clamp to 0 .. 255.  The clamp is
 * PER BYTE, not a clamp of r to 0 .. 65535: bicubic overshoot next to a saturated region gives a high byte of 255 and the low byte of r.
 * The horizontal pass runs first, over the crop's rows, into a uint16 intermediate (h, S) - that rounding is part of the contract - then the
 * vertical pass.  An axis whose crop length equals S is not resampled (Pillow skips that pass; its table is the single coefficient 1.0 and the
 * sample is copied).  FM_PIL_NEAREST: both axes are index gathers, idx = int((o + 0.5) * a), a = n / S in double.  This is NOT the repeated-
 * addition table of the section above: Pillow sends "I;16" (a "special" image type) through its generic affine transform, which evaluates
 * the coordinate of every output pixel in closed form, and not through the 8-bit affine scaler; the two tables differ on about one axis in
 * twenty (8 -> 7 is one).  The flip is applied last.  Modes "I", "F" and big-endian "I;16B" are outside this contract.
 *
 * Truncated standardisation of one crop of n = S S values v (0 .. 65535): lo = int(0.1 * n) and hi = int((1 - 0.1) * n) are computed by the
 * CALLER in double (Python's) and passed in, m = hi - lo >= 2.  Over the elements of sorted rank lo .. hi - 1 the exact integers M1 = sum v
 * and M2 = sum v^2;  mean = M1 / (m * 65535), one correctly rounded double division of two exactly representable integers;  var = (m M2 -
 * M1^2) / (m (m - 1) 65535^2): numerator and denominator are exact wide integers, each converted to double with one correct rounding (above
 * 64 bits: shifted to 64 bits with a sticky bit, converted, scaled back), then divided;  mean32 = (float)mean, var32 = (float)var;  x =
 * (float)((double)v / 65535.0) - what torch.Tensor(np.array(img) / (2**16 - 1.0)) holds - and out = (x - mean32) / sqrtf(var32 + 1e-6f) in
 * separately rounded fp32 operations.  The statistics are integer sums: they do not depend on the order of the reduction, two calls or two
 * workgroup shapes give the same bits.  No sort: the rank boundaries are found by a two-level 256-bin histogram select in LDS (integer LDS
 * atomics only, no floating-point atomics), one workgroup per crop;  the boundary values contribute only the share of their ties inside the
 * rank range.  Upstream sums in fp32, so its own result differs from this by the rounding of its sums (INTEGRATION.md has the measured figure).
 * The entry points were ADDED without raising FM_ABI_VERSION (it stays 11); a caller that needs them checks for the symbols.
 *
 * fm_pil_axis_table_f64: HOST function, no GPU call.  As fm_pil_axis_table with coef double (n_out, taps): the same start, count and taps
 *   from the same computation, the coefficients before quantisation.  FM_PIL_NEAREST and n_in = n_out: one tap of coefficient 1.0;  the
 *   start of FM_PIL_NEAREST is the closed-form index above (the one difference from fm_pil_axis_table's start and count).
 * fm_pil_crop_resize16: n_jobs crops in two launches (rows, then columns) over the fm_pil_crop_job list of the section above, with src_off
 *   and mid_off in bytes (both even) and tab_w / tab_h in int32 words (both even).  src: packed uint16 images (src_bytes);  tables (8-byte aligned, table_words int32 words): the
 *   table of one axis laid out start int32 (S) | count int32 (S) | coef double (S, taps), S (2 + 2 taps) words;  scratch: caller-owned
 *   (scratch_bytes) for the uint16 intermediates (h, S).  Outputs (either may be NULL, not both): out_i32 int32 (n_slots, S, S), the uint16
 *   values;  out_f32 f32 (n_slots, 1, S, S) = (float)((double)v / 65535.0).  Workgroups as in fm_pil_crop_resize.  The host copy of every job
 *   is validated before the first launch, with the refusals of fm_pil_crop_resize; a table entry is used as an index only after a check
 *   against the crop (a sample whose table row is inconsistent is written as 0).  Two calls give the same bytes.
 * fm_depth_standardize: values int32 (n_crops, n), each 0 .. 65535 (a value outside is read as its low 16 bits) -> out_f32 f32 (n_crops, n)
 *   (may be NULL) and stats f32 (n_crops, 2) = (mean32, var32) (may be NULL, not both).  One workgroup per crop.  Refused (-1): n < 2,
 *   n > 2^28, lo < 0, hi > n, hi - lo < 2. */
int fm_pil_axis_table_f64(int n_in, int n_out, int filter, int32_t* start, int32_t* count, double* coef);
int fm_pil_crop_resize16(const fm_pil_crop_job* jobs_host, const void* jobs_dev, int n_jobs, const void* src, int64_t src_bytes, const void* tables,
                         int64_t table_words, void* scratch, int64_t scratch_bytes, int S, void* out_i32, void* out_f32, int64_t n_slots, void* stream);
int fm_depth_standardize(const void* values_i32, int n_crops, int64_t n, int64_t lo, int64_t hi, void* out_f32, void* stats, void* stream);

/* CLIP text tower and CLIP score (csrc/clip_text.hip): the two ends of upstream's CLIP.encode_text / CLIP.forward (fourm/utils/clip/model.py
 * :407-440) that the trunk's kernels do not cover.  The blocks between them are the trunk's (LayerNorm, qkv GEMM, fm_attn_fwd / fm_attn_f32_fwd
 * with FM_MASK_DECODER and causal = 1, cs = modq = modk = NULL: blocked[q][k] = k > q, upstream's triu(1) mask; FM_EPI_QUICK_GELU).  Everything
 * here is fp32 and row-local: one wavefront owns a row, lane l accumulates elements l, l + 64, ... in index order, then the shuffle tree.  No
 * floating-point atomics: two calls on the same inputs give the same bits.  The normalisation of a finished fp32 sum (square roots, division)
 * is evaluated in double and rounded to fp32 once.
 * The entry points were ADDED without raising FM_ABI_VERSION (it stays 11); a caller that needs them checks for the symbols.
 *
 * fm_clip_text_embed: ids int64 (B, Lc) contiguous; token_embedding f32 (V, D); positional_embedding f32 (Lc, D); both contiguous, 16-byte
 *   aligned.  out f32 rows with row stride ldo: out[b Lc + t] = token_embedding[ids[b][t]] + positional_embedding[t], one fp32 add per element.
 *   eot_row int32 (B): b Lc + argmax_t ids[b][t], the FIRST maximum on ties (torch.argmax) - the row CLIP.encode_text projects.  eot_map
 *   int32 (B Lc), optional (may be NULL): the same pick as a row map of fm_layernorm_fwd - b at the end-of-text row of sample b, -1 at every
 *   other row - so that ln_final normalises exactly the B rows that are projected, without a gather in between.  An id outside
 *   [0, V) is never used as an index: its row is written as zeros and counted.  bad int32 (1): zeroed by the call, then the number of such ids
 *   (an integer atomic; the order cannot matter).  D and ldo multiples of 4.
 * fm_clip_pair_score: img f32 (B, E) with row stride ldi, txt f32 (B, E) with row stride ldt.  score f32 (B): 100 <img_b, txt_b> / (|img_b|
 *   |txt_b|) - dot product and squared norms accumulated in fp32 in the order above, 100 dot / (sqrt(n_i) sqrt(n_t)) in double, rounded once;
 *   a pair with a zero norm scores 0, not NaN.  sum f64 (1) += the sum of the B scores: every workgroup (4 pairs) leaves ((s0 + s1) + s2) + s3
 *   as one double in scratch (fm_clip_pair_score_scratch doubles; that function returns the count, or -1), a second launch adds the partials
 *   in index order.  count int64 (1) += B (may be NULL).  sum and count are ACCUMULATORS in device memory: the caller zeroes them.
 * fm_l2_normalize_rows: y[r] = x[r] * (f / |x[r]|), f = factor * (factor_dev ? factor_dev[0] : 1) with factor_dev f32 (1) in device memory or
 *   NULL; f / sqrt(sum of squares) in double, rounded to fp32 once, then one fp32 multiply per element.  A zero row stays zero.  x == y (in
 *   place) is allowed.  f32 rows (R, E) with row strides ldx, ldy.
 * Refused (-1) before anything is written: null or misaligned pointers, non-positive sizes, a row stride below the row length. */
int fm_clip_text_embed(const void* ids, const void* token_embedding, const void* positional_embedding, void* out, int ldo, void* eot_row,
                       void* eot_map, void* bad, int B, int Lc, int D, int V, void* stream);
int fm_clip_pair_score_scratch(int B);
int fm_clip_pair_score(const void* img, int ldi, const void* txt, int ldt, void* score, void* scratch, void* sum, void* count, int B, int E,
                       void* stream);
int fm_l2_normalize_rows(const void* x, int ldx, void* y, int ldy, int R, int E, const void* factor_dev, float factor, void* stream);

/* Flat k-NN index (csrc/knn.hip): the exact top-k search of nq query rows against n gallery rows of width d, everything fp32 - the search step
 * of 4M-21's retrieval (upstream: faiss.IndexFlatL2 / IndexFlatIP).  No score matrix goes to memory and there are no floating-point atomics.
 * The entry points were ADDED without raising FM_ABI_VERSION (it stays 11); a caller that needs them checks for the symbols.
 *
 * Score: s(q, x) = sum_i q_i x_i on v_mfma_f32_32x32x2_f32, ONE fp32 accumulation chain over i ascending.  It is a function of (query row,
 *   gallery row, d): the same bits wherever the gallery row sits and whatever nq, k, splits, query_tile or the batch are.
 * Key: FM_KNN_IP: s, larger is better.  FM_KNN_L2: kappa = fmaf(-2, s, |x|^2), smaller is better, with |x|^2 the fp32 row sum of
 *   fm_row_sqnorms (made once, in a fixed order); |q|^2 is constant per query and is left out.
 * Order: total, on (key, gallery index): better key first, lower index first on equal keys (-0 and +0 are equal).  The result is the first
 *   k of that order, so it does not depend on the split or on the order in which candidates were met.  Fewer than k gallery rows: the
 *   missing slots are index -1 with distance +inf (FM_KNN_L2) / -inf (FM_KNN_IP).  NaN inputs are not supported.
 * Split: the gallery is cut into `splits` chunks of per = ceil(ceil(n / 128) / splits) tiles of 128 rows (chunk c: rows [128 per c,
 *   128 per (c + 1)), the last ones possibly empty).  A workgroup owns (query tile, chunk), keeps a running top-k per query row in LDS and
 *   leaves k candidates per (query, chunk) in scratch; a merge workgroup per query sorts the splits k candidates.  splits k <=
 *   FM_KNN_MAX_MERGE.  fm_knn_splits proposes a count from nq, n, k and the CU count (a single query over a long gallery still fills the chip).
 * Query tile: 128 queries per workgroup, or 32 (a quarter of the matrix work per gallery byte: for a few queries the search is bound by the
 *   gallery read).  query_tile = 0 picks by nq (fm_knn_query_tile: 32 up to 64 queries).  Both give the same bits.
 * Sizes: 1 <= n <= 2^31 - 1 (offsets into the gallery are 64-bit), d a multiple of 4 up to FM_KNN_MAX_D, rows contiguous (row stride d) and
 *   16-byte aligned, 1 <= k <= FM_KNN_MAX_K, at most 65535 query tiles per call.
 *
 * fm_row_sqnorms: out f32 (n) = |x_r|^2 of x f32 (n, d): a wavefront per row, lane l adds elements 4 l .. 4 l + 3, 4 l + 256 .. in index
 *   order (fmaf), then the shuffle tree.
 * fm_knn_query_tile, fm_knn_splits, fm_knn_scratch_bytes: HOST functions, no GPU call.  The query tile chosen for nq; the proposed split count
 *   (cus = the device's compute units); *bytes = nq splits k 8.  -1 on a bad argument.
 * fm_knn_search: q f32 (nq, d), x f32 (n, d), xnorm f32 (n) (FM_KNN_L2; may be NULL for FM_KNN_IP), scratch caller-owned (scratch_bytes).
 *   out_d f32 (nq, k): the keys (s or kappa), best first;  out_i int64 (nq, k).  Two launches.
 * fm_knn_refine_l2: for the indices i_io int64 (nq, k) of an FM_KNN_L2 search: delta = sum_i (q_i - x_i)^2 in fp32 (the same lane order as
 *   fm_row_sqnorms; the terms are non-negative, no cancellation), the k entries re-ordered by (delta, index) in place, d_io f32 (nq, k) =
 *   delta.  An index outside [0, n) is never used as an offset: it is padding (-1, +inf) and goes last.
 * Refused (-1) before anything is launched or written: null or misaligned pointers, sizes outside the ranges above, an unknown metric or
 *   query tile, a scratch smaller than fm_knn_scratch_bytes.  No allocation, no host synchronisation. */
#define FM_KNN_IP 0
#define FM_KNN_L2 1
#define FM_KNN_MAX_K 64
#define FM_KNN_MAX_D 4096
#define FM_KNN_MAX_MERGE 4096
int fm_row_sqnorms(const void* x, int n, int d, void* out, void* stream);
int fm_knn_query_tile(int nq);
int fm_knn_splits(int nq, int n, int k, int cus);
int fm_knn_scratch_bytes(int nq, int k, int splits, int64_t* bytes);
int fm_knn_search(const void* q, int nq, const void* x, const void* xnorm, int n, int d, int k, int metric, int splits, int query_tile,
                  void* scratch, int64_t scratch_bytes, void* out_d, void* out_i, void* stream);
int fm_knn_refine_l2(const void* q, int nq, const void* x, int n, int d, int k, void* d_io, void* i_io, void* stream);

/* Inception tower (csrc/inception.hip): the kernels behind FID and the Inception score (fourm/utils/inception) - the FID variant of
 * InceptionV3 in fp32, as torchmetrics runs it.  Everything is fp32 NHWC "rows": a feature map of B images is a matrix (B H W, ld) with the
 * channels of a pixel contiguous and ld >= C floats between pixels, so a concatenation is written as channel slices of one buffer (the
 * caller passes out + c0).  No floating-point atomics: every output element is written once, in a summation order that depends on the
 * element alone, so two calls give the same bits.  The entry points were ADDED without raising FM_ABI_VERSION (it stays 11).
 *
 * fm_conv2d_nhwc_f32: out[b, oy, ox, n] = act(bias[n] + acc), acc = ONE fp32 accumulation chain, starting from 0, over
 *   k = (ky KW + kx) Cin + c ascending of x[b, oy stride - pad_h + ky, ox stride - pad_w + kx, c] * w[n, k]; taps outside the image contribute
 *   x = 0 (zero padding).  Ho = (H + 2 pad_h - KH) / stride + 1, Wo likewise.  x: f32 rows (B H W, ldx); w: f32 (Cout, KH KW Cin), tap-major and
 *   channel-minor, row stride ldw; bias: f32 (Cout) or NULL (zeros); out: f32 rows (B Ho Wo, ldo) at the pointer given; columns outside
 *   [0, Cout) of a row are never written.  act = ReLU when relu != 0.  KH, KW in 1..FM_CONV2D_MAX_K, stride 1 | 2 (both axes), pad_h, pad_w in
 *   0..FM_CONV2D_MAX_PAD, any Cin, Cout >= 1, fewer than 2^31 input and output rows.  Implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32, an fmaf
 *   chain over k): the activation tile is gathered into LDS with bounds checks, no im2col row goes to memory.  The tile (128 pixels x 32
 *   channels for Cout <= 32, else 64 x 64) is chosen by Cout alone and the k order is fixed, so an image's output is the same bits in any
 *   batch and at any position in it.  16-byte loads are used when Cin, ldx, ldw are multiples of 4 and x, w are 16-byte aligned; the bits
 *   do not depend on that.  A 1 x 1 convolution with H = W = 1 is a plain x w^T product (the fc head).
 * fm_pool2d_nhwc_f32: x f32 rows (B H W, ldx) -> out f32 rows, C channels, taps visited ky, kx ascending.  FM_POOL_MAX_3X3_S2: valid 3 x 3
 *   windows at stride 2, Ho = (H - 3) / 2 + 1.  FM_POOL_MAX_3X3_S1P1: stride 1, padding 1 that never wins.  FM_POOL_AVG_3X3_S1P1: stride 1,
 *   padding 1, count_include_pad = False: the fp32 sum of the valid taps times the fp32 reciprocal of their count.  FM_POOL_GLOBAL_AVG: out
 *   (B, ldo) = the fp32 sum over the H W rows of an image in row order, divided by H W.
 * fm_inception_preprocess: in (B, 3, H, W) uint8, or f32 when is_f32 (byte = trunc(255 v) in fp32, clamped to [0, 255]; NaN gives 0) ->
 *   bilinear resize to 299 x 299 WITHOUT half-pixel offset (TF1 / torch-fidelity) -> (v - 128) / 128, written as rows (B 299 299, 3).
 *   idx int32 (4, 299) = y0, y1, x0, x1 and wt f32 (2, 299) = wy, wx are the caller's axis tables (device memory): with s = in / 299 in
 *   double, src = o s, i0 = floor(src), i1 = min(i0 + 1, in - 1), w = src - i0 rounded to fp32.  top = fmaf(r - l, wx, l) on rows y0 and y1,
 *   then fmaf(bottom - top, wy, top).  Table indices are clamped to the image in the kernel.  One launch.
 * fm_feature_moments: feats f32 (n, d), row stride ld:  sum f64 (d) += column sums, outer f64 (d, d) += X^T X, count int64 (1) += n.  Every
 *   output element belongs to one thread and the rows are added in ascending order; a product of two floats is exact in double, so the
 *   result is the sequential float64 sum bit for bit.  d <= FM_MOMENTS_MAX_D.  Two launches.
 * Refused (-1) before anything is launched or written: null or misaligned pointers, sizes outside the ranges above, row strides smaller
 *   than the row, an unknown mode.  No allocation, no host synchronisation. */
#define FM_CONV2D_MAX_K 7
#define FM_CONV2D_MAX_PAD 3
#define FM_POOL_MAX_3X3_S2 0
#define FM_POOL_MAX_3X3_S1P1 1
#define FM_POOL_AVG_3X3_S1P1 2
#define FM_POOL_GLOBAL_AVG 3
#define FM_INCEPTION_SIZE 299
#define FM_MOMENTS_MAX_D 4096
typedef struct fm_conv2d_args {
    const void* x;
    const void* w;
    const void* bias;
    void* out;
    int B, H, W, Cin, Cout, KH, KW, stride, pad_h, pad_w;
    int ldx, ldw, ldo, relu;
} fm_conv2d_args;
int fm_conv2d_nhwc_f32(const fm_conv2d_args* a, void* stream);
int fm_pool2d_nhwc_f32(const void* x, int ldx, void* out, int ldo, int B, int H, int W, int C, int mode, void* stream);
int fm_inception_preprocess(const void* in, int is_f32, int B, int H, int W, const void* idx, const void* wt, void* out, void* stream);
int fm_feature_moments(const void* feats, int ld, int n, int d, void* sum, void* outer, void* count, void* stream);

/* LPIPS validation metric (csrc/lpips_metric.hip): the two kernels the AlexNet LPIPS metric of eval_metrics needs beyond the Inception tower's
 * (fourm/vq/percept_losses/lpips_alex.py, fourm.vq.metrics.LearnedPerceptualImagePatchSimilarity).  fp32, no floating-point atomics, one
 * summation order per output element: two calls give the same bits.  ADDED without raising FM_ABI_VERSION (it stays 11).
 *
 * fm_conv2d_stem_f32: a convolution for image stems, read straight from NCHW pixels.  img f32 (B, Cin, H, W) contiguous.  Per pixel value v:
 *   when clamp != 0, v = min(max(v, lo), hi); then s = fmaf(v, mul[c], add[c]) (one rounding; mul, add f32 (Cin), or both NULL: s = v).  Zero
 *   padding applies to s: a tap outside the image contributes 0, not add[c].  out[b, oy, ox, n] = act(bias[n] + acc), acc = ONE fp32
 *   accumulation chain from 0 over k = (ky KW + kx) Cin + c ascending of s * w[n, k] (the order of fm_conv2d_nhwc_f32).  w: f32 (Cout, KH KW Cin),
 *   row stride ldw; bias: f32 (Cout) or NULL; out: f32 NHWC rows (B Ho Wo, ldo), columns outside [0, Cout) never written; Ho = (H + 2 pad -
 *   KH) / stride + 1, Wo likewise; act = ReLU when relu != 0.  Cin in 1..FM_STEM_MAX_CIN, Cout in 1..FM_STEM_MAX_COUT, KH, KW in
 *   1..FM_STEM_MAX_K, stride in 1..FM_STEM_MAX_STRIDE, pad in 0..FM_STEM_MAX_PAD (both axes), H + 2 pad >= KH, W + 2 pad >= KW, fewer than
 *   2^31 output rows.  Implicit GEMM on v_mfma_f32_32x32x2_f32 with the gather (bounds-checked against the image) into LDS: no im2col or
 *   space-to-depth copy goes to memory.  The tile (128 pixels x 32 channels for Cout <= 32, else 64 x 64) is chosen by Cout alone and the k
 *   order is fixed: an image's output is the same bits in any batch and at any position in it.  One launch.
 * fm_lpips_score: a, b f32 rows (B P, C) with row strides lda, ldb; w f32 (C).  Per pixel na = sqrtf(eps + sum_c a_c^2), a^ = a / na, b^
 *   likewise; score[b] += (sum over the P pixels of sum_c w_c (a^_c - b^_c)^2) / P, all fp32.  score: f32 (B), zeroed by the caller before the
 *   first layer.  A first launch writes one partial per (sample, chunk of FM_LPIPS_SCORE_CHUNK pixels) to scratch (f32, fm_lpips_score_scratch
 *   values: that function returns the count, or -1), a second adds a sample's partials in chunk order onto score[b].  C % 4 == 0, C <=
 *   FM_LPIPS_SCORE_MAX_C, lda, ldb % 4 == 0 and >= C, all pointers 16-byte aligned, P >= 1, eps >= 0, B P < 2^31.  By construction: swapping
 *   a and b changes no bit; a against itself gives exactly 0; a pixel that is all zero on both sides contributes 0 (never NaN) when eps > 0.
 * Refused (-1) before anything is launched or written: null or misaligned pointers, sizes outside the ranges above, row strides smaller
 *   than the row, mul without add.  No allocation, no host synchronisation. */
#define FM_STEM_MAX_CIN 4
#define FM_STEM_MAX_COUT 128
#define FM_STEM_MAX_K 11
#define FM_STEM_MAX_STRIDE 4
#define FM_STEM_MAX_PAD 5
#define FM_LPIPS_SCORE_CHUNK 64
#define FM_LPIPS_SCORE_MAX_C 512
typedef struct fm_conv2d_stem_args {
    const void* img;
    const void* w;
    const void* bias;
    const void* mul;
    const void* add;
    void* out;
    int B, Cin, H, W, Cout, KH, KW, stride, pad;
    int ldw, ldo, relu, clamp, reserved;
    float lo, hi;
} fm_conv2d_stem_args;
int fm_conv2d_stem_f32(const fm_conv2d_stem_args* a, void* stream);
int fm_lpips_score_scratch(int B, int P);
int fm_lpips_score(const void* a, int lda, const void* b, int ldb, const void* w, int B, int P, int C, float eps, void* score, void* scratch, void* stream);

/* ---- LayerScale on the residual stream and the DINOv2 front end (csrc/layerscale.hip, csrc/dinov2.hip) ------------------------------
 * DINOv2's block is x = x + gamma1 * proj(attn(norm1(x))); x = x + gamma2 * mlp(norm2(x)) with learned per-channel gammas.  The arithmetic
 * of both sums is eager torch's: the product gamma[c] * float(delta) is rounded to fp32, then the sum is rounded to fp32 - never one fused
 * multiply-add - so x_out is the CPU's x + gamma * delta.float() bit for bit.
 * fm_layernorm_fwd_res_ls: fm_layernorm_fwd_res with gamma f32 (D) in front of the add: x_out = x + gamma[c] * float(delta) (delta bf16),
 *   y = LN(x_out) in one pass.  y, mean and rstd carry the bits fm_layernorm_fwd gives on that x_out; with gamma == 1 every output has the
 *   bits of fm_layernorm_fwd_res.  x_out may not alias x.  D % 4 == 0, D <= 2048, leading dims % 4 == 0 and >= D, delta and a bf16 y 8-byte
 *   aligned, every other pointer 16-byte aligned.
 * fm_layerscale_add: the same sum without the norm, delta bf16 or f32 (delta_is_f32; fp32 mode: the branch GEMM wrote it with FM_EPI_F32).
 *   x_out may be x itself (then ldx == ldxo).  D % 4 == 0 (no upper limit), leading dims and alignment as above.
 * fm_cls_pos_embed: the token assembly of DinoVisionTransformer.  patches bf16 or f32 (B G, ldp): patch-projection rows with the conv bias
 *   already added; cls f32 (D); reg f32 (n_reg, D) or NULL with n_reg == 0; pos f32 (1 + G, D): the position table of this patch grid.
 *   out f32 (B T, ldo), T = 1 + n_reg + G: row 0 of a sample = cls + pos[0], rows 1 .. n_reg = reg (no position), row 1 + n_reg + g =
 *   patch g + pos[1 + g].  One fp32 add per element, row-local.  D % 4 == 0, ldp, ldo % 4 == 0 and >= D, B T < 2^31.
 * Refused (-1) before anything is launched: null or misaligned pointers, sizes outside the ranges above.  One launch each, no allocation. */
int fm_layernorm_fwd_res_ls(const void* x, int ldx, const void* delta, int ldd, const void* gamma, void* x_out, int ldxo, const void* w,
                            const void* b, void* y, int ldy, int y_is_f32, void* mean, void* rstd, const int32_t* row_map, int R, int D,
                            float eps, void* stream);
int fm_layerscale_add(const void* x, int ldx, const void* delta, int ldd, int delta_is_f32, const void* gamma, void* x_out, int ldxo,
                      int R, int D, void* stream);
int fm_cls_pos_embed(const void* patches, int ldp, int patches_f32, const void* cls, const void* reg, int n_reg, const void* pos,
                     void* out, int ldo, int B, int G, int D, void* stream);

/* ---- lab(not part of the drop-in surface) ------------------------------------------------------------------------------------------
 * Experiment knobs of the GEMM kernels, used by tools/gemm_lab.cpp, the Python tools and the FOURM_NT3_LAB environment switch only: key 0 / 1
 * staggered workgroup start (groups, step), 2 gemm_nt3 mode override, 3 gemm_nt3 ablation flags (gemm_args.h NTArgs::lab), others reserved.
 * Process-global, not thread-safe, no effect on results except where an ablation flag says so.  Keys outside [0, 16) are ignored. */
void fm_lab_set(int key, int value);

#ifdef __cplusplus
}
#endif
#endif /* FOURM_HIP_H */
