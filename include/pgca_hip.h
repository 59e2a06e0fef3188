/*
 * pgca_hip.h - C ABI of libpgca_hip.so: the MI355X (gfx950) kernels behind the
 * Stage-1 NT-Xent and Stage-2 DPO steps of preference-guided captioning alignment.
 *
 * The reference (A-SHOJAEI/preference-guided-image-captioning-alignment) is 100 %
 * Python: it has no FFI of its own.  Its seam for this path is the Python surface
 * (models/model.py, models/components.py, training/trainer.py); each entry point
 * below names the reference call site whose ATen/cuBLAS/SDPA launches it replaces.
 * The binding a maintainer adds on the reference side is a ctypes stub - see
 * INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless
 *     stated otherwise; buffers are caller-owned (the Python host allocates them
 *     with torch's caching allocator and passes tensor.data_ptr()).
 *   - `stream` is a hipStream_t passed as void*; kernels are asynchronous on it,
 *     never allocate, never synchronise, keep no global mutable state except the
 *     thread-local last-error string.
 *   - bf16 = IEEE bfloat16 stored as uint16_t; f32 accumulation everywhere.
 *   - token ids / targets are int64 exactly as the reference supplies them.
 *   - return value: 0 on success, negative pgca_status otherwise.
 */
#ifndef PGCA_HIP_H
#define PGCA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum pgca_status {
  PGCA_OK = 0,
  PGCA_ERR_INVALID = -1, /* bad shape / alignment / null pointer */
  PGCA_ERR_LAUNCH = -2   /* hipLaunch failed; see pgca_last_error() */
} pgca_status;

#define PGCA_ABI_VERSION 306 /* bumped whenever a signature or struct layout below changes */
int pgca_version(void);        /* == PGCA_ABI_VERSION of the header the library was built from */
int pgca_sizeof_gemm_args(void); /* sizeof(pgca_gemm_args) as compiled: bindings compare it with their own layout */
const char* pgca_last_error(void);

/* ------------------------------------------------------------------ GEMM (MFMA bf16) */
/* Operand layouts.  "K" is the contraction dimension.
 *   PGCA_NT: A[M,K] row-major, B[N,K] row-major   (nn.Linear forward; dgrad through Conv1D)
 *   PGCA_NN: A[M,K] row-major, B[K,N] row-major   (GPT-2 Conv1D forward; dgrad through nn.Linear)
 *   PGCA_TN: A[K,M] row-major, B[K,N] row-major   (every weight gradient: X^t dY)
 * Constraints: lda/ldb multiples of 8 elements, base pointers 16-B aligned; for
 * operands whose contiguous dimension is K (A in NT/NN, B in NT) K % 8 == 0. */
enum { PGCA_NT = 0, PGCA_NN = 1, PGCA_TN = 2 };

/* Epilogues, applied to v = alpha*acc (+ bias[n]). */
enum {
  PGCA_EPI_NONE = 0,
  PGCA_EPI_GELU_NEW = 1,   /* GPT-2 MLP (modeling_gpt2.py:229-243); aux_out (opt.) <- pre-activation */
  PGCA_EPI_QUICK_GELU = 2, /* CLIP MLP (activations.py:117-123) */
  PGCA_EPI_RELU = 3,       /* projection heads (model.py:138,340) */
  PGCA_EPI_TANH = 4,       /* vision_projection (model.py:523) */
  PGCA_EPI_DGELU_NEW = 5,  /* v *= gelu_new'(aux_in[m,n]) (aux_in = saved pre-activation) */
  PGCA_EPI_DRELU = 6,      /* v *= aux_in[m,n] > 0       (aux_in = saved activation) */
  PGCA_EPI_DTANH = 7,      /* v *= 1 - aux_in[m,n]^2     (aux_in = saved activation) */
  PGCA_EPI_ROWSTATS = 8,   /* no C written: per-row partial (max, sum exp) over this block's columns
                              + target-logit pick; fused LM head / NT-Xent (model.py:1069-1079,988-998) */
  PGCA_EPI_DLOGITS = 9,    /* v = row_scale[m] * (exp(v - row_lse[m]) - (n == target[m])); 0 for n >= N;
                              aux_out (opt., bf16 [M, ld_aux]) <- bf16(v - bf16(v)): low half of a hi/lo split */
  PGCA_EPI_DQUICK_GELU = 10, /* v *= quick_gelu'(aux_in[m,n]) (aux_in = saved pre-activation; trainable CLIP tower) */
  /* The GPT-2 MLP pair that evaluates the sigmoid ONCE: the forward epilogue has it in registers for gelu_new and writes
   * gelu_new'(pre) beside the activation; the backward epilogue is then a plain multiply instead of exp + rcp + 8 FMAs
   * per element on the K = 1024 data-gradient GEMM whose epilogue was 40 % of its tile life. */
  PGCA_EPI_GELU_NEW_D = 11,  /* like GELU_NEW, but aux_out <- gelu_new'(pre-activation) (bf16) */
  PGCA_EPI_MUL_AUX = 12      /* v *= aux_in[m,n] (aux_in = the derivative saved by GELU_NEW_D); colsum_part allowed */
};

typedef struct pgca_gemm_args {
  const void* A;  /* bf16 */
  const void* B;  /* bf16 */
  int32_t M, N, K;
  int32_t lda, ldb;
  int32_t layout;
  int32_t epilogue;
  float alpha;            /* scale on the accumulator (1/tau for NT-Xent) */
  const float* bias;      /* [N] f32 or NULL */
  void* out_bf16;         /* [M, ld_out_bf16] or NULL */
  int32_t ld_out_bf16;
  float* out_f32;         /* [M, ld_out_f32] or NULL */
  int32_t ld_out_f32;
  int32_t accumulate;     /* out_f32 += v instead of = v (gradient accumulation) */
  const float* residual;  /* [M, ld_res] f32 added to v before the store, or NULL */
  int32_t ld_res;
  void* aux_out;          /* bf16 [M, ld_aux]: pre-activation written by *_GELU epilogues, or NULL */
  const void* aux_in;     /* bf16 [M, ld_aux]: operand of the D* epilogues */
  int32_t ld_aux;
  /* ROWSTATS / DLOGITS */
  const int64_t* targets; /* [M] column index per row, or NULL (NT-Xent: diagonal given explicitly) */
  float* stat_max;        /* [M, stat_ld]  partial row max   (ROWSTATS), one per 64-column strip */
  float* stat_sum;        /* [M, stat_ld]  partial sum exp(v - max) */
  int32_t stat_ld;        /* >= 2 * ceil(N / 128); both tile sizes write exactly columns [0, 2 * ceil(N / 128)) of a
                             row ((-inf, 0) for a strip wholly past N) and nothing beyond */
  float* target_val;      /* [M] v at the target column (ROWSTATS) */
  const float* row_lse;   /* [M] (DLOGITS) */
  const float* row_scale; /* [M] (DLOGITS) */
  int32_t out_cols;       /* DLOGITS: columns written (>= N, padding columns get 0) */
  /* fused dropout on the epilogue value (after the activation / derivative, before the residual add):
   * element (m, n) is multiplied by 0 or drop_scale according to pgca's counter hash of (drop_seed, m*N + n);
   * drop_threshold = p * 2^32, 0 disables.  Replaces nn.Dropout at model.py:139,341,524 and GPT-2 resid_dropout
   * (modeling_gpt2.py:224,242); the backward passes the same seed to replay the mask. */
  uint32_t drop_seed;
  uint32_t drop_threshold;
  float drop_scale;
  /* Optional, PGCA_EPI_DGELU_NEW / PGCA_EPI_MUL_AUX only: f32 [ceil(M/64), ld_colsum] - row b receives the column sums of the rows
   * 64b .. 64b+63 of the result (before its bf16 rounding); summed over b (pgca_colsum_finish) they are the bias gradient
   * of the layer whose pre-activation gradient this GEMM produces, without a second pass over the M x N result. */
  float* colsum_part;
  int32_t ld_colsum;
  /* Optional, packed (variable-length) token rows: drop_rows[m] is the row index the dropout hash is keyed on instead of m
   * (the token's position b*S + t in the PADDED [B, S] layout of the reference batch), so a packed launch draws exactly the
   * masks of the padded one.  int32 [M]; entries of padding rows may hold anything (their values are never used). */
  const int32_t* drop_rows;
} pgca_gemm_args;

int pgca_gemm_bf16(const pgca_gemm_args* args, void* stream);
/* Which kernel pgca_gemm_bf16 would launch for these arguments: schedule*1000000 + tile*100 + K-splits
 * (12801 = general 128^2 register-staged kernel; 256xx = 256^2 LDS-DMA tile with xx K-splits; schedule
 * 0 = 2-stage BK=64 loop (gemm256_kernel, default for the K-strided TN layout), 6 = phase-staggered 4-stage BK=32
 * loop (gemm256s_kernel, default for NT / NN)). */
int pgca_gemm_plan(const pgca_gemm_args* args);
/* Process-wide dispatch knobs (tests, micro-benchmarks, tuning).  Defaults come from the environment, read ONCE at
 * first use - no launch calls getenv:
 *   "gemm_tile"      0 automatic | 128 | 256                          (PGCA_GEMM_TILE)
 *   "gemm_schedule"  -1 automatic | 0 | 6 (see pgca_gemm_plan)         (PGCA_GEMM_RING)
 *   "gemm_group"     1 grouped launches (weight gradients, forward pair) | 0 one by one  (PGCA_GEMM_NO_GROUP=1 -> 0)
 *   "gemm_pair_order" tile order of a paired launch: 0 problem after problem | 1 alternating by 8-row-tile group
 *   "gemm_stagger"   0..64: start-delay step (x 1024 clocks) of the first wave of workgroups of a many-round
 *                    gemm256s launch, which de-phases the CUs' epilogue store bursts   (PGCA_GEMM_STAGGER)
 * Returns PGCA_ERR_INVALID for an unknown name or value. */
int pgca_set_option(const char* name, int32_t value);
/* `count` GEMMs in one launch.  Up to four TN problems with epilogue NONE and an f32 (accumulating) output - the four
 * weight gradients of one GPT-2 block (autograd of Conv1D c_attn / c_proj / c_fc / mlp.c_proj, reference
 * modeling_gpt2.py:203,222-224,229-243 under trainer.py:494,606 loss.backward()) - run as ONE grid with the whole K per
 * tile: no split-K, no atomics.
 * TWO NT or two NN problems of the same layout, M, N and K that would each run the phase-staggered 256^2 tile without a
 * K split, with forward epilogues (NONE .. TANH, GELU_NEW_D) - the same layer of the policy and of the frozen reference
 * policy (the four forwards of a DPO step, trainer.py:575-628) - run as ONE grid of 2 x tiles workgroups; each problem
 * keeps its whole pgca_gemm_args (operands,
 * epilogue, bias, residual, outputs, dropout) and every tile computes exactly what it computes in a launch of its own
 * (same k order, same epilogue code: bit-identical outputs), while the two part-filled last rounds of 256 workgroups
 * become one.  Anything else falls back to `count` ordinary pgca_gemm_bf16 launches. */
int pgca_gemm_bf16_grouped(const pgca_gemm_args* args, int32_t count, void* stream);

/* Skinny product for incremental decoding (generation with a K/V cache: reference models/model.py:657-675 -> HF generate,
 * modeling_gpt2.py:144-226 with layer_past): y[M, N] = epilogue(x[M, K] . W[K, N]) for 1 <= M <= PGCA_SKINNY_MAX_M rows,
 * W row-major [K, N] (GPT-2 Conv1D), one pass over W spread over every CU (column chunks x K splits, each storing its partial
 * [M, N] slab in `scratch`), then a per-row finish that sums the slabs in a fixed order (bitwise reproducible):
 * v = acc + bias[n]; act (PGCA_EPI_NONE | PGCA_EPI_GELU_NEW); + residual[m, n];
 * out_f32 / out_bf16 (either or both, arbitrary row strides - e.g. a K/V-cache row); optionally the LayerNorm of the finished
 * f32 row (ln_gamma/ln_beta/ln_eps -> ln_out_bf16 [M, ld_ln]: the operand of the next product, no separate LN launch).
 * scratch: pgca_gemm_skinny_workspace(M, N, K) bytes (16-B aligned), contents irrelevant on entry.
 * Constraints: N % 8 == 0, N <= 8192, ldw % 8 == 0, pointers 16-B aligned, row strides multiples of 4 elements. */
#define PGCA_SKINNY_MAX_M 64
typedef struct pgca_skinny_args {
  const void* x;   /* bf16 [M, lda] */
  const void* W;   /* bf16 [K, ldw] */
  int32_t M, N, K, lda, ldw;
  float* scratch;
  const float* bias;      /* [N] or NULL */
  int32_t act;
  const float* residual;  /* f32 [M, ld_res] or NULL */
  int32_t ld_res;
  float* out_f32;
  int32_t ld_out_f32;
  void* out_bf16;
  int32_t ld_out_bf16;
  const float* ln_gamma;
  const float* ln_beta;
  float ln_eps;
  void* ln_out_bf16;      /* NULL: no fused LayerNorm */
  int32_t ld_ln;
} pgca_skinny_args;
int pgca_gemm_skinny(const pgca_skinny_args* args, void* stream);
int64_t pgca_gemm_skinny_workspace(int32_t M, int32_t N, int32_t K);
int pgca_sizeof_skinny_args(void);

/* Per-row combine of ROWSTATS partials: lse[m] = log sum exp over all columns;
 * out_logprob[m] = target_val[m] - lse[m] (token log-prob, reference model.py:1074-1079). */
int pgca_rowstats_combine(const float* stat_max, const float* stat_sum, int32_t stat_ld, int32_t nparts,
                          const float* target_val, int32_t M, float* lse, float* out_logprob, void* stream);

/* ------------------------------------------------------------------ LayerNorm */
/* y = LN(x) * gamma + beta, eps as given (1e-5 everywhere in the reference).
 * x f32 [rows_in, H]; optional row_map[M] gathers rows (y row m <- x row row_map[m]);
 * y_bf16 / y_f32 [M, H] (either may be NULL); mean/rstd [M] saved for backward (may be NULL).
 * Replaces F.layer_norm at model.py:141,343,535,601 and HF ln_1/ln_2/ln_f, CLIP layer_norm*. */
int pgca_layernorm_fwd(const float* x, const int32_t* row_map, int32_t M, int32_t H, const float* gamma,
                       const float* beta, float eps, void* y_bf16, float* y_f32, float* mean, float* rstd,
                       void* stream);

/* dx = LN backward; dy given as bf16 (dy_bf16) or f32 (dy_f32), exactly one non-NULL.
 * dx_out[row] = (add_to ? add_to[row] : 0) + dx   with row = row_map ? row_map[m] : m.
 * dx_bf16 (optional) receives the same value rounded to bf16 (operand of the next dgrad GEMM).
 * dgamma/dbeta partial sums go to part[2, nblk, H] (nblk returned by pgca_layernorm_bwd_blocks);
 * pgca_colsum_finish folds them into the gradient buffers.  part_extra[2, nblk, H] (optional) receives the column
 * sums of add_to and of dx_out - the bias gradients of the two GEMMs around this LayerNorm, for free.
 * drop_add / drop_dx (HOST pointers to {seed, threshold, scale-as-float-bits}, or NULL) replay the dropout masks of
 * those two GEMM outputs: the add_to column sum uses drop_add; dx_bf16 and the dx column sum use drop_dx (dx_out
 * itself, the f32 residual-stream gradient, is never masked).  drop_rows (optional, int32 [rows]): the row index the two
 * dropout hashes are keyed on (see pgca_gemm_args::drop_rows; packed token rows). */
int pgca_layernorm_bwd_blocks(int32_t M);
int pgca_layernorm_bwd(const void* dy_bf16, const float* dy_f32, const float* x, const int32_t* row_map,
                       int32_t M, int32_t H, const float* gamma, const float* mean, const float* rstd,
                       const float* add_to, float* dx_out, void* dx_bf16, float* part, float* part_extra,
                       const uint32_t* drop_add, const uint32_t* drop_dx, const int32_t* drop_rows, void* stream);
/* out[h] (+)= sum_b part[b, h]; nparts rows of length H. */
int pgca_colsum_finish(const float* part, int32_t nparts, int32_t H, float* out, int32_t accumulate, void* stream);

/* Same for up to four planes part[plane][nparts][H] -> out0..out3 in one launch. */
int pgca_colsum_finish4(const float* part, int32_t nplanes, int32_t nparts, int32_t H, float* out0, float* out1,
                        float* out2, float* out3, int32_t accumulate, void* stream);

/* Column sums of a bf16 / f32 matrix (bias gradients): out[n] (+)= sum_m x[m, n]. */
int pgca_colsum_blocks(int32_t M);
int pgca_colsum(const void* x_bf16, const float* x_f32, int32_t M, int32_t N, int32_t ld, float* part, void* stream);

/* ------------------------------------------------------------------ attention (head_dim 64) */
/* qkv bf16 [B*S, 3*H] (q | k | v, head h at columns h*64), out bf16 [B*S, H], lse f32 [B, heads, S].
 * softmax(q k^t / 8 + mask) v with mask = causal AND key_mask[b, key] != 0 (key_mask int32 [B,S] or NULL).
 * Any S in the forward (one on-chip tile up to 128, key-tiled online softmax beyond); the backward keeps the dQ
 * accumulators of every 128-query block in registers: S <= PGCA_ATTN_MAX_S.  B <= 65535.
 * Replaces SDPA at modeling_gpt2.py:54-72,203-215 and modeling_clip.py:259-277.
 * Packed (variable-length) rows: with cu_seqlens (int32 [B+1], cu[0] = 0) sequence b occupies rows cu[b] .. cu[b+1]-1 of
 * qkv / out / dout / dqkv and has min(cu[b+1]-cu[b], S) tokens (a KV-cache decode step passes the cache stride in cu and
 * the filled length as S, with no mask, lse or dropout); in training S stays the PADDED length: key_mask, lse and the dropout index
 * keep their [B, S] geometry, so the result of every real token equals the padded launch's.  Padding positions of the
 * reference batch (model.py:1069-1083 zeroes their loss terms, :449-456 their pooling weight) are then never computed.
 * What is written: every row of out / dqkv that belongs to a sequence (packed: rows cu[b] .. cu[b] + len - 1, the filler
 * pseudo-sequences included; padded: all B*S rows, padding positions too) and the lse slots [b, h, t] with t < len; lse
 * slots beyond a packed sequence's length and rows outside every sequence are NEVER touched.
 * A query with NO allowed key (key_mask zero at every key up to the causal edge, e.g. a hole at position 0) gets
 * out = 0, lse = -inf and carries no gradient: its dq row is 0 and it adds nothing to dk / dv - the same in the one-tile
 * forward, the key-tiled forward and the backward.  (The reference's additive finfo.min bias would average ALL S keys
 * for such a row; right-padded captions, model.py:1069-1083, never contain one.) */
#define PGCA_ATTN_MAX_S 512
int pgca_attention_fwd(const void* qkv, const int32_t* key_mask, int32_t B, int32_t S, int32_t heads,
                       int32_t causal, void* out, float* lse, uint32_t drop_seed, uint32_t drop_threshold,
                       float drop_scale, const int32_t* cu_seqlens, void* stream);
/* dqkv bf16 [B*S, 3*H] from dout bf16 [B*S, H], the saved qkv / out / lse.  drop_*: attention-probability
 * dropout (element index ((b*heads + h)*S + q)*S + key; threshold 0 disables), replayed in the backward. */
int pgca_attention_bwd(const void* qkv, const void* out, const void* dout, const float* lse,
                       const int32_t* key_mask, int32_t B, int32_t S, int32_t heads, int32_t causal,
                       void* dqkv, uint32_t drop_seed, uint32_t drop_threshold, float drop_scale,
                       const int32_t* cu_seqlens, void* stream);
/* The same arguments, contract and results for 1 <= S <= PGCA_ATTN_SPLIT_MAX_S (GPT-2's 1024 positions; nothing longer is
 * tested): the work is split by role - one workgroup per (head, sequence, 128-key block) sweeps the query blocks for dK /
 * dV, one per (head, sequence, 128-query block) sweeps the key blocks for dQ - so a workgroup holds one block's
 * accumulators whatever S is.  Nothing is summed across workgroups: no atomics, no workspace, bitwise reproducible, and
 * every element is summed in pgca_attention_bwd's order (bit-identical to it wherever both run).  7 matmuls per
 * (key, query) pair instead of 5.  Both roles run in one grid. */
#define PGCA_ATTN_SPLIT_MAX_S 1024
int pgca_attention_bwd_split(const void* qkv, const void* out, const void* dout, const float* lse,
                             const int32_t* key_mask, int32_t B, int32_t S, int32_t heads, int32_t causal,
                             void* dqkv, uint32_t drop_seed, uint32_t drop_threshold, float drop_scale,
                             const int32_t* cu_seqlens, void* stream);

/* ------------------------------------------------------------------ embeddings */
/* Caption-decoder input (reference model.py:591-601 + modeling_gpt2.py:571-577):
 *   e = wte[ids[b,s]] + attended[b]; x = LN(e; attention_norm); h0[b,s] = x + wpe[s]
 * attended[b] = W_o(W_v pv_b + b_v) + b_o is the collapsed 1-key cross-attention.
 * Text tower (modeling_gpt2.py:568-577): attended == NULL and gamma == NULL -> h0 = wte[id] + wpe[s].
 * mean/rstd [B*S] saved when LN is applied. ids int64. */
/* Train-mode extras (all optional): attended is read at row b*att_stride (0 = one shared vector, i.e. b_o);
 * U [B, xheads, H] adds sum_h w(b,h,s) U[b,h,:] with w the replayable dropout multiplier of the 1-key
 * attention weight (drop_x, index (b*xheads + h)*S + s); drop_e is GPT-2's embedding dropout on h0
 * (index m*H + c).  drop_* are HOST pointers to {seed, threshold, scale bits} or NULL.
 * Packed rows: with row_ids (int32 [n_rows]) output row r (and mean/rstd[r]) is position m = row_ids[r] = b*S + t of the
 * padded batch (ids, positions and every dropout index stay keyed on m); row_ids[r] < 0 marks a filler row, written as
 * zeros.  Without row_ids n_rows is ignored and all B*S rows are produced. */
int pgca_embed_fwd(const int64_t* ids, int32_t B, int32_t S, int32_t H, const float* wte, const float* wpe,
                   const float* attended, const float* gamma, const float* beta, float eps, float* h0,
                   float* mean, float* rstd, int32_t att_stride, const float* U, int32_t xheads,
                   const uint32_t* drop_x, const uint32_t* drop_e, const int32_t* row_ids, int32_t n_rows,
                   void* stream);
/* Backward of the above given g = dL/dh0 [B*S, H] (f32):
 *   dwpe[s] += sum_b g; through LN (if gamma) -> de; dwte[ids] += de (rows with row_mask==0 skipped:
 *   their gradient is exactly zero); dattended[b] = sum_s de; dgamma/dbeta partials in part[2,nblk,H].
 * Packed rows: with cu_seqlens (int32 [B+1]) g, mean and rstd hold position (b, s) at row cu[b] + s, s < cu[b+1]-cu[b];
 * positions beyond a sequence's packed length contribute nothing (they are padding: row_mask is 0 there). */
int pgca_embed_bwd(const float* g, const int64_t* ids, const int32_t* row_mask, int32_t B, int32_t S, int32_t H,
                   const float* wte, const float* attended, const float* gamma, const float* mean,
                   const float* rstd, float* dwte, float* dwpe, float* dattended, float* part, int32_t att_stride,
                   const float* U, float* dU, int32_t xheads, const uint32_t* drop_x, const uint32_t* drop_e,
                   const int32_t* cu_seqlens, void* stream);
int pgca_embed_bwd_blocks(int32_t B, int32_t S);

/* ViT patch gather (modeling_clip.py:200-218): pixels f32 [B,3,I,I] -> bf16 [B*G*G, ld_out] in the
 * (c, ky, kx) order of the conv weight, so the bias-free Conv2d is one NT GEMM.  ld_out >= 3*P*P; columns
 * 3*P*P..ld_out-1 are written as zeros (ViT-L/14: 588 -> 640, K of the GEMM padded to its 64-deep tile).  P even. */
int pgca_patchify(const float* pixels, int32_t B, int32_t image, int32_t patch, int32_t ld_out, void* out_bf16,
                  void* stream);
/* x[b, 0] = cls + pos[0]; x[b, 1+p] = patches[b, p] + pos[1+p]  (f32 [B, T, H]). */
int pgca_vit_assemble(const float* patch_embeds, const float* cls, const float* pos, int32_t B, int32_t T,
                      int32_t H, float* x, void* stream);
/* Backward of pgca_vit_assemble for a trainable tower (reference model.py:150-164 leaves the CLIP tower trainable unless
 * freeze_vision_backbone): dx f32 [B, T, H] -> dpatch bf16 [B, T-1, H] (operand of the patch-embedding weight gradient),
 * dpos[t] += sum_b dx[b, t], dcls += sum_b dx[b, 0]  (both ACCUMULATE, like every parameter gradient). */
int pgca_vit_assemble_bwd(const float* dx, int32_t B, int32_t T, int32_t H, void* dpatch_bf16, float* dcls,
                          float* dpos, void* stream);

/* Image input transform of the reference's loader on the device (data/preprocessing.py:44-48,78: Resize((S, S)) ->
 * ToTensor -> Normalize on a PIL RGB image), BIT-EXACT with the host path: images u8 [B, H, W, 3]
 * (decoded RGB, HWC) -> Pillow's two-pass antialiased bilinear resample on 8-bit channels (22-bit fixed-point taps,
 * round half up and clip after EACH pass; Resample.c) -> float32(v) / 255 -> (t - mean) / std -> out f32 [B, 3, S, S].
 * x/ybounds int32 [S, 2] = (first tap, tap count), x/ycoef int32 [S, xk / yk]: Pillow's precompute_coeffs +
 * normalize_coeffs_8bpc for W -> S and H -> S (host side: pgca_amd.input.resample_tables).  tmp u8 [B, H, S, 3] is the
 * intermediate of the horizontal pass; resized_u8 (optional) u8 [B, S, S, 3] receives the resized image itself. */
int pgca_image_preprocess(const uint8_t* images, int32_t B, int32_t H, int32_t W, int32_t S, const int32_t* xbounds,
                          const int32_t* xcoef, int32_t xk, const int32_t* ybounds, const int32_t* ycoef, int32_t yk,
                          float mean0, float mean1, float mean2, float std0, float std1, float std2, uint8_t* tmp,
                          uint8_t* resized_u8, float* out, void* stream);

/* TRAINING transform of the reference's loader on the device (data/preprocessing.py:52-70, augment=True:
 * RandomResizedCrop(S, scale (0.8, 1), ratio (0.75, 1.33)) -> RandomHorizontalFlip -> ColorJitter(0.2, 0.2, 0.2, 0.1) ->
 * RandomRotation(5) -> ToTensor -> Normalize), BIT-EXACT with torchvision's PIL backend GIVEN the random draws, which
 * stay on the host (pgca_amd.input.draw_train_params restates torchvision's get_params).  Per image b:
 *   params int32 [B, PGCA_TRAIN_PARAM_INTS]: crop box i, j, h, w (top, left, height, width; inside the H x W image) | flip 0/1 |
 *     the four ColorJitter operations in their drawn order (0 brightness, 1 contrast, 2 saturation, 3 hue) |
 *     hue turn = uint8(hue_factor * 255) | rotate 0/1 (0: angle % 360 == 0, PIL copies) |
 *     a0 a1 a2 a3 a4 a5: Geometry.c affine_fixed's 16.16 integers of the output->input map | 3 unused;
 *   factors f32 [B, 3]: brightness, contrast, saturation (Blend.c alpha);
 *   x/ybounds int32 [B, S, 2], x/ycoef int32 [B, S, xk / yk]: resample taps for w_b -> S and h_b -> S (rows padded with
 *     zeros to the batch's widest table).
 * tmp u8 [B, H, S, 3] and resized_u8 u8 [B, S, S, 3] are scratch (the latter returns the cropped + resized image);
 * aug_u8 (optional) u8 [B, S, S, 3] receives the augmented image before ToTensor; out f32 [B, 3, S, S].
 * The jitter + rotation stage keeps one S x S x 3 image in LDS: S <= 230 (every shipped config uses 224). */
#define PGCA_TRAIN_PARAM_INTS 20 /* int32 values per image in `params` */
int pgca_image_train_transform(const uint8_t* images, int32_t B, int32_t H, int32_t W, int32_t S, const int32_t* params,
                               const float* factors, const int32_t* xbounds, const int32_t* xcoef, int32_t xk,
                               const int32_t* ybounds, const int32_t* ycoef, int32_t yk, float mean0, float mean1,
                               float mean2, float std0, float std1, float std2, uint8_t* tmp, uint8_t* resized_u8,
                               uint8_t* aug_u8, float* out, void* stream);

/* ------------------------------------------------------------------ sequence reduce + losses */
/* tok_lp f32 [nrows] are token log-probs of the COMPACT rows; row r belongs to sequence seq_of_row[r].
 * seq_lp[q] = sum (mode 0; components.py:357-362) or mean over the sequence's scored tokens
 * (mode 1; model.py:1082-1083; 0/0 = NaN when a caption has <= 1 real token, as the reference). */
int pgca_seq_reduce(const float* tok_lp, const int32_t* seq_of_row, int32_t nrows, int32_t nseq,
                    const int32_t* seq_count, int32_t mode, float* seq_lp, void* stream);
/* Token log-probs from MATERIALISED f32 logits (API-compatibility path of PreferenceLoss /
 * compute_sequence_logprobs, model.py:1069-1079, components.py:340-354):
 * out[r] = logits[row_map[r], targets[r]] - logsumexp(logits[row_map[r], 0:V]). */
int pgca_logits_logprob(const float* logits, int32_t ld, int32_t V, const int32_t* row_map, const int64_t* targets,
                        int32_t R, float* out, void* stream);
/* Backward of pgca_logits_logprob for callers that hold materialised logits WITH a gradient (the reference's loss objects
 * are differentiated by autograd: model.py:1069-1083, components.py:340-362): for each compact row r,
 * dlogits[row_map[r], 0:V] = g[r] * (onehot(targets[r]) - softmax(logits[row_map[r], 0:V])), g[r] = dLoss/d tok_lp[r];
 * rows that score no token are not written (the caller zero-fills dlogits). */
int pgca_logits_logprob_bwd(const float* logits, int32_t ld, int32_t V, const int32_t* row_map, const int64_t* targets,
                            const float* g, int32_t R, float* dlogits, void* stream);
/* DPO / preference loss over B pairs (components.py:210-231, model.py:1047-1048).
 * pol_w/pol_l/ref_w/ref_l f32 [B] (ref_* may be NULL = reference-free).
 * loss[0] = mean loss; dpol_w/dpol_l [B] = dLoss/dpol (f32), all zero when the loss is not finite (the reference skips
 * such a batch, trainer.py:606-613); metrics[4] = reward_margin, reward_accuracy, mean pol_w, mean pol_l
 * (components.py:234-247), all on device (no host sync). */
int pgca_dpo_loss(const float* pol_w, const float* pol_l, const float* ref_w, const float* ref_l, int32_t B,
                  float beta, float label_smoothing, float* loss, float* dpol_w, float* dpol_l, float* metrics,
                  void* stream);
/* The index work of the log-prob gather on the device (reference model.py:1069-1083, components.py:340-357: shift,
 * mask product, gather index), replacing the host pass of a collate function: for ids / mask int64 [Bq, S] keeps the
 * rows (b, t) with mask[b, t+1] != 0, sorted by sequence: row_map[r] = b*S + t, targets[r] = ids[b, t+1] (bit-exact),
 * seq_of_row[r] = b (each of capacity Bq*(S-1)); counts[b] = kept rows of sequence b; n_rows[0] = total;
 * mask32 (optional) = int32 0/1 copy of the mask (key mask of pgca_attention_*). */
int pgca_seq_batch_prepare(const int64_t* ids, const int64_t* mask, int32_t Bq, int32_t S, int32_t* counts,
                           int32_t* mask32, int32_t* row_map, int64_t* targets, int32_t* seq_of_row, int32_t* n_rows,
                           void* stream);
/* Packed (variable-length) row layout of a right-padded batch: only positions t < len[b] = 1 + (last t with mask[b,t] != 0)
 * are given a row, sequence after sequence (reference semantics: with a causal AND key-padding mask, a masked mean and a
 * masked loss - model.py:449-456,1069-1083, SURVEY 3.1 items 6-7 - nothing a padded position computes reaches a loss term or
 * a gradient).  With F = ceil((pad_to - 1) / S) filler pseudo-sequences (1 whenever S >= pad_to - 1):
 * mask32 int32 [Bq+F, S]: rows 0..Bq-1 as written by pgca_seq_batch_prepare; rows Bq.. are SET TO ONES here.
 *   lens[Bq]: the packed length of every sequence;
 *   cu[Bq+F+1]: cu[b] = first row of sequence b, cu[Bq] = n = sum len, cu[Bq+F] = n rounded up to a multiple of pad_to;
 *             rows cu[Bq]..cu[Bq+F]-1 are filler (extra unmasked "sequences" of zero embeddings, at most S rows each so
 *             that they obey the attention kernels' length bound) that keeps the row count a multiple of the GEMM K
 *             tile for the weight gradients;
 *   row_ids[cap]: row_ids[cu[b] + t] = b*S + t; filler rows get -1  (cap >= Bq*S rounded up to pad_to);
 *   n_packed[2] = {n, n rounded up};
 *   row_map (optional, in place, with counts from pgca_seq_batch_prepare): b*S + t  ->  cu[b] + t for the compact rows. */
int pgca_seq_pack_prepare(int32_t* mask32, int32_t Bq, int32_t S, int32_t pad_to, int32_t* lens, int32_t* cu,
                          int32_t* row_ids, int32_t* n_packed, const int32_t* counts, int32_t* row_map, void* stream);
/* row_scale[r] = +-dseq[seq_of_row[r]] * (mode & 1 ? 1/count : 1): dLoss/d tok_lp per compact row; mode & 2 negates
 * (the DLOGITS epilogue computes the cross-entropy form softmax - onehot, so it is fed -dLoss/dtok_lp). */
int pgca_row_scale(const float* dseq, const int32_t* seq_of_row, const int32_t* seq_count, int32_t nrows,
                   int32_t mode, float* row_scale, void* stream);
/* Language-model loss head over the compact rows (reference CaptionDecoder.forward(labels=...), model.py:561-619: HF's
 * ForCausalLMLoss, here over the scored tokens).  Row r counts iff seq_of_row == NULL or seq_of_row[r] < seq_limit; with
 * n counted rows, loss[0] = -(sum of the counted tok_lp) / n (n == 0: 0/0 = NaN, as the mean of pgca_seq_reduce).
 * metrics[4] (optional) = {sum of -tok_lp, n, loss, 1 if the loss is finite else 0}, all on the device (no host sync).
 * row_coef[nrows] (optional) = -dLoss/d tok_lp * grad_scale, the form the DLOGITS epilogue takes (pgca_row_scale with
 * mode bit 2): grad_scale / n on counted rows, 0 elsewhere.  accumulate 0 writes every element (all exactly 0 when the
 * loss is not finite, the rule of pgca_dpo_loss); accumulate 1 adds to the counted rows (nothing when it is not finite).
 * One workgroup; the sum is carried in double in a fixed order (two launches on one input are bitwise equal) and the
 * loss is rounded to f32 once.  LIMIT: sized for the compact rows of one micro-batch, nrows up to ~1e5 (12 us at 36 k
 * rows on an MI355X); the one workgroup makes two serial passes, so time grows linearly with nrows and nothing is spread
 * over the other CUs - a caller with millions of rows needs a different kernel, not this entry.  tok_lp is read in 16-byte vectors from its first 16-byte boundary when seq_of_row is
 * aligned at the same row, else row by row; any nrows >= 1. */
int pgca_token_nll(const float* tok_lp, const int32_t* seq_of_row, int32_t seq_limit, int32_t nrows, float grad_scale,
                   int32_t accumulate, float* loss, float* row_coef, float* metrics, void* stream);

/* ------------------------------------------------------------------ preference-pair mining (Stage-2 data from the model) */
/* The four steps between the ids that best-of-N sampling returns and a finished Stage-2 batch (reference
 * data/loader.py:416-451, UltraFeedbackDataset._process_scored_captions, applied to the model's own captions).  One wave
 * per candidate row or per image, no atomics, fixed-order sums: two launches on one input are bitwise equal.  Every
 * output is written in full.
 *
 * Generated ids -> training rows and scorer rows.  cand int64 [R, ld_cand] in the DECODER's vocabulary (base_vocab
 * ordinary ids, then [PAD] [BOS] [EOS]), lengths int64 [R] = generated tokens with [EOS]; len_r = min(lengths[r],
 * ld_cand, S) (a negative length counts as 0).
 *   dec_ids / dec_mask int64 [R, S]: cand[r, t] / 1 for t < len_r, else dec_pad / 0;
 *   text_ids int64 / text_mask int32 [R, S]: the tokens with 0 <= id < base_vocab, in order, compacted to the left, then
 *     text_pad / 0 - the decoder's special ids never reach the text tower, whose table ends at base_vocab + 2;
 *   text_len int32 [R] = kept tokens; out_len int32 [R] = len_r.
 * A row with an id outside [0, dec_vocab) in its first len_r columns is unusable: text_len = -1, out_len = 0, both rows
 * all pad with mask 0. */
int pgca_candidate_rows(const int64_t* cand, int32_t ld_cand, const int64_t* lengths, int32_t R, int32_t S,
                        int32_t base_vocab, int32_t dec_vocab, int64_t dec_pad, int64_t text_pad, int64_t* dec_ids,
                        int64_t* dec_mask, int64_t* text_ids, int32_t* text_mask, int32_t* text_len, int32_t* out_len,
                        void* stream);
/* score[b*n + j] = <img_b, txt_(bn+j)> / (max(|img_b|, 1e-12) * max(|txt_(bn+j)|, 1e-12)): F.normalize (model.py:828-829)
 * of both sides, then the dot product, in f32.  img f32 [B, P], txt f32 [B*n, P] (un-normalised), any P >= 1. */
int pgca_group_cosine(const float* img, const float* txt, int32_t B, int32_t n, int32_t P, float* score, void* stream);
/* The pairing rule, one wave per image, 1 <= n <= 64.  score f32 [B, n]; dec_ids [B*n, S] / out_len [B*n] as written by
 * pgca_candidate_rows; ok (optional) uint8 [B, n].  Candidate j is LEFT OUT when its score is not finite, ok is 0,
 * out_len < min_tokens, or an earlier candidate i < j of the image has the same out_len and the same ids.  The rest are
 * ranked by score descending, equal scores by ascending j (Python's stable sort(reverse=True), loader.py:435):
 * rank int32 [B, n], -1 when left out.  rule 0 ("adjacent", the reference's): for k = 0 .. kept-2, d = s[rank k] -
 * s[rank k+1] in f32, a pair (winner, loser, d) iff d >= threshold, in k order.  rule 1 ("best_worst"): at most one
 * pair, first rank against last, same test.  pair_win / pair_lose int32 and pair_margin f32 [B, n] hold candidate
 * indices within the image (unused slots: -1, -1, 0); pair_count int32 [B]. */
int pgca_mine_pairs(const float* score, const int64_t* dec_ids, const int32_t* out_len, const uint8_t* ok, int32_t B,
                    int32_t n, int32_t S, int32_t min_tokens, int32_t rule, float threshold, int32_t* rank,
                    int32_t* pair_win, int32_t* pair_lose, float* pair_margin, int32_t* pair_count, void* stream);
/* Batch assembly: pair p of image b lands at row sum(pair_count[0 .. b)) + p (images ascending: the reference's
 * `extend` order); every workgroup sums the counts before its image itself.  For the first n_pairs rows
 * preferred_* / rejected_* int64 [cap, S] are the winner's / loser's dec_ids and dec_mask rows, pair_image int32 [cap]
 * = b, preference_score f32 [cap] = the margin (loader.py:448); n_pairs int32 [1].  Rows n_pairs .. cap-1: dec_pad,
 * mask 0, pair_image -1, score 0.  cap >= max(1, B * (n - 1)). */
int pgca_pair_rows(const int32_t* pair_win, const int32_t* pair_lose, const float* pair_margin,
                   const int32_t* pair_count, const int64_t* dec_ids, const int64_t* dec_mask, int32_t B, int32_t n,
                   int32_t S, int32_t cap, int64_t dec_pad, int64_t* preferred_ids, int64_t* preferred_mask,
                   int64_t* rejected_ids, int64_t* rejected_mask, int32_t* pair_image, float* preference_score,
                   int32_t* n_pairs, void* stream);

/* ------------------------------------------------------------------ caption metrics over token ids */
/* The reference's evaluation formulas (evaluation/metrics.py) with a base-vocabulary token id in the place of a word.
 * Inputs are STRIPPED rows: ids int64 [.., S] as pgca_candidate_rows writes text_ids (0 <= id < base_vocab in the first
 * len columns), len int32 (a reference with len -1 is ABSENT, with len 0 present and empty; a len above S counts as S,
 * a negative prediction length as 0).  One 64-lane workgroup per image, no atomics, loops bounded by S, K and a 32-step
 * search, fixed-order sums: two launches on one input are bitwise equal.  Like BLEU and CIDEr here, ROUGE and METEOR over
 * BPE ids are not comparable with their word-level namesakes.  Limits, checked before any launch:
 * 1 <= S <= PGCA_EVAL_MAX_S, 1 <= K <= PGCA_EVAL_MAX_K, 1 <= base_vocab <= PGCA_EVAL_MAX_VOCAB, images (rows, groups)
 * 1 .. PGCA_EVAL_MAX_IMAGES - 1, no null pointer.
 *
 * An n-gram of order n <= 4 is the int64 KEY of its ids at 16 bits each, the first id most significant; the orders are
 * kept apart, so keys of different orders never meet.  base_vocab <= 65535 leaves the field 0xffff unused and -1 free
 * as "no n-gram here".  A key whose leading id is >= 32768 is negative: tables are sorted in SIGNED order (torch.sort on
 * int64) and searched in it. */
#define PGCA_EVAL_MAX_S 128
#define PGCA_EVAL_MAX_K 8
#define PGCA_EVAL_MAX_VOCAB 65535
#define PGCA_EVAL_MAX_IMAGES 16777216
/* keys_out int64 [G, K, S]: the key of the n-gram of `order` starting at each column, -1 where there is none.
 * distinct_per_group != 0: a key is written only at its first occurrence in the group (all K rows of image g, row
 * major) and -1 at the later ones - the reference's once-per-image document frequency (metrics.py:489-501). */
int pgca_ngram_keys(const int64_t* ids, const int32_t* len, int32_t G, int32_t K, int32_t S, int32_t order,
                    int32_t base_vocab, int32_t distinct_per_group, int64_t* keys_out, void* stream);
/* _compute_cider (metrics.py:463-572) per image, in float64.  table_keys / table_df int64 [table_len]: per order the
 * sorted distinct keys of the corpus and their document frequencies, order n in [table_off[n-1], table_off[n])
 * (table_off int64 [5], on the device; offsets are clamped to table_len).  Per order 1..4: prediction counts pc,
 * reference counts rc = sum over present references of count / K_present, idf = log(n_docs / (df + 1e-8)) with df = 1
 * for a key the table lacks; num = sum pc idf rc idf, pn = sum (pc idf)^2, rn = sum (rc idf)^2 over the n-grams of
 * either side; sim = num / sqrt(pn rn) when pn > 0 and rn > 0, else 0.  score = mean of the four sims times
 * exp(-(pred_len - mean ref_len)^2 / (2 sigma^2)) (0 when the mean is 0).  score_out FLOAT64 [N] (the x10 and the corpus
 * mean are the caller's); flag_out int32 [N] = 1 and score 0 for an image with no present reference, else 0. */
int pgca_cider_rows(const int64_t* pred_ids, const int32_t* pred_len, const int64_t* ref_ids, const int32_t* ref_len,
                    int32_t N, int32_t K, int32_t S, int32_t base_vocab, const int64_t* table_keys,
                    const int64_t* table_df, const int64_t* table_off, int64_t table_len, int32_t n_docs, float sigma,
                    void* score_out, int32_t* flag_out, void* stream);
/* stats_out int64 [N, 10]: clipped matches of orders 1..4 (sum over the distinct n-grams of the prediction of
 * min(prediction count, max over references of reference count)), possible matches max(0, pred_len - n + 1) of orders
 * 1..4, pred_len, and the MINIMUM length over the present references (0 when none is). */
int pgca_bleu_stats(const int64_t* pred_ids, const int32_t* pred_len, const int64_t* ref_ids, const int32_t* ref_len,
                    int32_t N, int32_t K, int32_t S, int32_t base_vocab, int64_t* stats_out, void* stream);
/* out int32 [R, 2] = |set(a_r) & set(b_r)|, |set(a_r) | set(b_r)| over the ids of the first len columns (the integers
 * of the reference's Jaccard similarity, metrics.py:638-661; the caller divides). */
int pgca_token_overlap(const int64_t* a_ids, const int32_t* a_len, const int64_t* b_ids, const int32_t* b_len,
                       int32_t R, int32_t S, int32_t* out, void* stream);
/* The integers of ROUGE-1 / ROUGE-2 / ROUGE-L (metrics.py:291-300) of the prediction against the FIRST PRESENT reference
 * (the lowest k with ref_len[i, k] >= 0).  out int32 [N, 6] = overlap_1, overlap_2 (sum over the distinct n-grams of
 * the reference of min(prediction count, reference count)), lcs (length of the longest common subsequence), pred_len,
 * ref_len, k_used; an image with no present reference gets k_used = -1 and 0 in the other five.  The caller forms
 * P = overlap_n / max(len - n + 1, 1), lcs / len and F = 2PR / (P + R).  The LCS is the bit-vector recurrence over the
 * ballot of the prediction row (two 64-bit words for S <= 128): ref_len wave-uniform steps. */
int pgca_rouge_stats(const int64_t* pred_ids, const int32_t* pred_len, const int64_t* ref_ids, const int32_t* ref_len,
                     int32_t N, int32_t K, int32_t S, int32_t base_vocab, int32_t* out, void* stream);
/* The integers of METEOR's exact-match stage (nltk meteor_score as HF `meteor` calls it, metrics.py:302-310) per
 * reference.  out int32 [N, K, 2] = m, chunks; an absent reference gets -1, -1.  Matching: the prediction's positions
 * from the last to the first, each to the highest still-unmatched reference position holding the same id; chunks = the
 * matches (i, j) whose predecessor (i - 1, j - 1) is not a match.  The caller forms P = m / pred_len, R = m / ref_len,
 * F = PR / (0.9 P + 0.1 R), score = (1 - 0.5 (chunks / m)^3) F and the maximum over the present references. */
int pgca_meteor_stats(const int64_t* pred_ids, const int32_t* pred_len, const int64_t* ref_ids,
                      const int32_t* ref_len, int32_t N, int32_t K, int32_t S, int32_t base_vocab, int32_t* out,
                      void* stream);

/* ------------------------------------------------------------------ pooling / normalise (Stage 1) */
/* pooled[b] = sum_s feats[b,s]*mask[b,s] / max(sum_s mask, 1)  (model.py:449-456); feats f32.
 * With cu_seqlens (int32 [B+1]) feats / dfeats are packed: position (b, s) is row cu[b] + s, s < cu[b+1]-cu[b]. */
int pgca_masked_mean_fwd(const float* feats, const int32_t* mask, int32_t B, int32_t S, int32_t H, float* pooled,
                         const int32_t* cu_seqlens, void* stream);
int pgca_masked_mean_bwd(const float* dpooled, const int32_t* mask, int32_t B, int32_t S, int32_t H,
                         float* dfeats, const int32_t* cu_seqlens, void* stream);
/* y = x / max(||x||, 1e-12) (F.normalize, model.py:828-829) and its backward dx = (dy - y (dy . y)) / norm; a row whose
 * norm was clamped (norm <= 1e-12) is divided by a constant, so its backward is dy / norm (autograd passes nothing through
 * clamp_min there). */
int pgca_l2norm_fwd(const float* x, int32_t B, int32_t P, float* y, float* norm, void* stream);
int pgca_l2norm_bwd(const float* dy, const float* y, const float* norm, int32_t B, int32_t P, float* dx,
                    void* stream);
/* NT-Xent pieces (model.py:988-998) on top of two ROWSTATS GEMMs (rows of S and rows of S^t):
 * loss[0] = (sum_i (lse_r[i] - diag[i]) + sum_i (lse_c[i] - diag[i])) / (2 * n_total) over n_local rows. */
int pgca_ntxent_loss(const float* lse_r, const float* lse_c, const float* diag, int32_t n_local, int32_t n_total,
                     float* loss, void* stream);

/* ------------------------------------------------------------------ optimiser (fused, flat buffers) */
/* Partial sums of squares of a flat f32 gradient buffer: part[blocks]; blocks = pgca_sqnorm_blocks(n). */
int pgca_sqnorm_blocks(int64_t n);
int pgca_sqnorm(const float* g, int64_t n, float* part, void* stream);
/* Device-side step control (no host sync): reads the partial sums of all segments, derives
 *   total_norm, finite flag, clip = min(1, max_norm/(norm+1e-6)) (clip_grad_norm_, trainer.py:511-515,619-623),
 * and - if finite - advances ctrl.step and evaluates the cosine warm-up lr (trainer.py:285-289).
 * ctrl layout (f32[8]): [0] total_norm [1] finite(1/0) [2] clip [3] lr [4] bias_corr1 [5] bias_corr2
 *                       [6] opt_step (as float) [7] sched_step (as float).
 * gate (device, optional): loss of the micro-batch that closes the accumulation group; non-finite -> the step is
 * skipped like a non-finite norm (the reference drops the group there, trainer.py:481-489 under accumulate()). */
int pgca_step_control(const float* part, int32_t nparts, float max_norm, float base_lr, int32_t warmup,
                      int32_t total_steps, int32_t sched_stride, float beta1, float beta2, float grad_scale,
                      const float* gate, float* ctrl, void* stream);
/* The reference's per-micro-batch clip_grad_norm_ (trainer.py:511-515,619-623) on a partially accumulated gradient,
 * without a host sync: coef[0] = min(1, max_norm / (norm + 1e-6)) and coef[1] = norm from the pgca_sqnorm partials of
 * all segments; pgca_scale_dev multiplies a flat buffer by coef[0]. */
int pgca_clip_coef(const float* part, int32_t nparts, float max_norm, float* coef, void* stream);
int pgca_scale_dev(float* x, int64_t n, const float* coef, void* stream);
/* AdamW (trainer.py:275-281: decoupled decay on every parameter) over a flat segment, gradient scaled by
 * ctrl.clip * grad_scale, skipped entirely when ctrl.finite == 0; refreshes the bf16 mirror. */
int pgca_adamw(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, const float* ctrl,
               float weight_decay, float beta1, float beta2, float eps, float grad_scale, void* stream);
/* f32 -> bf16 cast of a flat buffer (initial mirror / reference-policy snapshot). */
int pgca_cast_bf16(const float* x, void* y_bf16, int64_t n, void* stream);
/* bf16 -> f32 of a flat buffer (back from the bf16-compressed gradient all-reduce, dist.DataParallel). */
int pgca_cast_f32(const void* x_bf16, float* y, int64_t n, void* stream);
/* hi/lo bf16 split of an f32 matrix along K (NT-Xent similarity at f32-grade accuracy on the bf16 MFMA GEMM,
 * reference model.py:988-990 computes the similarity in fp32): x f32 [R, P] -> y bf16 [rows_out, 3P],
 * row r = [hi | hi | lo] (pattern 0, the A operand) or [hi | lo | hi] (pattern 1, the B operand), hi = bf16(x),
 * lo = bf16(x - hi); rows R..rows_out-1 are zero.  A.B^t over K = 3P then equals x.z up to the dropped lo.lo
 * term (~2^-17 relative).  P % 8 == 0. */
int pgca_split_bf16(const float* x, int32_t R, int32_t P, int32_t rows_out, int32_t pattern, void* y_bf16,
                    void* stream);
/* y (+)= alpha * x on flat f32 buffers (gradient un-scaling after all-reduce etc.). */
int pgca_axpy(const float* x, float alpha, float* y, int64_t n, int32_t accumulate, void* stream);
/* gather / scatter rows of an f32 or bf16 [*, H] matrix by int32 row_map. */
int pgca_gather_rows_bf16(const void* src, const int32_t* row_map, int32_t M, int32_t H, void* dst, void* stream);

/* ------------------------------------------------------------------ token selection (generation) */
/* One token per row of logits [R, ld] f32 (ld % 4 == 0, 16-B aligned base; columns >= V ignored), replacing the torch
 * chain after the LM head in CaptionDecoder.generate (model.py:621-678 -> HF logits processors + sampling).
 * Processors in HF's order, exactly CaptionDecoder._process_scores:
 *   repetition penalty on the raw score (s < 0 ? s * p : s / p), once per DISTINCT id of prev[r, 0 .. n_prev)
 *   (int64 [R, ld_prev]; n_prev may be 0); then, only when sampling (u != NULL): temperature (divide), top-k
 *   (0 = off; scores strictly below the k-th largest go, ties with it stay; top_k >= V is off), top-p (ascending, a
 *   class of equal scores goes iff the cumulative probability up to and including it is <= 1 - top_p; the largest
 *   always stays).
 * u == NULL: argmax of the penalised scores, lowest id among equals.  Otherwise u [R] f32 in (0, 1): inverse CDF over
 * the kept tokens in token-id order - the smallest j whose kept prefix mass >= u * Z_kept.
 * next [R] int64; next_logp [R] = log-softmax of the RAW logits at the chosen token.  done (optional, uint8 [R]): a
 * non-zero row yields pad_id and 0.  One workgroup per row, no sort, fixed-order sums: bit-identical from run to run.
 * With a penalty, ceil(V / 32) * 4 bytes of LDS hold the seen-id bitmask (V <= 491 520). */
int pgca_select_token(const float* logits, int32_t ld, int32_t V, int32_t R, const int64_t* prev, int32_t ld_prev,
                      int32_t n_prev, float repetition_penalty, float temperature, int32_t top_k, float top_p,
                      const float* u, const uint8_t* done, int64_t pad_id, int64_t* next, float* next_logp,
                      void* stream);
/* Beam-search candidates of B batch items with nb beams each (logits [B * nb, ld]), replacing the per-step
 * log_softmax -> processors -> + running_beam_scores -> topk / multinomial of HF's _beam_search: the processors above
 * act on the LOG-PROBABILITIES of each row (temperature / top-k / top-p only when warp != 0), acc = processed +
 * beam_scores[b * nb + beam]; the K (<= 64; 2 * nb) candidates with the largest key come out in descending key order,
 * equal keys by ascending flat index: cand_score [B, K] = acc, cand_index [B, K] int64 = beam * V + token.
 * use_noise == 0: key = acc.  Otherwise key = acc + g with Gumbel noise g = -log(-log u),
 *   u = ((hash32(f * 0x9E3779B1 + noise_seed) >> 8) + 0.5) * 2^-24,  f = (b * nb + beam) * V + token  (mod 2^32),
 * hash32 = the lowbias32 function of the dropout masks: the order is then the draw order of sampling K candidates
 * without replacement from softmax(acc) (beam-sample).  Fewer than K finite keys: the tail carries -inf and the
 * lowest unused flat indices.  nb <= 32, nb * V < 2^24; with a penalty nb * ceil(V / 32) * 4 bytes of LDS <= 60 KiB. */
int pgca_select_beam_candidates(const float* logits, int32_t ld, int32_t V, int32_t B, int32_t nb, const int64_t* prev,
                                int32_t ld_prev, int32_t n_prev, float repetition_penalty, int32_t warp,
                                float temperature, int32_t top_k, float top_p, const float* beam_scores, int32_t K,
                                int32_t use_noise, uint32_t noise_seed, float* cand_score, int64_t* cand_index,
                                void* stream);
/* The two entries above with HF's banning processors (NoRepeatNGram, MinLength / MinNewTokensLength, SuppressTokens):
 * a banned token's processed score is -inf whatever the repetition penalty made of it, so it drops out of argmax,
 * top-k, top-p, the draw and the beam keys (cand_score -inf).  next_logp and the beam kernel's log-softmax stay those
 * of the RAW row (HF normalises before the processors run).
 *   no_repeat_ngram_size n (0 = off): in a row with n_prev >= n - 1 previous ids, token prev[i + n - 1] is banned for
 *     every i with prev[i .. i + n - 2] == prev[n_prev - n + 1 .. n_prev - 1]; n == 1 bans every seen id; shorter rows
 *     ban nothing.
 *   ban_ids [n_ban] (device int64): banned in every row (suppress_tokens; the caller adds [EOS] while the sequence is
 *     shorter than the minimum length).  Ids outside [0, V) are ignored in both.
 * A row with every token banned yields the lowest id (token kernel; next_logp of that id) and -inf candidates with the
 * lowest flat indices (beam kernel).  The banned ids are a second bitmask next to the seen ids: with a penalty AND bans
 * 2 * rows * ceil(V / 32) * 4 bytes of LDS (rows = 1, or nb for the beam kernel) must fit 61 440 bytes - nb <= 4 at
 * V <= 61 440 - else PGCA_ERR_INVALID is returned and nothing is launched.  Empty options (all zero) give exactly the
 * entries above, which call these. */
typedef struct pgca_select_opts {
  int32_t no_repeat_ngram_size;
  int32_t n_ban;
  const int64_t* ban_ids;
} pgca_select_opts;
int pgca_sizeof_select_opts(void);
int pgca_select_token_ex(const float* logits, int32_t ld, int32_t V, int32_t R, const int64_t* prev, int32_t ld_prev,
                         int32_t n_prev, float repetition_penalty, float temperature, int32_t top_k, float top_p,
                         const float* u, const uint8_t* done, int64_t pad_id, int64_t* next, float* next_logp,
                         const pgca_select_opts* opts, void* stream);
int pgca_select_beam_candidates_ex(const float* logits, int32_t ld, int32_t V, int32_t B, int32_t nb,
                                   const int64_t* prev, int32_t ld_prev, int32_t n_prev, float repetition_penalty,
                                   int32_t warp, float temperature, int32_t top_k, float top_p,
                                   const float* beam_scores, int32_t K, int32_t use_noise, uint32_t noise_seed,
                                   float* cand_score, int64_t* cand_index, const pgca_select_opts* opts, void* stream);
/* The rest of one step of HF's _beam_search (generation/utils.py, transformers 5.x) once the K = 2 * nb candidates of
 * every batch item are known (cand_score / cand_index [B, K] as pgca_select_beam_candidates writes them): the helpers
 * _get_top_k_continuations (sequence part), _get_running_beams_for_next_iteration, _update_finished_beams and
 * _check_early_stop_heuristic in one launch, one workgroup per batch item.  cur = tokens generated so far (the column
 * this step fills), L = the most that may be generated, eos = the one [EOS] id; a candidate "hits" iff its token is eos
 * or cur + 1 >= L.
 *   running: the nb best candidates by cand_score + hit * -1e9 -> running_out [B, nb, L] (source row of running_in with
 *     column cur set), running_beam_scores [B, nb], tok [B * nb] (the token to feed), flat_src [B * nb] (b * nb + source
 *     beam: the K/V-cache rows to continue from).
 *   finished pool: candidate score cand_score / (cur + 1)^length_penalty, + -1e9 each when (early_stopping == 1 and the
 *     item's pool is full), when unsat[b] == 0, and when the candidate is not a hit ranked inside the first nb; the nb
 *     best of (pool, candidates) -> sequences_out [B, nb, L], beam_scores, is_sent_finished (uint8), gen_len (int64,
 *     tokens of each finished hypothesis) [B, nb].
 *   unsat [B] (uint8) &= any(running_beam_scores[b, 0] / h^length_penalty > (finished ? min(beam_scores[b]) : -1e9)),
 *     h = L when early_stopping == 2 ("never") and length_penalty > 0, else cur + 1.
 *   hits_all [B] (uint8) = every candidate of the item hit.
 * Every ranking is by score descending, then merged index ascending (pool before candidates).  Rows are gathered, so
 * the two sequence buffers are ping-pong pairs (in != out); columns 0 .. cur are written.  The divisions are
 * multiplications by the f32 reciprocal, as torch divides a device tensor by a host scalar.  nb <= 32. */
int pgca_beam_step(const float* cand_score, const int64_t* cand_index, int32_t B, int32_t nb, int32_t V, int32_t cur,
                   int32_t L, int64_t eos, float length_penalty, int32_t early_stopping, const int64_t* running_in,
                   int64_t* running_out, float* running_beam_scores, const int64_t* sequences_in,
                   int64_t* sequences_out, float* beam_scores, uint8_t* is_sent_finished, int64_t* gen_len,
                   uint8_t* unsat, int64_t* tok, int64_t* flat_src, uint8_t* hits_all, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PGCA_HIP_H */
