// Fused multi-head self-attention for head_dim 64, forward and backward, on MFMA 16x16x32 bf16: the C-ABI entry points.
// The kernels are the key-tiled ones of attention_tiled.hip for every sequence length (GPT-2 captions S = 128 / 256,
// CLIP ViT-B/32 T = 50, ViT-L/14 T = 257); at S <= 128 they run one tile per (batch, head), and the probabilities never
// cross LDS.
#include "common.h"

using namespace pgca;

// the problem both directions share, from an entry point's loose arguments (S is the padded length Sp as well)
static AttnProblem problem(const void* qkv, const int32_t* key_mask, int B, int S, int heads, int causal, Drop drop,
                           const int32_t* cu, void* stream) {
  return {(const bf16_t*)qkv, key_mask, B, S, heads, causal, drop, cu, S, (hipStream_t)stream};
}

extern "C" int pgca_attention_fwd(const void* qkv, const int32_t* key_mask, int32_t B, int32_t S, int32_t heads,
                                  int32_t causal, void* out, float* lse, uint32_t drop_seed, uint32_t drop_threshold,
                                  float drop_scale, const int32_t* cu_seqlens, void* stream) {
  if (!qkv || !out || B <= 0 || S <= 0 || heads <= 0 || B > 65535) {
    set_error("pgca_attention_fwd: bad arguments (B=%d S=%d heads=%d)", B, S, heads);
    return PGCA_ERR_INVALID;
  }
  const Drop drop{drop_seed, drop_threshold, drop_scale};
  return attention_fwd_tiled({problem(qkv, key_mask, B, S, heads, causal, drop, cu_seqlens, stream), (bf16_t*)out,
                              lse});
}

extern "C" int pgca_attention_bwd(const void* qkv, const void* out, const void* dout, const float* lse,
                                  const int32_t* key_mask, int32_t B, int32_t S, int32_t heads, int32_t causal,
                                  void* dqkv, uint32_t drop_seed, uint32_t drop_threshold, float drop_scale,
                                  const int32_t* cu_seqlens, void* stream) {
  if (!qkv || !out || !dout || !lse || !dqkv || B <= 0 || S <= 0 || S > PGCA_ATTN_MAX_S || heads <= 0 || B > 65535) {
    set_error("pgca_attention_bwd: bad arguments (B=%d S=%d heads=%d; S must be <= %d)", B, S, heads, PGCA_ATTN_MAX_S);
    return PGCA_ERR_INVALID;
  }
  const Drop drop{drop_seed, drop_threshold, drop_scale};
  return attention_bwd_tiled({problem(qkv, key_mask, B, S, heads, causal, drop, cu_seqlens, stream),
                              (const bf16_t*)out, (const bf16_t*)dout, lse, (bf16_t*)dqkv});
}

// The same contract on the two-role kernels (a dK/dV role per 128-key block, a dQ role per 128-query block): one block's
// accumulators per workgroup, so the sequence length is bounded by what is tested, not by registers.
extern "C" int pgca_attention_bwd_split(const void* qkv, const void* out, const void* dout, const float* lse,
                                        const int32_t* key_mask, int32_t B, int32_t S, int32_t heads, int32_t causal,
                                        void* dqkv, uint32_t drop_seed, uint32_t drop_threshold, float drop_scale,
                                        const int32_t* cu_seqlens, void* stream) {
  if (!qkv || !out || !dout || !lse || !dqkv || B <= 0 || S <= 0 || S > PGCA_ATTN_SPLIT_MAX_S || heads <= 0 ||
      B > 65535) {
    set_error("pgca_attention_bwd_split: bad arguments (B=%d S=%d heads=%d; S must be <= %d, B <= 65535)", B, S, heads,
              PGCA_ATTN_SPLIT_MAX_S);
    return PGCA_ERR_INVALID;
  }
  const Drop drop{drop_seed, drop_threshold, drop_scale};
  return attention_bwd_split({problem(qkv, key_mask, B, S, heads, causal, drop, cu_seqlens, stream),
                              (const bf16_t*)out, (const bf16_t*)dout, lse, (bf16_t*)dqkv});
}
