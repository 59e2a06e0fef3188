// Caption metrics over token ids, on the device (reference evaluation/metrics.py applied to base-vocabulary ids):
//   pgca_ngram_keys     n-gram keys of stripped rows, optionally once per group (document frequency, diversity)
//   pgca_cider_rows     _compute_cider (metrics.py:463-572) per image, in float64
//   pgca_bleu_stats     the ten integers of corpus BLEU per image
//   pgca_token_overlap  |set(a) & set(b)| and |set(a) | set(b)| (_compute_text_similarity, metrics.py:638-661)
//   pgca_rouge_stats    n-gram overlaps of orders 1 and 2 and the longest common subsequence, against the first reference
//   pgca_meteor_stats   matches and chunks of METEOR's exact-match stage, per reference
// One 64-lane workgroup per image (or row pair); the keys of the image sit in LDS and every lane scans them for its own
// positions.  The order-sensitive pair works on ballots instead: a whole row compared with one id is one 64-bit mask per
// 64 columns, the same in every lane.  No atomics, nothing between workgroups, no waiting; every loop is bounded by S,
// K or the 32 steps of the table search; every floating-point sum is lane-strided in ascending order and then the xor
// tree: two launches on one input are bitwise equal.
#include "common.h"

namespace pgca {
namespace {

constexpr int EVAL_MAX_S = PGCA_EVAL_MAX_S, EVAL_MAX_K = PGCA_EVAL_MAX_K;
constexpr long long NO_KEY = -1;  // 0xffff in every field: no id reaches 65535, so no n-gram has this key

__device__ __forceinline__ int clamp_len(int len, int S) { return len < 0 ? 0 : (len > S ? S : len); }

// Key of the n-gram that starts at column t of a stripped row: n ids at 16 bits each, the first most significant.
__device__ __forceinline__ long long ngram_key(const long long* __restrict__ row, int len, int t, int n) {
  if (t + n > len) return NO_KEY;
  unsigned long long k = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < n) k = (k << 16) | ((unsigned long long)row[t + i] & 0xffffull);
  return (long long)k;
}

// dst[0 .. S) = the keys of one row (a row with len <= 0 has none)
__device__ __forceinline__ void fill_keys(long long* dst, const long long* __restrict__ row, int len, int S, int n,
                                          int lane) {
  for (int t = lane; t < S; t += 64) dst[t] = ngram_key(row, len, t, n);
}

// segment 0 = the prediction's keys, segment 1 + k = reference k's; between two barriers
__device__ __forceinline__ void fill_image(long long* keys, const long long* __restrict__ pred, int plen,
                                           const long long* __restrict__ refs, const int* __restrict__ rlen, int K, int S,
                                           int n, int lane) {
  __syncthreads();
  fill_keys(keys, pred, plen, S, n, lane);
  for (int k = 0; k < K; ++k) fill_keys(keys + (1 + k) * S, refs + (size_t)k * S, clamp_len(rlen[k], S), S, n, lane);
  __syncthreads();
}

__global__ void __launch_bounds__(64)
ngram_keys_kernel(const long long* __restrict__ ids, const int* __restrict__ len, int K, int S, int n, int distinct,
                  long long* __restrict__ out) {
  __shared__ long long keys[EVAL_MAX_K * EVAL_MAX_S];
  const int g = blockIdx.x, lane = threadIdx.x;
  const int slots = K * S;
  for (int k = 0; k < K; ++k)
    fill_keys(keys + k * S, ids + ((size_t)g * K + k) * S, clamp_len(len[(size_t)g * K + k], S), S, n, lane);
  __syncthreads();
  for (int p = lane; p < slots; p += 64) {
    long long key = keys[p];
    if (distinct && key != NO_KEY) {
      bool seen = false;  // an earlier position of the group (any reference of the image) holds the same n-gram
      for (int q = 0; q < p; ++q) seen |= keys[q] == key;
      if (seen) key = NO_KEY;
    }
    out[(size_t)g * slots + p] = key;
  }
}

// df of `key` in the sorted (signed ascending) keys[0 .. count): 32 halvings cover any count below 2^32
__device__ __forceinline__ double table_df_of(const long long* __restrict__ keys, const long long* __restrict__ df,
                                              long long count, long long key) {
  long long lo = 0, hi = count;
  for (int step = 0; step < 32; ++step) {
    if (lo < hi) {
      const long long mid = lo + ((hi - lo) >> 1);
      if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
  }
  return (lo < count && keys[lo] == key) ? (double)df[lo] : 1.0;
}

__global__ void __launch_bounds__(64)
cider_rows_kernel(const long long* __restrict__ pred_ids, const int* __restrict__ pred_len,
                  const long long* __restrict__ ref_ids, const int* __restrict__ ref_len, int K, int S,
                  const long long* __restrict__ table_keys, const long long* __restrict__ table_df,
                  const long long* __restrict__ table_off, long long table_len, double n_docs, double sigma,
                  double* __restrict__ score_out, int* __restrict__ flag_out) {
  __shared__ long long keys[(1 + EVAL_MAX_K) * EVAL_MAX_S];
  const int b = blockIdx.x, lane = threadIdx.x;
  const long long* pred = pred_ids + (size_t)b * S;
  const long long* refs = ref_ids + (size_t)b * K * S;
  const int* rlen = ref_len + (size_t)b * K;
  const int plen = clamp_len(pred_len[b], S);
  int present = 0, len_sum = 0;
  for (int k = 0; k < K; ++k) {
    const int l = rlen[k];
    present += l >= 0 ? 1 : 0;
    len_sum += clamp_len(l, S);
  }
  if (present == 0) {  // the whole workgroup leaves: no barrier was reached
    if (lane == 0) {
      score_out[b] = 0.0;
      flag_out[b] = 1;
    }
    return;
  }
  const double k_present = (double)present;
  const int slots = (1 + K) * S;
  double total = 0.0;
  for (int n = 1; n <= 4; ++n) {
    fill_image(keys, pred, plen, refs, rlen, K, S, n, lane);
    long long t0 = table_off[n - 1], t1 = table_off[n];
    t0 = t0 < 0 ? 0 : (t0 > table_len ? table_len : t0);
    t1 = t1 < t0 ? t0 : (t1 > table_len ? table_len : t1);
    double num = 0.0, pn = 0.0, rn = 0.0;
    for (int p = lane; p < slots; p += 64) {
      const long long key = keys[p];
      if (key == NO_KEY) continue;
      // the n-gram is handled at its first position among prediction and references
      bool first = true;
      int pc = 0;
      for (int t = 0; t < S; ++t) {
        const bool m = keys[t] == key;
        pc += m ? 1 : 0;
        first &= !(m && t < p);
      }
      double rc = 0.0;  // sum over the references, in their order, of count / references present
      for (int k = 0; k < K; ++k) {
        int c = 0;
        for (int t = 0; t < S; ++t) {
          const int q = (1 + k) * S + t;
          const bool m = keys[q] == key;
          c += m ? 1 : 0;
          first &= !(m && q < p);
        }
        rc += (double)c / k_present;
      }
      if (!first) continue;
      const double df = table_df_of(table_keys + t0, table_df + t0, t1 - t0, key);
      const double idf = log(n_docs / (df + 1e-8));
      const double pw = (double)pc * idf, rw = rc * idf;
      num += pw * rw;
      pn += pw * pw;
      rn += rw * rw;
    }
    num = wave_sum(num);
    pn = wave_sum(pn);
    rn = wave_sum(rn);
    total += (pn > 0.0 && rn > 0.0) ? num / sqrt(pn * rn) : 0.0;
  }
  if (lane == 0) {
    const double avg = (double)len_sum / k_present;
    const double d = (double)plen - avg;
    const double penalty = avg > 0.0 ? exp(-(d * d) / (2.0 * (sigma * sigma))) : 0.0;
    score_out[b] = total / 4.0 * penalty;
    flag_out[b] = 0;
  }
}

__global__ void __launch_bounds__(64)
bleu_stats_kernel(const long long* __restrict__ pred_ids, const int* __restrict__ pred_len,
                  const long long* __restrict__ ref_ids, const int* __restrict__ ref_len, int K, int S,
                  long long* __restrict__ stats) {
  __shared__ long long keys[(1 + EVAL_MAX_K) * EVAL_MAX_S];
  const int b = blockIdx.x, lane = threadIdx.x;
  const long long* pred = pred_ids + (size_t)b * S;
  const long long* refs = ref_ids + (size_t)b * K * S;
  const int* rlen = ref_len + (size_t)b * K;
  const int plen = clamp_len(pred_len[b], S);
  int shortest = -1;  // the shortest present reference
  for (int k = 0; k < K; ++k) {
    const int l = rlen[k];
    if (l >= 0 && (shortest < 0 || clamp_len(l, S) < shortest)) shortest = clamp_len(l, S);
  }
  long long* out = stats + (size_t)b * 10;
  for (int n = 1; n <= 4; ++n) {
    fill_image(keys, pred, plen, refs, rlen, K, S, n, lane);
    int clipped = 0;
    for (int p = lane; p < S; p += 64) {
      const long long key = keys[p];
      if (key == NO_KEY) continue;
      bool first = true;
      int pc = 0;
      for (int t = 0; t < S; ++t) {
        const bool m = keys[t] == key;
        pc += m ? 1 : 0;
        first &= !(m && t < p);
      }
      int most = 0;
      for (int k = 0; k < K; ++k) {
        int c = 0;
        for (int t = 0; t < S; ++t) c += keys[(1 + k) * S + t] == key ? 1 : 0;
        most = c > most ? c : most;
      }
      clipped += first ? (pc < most ? pc : most) : 0;
    }
    clipped = wave_sum(clipped);
    if (lane == 0) {
      out[n - 1] = clipped;
      out[4 + n - 1] = plen - n + 1 > 0 ? plen - n + 1 : 0;
    }
  }
  if (lane == 0) {
    out[8] = plen;
    out[9] = shortest < 0 ? 0 : shortest;
  }
}

__global__ void __launch_bounds__(64)
token_overlap_kernel(const long long* __restrict__ a_ids, const int* __restrict__ a_len,
                     const long long* __restrict__ b_ids, const int* __restrict__ b_len, int S, int* __restrict__ out) {
  __shared__ long long a[EVAL_MAX_S], bb[EVAL_MAX_S];
  const int r = blockIdx.x, lane = threadIdx.x;
  const int alen = clamp_len(a_len[r], S), blen = clamp_len(b_len[r], S);
  for (int t = lane; t < S; t += 64) {
    a[t] = a_ids[(size_t)r * S + t];
    bb[t] = b_ids[(size_t)r * S + t];
  }
  __syncthreads();
  int na = 0, nb = 0, both = 0;  // distinct ids of a, of b, of both: each id counted at its first column
  for (int t = lane; t < S; t += 64) {
    if (t < alen) {
      const long long id = a[t];
      bool first = true, in_b = false;
      for (int q = 0; q < S; ++q) {
        first &= !(q < t && a[q] == id);
        in_b |= q < blen && bb[q] == id;
      }
      na += first ? 1 : 0;
      both += (first && in_b) ? 1 : 0;
    }
    if (t < blen) {
      const long long id = bb[t];
      bool first = true;
      for (int q = 0; q < t; ++q) first &= bb[q] != id;
      nb += first ? 1 : 0;
    }
  }
  na = wave_sum(na);
  nb = wave_sum(nb);
  both = wave_sum(both);
  if (lane == 0) {
    out[(size_t)r * 2] = both;
    out[(size_t)r * 2 + 1] = na + nb - both;
  }
}

// the first len of 64 positions starting at column `from`, as a bit mask
__device__ __forceinline__ unsigned long long live_mask(int len, int from) {
  const int n = len - from;
  return n <= 0 ? 0ull : (n >= 64 ? ~0ull : ((1ull << n) - 1ull));
}

__global__ void __launch_bounds__(64)
rouge_stats_kernel(const long long* __restrict__ pred_ids, const int* __restrict__ pred_len,
                   const long long* __restrict__ ref_ids, const int* __restrict__ ref_len, int K, int S,
                   int* __restrict__ stats) {
  __shared__ long long keys[2 * EVAL_MAX_S];  // the prediction's keys, then the reference's
  const int b = blockIdx.x, lane = threadIdx.x;
  const int* rlen = ref_len + (size_t)b * K;
  int* out = stats + (size_t)b * 6;
  int used = -1;  // the first present reference
  for (int k = K - 1; k >= 0; --k) used = rlen[k] >= 0 ? k : used;
  if (used < 0) {  // the whole workgroup leaves: no barrier was reached
    if (lane < 6) out[lane] = lane == 5 ? -1 : 0;
    return;
  }
  const long long* pred = pred_ids + (size_t)b * S;
  const long long* ref = ref_ids + ((size_t)b * K + used) * S;
  const int plen = clamp_len(pred_len[b], S), len = clamp_len(rlen[used], S);
  // ROUGE-1 / ROUGE-2: every distinct n-gram of the reference, at its first position there
  for (int n = 1; n <= 2; ++n) {
    __syncthreads();
    fill_keys(keys, pred, plen, S, n, lane);
    fill_keys(keys + S, ref, len, S, n, lane);
    __syncthreads();
    int overlap = 0;
    for (int p = lane; p < S; p += 64) {
      const long long key = keys[S + p];
      if (key == NO_KEY) continue;
      bool first = true;
      int pc = 0, rc = 0;
      for (int t = 0; t < S; ++t) {
        const bool m = keys[S + t] == key;
        rc += m ? 1 : 0;
        first &= !(m && t < p);
        pc += keys[t] == key ? 1 : 0;
      }
      overlap += first ? (pc < rc ? pc : rc) : 0;
    }
    overlap = wave_sum(overlap);
    if (lane == 0) out[n - 1] = overlap;
  }
  // ROUGE-L: bit t of word w is prediction column 64 w + t.  V starts all ones; per reference id with match vector M:
  // U = V & M, V = (V + U) | (V & ~U), the add carrying from word 0 into word 1; the zero bits of V among the live
  // columns count the longest common subsequence.  Every value below is the same in all lanes.
  const long long a0 = lane < plen ? pred[lane] : 0, a1 = 64 + lane < plen ? pred[64 + lane] : 0;
  const unsigned long long live0 = live_mask(plen, 0), live1 = live_mask(plen, 64);
  unsigned long long v0 = ~0ull, v1 = ~0ull;
  for (int j = 0; j < len; ++j) {
    const long long id = ref[j];
    const unsigned long long u0 = v0 & __ballot(a0 == id) & live0, u1 = v1 & __ballot(a1 == id) & live1;
    const unsigned long long s0 = v0 + u0;
    const unsigned long long s1 = v1 + u1 + (s0 < v0 ? 1ull : 0ull);
    v0 = s0 | (v0 & ~u0);
    v1 = s1 | (v1 & ~u1);
  }
  if (lane == 0) {
    out[2] = __popcll(~v0 & live0) + __popcll(~v1 & live1);
    out[3] = plen;
    out[4] = len;
    out[5] = used;
  }
}

__global__ void __launch_bounds__(64)
meteor_stats_kernel(const long long* __restrict__ pred_ids, const int* __restrict__ pred_len,
                    const long long* __restrict__ ref_ids, const int* __restrict__ ref_len, int K, int S,
                    int* __restrict__ stats) {
  __shared__ long long pred[EVAL_MAX_S];
  __shared__ int match[EVAL_MAX_S];  // the reference position matched to each prediction position, -1 for none
  const int b = blockIdx.x, lane = threadIdx.x;
  const int plen = clamp_len(pred_len[b], S);
  for (int t = lane; t < S; t += 64) pred[t] = pred_ids[(size_t)b * S + t];
  __syncthreads();
  for (int k = 0; k < K; ++k) {
    int* out = stats + ((size_t)b * K + k) * 2;
    const int l = ref_len[(size_t)b * K + k];
    if (l < 0) {  // the same in every lane: nobody waits below
      if (lane < 2) out[lane] = -1;
      continue;
    }
    const int len = clamp_len(l, S);
    const long long* ref = ref_ids + ((size_t)b * K + k) * S;
    // bit t of word w is reference column 64 w + t; free0 / free1 are the positions not yet matched
    const long long r0 = lane < len ? ref[lane] : 0, r1 = 64 + lane < len ? ref[64 + lane] : 0;
    unsigned long long free0 = live_mask(len, 0), free1 = live_mask(len, 64);
    for (int i = plen - 1; i >= 0; --i) {
      const long long id = pred[i];
      const unsigned long long m0 = __ballot(r0 == id) & free0, m1 = __ballot(r1 == id) & free1;
      int j = -1;
      if (m1) {
        j = 63 - __builtin_clzll(m1);
        free1 &= ~(1ull << j);
        j += 64;
      } else if (m0) {
        j = 63 - __builtin_clzll(m0);
        free0 &= ~(1ull << j);
      }
      if (lane == 0) match[i] = j;
    }
    __syncthreads();
    int m = 0, chunks = 0;
    for (int i = lane; i < plen; i += 64) {
      const int j = match[i];
      if (j < 0) continue;
      m += 1;
      chunks += (i > 0 && j > 0 && match[i - 1] == j - 1) ? 0 : 1;
    }
    m = wave_sum(m);
    chunks = wave_sum(chunks);
    if (lane == 0) {
      out[0] = m;
      out[1] = chunks;
    }
    __syncthreads();  // match is rewritten for the next reference
  }
}

}  // namespace
}  // namespace pgca

using namespace pgca;

#define EVAL_LIMITS(who, N, K, S, base_vocab)                                  \
  REQUIRE(S >= 1 && S <= PGCA_EVAL_MAX_S, who);                                \
  REQUIRE(K >= 1 && K <= PGCA_EVAL_MAX_K, who);                                \
  REQUIRE(base_vocab >= 1 && base_vocab <= PGCA_EVAL_MAX_VOCAB, who);          \
  REQUIRE(N >= 1 && N < PGCA_EVAL_MAX_IMAGES, who)

extern "C" int pgca_ngram_keys(const int64_t* ids, const int32_t* len, int32_t G, int32_t K, int32_t S, int32_t order,
                               int32_t base_vocab, int32_t distinct_per_group, int64_t* keys_out, void* stream) {
  REQUIRE(ids && len && keys_out, "pgca_ngram_keys");
  EVAL_LIMITS("pgca_ngram_keys", G, K, S, base_vocab);
  REQUIRE(order >= 1 && order <= 4, "pgca_ngram_keys");
  hipLaunchKernelGGL(ngram_keys_kernel, dim3(G), dim3(64), 0, (hipStream_t)stream, (const long long*)ids, len, K, S,
                     order, distinct_per_group != 0 ? 1 : 0, (long long*)keys_out);
  return check_launch("pgca_ngram_keys");
}

extern "C" int pgca_cider_rows(const int64_t* pred_ids, const int32_t* pred_len, const int64_t* ref_ids,
                               const int32_t* ref_len, int32_t N, int32_t K, int32_t S, int32_t base_vocab,
                               const int64_t* table_keys, const int64_t* table_df, const int64_t* table_off,
                               int64_t table_len, int32_t n_docs, float sigma, void* score_out, int32_t* flag_out,
                               void* stream) {
  REQUIRE(pred_ids && pred_len && ref_ids && ref_len, "pgca_cider_rows");
  REQUIRE(table_keys && table_df && table_off && score_out && flag_out, "pgca_cider_rows");
  EVAL_LIMITS("pgca_cider_rows", N, K, S, base_vocab);
  REQUIRE(table_len >= 0 && n_docs >= 1 && sigma > 0.f, "pgca_cider_rows");
  hipLaunchKernelGGL(cider_rows_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, (const long long*)pred_ids, pred_len,
                     (const long long*)ref_ids, ref_len, K, S, (const long long*)table_keys, (const long long*)table_df,
                     (const long long*)table_off, (long long)table_len, (double)n_docs, (double)sigma,
                     (double*)score_out, flag_out);
  return check_launch("pgca_cider_rows");
}

extern "C" int pgca_bleu_stats(const int64_t* pred_ids, const int32_t* pred_len, const int64_t* ref_ids,
                               const int32_t* ref_len, int32_t N, int32_t K, int32_t S, int32_t base_vocab,
                               int64_t* stats_out, void* stream) {
  REQUIRE(pred_ids && pred_len && ref_ids && ref_len && stats_out, "pgca_bleu_stats");
  EVAL_LIMITS("pgca_bleu_stats", N, K, S, base_vocab);
  hipLaunchKernelGGL(bleu_stats_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, (const long long*)pred_ids, pred_len,
                     (const long long*)ref_ids, ref_len, K, S, (long long*)stats_out);
  return check_launch("pgca_bleu_stats");
}

extern "C" int pgca_token_overlap(const int64_t* a_ids, const int32_t* a_len, const int64_t* b_ids,
                                  const int32_t* b_len, int32_t R, int32_t S, int32_t* out, void* stream) {
  REQUIRE(a_ids && a_len && b_ids && b_len && out, "pgca_token_overlap");
  REQUIRE(S >= 1 && S <= PGCA_EVAL_MAX_S, "pgca_token_overlap");
  REQUIRE(R >= 1 && R < PGCA_EVAL_MAX_IMAGES, "pgca_token_overlap");
  hipLaunchKernelGGL(token_overlap_kernel, dim3(R), dim3(64), 0, (hipStream_t)stream, (const long long*)a_ids, a_len,
                     (const long long*)b_ids, b_len, S, out);
  return check_launch("pgca_token_overlap");
}

extern "C" int pgca_rouge_stats(const int64_t* pred_ids, const int32_t* pred_len, const int64_t* ref_ids,
                                const int32_t* ref_len, int32_t N, int32_t K, int32_t S, int32_t base_vocab,
                                int32_t* out, void* stream) {
  REQUIRE(pred_ids && pred_len && ref_ids && ref_len && out, "pgca_rouge_stats");
  EVAL_LIMITS("pgca_rouge_stats", N, K, S, base_vocab);
  hipLaunchKernelGGL(rouge_stats_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, (const long long*)pred_ids,
                     pred_len, (const long long*)ref_ids, ref_len, K, S, out);
  return check_launch("pgca_rouge_stats");
}

extern "C" int pgca_meteor_stats(const int64_t* pred_ids, const int32_t* pred_len, const int64_t* ref_ids,
                                 const int32_t* ref_len, int32_t N, int32_t K, int32_t S, int32_t base_vocab,
                                 int32_t* out, void* stream) {
  REQUIRE(pred_ids && pred_len && ref_ids && ref_len && out, "pgca_meteor_stats");
  EVAL_LIMITS("pgca_meteor_stats", N, K, S, base_vocab);
  hipLaunchKernelGGL(meteor_stats_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, (const long long*)pred_ids,
                     pred_len, (const long long*)ref_ids, ref_len, K, S, out);
  return check_launch("pgca_meteor_stats");
}
