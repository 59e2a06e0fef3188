// Preference-pair mining on the device: the model's own sampled captions -> Stage-2 batches.
//   pgca_candidate_rows  generated ids -> decoder training rows + text-tower (scorer) rows
//   pgca_group_cosine    image embedding x its n caption embeddings -> alignment scores
//   pgca_mine_pairs      reference data/loader.py:416-451 (_process_scored_captions): stable descending sort by score,
//                        neighbours paired when the f32 score difference reaches the threshold
//   pgca_pair_rows       the pairs of every image, in image order, as one right-padded Stage-2 batch
// One wave (64 lanes) per candidate row or per image; no atomics, every sum in a fixed order: two launches on one input
// are bitwise equal.
#include "common.h"

namespace pgca {
namespace {

constexpr int WAVES = 4;  // waves per 256-thread workgroup in the row kernels

__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }
__device__ __forceinline__ bool finite_f32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// One wave per candidate row r.
__global__ void candidate_rows_kernel(const long long* __restrict__ cand, int ld_cand,
                                      const long long* __restrict__ lengths, int R, int S, long long base_vocab,
                                      long long dec_vocab, long long dec_pad, long long text_pad,
                                      long long* __restrict__ dec_ids, long long* __restrict__ dec_mask,
                                      long long* __restrict__ text_ids, int* __restrict__ text_mask,
                                      int* __restrict__ text_len, int* __restrict__ out_len) {
  const int r = blockIdx.x * WAVES + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= R) return;
  const long long* row = cand + (size_t)r * ld_cand;
  long long len64 = lengths[r];
  len64 = len64 < 0 ? 0 : len64;
  int len = (int)(len64 < (long long)ld_cand ? len64 : (long long)ld_cand);
  len = len < S ? len : S;
  // an id outside the decoder's vocabulary in the live columns makes the whole row unusable
  bool bad = false;
  for (int t = lane; t < len; t += 64) {
    const long long id = row[t];
    bad |= id < 0 || id >= dec_vocab;
  }
  const bool unusable = __ballot(bad) != 0ull;
  if (unusable) len = 0;
  int kept = 0;  // scorer tokens written so far (wave-uniform)
  for (int t0 = 0; t0 < S; t0 += 64) {
    const int t = t0 + lane;
    const bool live = t < len;
    const long long id = live ? row[t] : dec_pad;
    if (t < S) {
      dec_ids[(size_t)r * S + t] = id;
      dec_mask[(size_t)r * S + t] = live ? 1 : 0;
    }
    // [PAD] / [BOS] / [EOS] of the decoder (base .. base + 2) never reach the text tower
    const bool keep = live && id < base_vocab;
    const unsigned long long bal = __ballot(keep);
    if (keep) text_ids[(size_t)r * S + kept + __popcll(bal & lanes_below(lane))] = id;
    kept += __popcll(bal);
  }
  for (int t = lane; t < S; t += 64) {
    if (t >= kept) text_ids[(size_t)r * S + t] = text_pad;
    text_mask[(size_t)r * S + t] = t < kept ? 1 : 0;
  }
  if (lane == 0) {
    text_len[r] = unusable ? -1 : kept;
    out_len[r] = len;
  }
}

// One wave per candidate row: lane-strided partial sums, then the xor tree (a fixed order).
__global__ void group_cosine_kernel(const float* __restrict__ img, const float* __restrict__ txt, int R, int n, int P,
                                    float* __restrict__ score) {
  const int r = blockIdx.x * WAVES + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= R) return;
  const float* a = img + (size_t)(r / n) * P;
  const float* b = txt + (size_t)r * P;
  float dot = 0.f, aa = 0.f, bb = 0.f;
  for (int c = lane; c < P; c += 64) {
    const float x = a[c], y = b[c];
    dot += x * y;
    aa += x * x;
    bb += y * y;
  }
  dot = wave_sum(dot);
  aa = wave_sum(aa);
  bb = wave_sum(bb);
  if (lane == 0) score[r] = dot / (fmaxf(sqrtf(aa), 1e-12f) * fmaxf(sqrtf(bb), 1e-12f));
}

// One wave per image, lane j = candidate j (n <= 64).
__global__ void mine_pairs_kernel(const float* __restrict__ score, const long long* __restrict__ dec_ids,
                                  const int* __restrict__ out_len, const unsigned char* __restrict__ ok, int n, int S,
                                  int min_tokens, int rule, float threshold, int* __restrict__ rank,
                                  int* __restrict__ pair_win, int* __restrict__ pair_lose,
                                  float* __restrict__ pair_margin, int* __restrict__ pair_count) {
  const int b = blockIdx.x;
  const int j = threadIdx.x;
  const size_t base = (size_t)b * n;
  const bool in = j < n;
  const float s = in ? score[base + j] : 0.f;
  int len = in ? out_len[base + j] : 0;
  len = len < 0 ? 0 : (len > S ? S : len);
  bool kept = in && finite_f32(s) && (!ok || ok[base + j] != 0) && len >= min_tokens;
  // de-duplication: an earlier candidate with the same tokens wins the place
  if (kept) {
    const long long* mine = dec_ids + (base + j) * S;
    for (int i = 0; i < j && kept; ++i) {
      if (out_len[base + i] != len) continue;
      const long long* other = dec_ids + (base + i) * S;
      bool same = true;
      for (int t = 0; t < len && same; ++t) same = mine[t] == other[t];
      if (same) kept = false;
    }
  }
  // counting rank = position in Python's stable sort(reverse=True): larger scores first, equal scores by index
  int rk = 0;
  for (int i = 0; i < n; ++i) {
    const float si = __shfl(s, i);
    const int ki = __shfl((int)kept, i);
    rk += (ki && (si > s || (si == s && i < j))) ? 1 : 0;
  }
  rk = kept ? rk : -1;
  if (in) rank[base + j] = rk;
  const int K = __popcll(__ballot(kept));
  // lane k looks at ranks k (winner) and k + 1 (loser); best_worst: lane 0 at ranks 0 and K - 1
  const int want_w = j, want_l = rule == 1 ? K - 1 : j + 1;
  int w = -1, l = -1;
  float sw = 0.f, sl = 0.f;
  for (int i = 0; i < n; ++i) {
    const float si = __shfl(s, i);
    const int ri = __shfl(rk, i);
    if (ri >= 0 && ri == want_w) { w = i; sw = si; }
    if (ri >= 0 && ri == want_l) { l = i; sl = si; }
  }
  const bool slot = rule == 1 ? (j == 0 && K >= 2) : (j + 1 < K);
  const float d = sw - sl;
  const bool emit = slot && w >= 0 && l >= 0 && d >= threshold;
  const unsigned long long bal = __ballot(emit);
  const int count = __popcll(bal);
  if (emit) {
    const int p = __popcll(bal & lanes_below(j));
    pair_win[base + p] = w;
    pair_lose[base + p] = l;
    pair_margin[base + p] = d;
  }
  if (in && j >= count) {  // unused slots hold a fixed value: the outputs are written in full
    pair_win[base + j] = -1;
    pair_lose[base + j] = -1;
    pair_margin[base + j] = 0.f;
  }
  if (j == 0) pair_count[b] = count;
}

// Workgroup b copies the pairs of image b to rows off_b .. off_b + count_b - 1 (off_b = the counts before it, summed by
// every wave for itself) and pads its share of the tail rows total .. cap - 1 (rows total + b, total + b + B, ...).
__global__ void pair_rows_kernel(const int* __restrict__ pair_win, const int* __restrict__ pair_lose,
                                 const float* __restrict__ pair_margin, const int* __restrict__ pair_count,
                                 const long long* __restrict__ dec_ids, const long long* __restrict__ dec_mask, int B,
                                 int n, int S, int cap, long long dec_pad, long long* __restrict__ pref_ids,
                                 long long* __restrict__ pref_mask, long long* __restrict__ rej_ids,
                                 long long* __restrict__ rej_mask, int* __restrict__ pair_image,
                                 float* __restrict__ pref_score, int* __restrict__ n_pairs) {
  const int b = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int most = n - 1;  // pairs one image can hold; a count outside [0, n - 1] is clamped, never followed
  int off = 0, total = 0;
  for (int i = lane; i < B; i += 64) {
    int c = pair_count[i];
    c = c < 0 ? 0 : (c > most ? most : c);
    total += c;
    if (i < b) off += c;
  }
  off = wave_sum(off);
  total = wave_sum(total);
  int count = pair_count[b];
  count = count < 0 ? 0 : (count > most ? most : count);
  if (b == 0 && threadIdx.x == 0) n_pairs[0] = total;
  for (int p = wave; p < count; p += WAVES) {
    const size_t row = (size_t)(off + p) * S;
    const int w = pair_win[(size_t)b * n + p], l = pair_lose[(size_t)b * n + p];
    const bool good = w >= 0 && w < n && l >= 0 && l < n;
    const size_t rw = ((size_t)b * n + (good ? w : 0)) * S, rl = ((size_t)b * n + (good ? l : 0)) * S;
    for (int t = lane; t < S; t += 64) {
      pref_ids[row + t] = good ? dec_ids[rw + t] : dec_pad;
      pref_mask[row + t] = good ? dec_mask[rw + t] : 0;
      rej_ids[row + t] = good ? dec_ids[rl + t] : dec_pad;
      rej_mask[row + t] = good ? dec_mask[rl + t] : 0;
    }
    if (lane == 0) {
      pair_image[off + p] = good ? b : -1;
      pref_score[off + p] = good ? pair_margin[(size_t)b * n + p] : 0.f;
    }
  }
  for (long long q = (long long)total + b + (long long)wave * B; q < cap; q += (long long)WAVES * B) {
    const size_t row = (size_t)q * S;
    for (int t = lane; t < S; t += 64) {
      pref_ids[row + t] = dec_pad;
      pref_mask[row + t] = 0;
      rej_ids[row + t] = dec_pad;
      rej_mask[row + t] = 0;
    }
    if (lane == 0) {
      pair_image[q] = -1;
      pref_score[q] = 0.f;
    }
  }
}

}  // namespace
}  // namespace pgca

using namespace pgca;

extern "C" int pgca_candidate_rows(const int64_t* cand, int32_t ld_cand, const int64_t* lengths, int32_t R, int32_t S,
                                   int32_t base_vocab, int32_t dec_vocab, int64_t dec_pad, int64_t text_pad,
                                   int64_t* dec_ids, int64_t* dec_mask, int64_t* text_ids, int32_t* text_mask,
                                   int32_t* text_len, int32_t* out_len, void* stream) {
  REQUIRE(cand && lengths, "pgca_candidate_rows");
  REQUIRE(dec_ids && dec_mask && text_ids && text_mask && text_len && out_len, "pgca_candidate_rows");
  REQUIRE(R > 0 && S > 0, "pgca_candidate_rows");
  REQUIRE(ld_cand >= 1, "pgca_candidate_rows");
  REQUIRE(base_vocab > 0 && dec_vocab >= base_vocab, "pgca_candidate_rows");
  hipLaunchKernelGGL(candidate_rows_kernel, dim3((R + WAVES - 1) / WAVES), dim3(64 * WAVES), 0, (hipStream_t)stream,
                     (const long long*)cand, ld_cand, (const long long*)lengths, R, S, (long long)base_vocab,
                     (long long)dec_vocab, (long long)dec_pad, (long long)text_pad, (long long*)dec_ids,
                     (long long*)dec_mask, (long long*)text_ids, text_mask, text_len, out_len);
  return check_launch("pgca_candidate_rows");
}

extern "C" int pgca_group_cosine(const float* img, const float* txt, int32_t B, int32_t n, int32_t P, float* score,
                                 void* stream) {
  REQUIRE(img && txt && score, "pgca_group_cosine");
  REQUIRE(B > 0 && n > 0 && P >= 1, "pgca_group_cosine");
  REQUIRE((long long)B * n <= 0x7fffffffLL, "pgca_group_cosine");
  const int R = B * n;
  hipLaunchKernelGGL(group_cosine_kernel, dim3((R + WAVES - 1) / WAVES), dim3(64 * WAVES), 0, (hipStream_t)stream, img,
                     txt, R, n, P, score);
  return check_launch("pgca_group_cosine");
}

extern "C" int pgca_mine_pairs(const float* score, const int64_t* dec_ids, const int32_t* out_len, const uint8_t* ok,
                               int32_t B, int32_t n, int32_t S, int32_t min_tokens, int32_t rule, float threshold,
                               int32_t* rank, int32_t* pair_win, int32_t* pair_lose, float* pair_margin,
                               int32_t* pair_count, void* stream) {
  REQUIRE(score && dec_ids && out_len, "pgca_mine_pairs");
  REQUIRE(rank && pair_win && pair_lose && pair_margin && pair_count, "pgca_mine_pairs");
  REQUIRE(n >= 1 && n <= 64, "pgca_mine_pairs");
  REQUIRE(B > 0 && S > 0, "pgca_mine_pairs");
  REQUIRE(rule == 0 || rule == 1, "pgca_mine_pairs");
  REQUIRE(threshold == threshold, "pgca_mine_pairs");
  hipLaunchKernelGGL(mine_pairs_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, score, (const long long*)dec_ids,
                     out_len, ok, n, S, min_tokens, rule, threshold, rank, pair_win, pair_lose, pair_margin, pair_count);
  return check_launch("pgca_mine_pairs");
}

extern "C" int pgca_pair_rows(const int32_t* pair_win, const int32_t* pair_lose, const float* pair_margin,
                              const int32_t* pair_count, const int64_t* dec_ids, const int64_t* dec_mask, int32_t B,
                              int32_t n, int32_t S, int32_t cap, int64_t dec_pad, int64_t* preferred_ids,
                              int64_t* preferred_mask, int64_t* rejected_ids, int64_t* rejected_mask,
                              int32_t* pair_image, float* preference_score, int32_t* n_pairs, void* stream) {
  REQUIRE(pair_win && pair_lose && pair_margin && pair_count && dec_ids && dec_mask, "pgca_pair_rows");
  REQUIRE(preferred_ids && preferred_mask && rejected_ids && rejected_mask && pair_image && preference_score && n_pairs,
          "pgca_pair_rows");
  REQUIRE(n >= 1 && n <= 64, "pgca_pair_rows");
  REQUIRE(B > 0 && S > 0, "pgca_pair_rows");
  REQUIRE(cap >= 1 && (long long)cap >= (long long)B * (n - 1), "pgca_pair_rows");
  hipLaunchKernelGGL(pair_rows_kernel, dim3(B), dim3(64 * WAVES), 0, (hipStream_t)stream, pair_win, pair_lose,
                     pair_margin, pair_count, (const long long*)dec_ids, (const long long*)dec_mask, B, n, S, cap,
                     (long long)dec_pad, (long long*)preferred_ids, (long long*)preferred_mask,
                     (long long*)rejected_ids, (long long*)rejected_mask, pair_image, preference_score, n_pairs);
  return check_launch("pgca_pair_rows");
}
