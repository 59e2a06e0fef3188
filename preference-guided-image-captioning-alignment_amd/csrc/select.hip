// Token selection after the LM head (reference model.py:621-678 -> HF generate's logits processors, sampling and
// beam-candidate ranking): pgca_select_token(_ex) and pgca_select_beam_candidates(_ex).
//
// A row of 50 260 f32 logits (200 KB) does not fit the LDS, and sorting it is what the torch path pays for.  Both kernels
// instead make several passes over the row (L2 hits after the first): max, sum-exp, then a 4-bit-per-pass radix select
// on the order-preserving bit pattern of the processed score - weighted by count for top-k / top-K and by probability
// mass for top-p - and finally a prefix scan in token-id order for the draw.  One 1024-thread workgroup serves a row
// (token kernel) or a batch item's nb rows (beam kernel); wave w owns a contiguous slice of the row and reads it with
// float4 loads.  Every sum is a fixed-order tree (lane-sequential, wave butterfly, 16 wave totals in order): there are
// no float atomics, so results are bit-identical from run to run.  The only LDS atomics are integer (seen-id and
// banned-id bitmasks, candidate slots), whose outcome does not depend on arrival order once the candidates are ranked.
// The _ex entries add a second bitmask plane per row: the ids HF's NoRepeatNGram / MinLength / SuppressTokens
// processors set to -inf.
#include "common.h"

#include <math.h>

namespace pgca {
namespace {

constexpr int SEL_THREADS = 1024;
constexpr int SEL_WAVES = SEL_THREADS / 64;
constexpr int SEL_CAP = 128;     // candidate slots of the beam kernel (K <= 64 plus ties)
constexpr int SEL_MAX_NB = 32;
constexpr float GUMBEL_MAX = 17.5f;  // -log(-log(1 - 2^-25)) = 17.33: no key exceeds acc + GUMBEL_MAX

struct SelScratch {
  float red[SEL_WAVES];
  unsigned long long red64[SEL_WAVES];
  float hist[SEL_WAVES][16];
  float tot[16];
};

// order-preserving map f32 -> u32 (a < b  <=>  okey(a) < okey(b); -inf lowest, +inf highest) and its inverse
__device__ __forceinline__ unsigned okey(float f) {
  const unsigned b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float okey_inv(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// One logits row seen through HF's processors: repetition penalty (once per distinct seen id: the ids are a bitmask),
// then the bans (-inf whatever the penalty made of the score), then - when warping - the temperature.  For the beam
// kernel the processors act on log-probabilities: ``shift`` is the row's max and ``shift_log`` the log of its sum-exp,
// subtracted one after the other as torch's log_softmax does (their sum, rounded once at magnitude ~30, would cost
// 1e-6); both are 0 for the token kernel.
struct RowView {
  const float* x;
  const unsigned* seen;  // LDS bitmask over [0, V), or nullptr
  const unsigned* ban;   // LDS bitmask of the banned ids, or nullptr
  int V, nvec;
  float shift, shift_log, penalty, temperature;
  bool warp;
  __device__ __forceinline__ float score(float xv, int j) const {
    float s = (xv - shift) - shift_log;
    if (seen && ((seen[j >> 5] >> (j & 31)) & 1u)) s = s < 0.f ? s * penalty : s / penalty;
    if (ban && ((ban[j >> 5] >> (j & 31)) & 1u)) s = -INFINITY;
    if (warp) s = s / temperature;
    return s + 0.0f;  // -0 -> +0: one key per value
  }
};

// f(j, x[j]) for every j < V: wave w owns vectors [w * per, (w + 1) * per), lanes stride float4
template <class F>
__device__ __forceinline__ void for_each(const RowView& r, F f) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int per = (r.nvec + SEL_WAVES - 1) / SEL_WAVES;
  const int beg = wave * per, end = min(beg + per, r.nvec);
  for (int v = beg + lane; v < end; v += 64) {
    const float4 q = reinterpret_cast<const float4*>(r.x)[v];
    const int j = v * 4;
    f(j, q.x);
    if (j + 1 < r.V) f(j + 1, q.y);
    if (j + 2 < r.V) f(j + 2, q.z);
    if (j + 3 < r.V) f(j + 3, q.w);
  }
}

__device__ __forceinline__ float block_sum(float v, SelScratch& sm) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sm.red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int w = 0; w < SEL_WAVES; ++w) t += sm.red[w];
  __syncthreads();
  return t;
}
__device__ __forceinline__ float block_max(float v, SelScratch& sm) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) sm.red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = sm.red[0];
#pragma unroll
  for (int w = 1; w < SEL_WAVES; ++w) t = fmaxf(t, sm.red[w]);
  __syncthreads();
  return t;
}
__device__ __forceinline__ unsigned long long block_max64(unsigned long long v, SelScratch& sm) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long n = __shfl_xor(v, o);
    v = n > v ? n : v;
  }
  if ((threadIdx.x & 63) == 0) sm.red64[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long t = sm.red64[0];
#pragma unroll
  for (int w = 1; w < SEL_WAVES; ++w) t = sm.red64[w] > t ? sm.red64[w] : t;
  __syncthreads();
  return t;
}

// (score, id) -> one u64 whose maximum is the highest score, lowest id among equals
__device__ __forceinline__ unsigned long long pack_best(float s, int j) {
  return ((unsigned long long)okey(s) << 32) | (unsigned)(0xffffffffu - (unsigned)j);
}

// Smallest 32-bit key v with  W(key <= v) > thr,  W = sum of the weights: 8 passes of 4 bits, 16 per-thread bins.
// ``visit(f, lo)`` calls f(key, weight_fn) for every element; ``lo`` is the lowest value the keys still in play can
// have (NaN on the first pass), so a visitor may skip an element it can bound below ``lo`` without computing its key.
// Returns 0xffffffff-ish prefixes when no key qualifies (callers clamp to the largest key present).
template <class Visit>
__device__ unsigned radix_select(Visit visit, float thr, SelScratch& sm, float* below, float* at, int top_shift = 28) {
  unsigned prefix = 0;
  float base = 0.f, chosen = 0.f;
  for (int shift = top_shift; shift >= 0; shift -= 4) {
    float acc[16];
#pragma unroll
    for (int b = 0; b < 16; ++b) acc[b] = 0.f;
    const unsigned himask = shift >= 28 ? 0u : (0xffffffffu << (shift + 4));
    visit(
        [&](unsigned key, auto weight) {
          if (((key ^ prefix) & himask) == 0u) {
            const unsigned d = (key >> shift) & 15u;
            const float w = weight();
#pragma unroll
            for (int b = 0; b < 16; ++b) acc[b] += (d == (unsigned)b) ? w : 0.f;
          }
        },
        okey_inv(prefix));
#pragma unroll
    for (int b = 0; b < 16; ++b) acc[b] = wave_sum(acc[b]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int b = 0; b < 16; ++b) sm.hist[threadIdx.x >> 6][b] = acc[b];
    }
    __syncthreads();
    if (threadIdx.x < 16) {
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < SEL_WAVES; ++w) t += sm.hist[w][threadIdx.x];
      sm.tot[threadIdx.x] = t;
    }
    __syncthreads();
    float run = base;
    unsigned digit = 15u;
    bool found = false;
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const float t = sm.tot[b];
      if (!found) {
        if (run + t > thr) {
          found = true;
          digit = b;
          chosen = t;
        } else if (b < 15) {
          run += t;
        } else {
          chosen = t;
        }
      }
    }
    base = run;
    prefix |= digit << shift;
  }
  if (below) *below = base;
  if (at) *at = chosen;
  return prefix;
}

// bitmask of the distinct ids in prev[0 .. n_prev): the penalty is applied once per id however often it occurs
__device__ __forceinline__ void build_seen(unsigned* seen, int words, const long long* prev, int n_prev, int V) {
  for (int i = threadIdx.x; i < words; i += SEL_THREADS) seen[i] = 0u;
  __syncthreads();
  for (int i = threadIdx.x; i < n_prev; i += SEL_THREADS) {
    const long long id = prev[i];
    if (id >= 0 && id < V) atomicOr(&seen[id >> 5], 1u << (id & 31));
  }
  __syncthreads();
}

// bitmask of the ids banned for one row: HF's NoRepeatNGramLogitsProcessor (n > 0: the token that followed every
// earlier occurrence of the row's last n - 1 ids; n == 1: every seen id; fewer than n - 1 ids: nothing) and a list
// banned in every row.  Ids outside [0, V) are ignored.
__device__ __forceinline__ void build_ban(unsigned* ban, int words, const long long* prev, int n_prev, int V, int n,
                                          const long long* ban_ids, int n_ban) {
  for (int i = threadIdx.x; i < words; i += SEL_THREADS) ban[i] = 0u;
  __syncthreads();
  if (n > 0 && n_prev >= n) {
    const long long* tail = prev + (n_prev - n + 1);   // the last n - 1 ids (read only when i < n_prev - n + 1)
    for (int i = threadIdx.x; i < n_prev - n + 1; i += SEL_THREADS) {
      bool match = true;
      for (int k = 0; k < n - 1; ++k) match = match && prev[i + k] == tail[k];
      const long long id = prev[i + n - 1];
      if (match && id >= 0 && id < V) atomicOr(&ban[id >> 5], 1u << (id & 31));
    }
  }
  for (int i = threadIdx.x; i < n_ban; i += SEL_THREADS) {
    const long long id = ban_ids[i];
    if (id >= 0 && id < V) atomicOr(&ban[id >> 5], 1u << (id & 31));
  }
  __syncthreads();
}

// Threshold key of the warpers for one row: a token is kept iff okey(score) >= the returned key.
//   top-k: strictly below the k-th largest goes (ties with the k-th stay);
//   top-p: ascending, a class of equal scores goes iff the cumulative probability up to and including it is
//          <= 1 - top_p (softmax over what top-k kept); the largest always stays.
__device__ unsigned warp_threshold(const RowView& r, unsigned key_max, int top_k, float top_p, SelScratch& sm) {
  const float m = okey_inv(key_max);
  unsigned tk = 0u;
  if (top_k > 0 && top_k < r.V) {
    auto visit = [&](auto f, float) {
      for_each(r, [&](int j, float xv) { f(okey(r.score(xv, j)), [] { return 1.f; }); });
    };
    tk = radix_select(visit, (float)(r.V - top_k), sm, nullptr, nullptr);
  }
  unsigned tp = 0u;
  if (top_p < 1.f) {
    float z = 0.f;
    for_each(r, [&](int j, float xv) {
      const float s = r.score(xv, j);
      if (okey(s) >= tk) z += expf(s - m);
    });
    z = block_sum(z, sm);
    auto visit = [&](auto f, float) {
      for_each(r, [&](int j, float xv) {
        const float s = r.score(xv, j);
        const unsigned k = okey(s);
        if (k >= tk) f(k, [&] { return expf(s - m); });
      });
    };
    tp = radix_select(visit, (1.f - top_p) * z, sm, nullptr, nullptr);
  }
  const unsigned t = tk > tp ? tk : tp;
  return t < key_max ? t : key_max;
}

__global__ __launch_bounds__(SEL_THREADS) void select_token_kernel(
    const float* __restrict__ logits, int ld, int V, const long long* __restrict__ prev, int ld_prev, int n_prev,
    float penalty, float temperature, int top_k, float top_p, const float* __restrict__ u,
    const unsigned char* __restrict__ done, long long pad_id, long long* __restrict__ next,
    float* __restrict__ next_logp, int ngram, const long long* __restrict__ ban_ids, int n_ban) {
  extern __shared__ unsigned seen_lds[];
  __shared__ SelScratch sm;
  __shared__ int pick;
  const int row = blockIdx.x;
  if (done && done[row]) {
    if (threadIdx.x == 0) {
      next[row] = pad_id;
      next_logp[row] = 0.f;
    }
    return;
  }
  const bool sample = u != nullptr;
  RowView r;
  r.x = logits + (size_t)row * ld;
  r.V = V;
  r.nvec = (V + 3) / 4;
  r.shift = 0.f;
  r.shift_log = 0.f;
  r.penalty = penalty;
  r.temperature = temperature;
  r.warp = sample;
  r.seen = nullptr;
  if (penalty != 1.f && n_prev > 0) {
    build_seen(seen_lds, (V + 31) / 32, prev + (size_t)row * ld_prev, n_prev, V);
    r.seen = seen_lds;
  }
  r.ban = nullptr;
  if (ngram > 0 || n_ban > 0) {   // second plane, after the seen plane when there is one
    unsigned* ban = seen_lds + (r.seen ? (V + 31) / 32 : 0);
    build_ban(ban, (V + 31) / 32, prev + (size_t)row * ld_prev, n_prev, V, ngram, ban_ids, n_ban);
    r.ban = ban;
  }
  // pass 1: raw max (for the log-softmax) and the best processed score (lowest id among equals)
  float mr = -INFINITY;
  unsigned long long best = 0ull;
  for_each(r, [&](int j, float xv) {
    mr = fmaxf(mr, xv);
    const unsigned long long c = pack_best(r.score(xv, j), j);
    best = c > best ? c : best;
  });
  mr = block_max(mr, sm);
  best = block_max64(best, sm);
  // pass 2: normaliser of the raw logits
  float zr = 0.f;
  for_each(r, [&](int, float xv) { zr += expf(xv - mr); });
  zr = block_sum(zr, sm);
  int chosen = best ? (int)(0xffffffffu - (unsigned)(best & 0xffffffffull)) : 0;   // all-NaN row: id 0
  // every token banned: the lowest id (``best`` above), nothing to draw from
  if (sample && (unsigned)(best >> 32) > okey(-INFINITY)) {
    const unsigned key_max = (unsigned)(best >> 32);
    const float m = okey_inv(key_max);
    const unsigned t = warp_threshold(r, key_max, top_k, top_p, sm);
    // draw: inverse CDF over the kept tokens in id order.  Prefix of an element = (total of the waves before) + (total of
    // this wave's earlier iterations) + (inclusive lane scan); the second sweep repeats the first's operations, so the
    // crossing it finds is consistent with the totals that chose the wave.
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int per = (r.nvec + SEL_WAVES - 1) / SEL_WAVES;
    const int beg = wave * per, end = min(beg + per, r.nvec);
    auto sweep = [&](float before, float target, bool find) -> float {
      float carry = 0.f;
      int last_kept = -1, hit = -1;
      for (int v0 = beg; v0 < end && hit < 0; v0 += 64) {
        const int v = v0 + lane;
        float w[4] = {0.f, 0.f, 0.f, 0.f};
        if (v < end) {
          const float4 q = reinterpret_cast<const float4*>(r.x)[v];
          const float xs[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int j = v * 4 + c;
            if (j < V) {
              const float s = r.score(xs[c], j);
              if (okey(s) >= t) w[c] = expf(s - m);
            }
          }
        }
        const float ls = ((w[0] + w[1]) + w[2]) + w[3];
        float sc = ls;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const float n = __shfl_up(sc, o);
          if (lane >= o) sc += n;
        }
        if (find) {
          float excl = __shfl_up(sc, 1);
          if (lane == 0) excl = 0.f;
          const unsigned long long kept = __ballot(ls > 0.f);
          const unsigned long long cross = __ballot(ls > 0.f && before + (carry + sc) >= target);
          const int src = cross ? __ffsll((long long)cross) - 1 : (kept ? 63 - __clzll((long long)kept) : -1);
          if (src >= 0 && lane == src) {   // first component that crosses, else the lane's last kept one
            float run = 0.f;
            int lastc = 0, got = -1;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              if (w[c] > 0.f) {
                run += w[c];
                lastc = c;
                if (got < 0 && before + (carry + (excl + run)) >= target) got = c;
              }
            }
            last_kept = v * 4 + (got >= 0 ? got : lastc);
          }
          if (src >= 0) last_kept = __shfl(last_kept, src);
          if (cross) hit = last_kept;
        }
        carry += __shfl(sc, 63);
      }
      if (find && lane == 0) pick = hit >= 0 ? hit : last_kept;
      return carry;
    };
    const float mine = sweep(0.f, 0.f, false);
    if (lane == 0) sm.red[wave] = mine;
    __syncthreads();
    float z = 0.f, before = 0.f;
    for (int w = 0; w < SEL_WAVES; ++w) z += sm.red[w];
    const float target = fmaxf(u[row] * z, 1.17549435e-38f);
    int wsel = SEL_WAVES - 1;
    {
      float run = 0.f;
      bool found = false;
      for (int w = 0; w < SEL_WAVES; ++w) {
        if (!found) {
          if (run + sm.red[w] >= target) {
            found = true;
            wsel = w;
            before = run;
          } else {
            run += sm.red[w];
          }
        }
      }
      if (!found) {   // rounding left the total short of the target: the last wave that holds mass
        run = 0.f;
        for (int w = 0; w < SEL_WAVES; ++w) {
          if (sm.red[w] > 0.f) {
            wsel = w;
            before = run;
          }
          run += sm.red[w];
        }
      }
    }
    if (threadIdx.x == 0) pick = chosen;   // the argmax is always kept: the answer should the sweep find nothing
    __syncthreads();
    if (wave == wsel) sweep(before, target, true);
    __syncthreads();
    chosen = pick >= 0 ? pick : chosen;
  }
  if (threadIdx.x == 0) {
    next[row] = chosen;
    next_logp[row] = (r.x[chosen] - mr) - logf(zr);
  }
}

// Gumbel noise of one candidate: u = ((hash32(flat * 0x9E3779B1 + seed) >> 8) + 0.5) * 2^-24, g = -log(-log u).
// -log u is formed from whichever of u, 1 - u is exact in f32, so u near 1 does not round to 1.
__device__ __forceinline__ float gumbel(unsigned flat, unsigned seed) {
  const unsigned n = hash32(flat * 0x9E3779B1u + seed) >> 8;
  float t;
  if (n < (1u << 23)) {
    t = -logf(((float)n + 0.5f) * 5.9604644775390625e-8f);
  } else {
    t = -log1pf(-((float)((1u << 24) - n) - 0.5f) * 5.9604644775390625e-8f);
  }
  return -logf(t);
}

__global__ __launch_bounds__(SEL_THREADS) void select_beam_kernel(
    const float* __restrict__ logits, int ld, int V, int nb, const long long* __restrict__ prev, int ld_prev,
    int n_prev, float penalty, int warp, float temperature, int top_k, float top_p,
    const float* __restrict__ beam_scores, int K, int use_noise, unsigned noise_seed, float* __restrict__ cand_score,
    long long* __restrict__ cand_index, int ngram, const long long* __restrict__ ban_ids, int n_ban) {
  extern __shared__ unsigned seen_lds[];
  __shared__ SelScratch sm;
  __shared__ float row_max[SEL_MAX_NB], row_logz[SEL_MAX_NB], row_bs[SEL_MAX_NB];
  __shared__ unsigned row_thr[SEL_MAX_NB];
  __shared__ unsigned ckey[SEL_CAP], cidx[SEL_CAP];
  __shared__ float cacc[SEL_CAP];
  __shared__ int ncand;
  const int b = blockIdx.x;
  const int words = (V + 31) / 32;
  const bool pen = penalty != 1.f && n_prev > 0;
  const bool bans = ngram > 0 || n_ban > 0;
  unsigned* ban_lds = seen_lds + (pen ? (size_t)nb * words : 0);   // the ban planes follow the seen planes
  auto view = [&](int i) {
    RowView r;
    r.x = logits + (size_t)(b * nb + i) * ld;
    r.V = V;
    r.nvec = (V + 3) / 4;
    r.penalty = penalty;
    r.temperature = temperature;
    r.warp = warp != 0;
    r.seen = pen ? seen_lds + (size_t)i * words : nullptr;
    r.ban = bans ? ban_lds + (size_t)i * words : nullptr;
    r.shift = 0.f;
    r.shift_log = 0.f;
    return r;
  };
  // per row: log-softmax normaliser, then the warpers' threshold on the processed log-probabilities
  for (int i = 0; i < nb; ++i) {
    RowView r = view(i);
    if (pen) build_seen(seen_lds + (size_t)i * words, words, prev + (size_t)(b * nb + i) * ld_prev, n_prev, V);
    if (bans) {
      build_ban(ban_lds + (size_t)i * words, words, prev + (size_t)(b * nb + i) * ld_prev, n_prev, V, ngram, ban_ids,
                n_ban);
    }
    float mr = -INFINITY;
    for_each(r, [&](int, float xv) { mr = fmaxf(mr, xv); });
    mr = block_max(mr, sm);
    float zr = 0.f;
    for_each(r, [&](int, float xv) { zr += expf(xv - mr); });
    zr = block_sum(zr, sm);
    r.shift = mr;
    r.shift_log = logf(zr);
    unsigned thr = 0u;
    if (warp && ((top_k > 0 && top_k < V) || top_p < 1.f)) {
      unsigned long long best = 0ull;
      for_each(r, [&](int j, float xv) {
        const unsigned long long c = pack_best(r.score(xv, j), j);
        best = c > best ? c : best;
      });
      best = block_max64(best, sm);
      if ((unsigned)(best >> 32) > okey(-INFINITY)) thr = warp_threshold(r, (unsigned)(best >> 32), top_k, top_p, sm);
    }
    if (threadIdx.x == 0) {
      row_max[i] = r.shift;
      row_logz[i] = r.shift_log;
      row_thr[i] = thr;
      row_bs[i] = beam_scores[b * nb + i];
    }
  }
  if (threadIdx.x == 0) ncand = 0;
  __syncthreads();
  const unsigned KEY_NINF = okey(-INFINITY);
  // g(flat, acc, key_fn) for every candidate of the batch item; ``lo``: see radix_select
  auto candidates = [&](auto g, float lo) {
    for (int i = 0; i < nb; ++i) {
      RowView r = view(i);
      r.shift = row_max[i];
      r.shift_log = row_logz[i];
      const unsigned thr = row_thr[i];
      const float bs = row_bs[i];
      const unsigned f0 = (unsigned)i * (unsigned)V;
      const unsigned h0 = (unsigned)(b * nb + i) * (unsigned)V;   // noise index: distinct across batch items
      for_each(r, [&](int j, float xv) {
        const float s = r.score(xv, j);
        if (okey(s) < thr) {
          g(f0 + j, -INFINITY, [&] { return KEY_NINF; });
        } else {
          const float acc = s + bs;
          if (!use_noise) {
            g(f0 + j, acc, [&] { return okey(acc); });
          } else if (!(acc + GUMBEL_MAX < lo)) {
            g(f0 + j, acc, [&] { return okey(acc + gumbel(h0 + j, noise_seed)); });
          }
        }
      });
    }
  };
  // the K-th largest key: ascending rank N - K + 1
  const int N = nb * V;
  auto by_key = [&](auto f, float lo) {
    candidates([&](unsigned, float, auto key) { f(key(), [] { return 1.f; }); }, lo);
  };
  float below = 0.f, at = 0.f;
  const unsigned kth = radix_select(by_key, (float)(N - K), sm, &below, &at);
  const float n_gt = (float)N - below - at;   // counts are exact in f32 (N < 2^24)
  // more ties with the K-th key than slots: the lowest flat indices among them fill what is left
  unsigned idx_cut = 0xffffffffu;
  if (n_gt + at > (float)SEL_CAP) {
    auto by_index = [&](auto f, float) {
      candidates([&](unsigned flat, float, auto key) { if (key() == kth) f(flat, [] { return 1.f; }); }, okey_inv(kth));
    };
    idx_cut = radix_select(by_index, (float)K - n_gt - 1.f, sm, nullptr, nullptr, 20);
  }
  candidates(
      [&](unsigned flat, float acc, auto key) {
        const unsigned k = key();
        if (k > kth || (k == kth && flat <= idx_cut)) {
          const int slot = atomicAdd(&ncand, 1);
          if (slot < SEL_CAP) {
            ckey[slot] = k;
            cacc[slot] = acc;
            cidx[slot] = flat;
          }
        }
      },
      okey_inv(kth));
  __syncthreads();
  const int n = min(ncand, SEL_CAP);
  if ((int)threadIdx.x < n) {   // rank by (key descending, flat index ascending)
    const unsigned k = ckey[threadIdx.x], f = cidx[threadIdx.x];
    int rank = 0;
    for (int o = 0; o < n; ++o) rank += (ckey[o] > k || (ckey[o] == k && cidx[o] < f)) ? 1 : 0;
    if (rank < K) {
      cand_score[(size_t)b * K + rank] = cacc[threadIdx.x];
      cand_index[(size_t)b * K + rank] = f;
    }
  }
}

constexpr size_t SEL_MAX_DYN_LDS = 60 * 1024;

}  // namespace
}  // namespace pgca

using namespace pgca;

namespace {
const pgca_select_opts NO_OPTS = {0, 0, nullptr};
}

extern "C" int pgca_select_token_ex(const float* logits, int32_t ld, int32_t V, int32_t R, const int64_t* prev,
                                    int32_t ld_prev, int32_t n_prev, float repetition_penalty, float temperature,
                                    int32_t top_k, float top_p, const float* u, const uint8_t* done, int64_t pad_id,
                                    int64_t* next, float* next_logp, const pgca_select_opts* opts, void* stream) {
  REQUIRE(logits && next && next_logp && R > 0 && V > 0 && ld >= V && (ld % 4) == 0 &&
              (((uintptr_t)logits & 15) == 0) && n_prev >= 0 && (n_prev == 0 || (prev && ld_prev >= n_prev)) &&
              repetition_penalty > 0.f && temperature > 0.f && top_k >= 0 && top_p > 0.f && opts &&
              opts->no_repeat_ngram_size >= 0 && opts->n_ban >= 0 && (opts->n_ban == 0 || opts->ban_ids),
          "pgca_select_token");
  const size_t plane = (size_t)((V + 31) / 32) * 4;
  const size_t lds = ((repetition_penalty != 1.f && n_prev > 0) ? plane : 0) +
                     ((opts->no_repeat_ngram_size > 0 || opts->n_ban > 0) ? plane : 0);
  if (lds > SEL_MAX_DYN_LDS) {
    set_error("pgca_select_token: the seen-id and banned-id bitmasks need more than the 61440 bytes of LDS available");
    return PGCA_ERR_INVALID;
  }
  hipLaunchKernelGGL(select_token_kernel, dim3(R), dim3(SEL_THREADS), lds, (hipStream_t)stream, logits, ld, V,
                     (const long long*)prev, ld_prev, n_prev, repetition_penalty, temperature, top_k, top_p, u, done,
                     (long long)pad_id, (long long*)next, next_logp, opts->no_repeat_ngram_size,
                     (const long long*)opts->ban_ids, opts->n_ban);
  return check_launch("pgca_select_token");
}

extern "C" int pgca_select_token(const float* logits, int32_t ld, int32_t V, int32_t R, const int64_t* prev,
                                 int32_t ld_prev, int32_t n_prev, float repetition_penalty, float temperature,
                                 int32_t top_k, float top_p, const float* u, const uint8_t* done, int64_t pad_id,
                                 int64_t* next, float* next_logp, void* stream) {
  return pgca_select_token_ex(logits, ld, V, R, prev, ld_prev, n_prev, repetition_penalty, temperature, top_k, top_p, u,
                              done, pad_id, next, next_logp, &NO_OPTS, stream);
}

extern "C" int pgca_select_beam_candidates_ex(const float* logits, int32_t ld, int32_t V, int32_t B, int32_t nb,
                                              const int64_t* prev, int32_t ld_prev, int32_t n_prev,
                                              float repetition_penalty, int32_t warp, float temperature, int32_t top_k,
                                              float top_p, const float* beam_scores, int32_t K, int32_t use_noise,
                                              uint32_t noise_seed, float* cand_score, int64_t* cand_index,
                                              const pgca_select_opts* opts, void* stream) {
  REQUIRE(logits && beam_scores && cand_score && cand_index && B > 0 && nb > 0 && nb <= SEL_MAX_NB && V > 0 &&
              ld >= V && (ld % 4) == 0 && (((uintptr_t)logits & 15) == 0) && n_prev >= 0 &&
              (n_prev == 0 || (prev && ld_prev >= n_prev)) && repetition_penalty > 0.f && temperature > 0.f &&
              top_k >= 0 && top_p > 0.f && K > 0 && K <= 64 && (int64_t)nb * V >= K &&
              (int64_t)nb * V < (1 << 24) && opts && opts->no_repeat_ngram_size >= 0 && opts->n_ban >= 0 &&
              (opts->n_ban == 0 || opts->ban_ids),
          "pgca_select_beam_candidates");
  const size_t plane = (size_t)nb * ((V + 31) / 32) * 4;
  const size_t lds = ((repetition_penalty != 1.f && n_prev > 0) ? plane : 0) +
                     ((opts->no_repeat_ngram_size > 0 || opts->n_ban > 0) ? plane : 0);
  if (lds > SEL_MAX_DYN_LDS) {
    set_error("pgca_select_beam_candidates: the seen-id and banned-id bitmasks of nb rows need more than the 61440 "
              "bytes of LDS available");
    return PGCA_ERR_INVALID;
  }
  hipLaunchKernelGGL(select_beam_kernel, dim3(B), dim3(SEL_THREADS), lds, (hipStream_t)stream, logits, ld, V, nb,
                     (const long long*)prev, ld_prev, n_prev, repetition_penalty, warp, temperature, top_k, top_p,
                     beam_scores, K, use_noise, noise_seed, cand_score, (long long*)cand_index,
                     opts->no_repeat_ngram_size, (const long long*)opts->ban_ids, opts->n_ban);
  return check_launch("pgca_select_beam_candidates");
}

extern "C" int pgca_select_beam_candidates(const float* logits, int32_t ld, int32_t V, int32_t B, int32_t nb,
                                           const int64_t* prev, int32_t ld_prev, int32_t n_prev,
                                           float repetition_penalty, int32_t warp, float temperature, int32_t top_k,
                                           float top_p, const float* beam_scores, int32_t K, int32_t use_noise,
                                           uint32_t noise_seed, float* cand_score, int64_t* cand_index, void* stream) {
  return pgca_select_beam_candidates_ex(logits, ld, V, B, nb, prev, ld_prev, n_prev, repetition_penalty, warp,
                                        temperature, top_k, top_p, beam_scores, K, use_noise, noise_seed, cand_score,
                                        cand_index, &NO_OPTS, stream);
}
