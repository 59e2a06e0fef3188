// One step of HF's beam-search bookkeeping (transformers 5.x generation/utils.py: _get_top_k_continuations,
// _get_running_beams_for_next_iteration, _update_finished_beams, _check_early_stop_heuristic) in one launch:
// pgca_beam_step.  It follows pgca_select_beam_candidates, which leaves K = 2 * nb ranked candidates per batch item.
//
// One 256-thread workgroup per batch item; nothing is shared between workgroups.  Everything but the sequence rows is
// a few dozen scalars: they are read into the LDS, ranked there by counting (rank = how many entries beat this one -
// score descending, then merged index ascending, which fixes the order torch.topk leaves open for equal keys) and
// written back in place once every read is done.  Sequence rows are gathered from one buffer of a ping-pong pair into
// the other, columns 0 .. cur only: later columns hold the pad id in both buffers from their allocation on.
// HF masks with additive -1e9 terms, not selects; the terms are added here in HF's order, in float32, as HF does.
#include "common.h"

#include <math.h>

namespace pgca {
namespace {

constexpr int BEAM_THREADS = 256;
constexpr int BEAM_MAX_NB = 32;
constexpr int BEAM_MAX_K = 2 * BEAM_MAX_NB;
constexpr float MASKED = -1.0e9f;

// a before b: score descending, then index ascending
__device__ __forceinline__ bool beats(float sa, int ia, float sb, int ib) { return sa > sb || (sa == sb && ia < ib); }

__global__ __launch_bounds__(BEAM_THREADS) void beam_step_kernel(
    const float* __restrict__ cand_score, const long long* __restrict__ cand_index, int nb, int V, int cur, int L,
    long long eos, float inv_fin, float inv_best, int early_stopping, const long long* __restrict__ running_in,
    long long* __restrict__ running_out, float* __restrict__ running_beam_scores,
    const long long* __restrict__ sequences_in, long long* __restrict__ sequences_out, float* __restrict__ beam_scores,
    unsigned char* __restrict__ is_sent_finished, long long* __restrict__ gen_len, unsigned char* __restrict__ unsat,
    long long* __restrict__ tok, long long* __restrict__ flat_src, unsigned char* __restrict__ hits_all) {
  __shared__ int src[BEAM_MAX_K];            // candidate -> the running beam it continues
  __shared__ long long tid[BEAM_MAX_K];      // candidate -> its token
  __shared__ int hit[BEAM_MAX_K];
  __shared__ float run_lp[BEAM_MAX_K];
  __shared__ float m_sc[BEAM_MAX_NB + BEAM_MAX_K];   // merged scores: the pool, then the candidates
  __shared__ int old_fin[BEAM_MAX_NB];
  __shared__ long long old_len[BEAM_MAX_NB];
  __shared__ int nxt[BEAM_MAX_NB];           // running slot -> candidate
  __shared__ int keep[BEAM_MAX_NB];          // pool slot -> merged index
  const int b = blockIdx.x, t = threadIdx.x;
  const int K = 2 * nb, M = nb + K;
  const bool open = unsat[b] != 0;
  if (t < K) {
    const long long idx = cand_index[(size_t)b * K + t];
    const int s = (int)(idx / V);
    src[t] = min(max(s, 0), nb - 1);
    const long long id = idx - (long long)s * V;
    tid[t] = id;
    const int h = (id == eos || cur + 1 >= L) ? 1 : 0;
    hit[t] = h;
    run_lp[t] = cand_score[(size_t)b * K + t] + (float)h * MASKED;
  }
  if (t < nb) {
    m_sc[t] = beam_scores[b * nb + t];
    old_fin[t] = is_sent_finished[b * nb + t];
    old_len[t] = gen_len[b * nb + t];
    nxt[t] = t;    // NaN scores leave ranks unassigned: every slot still names a valid candidate
    keep[t] = t;
  }
  __syncthreads();
  if (t < K) {
    bool full = early_stopping == 1;
    for (int i = 0; i < nb; ++i) full = full && old_fin[i] != 0;
    const int just = (hit[t] && t < nb) ? 1 : 0;
    float f = cand_score[(size_t)b * K + t] * inv_fin;
    f += (float)(full ? 1 : 0) * MASKED;
    f += (float)(open ? 0 : 1) * MASKED;
    f += (float)(1 - just) * MASKED;
    m_sc[nb + t] = f;
    int rank = 0;
    for (int o = 0; o < K; ++o) rank += beats(run_lp[o], o, run_lp[t], t) ? 1 : 0;
    if (rank < nb) nxt[rank] = t;
  }
  __syncthreads();
  if (t < M) {
    int rank = 0;
    for (int o = 0; o < M; ++o) rank += beats(m_sc[o], o, m_sc[t], t) ? 1 : 0;
    if (rank < nb) keep[rank] = t;
  }
  __syncthreads();
  // scalars: every read of the old state is in the LDS by now
  if (t < nb) {
    const int c = nxt[t];
    running_beam_scores[b * nb + t] = run_lp[c];
    tok[b * nb + t] = tid[c];
    flat_src[b * nb + t] = (long long)b * nb + src[c];
    const int m = keep[t];
    beam_scores[b * nb + t] = m_sc[m];
    is_sent_finished[b * nb + t] = (unsigned char)(m < nb ? old_fin[m] : ((hit[m - nb] && m - nb < nb) ? 1 : 0));
    gen_len[b * nb + t] = m < nb ? old_len[m] : (long long)(cur + 1);
  }
  if (t == 0) {
    float worst = m_sc[keep[0]];
    for (int i = 1; i < nb; ++i) worst = fminf(worst, m_sc[keep[i]]);
    const float best = run_lp[nxt[0]] * inv_best;
    bool any = false;
    for (int i = 0; i < nb; ++i) {
      const int m = keep[i];
      const bool fin = m < nb ? old_fin[m] != 0 : (hit[m - nb] && m - nb < nb);
      any = any || best > (fin ? worst : MASKED);
    }
    unsat[b] = (unsigned char)((open && any) ? 1 : 0);
    bool all = true;
    for (int i = 0; i < K; ++i) all = all && hit[i] != 0;
    hits_all[b] = (unsigned char)(all ? 1 : 0);
  }
  // sequence rows, columns 0 .. cur
  const int cols = min(cur + 1, L);
  const size_t base = (size_t)b * nb * L;
  for (int e = t; e < nb * cols; e += BEAM_THREADS) {
    const int r = e / cols, c = e - r * cols;
    const int cn = nxt[r];
    running_out[base + (size_t)r * L + c] = c == cur ? tid[cn] : running_in[base + (size_t)src[cn] * L + c];
    const int m = keep[r];
    long long v;
    if (m < nb) {
      v = sequences_in[base + (size_t)m * L + c];
    } else {
      v = c == cur ? tid[m - nb] : running_in[base + (size_t)src[m - nb] * L + c];
    }
    sequences_out[base + (size_t)r * L + c] = v;
  }
}

}  // namespace
}  // namespace pgca

using namespace pgca;

extern "C" int pgca_beam_step(const float* cand_score, const int64_t* cand_index, int32_t B, int32_t nb, int32_t V,
                              int32_t cur, int32_t L, int64_t eos, float length_penalty, int32_t early_stopping,
                              const int64_t* running_in, int64_t* running_out, float* running_beam_scores,
                              const int64_t* sequences_in, int64_t* sequences_out, float* beam_scores,
                              uint8_t* is_sent_finished, int64_t* gen_len, uint8_t* unsat, int64_t* tok,
                              int64_t* flat_src, uint8_t* hits_all, void* stream) {
  if (!(cand_score && cand_index && running_in && running_out && running_beam_scores && sequences_in &&
        sequences_out && beam_scores && is_sent_finished && gen_len && unsat && tok && flat_src && hits_all &&
        running_in != running_out && sequences_in != sequences_out && B > 0 && nb > 0 && nb <= BEAM_MAX_NB && V > 0 &&
        cur >= 0 && cur < L && early_stopping >= 0 && early_stopping <= 2)) {
    set_error("pgca_beam_step: bad arguments (null or aliased buffer, nb outside [1, 32], cur outside [0, L), "
              "early_stopping outside {0, 1, 2})");
    return PGCA_ERR_INVALID;
  }
  // the scalars torch divides by are Python doubles rounded to f32; 1 / that in f32 is what its kernels multiply by
  const int hyp = (early_stopping == 2 && length_penalty > 0.f) ? L : cur + 1;
  const float inv_fin = 1.0f / (float)pow((double)(cur + 1), (double)length_penalty);
  const float inv_best = 1.0f / (float)pow((double)hyp, (double)length_penalty);
  hipLaunchKernelGGL(beam_step_kernel, dim3(B), dim3(BEAM_THREADS), 0, (hipStream_t)stream, cand_score,
                     (const long long*)cand_index, nb, V, cur, L, (long long)eos, inv_fin, inv_best, early_stopping,
                     (const long long*)running_in, (long long*)running_out, running_beam_scores,
                     (const long long*)sequences_in, (long long*)sequences_out, beam_scores, is_sent_finished,
                     (long long*)gen_len, unsat, (long long*)tok, (long long*)flat_src, hits_all);
  return check_launch("pgca_beam_step");
}
