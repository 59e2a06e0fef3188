// Key-tiled (flash-style) multi-head self-attention for head_dim 64 and every sequence length of the hot path:
// GPT-2 captions at S = 128 (one tile) and S = 256 (configs C4/C5, causal + key padding + replayed probability
// dropout), CLIP ViT-B/32 at T = 50 and ViT-L/14 at T = 257 (no mask).  Entry points: attention.hip.
//
// Forward: one workgroup (8 waves) per (head, batch, 128-query block); wave w owns 16 queries and sweeps the key
// tiles with an online softmax.  Scores are computed TRANSPOSED (S^t = K Q^t) so a lane holds 4 keys of ONE query per
// MFMA tile: the row maximum / sum are in-lane plus two shuffles, and - the point of the layout - the exponentiated
// accumulator IS the B operand of the next product O^t += V^t P^t (lane (g, n = query) holds the k-slots 8g..8g+7;
// the k-slot <-> key map is the bijection {32s+4g+j, 32s+16+4g+j} and the V^t fragment is read with the same
// map by ds_read_b64_tr_b16), so the probabilities never touch LDS.  O^t rows live on the same lanes as the softmax
// statistics, so the running rescale is a per-lane scalar.  O leaves through a wave-private LDS transpose as 16-byte
// row-contiguous stores.  One-tile sequences (S <= 128) take a four-wave kernel built from the same pieces: the two
// forward kernels agree bit for bit wherever both can run.
//
// Backward: one workgroup per (head, batch) sweeps (key block, query block) pairs.  S and dP are computed with the KEY
// on the lane, so P and dS accumulators feed dV^t += dO^t P and dK^t += Q^t dS directly as B operands; only dS crosses
// LDS (once, transposed, 8-byte stores) for dQ += dS K, whose accumulators stay in registers for every query block
// (template NQB <= 4, S <= 512): no atomics, nothing summed across workgroups, bitwise reproducible.
// Backward, split by role (S <= 1024): a dK/dV workgroup per 128-key block sweeps the query blocks, a dQ workgroup per
// 128-query block sweeps the key blocks, each holding ONE block's accumulators.  Both are built from the one-pass
// kernel's pieces, so every element sees the same products in the same order: the two entries agree bit for bit.
#include "common.h"

using namespace pgca;

namespace {

constexpr int TNT = 512;       // 8 waves
constexpr int TB = 128;        // rows per query / key block
constexpr int DH = 64;
constexpr int QS = 144;        // byte stride of a [.][64] bf16 row (128 + 16 pad)
constexpr int PS = 272;        // byte stride of a [.][128] bf16 row (256 + 16 pad)
constexpr int TILE_QKV = TB * QS;  // 18432
constexpr int TILE_P = TB * PS;    // 34816

// rows row0 .. row0+127 of a [S][64] head slice (row stride ld elements) -> LDS image, zero rows >= S; NT threads
template <int NT = TNT>
__device__ __forceinline__ void stage_rows(unsigned char* lds, const bf16_t* g, int ld, int row0, int S, int t) {
#pragma unroll
  for (int i = 0; i < 1024 / NT; ++i) {
    const int idx = t + NT * i;
    const int row = idx >> 3, c = idx & 7;
    u32x4 v = (u32x4){0u, 0u, 0u, 0u};
    if (row0 + row < S) v = *reinterpret_cast<const u32x4*>(g + (size_t)(row0 + row) * ld + c * 8);
    *reinterpret_cast<u32x4*>(lds + row * QS + c * 16) = v;
  }
}

// the same in two halves, so that the global loads of several tiles can be in flight together before any of them is waited for
template <int NT>
struct StageRegs {
  u32x4 v[1024 / NT];
};
template <int NT>
__device__ __forceinline__ void stage_load(StageRegs<NT>& r, const bf16_t* g, int ld, int row0, int S, int t) {
#pragma unroll
  for (int i = 0; i < 1024 / NT; ++i) {
    const int idx = t + NT * i;
    const int row = idx >> 3, c = idx & 7;
    r.v[i] = (u32x4){0u, 0u, 0u, 0u};
    if (row0 + row < S) r.v[i] = *reinterpret_cast<const u32x4*>(g + (size_t)(row0 + row) * ld + c * 8);
  }
}
template <int NT>
__device__ __forceinline__ void stage_store(const StageRegs<NT>& r, unsigned char* lds, int t) {
#pragma unroll
  for (int i = 0; i < 1024 / NT; ++i) {
    const int idx = t + NT * i;
    *reinterpret_cast<u32x4*>(lds + (idx >> 3) * QS + (idx & 7) * 16) = r.v[i];
  }
}

// MFMA operand whose 16 rows (A) / 16 columns (B) are image rows row0..row0+15 and whose k is contiguous (64-deep image)
__device__ __forceinline__ bf16x8 frag_rows64(const unsigned char* lds, int row0, int kk, int lane) {
  return *reinterpret_cast<const bf16x8*>(lds + (row0 + (lane & 15)) * QS + kk * 64 + (lane >> 4) * 16);
}
// k-strided fragment, standard k map: k-slot (g, j) <-> image row k0 + 8g + j; 16 columns at col0
__device__ __forceinline__ bf16x8 frag_tr(const unsigned char* lds, int stride, int k0, int col0, int lane) {
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const unsigned char* a0 = lds + (k0 + 8 * g + q) * stride + (col0 + 4 * p) * 2;
  return tr_frag(a0, a0 + 4 * stride);
}
// k-strided fragment, ACCUMULATOR k map: k-slot (g, j < 4) <-> row k0 + 4g + j, (g, j >= 4) <-> row k0 + 16 + 4g + j - 4:
// the order in which two stacked 16x16 accumulator tiles present their rows to a lane
__device__ __forceinline__ bf16x8 frag_tr_acc(const unsigned char* lds, int stride, int k0, int col0, int lane) {
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const unsigned char* a0 = lds + (k0 + 4 * g + q) * stride + (col0 + 4 * p) * 2;
  return tr_frag(a0, a0 + 16 * stride);
}
// two accumulator tiles -> the bf16 B operand (same k map as frag_tr_acc)
__device__ __forceinline__ bf16x8 pack_acc(const float (&lo)[4], const float (&hi)[4]) {
  u32x4 v;
  v[0] = pack2(lo[0], lo[1]);
  v[1] = pack2(lo[2], lo[3]);
  v[2] = pack2(hi[0], hi[1]);
  v[3] = pack2(hi[2], hi[3]);
  return __builtin_bit_cast(bf16x8, v);
}

// a wave's 16 x 64 bf16 tile, staged in its private LDS rows (row stride `stride` bytes, 128 bytes used per row),
// leaves as 16-byte stores: 8 lanes cover one 128-byte row
__device__ __forceinline__ void store_rows16(const unsigned char* stage, int stride, bf16_t* gbase, size_t grow_stride,
                                             int row0, int nrows_valid, int lane) {
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int cid = lane + 64 * it;
    const int row = cid >> 3, c = cid & 7;
    const u32x4 v = *reinterpret_cast<const u32x4*>(stage + row * stride + c * 16);
    if (row < nrows_valid) *reinterpret_cast<u32x4*>(gbase + (size_t)(row0 + row) * grow_stride + c * 8) = v;
  }
}

// ------------------------------------------------------------------------------------ both directions
// What a workgroup of either direction knows about its (head, sequence): the clamped length, the head's base in qkv and
// the thread indices.  row0 is the sequence's first token row (packed rows: see AttnProblem).
struct HeadSeq {
  const bf16_t* base;
  int row0, S, H, ld, b, t, lane, w, g, i16;
  unsigned bh;
};
__device__ __forceinline__ HeadSeq head_seq(const AttnProblem& a) {
  HeadSeq c;
  const int h = blockIdx.x;
  c.b = blockIdx.y;
  c.row0 = a.cu ? a.cu[c.b] : c.b * a.Sp;
  c.S = a.cu ? min(a.S, a.cu[c.b + 1] - c.row0) : a.S;
  c.H = a.heads * DH;
  c.ld = 3 * c.H;
  c.t = threadIdx.x;
  c.lane = c.t & 63;
  c.w = __builtin_amdgcn_readfirstlane(c.t >> 6);
  c.g = c.lane >> 4;
  c.i16 = c.lane & 15;
  c.base = a.qkv + (size_t)c.row0 * c.ld + h * DH;
  c.bh = (unsigned)c.b * a.heads + h;
  return c;
}

// validity of the 128 keys from k0 (folds key < S)
__device__ __forceinline__ void fill_kms(const AttnProblem& a, const HeadSeq& c, unsigned char* kms, int k0) {
  if (c.t < TB) kms[c.t] = (k0 + c.t < c.S && (!a.kmask || a.kmask[c.b * a.Sp + k0 + c.t] != 0)) ? 1 : 0;
}

// ------------------------------------------------------------------------------------ forward: the shared pieces
// A forward workgroup's LDS is K | V | kms; one (16-query block, key tile) step is score_step -> prob_step -> pv_step, and
// a block leaves through finish_block -> store_block.  Both kernels below are loops around these five, so every element
// sees the same products in the same order whichever kernel computes it: with an incoming maximum of -inf the key-tiled
// kernel's first rescale multiplies exact zeros, and the two agree bit for bit wherever both can run.
struct FwdBlock : HeadSeq {
  unsigned char *Ks, *Vs;  // [128][64] bf16 images of the current key tile
  unsigned char* kms;      // [128]
  bf16_t* obase;
  float* lse_row;          // NULL when the caller keeps no lse
};
__device__ __forceinline__ FwdBlock fwd_block(unsigned char* smem, const AttnFwd& a) {
  FwdBlock c;
  static_cast<HeadSeq&>(c) = head_seq(a);
  c.Ks = smem;
  c.Vs = smem + TILE_QKV;
  c.kms = smem + 2 * TILE_QKV;
  c.obase = a.out + (size_t)c.row0 * c.H + blockIdx.x * DH;
  c.lse_row = a.lse ? a.lse + (size_t)c.bh * a.Sp : nullptr;
  return c;
}

// lane (g, i16)'s share of the Q rows of a 16-query block as the B operand of S^t = K Q^t (n = query q), zero for q >= S
__device__ __forceinline__ void q_frags(const FwdBlock& c, int q, bf16x8 (&fq)[2]) {
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    u32x4 v = (u32x4){0u, 0u, 0u, 0u};
    if (q < c.S) v = *reinterpret_cast<const u32x4*>(c.base + (size_t)q * c.ld + kk * 32 + c.g * 8);
    fq[kk] = __builtin_bit_cast(bf16x8, v);
  }
}

// Scores of query q against the first ntile 16-key tiles of the staged key tile (keys k0 ..): scaled, -inf where the key
// is invalid (kms already folds key < S), past the diagonal or in a tile the block does not need.  The keys of a query
// live on (mi, g, r).  Returns the query's maximum folded with mx.
__device__ __forceinline__ float score_step(const AttnProblem& a, const FwdBlock& c, const bf16x8 (&fq)[2], int k0, int q,
                                            int ntile, float mx, f32x4 (&acc)[8]) {
  const float scale = 0.125f;
#pragma unroll
  for (int mi = 0; mi < 8; ++mi) {
    acc[mi] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (mi < ntile) {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
        acc[mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_rows64(c.Ks, mi * 16, kk, c.lane), fq[kk], acc[mi], 0, 0, 0);
    }
  }
#pragma unroll
  for (int mi = 0; mi < 8; ++mi) {
    // the 4 validity bytes of this lane's keys of tile mi in one LDS word
    const unsigned kv = *reinterpret_cast<const unsigned*>(c.kms + mi * 16 + c.g * 4);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int key = k0 + mi * 16 + c.g * 4 + r;
      const bool ok = mi < ntile && ((kv >> (8 * r)) & 1u) && (!a.causal || key <= q);
      const float s = ok ? acc[mi][r] * scale : -INFINITY;
      acc[mi][r] = s;
      mx = fmaxf(mx, s);
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16));
  return fmaxf(mx, __shfl_xor(mx, 32));
}

// Scores -> dropped probabilities exp(s - mx) * m, in place; returns this lane's share of the UNDROPPED row sum.
// Attention-probability dropout (GPT-2 attn_dropout, modeling_gpt2.py:66) acts on the NORMALISED probability: the mask
// multiplies the numerator only.
__device__ __forceinline__ float prob_step(const AttnProblem& a, const FwdBlock& c, int k0, int q, int ntile, float mx,
                                           f32x4 (&acc)[8]) {
  const unsigned dbase = (c.bh * a.Sp + q) * a.Sp;
  float psum = 0.f;
#pragma unroll
  for (int mi = 0; mi < 8; ++mi) {
    float dm[4] = {1.f, 1.f, 1.f, 1.f};
    if (a.drop.on() && mi < ntile) a.drop.mul4(dbase + (unsigned)(k0 + mi * 16 + c.g * 4), dm);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p = acc[mi][r] > -INFINITY ? __expf(acc[mi][r] - mx) : 0.f;
      psum += p;
      acc[mi][r] = p * dm[r];
    }
  }
  return psum;
}

// O^t[d][q] += V^t[d][key] P^t[key][q], 32 keys per step: two stacked probability tiles are the B operand as they stand
__device__ __forceinline__ void pv_step(const FwdBlock& c, int ntile, const f32x4 (&acc)[8], f32x4 (&oT)[4]) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (2 * s < ntile) {
      const float lo[4] = {acc[2 * s][0], acc[2 * s][1], acc[2 * s][2], acc[2 * s][3]};
      const float hi[4] = {acc[2 * s + 1][0], acc[2 * s + 1][1], acc[2 * s + 1][2], acc[2 * s + 1][3]};
      const bf16x8 fp = pack_acc(lo, hi);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
        oT[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_tr_acc(c.Vs, QS, s * 32, dt * 16, c.lane), fp, oT[dt], 0, 0, 0);
    }
  }
}

// The end of query q's row: the four g-lanes' partial sums make l, lse = m + log l goes out, O^t / l is packed to bf16
__device__ __forceinline__ void finish_block(const FwdBlock& c, int q, float m, float l, const f32x4 (&oT)[4],
                                             u32x2 (&opk)[4]) {
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  const float inv = l > 0.f ? 1.f / l : 0.f;
  if (c.lane < 16 && q < c.S && c.lse_row) c.lse_row[q] = m + __logf(l);
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    opk[dt][0] = pack2(oT[dt][0] * inv, oT[dt][1] * inv);
    opk[dt][1] = pack2(oT[dt][2] * inv, oT[dt][3] * inv);
  }
}

// The packed block of the queries qw .. qw+15 (block-local rows lrow ..) leaves through K's LDS rows lrow .. lrow+15, which
// only this wave touches once every wave is done with K
__device__ __forceinline__ void store_block(const FwdBlock& c, int lrow, int qw, const u32x2 (&opk)[4]) {
  unsigned char* stage = c.Ks + lrow * QS;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) *reinterpret_cast<u32x2*>(stage + c.i16 * QS + (dt * 16 + c.g * 4) * 2) = opk[dt];
  store_rows16(stage, QS, c.obase, c.H, qw, min(16, c.S - qw), c.lane);
}

// ------------------------------------------------------------------------------------ forward, any S
// One 8-wave workgroup per (head, sequence, 128-query block): wave w owns 16 queries and sweeps the key tiles with an
// online softmax - the rescale by alpha is all this kernel adds to the shared pieces.
__global__ __launch_bounds__(TNT, 4) void attn_fwd_tiled_kernel(const AttnFwd a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const FwdBlock c = fwd_block(smem, a);
  const int S = c.S, w = c.w, qb = blockIdx.z;
  if (qb * TB >= S) return;  // block-uniform: a short (or empty) sequence has no such query block
  const int qw = qb * TB + 16 * w;  // this wave's first query
  const int q = qw + c.i16;
  const bool wave_on = qw < S;      // wave-uniform
  bf16x8 fq[2];
  q_frags(c, q, fq);

  float m_run = -INFINITY, l_run = 0.f;
  f32x4 oT[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) oT[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int nkt = a.causal ? qb + 1 : (S + TB - 1) / TB;

  for (int kt = 0; kt < nkt; ++kt) {
    const int k0 = kt * TB;
    __syncthreads();  // every wave is done with the previous key tile
    stage_rows(c.Ks, c.base + c.H, c.ld, k0, S, c.t);
    stage_rows(c.Vs, c.base + 2 * c.H, c.ld, k0, S, c.t);
    fill_kms(a, c, c.kms, k0);
    __syncthreads();
    if (!wave_on) continue;

    const int nvalid = min(8, (S - k0 + 15) >> 4);
    const int ntile = (a.causal && kt == qb) ? min(w + 1, nvalid) : nvalid;  // 16-key tiles this wave needs
    f32x4 acc[8];
    const float mx = score_step(a, c, fq, k0, q, ntile, m_run, acc);
    const float alpha = mx > -INFINITY ? __expf(m_run - mx) : 1.f;  // exp(-inf) = 0 when this is the first live tile
    m_run = mx;
    const float psum = prob_step(a, c, k0, q, ntile, mx, acc);
    l_run = l_run * alpha + psum;  // per-lane partial; the four g-lanes of a query are summed once at the end
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) oT[dt][r] *= alpha;
    pv_step(c, ntile, acc, oT);
  }

  u32x2 opk[4];
  finish_block(c, q, m_run, l_run, oT, opk);
  __syncthreads();  // Ks is free: it becomes the output staging (wave w uses rows 16w..16w+15 only)
  if (wave_on) store_block(c, 16 * w, qw, opk);
}

// ------------------------------------------------------------------------------------ forward, S <= 128
// One-tile sequences (every training shape, the ViT-B towers, the decode cache up to 128 tokens): a FOUR-wave workgroup per
// (sequence, head).  K and V are staged once; each wave then walks up to two 16-query blocks (rows 16w.. and 64+16w..) one
// after the other.  Against the eight-wave kernel above this (i) puts four workgroups on a CU instead of two at the same
// 128 registers - twice as many staging loads in flight for a kernel that mostly waits for memory -, (ii) leaves no wave
// idle when the sequence is short (packed captions average 72 tokens: 5 of 8 waves had queries, and a sequence of <= 64
// tokens now occupies 4 wave slots instead of 8), (iii) needs no online-softmax rescale: one key tile, one maximum.
constexpr int FNT = 256;
__global__ __launch_bounds__(FNT, 4) void attn_fwd_one_kernel(const AttnFwd a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const FwdBlock c = fwd_block(smem, a);
  const int S = c.S, w = c.w;
  if (S <= 0) return;

  // all of this workgroup's loads are requested before anything waits: K, V (4 + 4 chunks per thread) and both Q blocks.
  // (K and V share one bounds test here instead of two stage_load calls: behind those the compiler waits for six of the
  // twelve requests instead of three, 1 % of the kernel on packed captions.)
  StageRegs<FNT> rk, rv;
#pragma unroll
  for (int i = 0; i < 1024 / FNT; ++i) {
    const int idx = c.t + FNT * i, row = idx >> 3, ch = idx & 7;
    rk.v[i] = rv.v[i] = (u32x4){0u, 0u, 0u, 0u};
    if (row < S) {
      rk.v[i] = *reinterpret_cast<const u32x4*>(c.base + c.H + (size_t)row * c.ld + ch * 8);
      rv.v[i] = *reinterpret_cast<const u32x4*>(c.base + 2 * c.H + (size_t)row * c.ld + ch * 8);
    }
  }
  bf16x8 fq[2][2];
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) q_frags(c, 64 * ps + 16 * w + c.i16, fq[ps]);
  fill_kms(a, c, c.kms, 0);
  stage_store(rk, c.Ks, c.t);
  stage_store(rv, c.Vs, c.t);
  __syncthreads();

  const int nvalid = min(8, (S + 15) >> 4);
  u32x2 opk[2][4];  // the two blocks' outputs, packed bf16, until K's space can stage them
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) opk[ps][dt] = (u32x2){0u, 0u};
    const int qw = 64 * ps + 16 * w;  // this wave's first query of the block
    if (qw < S) {                      // wave-uniform
      const int q = qw + c.i16;
      const int ntile = a.causal ? min((qw >> 4) + 1, nvalid) : nvalid;  // 16-key tiles this block needs
      f32x4 acc[8], oT[4];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) oT[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      const float mx = score_step(a, c, fq[ps], 0, q, ntile, -INFINITY, acc);
      const float l = prob_step(a, c, 0, q, ntile, mx, acc);
      pv_step(c, ntile, acc, oT);
      finish_block(c, q, mx, l, oT, opk[ps]);
    }
  }
  __syncthreads();  // every wave is done with K: its rows become the output staging (block ps of wave w: rows 64ps + 16w ..)
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    const int qw = 64 * ps + 16 * w;
    if (qw < S) store_block(c, qw, qw, opk[ps]);
  }
}

// ------------------------------------------------------------------------------------ backward: the shared pieces
// What a backward workgroup knows about its (head, sequence): the LDS carve-up K | V | Q | dO | [dS^t] | lse | delta | kms,
// the head's other global bases and, from HeadSeq, the clamped length and the thread indices.  ALIAS (one (key, query) pair
// at a time only): the dS^t image lives where V and Q were - both are dead once phase A is over - so a workgroup needs
// 75 KiB of LDS instead of 109 and two of them share a CU (registers capped at 128 for that).
struct BwdBlock : HeadSeq {
  unsigned char *Ks, *Vs, *Qs, *dOs;  // [128][64] bf16 images
  unsigned char* dSs;                 // dS^t image [128 keys][128 queries]
  unsigned char* mine;                // this wave's own 16 rows of the dS^t image (also its store staging)
  float *lses, *dels;                 // [NQB * 128] each
  unsigned char* kms;                 // [128]
  const bf16_t *obase, *dobase;
  bf16_t* dbase_g;
  const float* lse_row;
};
template <int NQB, bool ALIAS>
__device__ __forceinline__ BwdBlock bwd_block(unsigned char* smem, const AttnBwd& a) {
  static_assert(!ALIAS || (NQB == 1 && TILE_P <= 2 * TILE_QKV), "the dS^t image must fit where V and Q were");
  BwdBlock c;
  static_cast<HeadSeq&>(c) = head_seq(a);
  c.Ks = smem;
  c.Vs = smem + TILE_QKV;
  c.Qs = smem + 2 * TILE_QKV;
  c.dOs = smem + 3 * TILE_QKV;
  c.dSs = ALIAS ? c.Vs : smem + 4 * TILE_QKV;
  c.lses = reinterpret_cast<float*>(smem + 4 * TILE_QKV + (ALIAS ? 0 : TILE_P));
  c.dels = c.lses + NQB * TB;
  c.kms = reinterpret_cast<unsigned char*>(c.dels + NQB * TB);
  const int h = blockIdx.x;
  c.mine = c.dSs + (16 * c.w) * PS;
  c.obase = a.O + (size_t)c.row0 * c.H + h * DH;
  c.dobase = a.dO + (size_t)c.row0 * c.H + h * DH;
  c.dbase_g = a.dqkv + (size_t)c.row0 * c.ld + h * DH;
  c.lse_row = a.lse + (size_t)c.bh * a.Sp;
  return c;
}

// rows of one 128-query block: delta[row] = sum_d dO[row, d] O[row, d] from the requested registers (8 lanes per row; the
// (row, chunk) map is stage_load's)
__device__ __forceinline__ void delta_rows(const StageRegs<TNT>& po, const StageRegs<TNT>& pdo, float* dels, int t) {
#pragma unroll
  for (int i = 0; i < 1024 / TNT; ++i) {
    const int idx = t + TNT * i;
    const int row = idx >> 3, c = idx & 7;
    const bf16x8 a = __builtin_bit_cast(bf16x8, po.v[i]);
    const bf16x8 gg = __builtin_bit_cast(bf16x8, pdo.v[i]);
    float d = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) d += (float)a[e] * (float)gg[e];
    d += __shfl_xor(d, 1);
    d += __shfl_xor(d, 2);
    d += __shfl_xor(d, 4);
    if (c == 0) dels[row] = d;
  }
}

// A workgroup's memory latency is hidden by at most one other workgroup on its CU (none when S > 128): everything the
// first (key block, query block) pair needs - the K, V, Q, dO tiles and the row constants' inputs (O rows for delta, NROWS
// of lse from q0 on) - is REQUESTED together into registers and stored to LDS afterwards: one HBM round trip in front of
// the first MFMA instead of three.  With packed sequences (mean length 72 of 128) most workgroups have exactly one pair.
template <int NROWS>
struct PairRegs {
  StageRegs<TNT> k, v, q, dO, o;
  float lse[(NROWS + TNT - 1) / TNT];
};
template <int NROWS>
__device__ __forceinline__ void load_q_block(const BwdBlock& c, int q0, int t, PairRegs<NROWS>& r) {
  stage_load(r.q, c.base, c.ld, q0, c.S, t);
  stage_load(r.dO, c.dobase, c.H, q0, c.S, t);
  stage_load(r.o, c.obase, c.H, q0, c.S, t);
#pragma unroll
  for (int j = 0; j * TNT < NROWS; ++j) {
    const int i = t + TNT * j;
    r.lse[j] = (i < NROWS && q0 + i < c.S) ? c.lse_row[q0 + i] : 0.f;
  }
}
template <int NROWS>
__device__ __forceinline__ void load_first_pair(const BwdBlock& c, int k0, int q0, PairRegs<NROWS>& r) {
  stage_load(r.k, c.base + c.H, c.ld, k0, c.S, c.t);
  stage_load(r.v, c.base + 2 * c.H, c.ld, k0, c.S, c.t);
  load_q_block(c, q0, c.t, r);
}
// the row constants of the requested query rows: delta of the first 128, lse of all NROWS
template <int NROWS>
__device__ __forceinline__ void store_row_consts(const BwdBlock& c, int t, const PairRegs<NROWS>& r) {
  delta_rows(r.o, r.dO, c.dels, t);
#pragma unroll
  for (int j = 0; j * TNT < NROWS; ++j)
    if (t + TNT * j < NROWS) c.lses[t + TNT * j] = r.lse[j];
}
template <int NROWS>
__device__ __forceinline__ void store_first_pair(const BwdBlock& c, const PairRegs<NROWS>& r) {
  stage_store(r.k, c.Ks, c.t);
  stage_store(r.v, c.Vs, c.t);
  stage_store(r.q, c.Qs, c.t);
  stage_store(r.dO, c.dOs, c.t);
  store_row_consts(c, c.t, r);
}

// this wave's 16 keys of the staged K and V as B operands (n = key)
__device__ __forceinline__ void key_frags(const BwdBlock& c, int lane, bf16x8 (&fk)[2], bf16x8 (&fv)[2]) {
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    fk[kk] = frag_rows64(c.Ks, 16 * c.w, kk, lane);
    fv[kk] = frag_rows64(c.Vs, 16 * c.w, kk, lane);
  }
}

// One 32-query step of phase A for this wave's 16 keys: S and dP with the key on the lane -> the dropped probabilities
// and dS of two stacked 16x16 tiles.  lses / dels point at the rows of the CURRENT query block (q0 ..).
__device__ __forceinline__ void pair_step(const AttnBwd& a, const BwdBlock& c, const float* lses, const float* dels,
                                          const bf16x8 (&fk)[2], const bf16x8 (&fv)[2], int s, int q0, int key,
                                          bool kvalid, int lane, float (&pd)[2][4], float (&ds)[2][4]) {
  const float scale = 0.125f;
  const int g = lane >> 4;
  f32x4 sa[2], da[2];
#pragma unroll
  for (int tt = 0; tt < 2; ++tt) {
    sa[tt] = da[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      sa[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_rows64(c.Qs, (2 * s + tt) * 16, kk, lane), fk[kk], sa[tt], 0,
                                                       0, 0);
      da[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_rows64(c.dOs, (2 * s + tt) * 16, kk, lane), fv[kk], da[tt], 0,
                                                       0, 0);
    }
  }
#pragma unroll
  for (int tt = 0; tt < 2; ++tt) {
    const int ql = (2 * s + tt) * 16 + g * 4;
    const f32x4 l4 = *reinterpret_cast<const f32x4*>(lses + ql);
    const f32x4 d4 = *reinterpret_cast<const f32x4*>(dels + ql);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = q0 + ql + r;
      const bool ok = kvalid && q < c.S && (!a.causal || key <= q);
      const float pu = ok ? __expf(sa[tt][r] * scale - l4[r]) : 0.f;  // undropped probability
      // (the key runs along the lanes here, so each element has its own pair hash)
      const float m = a.drop.on() ? a.drop.mul((c.bh * a.Sp + q) * a.Sp + key) : 1.f;
      ds[tt][r] = pu * (da[tt][r] * m - d4[r]) * scale;               // dP = dP_dropped * m
      pd[tt][r] = pu * m;                                              // dV uses the dropped probabilities
    }
  }
}

// the step's P and dS accumulators are the B operands of dV^t += dO^t P and dK^t += Q^t dS
__device__ __forceinline__ void dkv_step(const BwdBlock& c, int s, const float (&pd)[2][4], const float (&ds)[2][4],
                                         f32x4 (&dvT)[4], f32x4 (&dkT)[4]) {
  const bf16x8 fp = pack_acc(pd[0], pd[1]);
  const bf16x8 fds = pack_acc(ds[0], ds[1]);
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    dvT[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_tr_acc(c.dOs, QS, s * 32, dt * 16, c.lane), fp, dvT[dt], 0, 0, 0);
    dkT[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_tr_acc(c.Qs, QS, s * 32, dt * 16, c.lane), fds, dkT[dt], 0, 0, 0);
  }
}

__device__ __forceinline__ u32x2 pack_ds(const float (&ds)[4]) {
  u32x2 pk;
  pk[0] = pack2(ds[0], ds[1]);
  pk[1] = pack2(ds[2], ds[3]);
  return pk;
}
// a wave with no real key in its rows: the dQ product must read zeros there
__device__ __forceinline__ void zero_dsp(u32x2 (&dsp)[8]) {
#pragma unroll
  for (int mi = 0; mi < 8; ++mi) dsp[mi] = (u32x2){0u, 0u};
}
// the held dS of this wave's 16 keys -> its rows of the dS^t image
__device__ __forceinline__ void write_ds_image(unsigned char* mine, const u32x2 (&dsp)[8], int i16, int g) {
#pragma unroll
  for (int mi = 0; mi < 8; ++mi) *reinterpret_cast<u32x2*>(mine + i16 * PS + (mi * 16 + g * 4) * 2) = dsp[mi];
}

// phase B of one (key block, query block) pair: dqt[q][d] = dS[q][key] K[key][d] for this wave's 16 queries of the block,
// a fresh partial per key block
__device__ __forceinline__ void phase_b(const BwdBlock& c, int k0, bool diagonal, f32x4 (&dqt)[4]) {
  int nks = (min(TB, c.S - k0) + 31) >> 5;
  if (diagonal) nks = min(nks, (c.w >> 1) + 1);
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) dqt[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int ks = 0; ks < nks; ++ks) {
    const bf16x8 fa = frag_tr(c.dSs, PS, ks * 32, 16 * c.w, c.lane);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
      dqt[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, frag_tr(c.Ks, QS, ks * 32, nt * 16, c.lane), dqt[nt], 0, 0, 0);
  }
}

// dK, dV of a key block: dkT[dt][r] = dK[key = keyw + i16][d = dt*16 + 4g + r], through the wave's own rows
__device__ __forceinline__ void store_dkv(const BwdBlock& c, const f32x4 (&dkT)[4], const f32x4 (&dvT)[4], int keyw) {
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    u32x2 pk, pv;
    pk[0] = pack2(dkT[dt][0], dkT[dt][1]);
    pk[1] = pack2(dkT[dt][2], dkT[dt][3]);
    pv[0] = pack2(dvT[dt][0], dvT[dt][1]);
    pv[1] = pack2(dvT[dt][2], dvT[dt][3]);
    *reinterpret_cast<u32x2*>(c.mine + c.i16 * PS + (dt * 16 + c.g * 4) * 2) = pk;
    *reinterpret_cast<u32x2*>(c.mine + c.i16 * PS + 128 + (dt * 16 + c.g * 4) * 2) = pv;
  }
  if (keyw < c.S) {  // wave-uniform
    const int nv = min(16, c.S - keyw);
    store_rows16(c.mine, PS, c.dbase_g + c.H, c.ld, keyw, nv, c.lane);
    store_rows16(c.mine + 128, PS, c.dbase_g + 2 * c.H, c.ld, keyw, nv, c.lane);
  }
}

// dQ of a query block: dq[nt][r] = dQ[q = qw + 4g + r][d = nt*16 + i16]
__device__ __forceinline__ void store_dq(const BwdBlock& c, const f32x4 (&dq)[4], int qw) {
  if (qw < c.S) {  // wave-uniform
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        *reinterpret_cast<bf16_t*>(c.mine + (c.g * 4 + r) * PS + (nt * 16 + c.i16) * 2) = f2bf(dq[nt][r]);
    store_rows16(c.mine, PS, c.dbase_g, c.ld, qw, min(16, c.S - qw), c.lane);
  }
}

// ------------------------------------------------------------------------------------ backward, one pass (S <= 512)
template <int NQB, bool ALIAS>
__global__ __launch_bounds__(TNT, ALIAS ? 4 : 2) void attn_bwd_tiled_kernel(const AttnBwd a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const BwdBlock c = bwd_block<NQB, ALIAS>(smem, a);
  const int S = c.S, t = c.t, w = c.w;
  if (S <= 0) return;

  // row constants of every query: lse and delta.  Rows of the first query block come with the first pair (0 in both
  // mask modes), later blocks' delta from memory.
  PairRegs<NQB * TB> first;
  load_first_pair(c, 0, 0, first);
  store_row_consts(c, t, first);
  for (int idx = t + 1024; idx < NQB * TB * 8; idx += TNT) {
    const int row = idx >> 3, ch = idx & 7;
    float d = 0.f;
    if (row < S) {
      const bf16x8 o8 = *reinterpret_cast<const bf16x8*>(c.obase + (size_t)row * c.H + ch * 8);
      const bf16x8 gg = *reinterpret_cast<const bf16x8*>(c.dobase + (size_t)row * c.H + ch * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) d += (float)o8[e] * (float)gg[e];
    }
    d += __shfl_xor(d, 1);
    d += __shfl_xor(d, 2);
    d += __shfl_xor(d, 4);
    if (ch == 0) c.dels[row] = d;
  }

  f32x4 dq[NQB][4];
#pragma unroll
  for (int qb = 0; qb < NQB; ++qb)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) dq[qb][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nblk = NQB == 1 ? 1 : (S + TB - 1) / TB;  // key blocks == query blocks (<= NQB; S > 0 here)

  for (int kb = 0; kb < nblk; ++kb) {
    const int k0 = kb * TB;
    // (the barrier that closes the previous pair protects Ks / Vs / kms)
    if (kb == 0) {   // requested at the top.  (The tile stores stay in here: in straight line behind the requests the
                     // compiler waits three times among the ten loads instead of once after them.)
      stage_store(first.k, c.Ks, t);
      stage_store(first.v, c.Vs, t);
      stage_store(first.q, c.Qs, t);
      stage_store(first.dO, c.dOs, t);
    } else {
      stage_rows(c.Ks, c.base + c.H, c.ld, k0, S, t);
      stage_rows(c.Vs, c.base + 2 * c.H, c.ld, k0, S, t);
    }
    fill_kms(a, c, c.kms, k0);
    __syncthreads();
    const int keyw = k0 + 16 * w;            // this wave's first key
    const bool has_keys = keyw < S;          // wave-uniform
    const int key = keyw + c.i16;
    bf16x8 fk[2], fv[2];                     // loop-invariant over the query blocks
    key_frags(c, c.lane, fk, fv);
    const bool kvalid = key < S && c.kms[16 * w + c.i16];
    f32x4 dvT[4], dkT[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dvT[dt] = dkT[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // runtime loop (one copy of the body); only the dQ accumulators are indexed statically, at the end of the pair
#pragma unroll 1
    for (int qb = a.causal ? kb : 0; qb < nblk; ++qb) {
      const int q0 = qb * TB;
      if (kb != 0 || qb != 0) {   // (pair (0, 0) was staged with the key block)
        stage_rows(c.Qs, c.base, c.ld, q0, S, t);
        stage_rows(c.dOs, c.dobase, c.H, q0, S, t);
        __syncthreads();
      }
      // ---- phase A: S, dP (key on the lane) -> P, dS -> dV^t, dK^t; dS^t to LDS
      const int nqt = min(8, (S - q0 + 15) >> 4);          // 16-query tiles with a real row
      // on the diagonal block queries below this wave's first key see none of its keys
      const int mi_lo = (a.causal && qb == kb) ? w : 0;
      u32x2 dsp[ALIAS ? 8 : 1];
      auto phase_a = [&](const int s) {
        float pd[2][4], ds[2][4] = {};
        if (2 * s < nqt && 2 * s + 1 >= mi_lo) {
          pair_step(a, c, c.lses + q0, c.dels + q0, fk, fv, s, q0, key, kvalid, c.lane, pd, ds);
          dkv_step(c, s, pd, ds, dvT, dkT);
        }
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
          if constexpr (ALIAS) dsp[2 * s + tt] = pack_ds(ds[tt]);   // V / Q are still being read: held until the barrier
          else *reinterpret_cast<u32x2*>(c.mine + c.i16 * PS + ((2 * s + tt) * 16 + c.g * 4) * 2) = pack_ds(ds[tt]);
        }
      };
      if constexpr (ALIAS) {
        if (has_keys) {
#pragma unroll
          for (int s = 0; s < 4; ++s) phase_a(s);
        } else {
          zero_dsp(dsp);
        }
        __syncthreads();  // every wave is done with V and Q: their space takes the dS^t image
        write_ds_image(c.mine, dsp, c.i16, c.g);
      } else if (has_keys) {
#pragma unroll 1
        for (int s = 0; s < 4; ++s) phase_a(s);
      } else {  // no real key in this wave's rows: the dQ product must read zeros there
#pragma unroll
        for (int mi = 0; mi < 8; ++mi)
          *reinterpret_cast<u32x2*>(c.mine + c.i16 * PS + (mi * 16 + c.g * 4) * 2) = (u32x2){0u, 0u};
      }
      __syncthreads();
      if (q0 + 16 * w < S) {
        f32x4 dqt[4];
        phase_b(c, k0, a.causal && qb == kb, dqt);
#pragma unroll
        for (int j = 0; j < NQB; ++j)
          if (j == qb) {  // wave-uniform select keeps dq[][] in registers (no runtime-indexed vector array)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) dq[j][nt] += dqt[nt];
          }
      }
      __syncthreads();  // Qs / dOs / dSs are re-filled by the next pair
    }
    store_dkv(c, dkT, dvT, keyw);
  }

#pragma unroll
  for (int qb = 0; qb < NQB; ++qb) store_dq(c, dq[qb], qb * TB + 16 * w);
}

// ------------------------------------------------------------------------------------ backward, split by role (S <= 1024)
// 7 matmuls per (key, query) pair instead of 5, for nkb + nqb workgroups per (head, sequence) instead of one.  Both roles
// use the ALIAS layout and stay within 128 registers: two workgroups per CU, and one grid can carry both roles.  lse /
// delta live in LDS for ONE 128-query block at a time, so LDS use does not grow with S.

// dK/dV role: phase A only; dK^t / dV^t accumulate in ascending query-block order.  No dS image, no dQ.
__device__ __forceinline__ void dkv_role(unsigned char* smem, const AttnBwd& a, int kb) {
  const BwdBlock c = bwd_block<1, true>(smem, a);
  const int S = c.S, t = c.t, w = c.w;
  const int k0 = kb * TB;
  if (k0 >= S) return;  // block-uniform: a short (or empty) sequence has no such key block
  const int nblk = (S + TB - 1) / TB;
  const int qb0 = a.causal ? kb : 0;
  PairRegs<TB> r;
  load_first_pair(c, k0, qb0 * TB, r);
  store_first_pair(c, r);
  fill_kms(a, c, c.kms, k0);
  const int keyw = k0 + 16 * w;            // this wave's first key
  const bool has_keys = keyw < S;          // wave-uniform
  const int key = keyw + c.i16;
  f32x4 dvT[4], dkT[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dvT[dt] = dkT[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
  for (int qb = qb0; qb < nblk; ++qb) {
    // opaque to the optimizer: otherwise every per-lane value that is linear in q0 (the dropout row bases, the staging
    // addresses) becomes an induction variable of its own, and the 128-register budget has no room for them
    int q0 = qb * TB;
    asm volatile("" : "+s"(q0));
    // (the barrier that closes the previous block protects Qs / dOs / lses / dels)
    if (qb != qb0) {  // (the first block came with K and V)
      int tl = t;
      asm volatile("" : "+v"(tl));
      load_q_block(c, q0, tl, r);
      stage_store(r.q, c.Qs, tl);
      stage_store(r.dO, c.dOs, tl);
      store_row_consts(c, tl, r);
    }
    __syncthreads();
    const bool kvalid = key < S && c.kms[16 * w + c.i16];
    if (has_keys) {
      bf16x8 fk[2], fv[2];
      key_frags(c, c.lane, fk, fv);
      const int nqt = min(8, (S - q0 + 15) >> 4);          // 16-query tiles with a real row
      // on the diagonal block queries below this wave's first key see none of its keys
      const int mi_lo = (a.causal && qb == kb) ? w : 0;
#pragma unroll 1
      for (int s = 0; s < 4; ++s) {
        if (2 * s < nqt && 2 * s + 1 >= mi_lo) {
          float pd[2][4], ds[2][4];
          pair_step(a, c, c.lses, c.dels, fk, fv, s, q0, key, kvalid, c.lane, pd, ds);
          dkv_step(c, s, pd, ds, dvT, dkT);
        }
      }
    }
    __syncthreads();  // Qs / dOs / lses / dels are re-filled by the next block
  }
  store_dkv(c, dkT, dvT, keyw);  // (every image is free by now)
}

// dQ role: dO, lse and delta are staged once; S, dP and dS are recomputed per key block, dS crosses LDS and phase B adds a
// fresh dqt per key block in ascending key-block order.
__device__ __forceinline__ void dq_role(unsigned char* smem, const AttnBwd& a, int qb) {
  const BwdBlock c = bwd_block<1, true>(smem, a);
  const int S = c.S, t = c.t, w = c.w;
  const int q0_ = qb * TB;
  if (q0_ >= S) return;  // block-uniform: a short (or empty) sequence has no such query block
  PairRegs<TB> r;
  load_first_pair(c, 0, q0_, r);
  store_first_pair(c, r);  // (dO, lse and delta stay for every key block)

  f32x4 dq[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) dq[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int nkb = a.causal ? qb + 1 : (S + TB - 1) / TB;
  const int nqt = min(8, (S - q0_ + 15) >> 4);  // 16-query tiles with a real row

#pragma unroll 1
  for (int kb = 0; kb < nkb; ++kb) {
    const int k0 = kb * TB;
    // what depends on the query alone (its 32 dropout row bases per lane) is recomputed per key block instead of being
    // hoisted into registers that the 128-register budget does not have
    int q0 = q0_;
    asm volatile("" : "+s"(q0));
    // (the barrier that closes the previous key block protects Ks / Vs / Qs / kms)
    if (kb != 0) {  // V and Q were overwritten by the dS^t image
      int tl = t;   // (the per-thread row addresses are rebuilt here too)
      asm volatile("" : "+v"(tl));
      stage_rows(c.Ks, c.base + c.H, c.ld, k0, S, tl);
      stage_rows(c.Vs, c.base + 2 * c.H, c.ld, k0, S, tl);
      stage_rows(c.Qs, c.base, c.ld, q0, S, tl);
    }
    fill_kms(a, c, c.kms, k0);
    __syncthreads();
    const int keyw = k0 + 16 * w;            // this wave's first key
    int ll = c.lane;   // (so are the per-lane tile offsets)
    asm volatile("" : "+v"(ll));
    const int gl = ll >> 4, il = ll & 15;
    const int key = keyw + il;
    const bool kvalid = key < S && c.kms[16 * w + il];
    const int mi_lo = (a.causal && qb == kb) ? w : 0;
    u32x2 dsp[8];  // V / Q are still being read by other waves: held until the barrier
    if (keyw < S) {  // wave-uniform
      bf16x8 fk[2], fv[2];
      key_frags(c, ll, fk, fv);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        float pd[2][4], ds[2][4] = {};
        if (2 * s < nqt && 2 * s + 1 >= mi_lo) pair_step(a, c, c.lses, c.dels, fk, fv, s, q0, key, kvalid, ll, pd, ds);
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) dsp[2 * s + tt] = pack_ds(ds[tt]);
      }
    } else {
      zero_dsp(dsp);
    }
    __syncthreads();  // every wave is done with V and Q: their space takes the dS^t image
    write_ds_image(c.mine, dsp, il, gl);
    __syncthreads();
    if (q0 + 16 * w < S) {
      f32x4 dqt[4];
      phase_b(c, k0, a.causal && qb == kb, dqt);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) dq[nt] += dqt[nt];
    }
    __syncthreads();  // Ks / Vs / Qs are re-filled by the next key block
  }
  store_dq(c, dq, q0_ + 16 * w);
}

// Both roles in one grid of 2 * nblk workgroups per (head, sequence); the heaviest first when causal: key block 0 sweeps
// every query block, the last query block every key block.  (A launch per role was measured and lost at every shape.)
__global__ __launch_bounds__(TNT, 4) void attn_bwd_split_kernel(const AttnBwd a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int nblk = gridDim.z >> 1;
  if ((int)blockIdx.z < nblk) dkv_role(smem, a, blockIdx.z);
  else dq_role(smem, a, gridDim.z - 1 - blockIdx.z);
}

constexpr size_t TFWD_LDS = 2 * TILE_QKV + TB;
constexpr size_t bwd_lds(int nqb, bool alias) {
  return 4 * TILE_QKV + (alias ? 0 : TILE_P) + 2 * (size_t)nqb * TB * sizeof(float) + TB;
}

// One-block sequences (S <= 128: every training shape) take the aliased layout, two workgroups per CU.
template <int NQB>
int launch_bwd(const AttnBwd& a) {
  constexpr bool ALIAS = NQB == 1;
  constexpr size_t lds = bwd_lds(NQB, ALIAS);
  static const hipError_t attr = hipFuncSetAttribute((const void*)attn_bwd_tiled_kernel<NQB, ALIAS>,
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (attr != hipSuccess) {
    set_error("attention (tiled backward): cannot raise dynamic LDS limit");
    return PGCA_ERR_LAUNCH;
  }
  hipLaunchKernelGGL((attn_bwd_tiled_kernel<NQB, ALIAS>), dim3(a.heads, a.B), dim3(TNT), lds, a.stream, a);
  return check_launch("pgca_attention_bwd(tiled)");
}

}  // namespace

namespace pgca {

int attention_bwd_split(const AttnBwd& a) {
  constexpr size_t lds = bwd_lds(1, true);
  static const hipError_t attr = hipFuncSetAttribute((const void*)attn_bwd_split_kernel,
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (attr != hipSuccess) {
    set_error("attention (split backward): cannot raise dynamic LDS limit");
    return PGCA_ERR_LAUNCH;
  }
  const int nblk = (a.S + TB - 1) / TB;
  hipLaunchKernelGGL(attn_bwd_split_kernel, dim3(a.heads, a.B, 2 * nblk), dim3(TNT), lds, a.stream, a);
  return check_launch("pgca_attention_bwd_split");
}

int attention_fwd_tiled(const AttnFwd& a) {
  static const hipError_t attr = hipFuncSetAttribute((const void*)attn_fwd_tiled_kernel,
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)TFWD_LDS);
  if (attr != hipSuccess) {
    set_error("attention (tiled forward): cannot raise dynamic LDS limit");
    return PGCA_ERR_LAUNCH;
  }
  if (a.S <= TB) {  // one key tile: the four-wave kernel
    hipLaunchKernelGGL(attn_fwd_one_kernel, dim3(a.heads, a.B), dim3(FNT), TFWD_LDS, a.stream, a);
    return check_launch("pgca_attention_fwd(one tile)");
  }
  const int nqb = (a.S + TB - 1) / TB;
  hipLaunchKernelGGL(attn_fwd_tiled_kernel, dim3(a.heads, a.B, nqb), dim3(TNT), TFWD_LDS, a.stream, a);
  return check_launch("pgca_attention_fwd(tiled)");
}

int attention_bwd_tiled(const AttnBwd& a) {
  switch ((a.S + TB - 1) / TB) {
    case 1: return launch_bwd<1>(a);
    case 2: return launch_bwd<2>(a);
    case 3: return launch_bwd<3>(a);
    case 4: return launch_bwd<4>(a);
    default:
      set_error("pgca_attention_bwd: S=%d exceeds the %d-token limit of the register-resident dQ accumulators", a.S,
                PGCA_ATTN_MAX_S);
      return PGCA_ERR_INVALID;
  }
}

}  // namespace pgca
