// bf16 MFMA GEMM for gfx950 (MI355X): C[M,N] = epilogue(alpha * A·B + bias).  This file holds the planner, the C entry
// points and two of the kernel families; the third (phase-staggered 256^2) is gemm_phase.hip / gemm_pair.hip.
//
// Every kernel serves the three operand layouts of the hot path (pgca_hip.h):
//   NT  A[M,K] · B[N,K]^t   both operands contiguous along K   -> ds_read_b128 fragments
//   NN  A[M,K] · B[K,N]     B strided along K                  -> ds_read_b64_tr_b16 fragments
//   TN  A[K,M]^t · B[K,N]   both strided along K (wgrad X^t dY) -> ds_read_b64_tr_b16 fragments
// so forward, dgrad and wgrad all read the reference's native weight layouts
// (Conv1D [in,out], nn.Linear [out,in]) from ONE bf16 mirror - no transposed copies.
//
//   gemm_kernel              128x128 tile, BK = 64, 4 waves (2x2): any shape; the small and the K-unaligned problems.
//                            Global -> VGPR (buffer loads, OOB lanes read 0) -> LDS (XOR-swizzled, conflict-free for
//                            both fragment read kinds), double-buffered: the next tile's global loads are issued before
//                            the current tile's MFMAs and written to the other LDS buffer after them (one barrier per
//                            K tile).
//   gemm256_kernel           256x256 tile, BK = 64, 8 waves (2x4), operands by LDS-DMA, 2 stages; split-K for the
//                            weight gradients (schedule 0: the TN layout).
//   gemm256_group_tn_kernel  up to four TN problems as one grid of that tile.
//   gemm256s_kernel / gemm256s_pair_kernel (gemm_phase.hip, gemm_pair.hip)  the same tile with a phase-staggered
//                            4-stage BK = 32 loop (schedule 6: NT and NN).
// plan_gemm chooses among them; every kernel ends in run_epilogue (gemm_epilogue.h) per 64 x 64 accumulator block and
// orders its tiles with xcd_remap + group_m_tile (gemm_device.h).
#include <string>

#include "gemm_device.h"

namespace {

template <int LA, int LB>
__global__ __launch_bounds__(256, 2) void gemm_kernel(const pgca_gemm_args a, int ntm, int ntn) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2][2][TILE_BYTES];

  int tm, tn;
  group_m_tile(xcd_remap(blockIdx.x, ntm * ntn), ntm, ntn, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;

  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  const bf16_t* A = reinterpret_cast<const bf16_t*>(a.A);
  const bf16_t* B = reinterpret_cast<const bf16_t*>(a.B);

  Stage<LA> sa;
  Stage<LB> sb;
  sa.init(t, a.lda, m0, LA == 0 ? a.M : ((a.M + 7) & ~7));
  sb.init(t, a.ldb, n0, LB == 0 ? a.N : ((a.N + 7) & ~7));
  const bf16_t* abase = LA == 0 ? A + (size_t)m0 * a.lda : A + m0;
  const bf16_t* bbase = LB == 0 ? B + (size_t)n0 * a.ldb : B + n0;
  const size_t astep = LA == 0 ? (size_t)BK : (size_t)BK * a.lda;
  const size_t bstep = LB == 0 ? (size_t)BK : (size_t)BK * a.ldb;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nk = (a.K + BK - 1) / BK;
  u32x4 ra[4], rb[4];
  sa.load(abase, a.K, ra);
  sb.load(bbase, a.K, rb);
  sa.store(smem[0][0], ra);
  sb.store(smem[0][1], rb);
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const bool more = (kt + 1) < nk;
    if (more) {
      sa.load(abase + (size_t)(kt + 1) * astep, a.K - (kt + 1) * BK, ra);
      sb.load(bbase + (size_t)(kt + 1) * bstep, a.K - (kt + 1) * BK, rb);
    }
    const unsigned char* la = smem[cur][0];
    const unsigned char* lb = smem[cur][1];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 fa[4], fb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[i] = read_frag<LA>(la, wm * 64, i, kk, lane);
#pragma unroll
      for (int j = 0; j < 4; ++j) fb[j] = read_frag<LB>(lb, wn * 64, j, kk, lane);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    if (more) {
      sa.store(smem[cur ^ 1][0], ra);
      sb.store(smem[cur ^ 1][1], rb);
    }
    __syncthreads();
  }

  // ------------------------------------------------------------------------------- epilogue
  run_epilogue(a, acc, &smem[0][0][0], m0 + wm * 64, n0 + wn * 64, lane, wave);
}

__global__ void rowstats_combine_kernel(const float* __restrict__ smax, const float* __restrict__ ssum, int stat_ld,
                                        int nparts, const float* __restrict__ tval, int M, float* __restrict__ lse,
                                        float* __restrict__ out_lp) {
  // one wave per row
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= M) return;
  float mx = -INFINITY;
  for (int i = lane; i < nparts; i += 64) mx = fmaxf(mx, smax[(size_t)row * stat_ld + i]);
  mx = wave_max(mx);
  float s = 0.f;
  for (int i = lane; i < nparts; i += 64) {
    const float pm = smax[(size_t)row * stat_ld + i];
    if (pm > -INFINITY) s += ssum[(size_t)row * stat_ld + i] * __expf(pm - mx);
  }
  s = wave_sum(s);
  if (lane == 0) {
    const float l = mx + __logf(s);
    if (lse) lse[row] = l;
    if (out_lp) out_lp[row] = tval[row] - l;
  }
}


// ================================================================================================
// 256 x 256 x 64 tile, 8 waves (2 x 4, each 128 x 64), operands brought in by LDS-DMA
// (buffer_load ... lds, 16 B per lane, 1 KiB per wave-instruction) into a double-buffered 128 KiB
// LDS image: no VGPR staging and no ds_write traffic - on gfx950 the VGPR->LDS write path
// (~79 B/clk/CU for ds_write_b128) plus the fragment reads saturate the LDS port at the 128^2 tile.
// The LDS image of each DMA instruction is lane-linear, so the XOR swizzles are applied to the
// SOURCE address (same involution as the fragment readers).  Edges: M/N by clamping the source
// row/column (clamped rows only feed outputs the epilogue masks), K must be a multiple of 64.
// ================================================================================================
// RAW: bid_in is already the tile (tm * ntn + tn) - the grouped launch places its tiles itself.
template <int LA, int LB, bool RAW = false>
__device__ __forceinline__ void gemm256_body(const pgca_gemm_args& a, int ntm, int ntn, int nk_per_split, int bid_in,
                                             int ksplit, unsigned char* smem2) {  // smem2: [2 stages][A | B][32 KiB]
  int tm, tn;
  if (RAW) {
    tm = bid_in / ntn;
    tn = bid_in - tm * ntn;
  } else {
    group_m_tile(xcd_remap(bid_in, ntm * ntn), ntm, ntn, tm, tn);
  }
  const int m0 = tm * BM2, n0 = tn * BN2;

  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wave >> 2, wn = wave & 3;

  const bf16_t* A = reinterpret_cast<const bf16_t*>(a.A);
  const bf16_t* B = reinterpret_cast<const bf16_t*>(a.B);

  Dma<LA, BK> da;
  Dma<LB, BK> db;
  da.init(lane, wave, a.lda, m0, LA == 0 ? a.M : ((a.M + 7) & ~7));
  db.init(lane, wave, a.ldb, n0, LB == 0 ? a.N : ((a.N + 7) & ~7));
  const bf16_t* abase = LA == 0 ? A + (size_t)m0 * a.lda : A + m0;
  const bf16_t* bbase = LB == 0 ? B + (size_t)n0 * a.ldb : B + n0;
  const size_t astep = LA == 0 ? (size_t)BK : (size_t)BK * a.lda;
  const size_t bstep = LB == 0 ? (size_t)BK : (size_t)BK * a.ldb;

  f32x4 acc[2][4][4];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[h][i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // split-K: blockIdx.y owns K tiles [kt0, kt0 + nk) and adds its partial with f32 atomics (accumulate == 2)
  const int kt0 = ksplit * nk_per_split;
  const int nk = min(nk_per_split, a.K / BK - kt0);
  abase += (size_t)kt0 * astep;
  bbase += (size_t)kt0 * bstep;
#ifdef PGCA_GEMM_TIMING
  unsigned long long ts0, ts1, ts2, ts3;
#endif
  TSTAMP(ts0);
  da.issue(abase, smem2, wave);
  db.issue(bbase, smem2 + TILE2_BYTES, wave);
  dma_wait();
  __syncthreads();
  TSTAMP(ts1);

  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) {
      unsigned char* nxt = smem2 + (cur ^ 1) * 2 * TILE2_BYTES;
      da.issue(abase + (size_t)(kt + 1) * astep, nxt, wave);
      db.issue(bbase + (size_t)(kt + 1) * bstep, nxt + TILE2_BYTES, wave);
    }
    const unsigned char* la = smem2 + cur * 2 * TILE2_BYTES;
    const unsigned char* lb = la + TILE2_BYTES;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 fb[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) fb[j] = read_frag<LB, 512>(lb, wn * 64, j, kk, lane);
      mma_half<LA>(la, wm * 128, kk, lane, fb, acc[0]);
      mma_half<LA>(la, wm * 128 + 64, kk, lane, fb, acc[1]);
    }
    dma_wait();       // tile kt+1 has landed (this wave's pieces) ...
    __syncthreads();  // ... and every wave is done reading tile kt
  }

  TSTAMP(ts2);
  run_epilogue(a, acc[0], smem2, m0 + wm * 128, n0 + wn * 64, lane, wave);
  run_epilogue(a, acc[1], smem2, m0 + wm * 128 + 64, n0 + wn * 64, lane, wave);
#ifdef PGCA_GEMM_TIMING
  dma_wait();  // the stores have left
  TSTAMP(ts3);
  if (a.stat_max && a.epilogue != PGCA_EPI_ROWSTATS && lane == 0) {
    float* o = a.stat_max + ((size_t)blockIdx.x * 8 + wave) * 8;
    o[0] = (float)(ts1 - ts0); o[1] = (float)(ts2 - ts1); o[2] = (float)(ts3 - ts2); o[3] = (float)nk;
  }
#endif
}

template <int LA, int LB>
__global__ __launch_bounds__(512, 2) void gemm256_kernel(const pgca_gemm_args a, int ntm, int ntn, int nk_per_split) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem2[];
  gemm256_body<LA, LB>(a, ntm, ntn, nk_per_split, blockIdx.x, blockIdx.y, smem2);
}

// Grouped launch of up to four TN (weight-gradient) problems: C_p (+)= A_p^t B_p.  One decoder layer has four weight
// gradients with 16-64 output tiles each; launched one by one each needs split-K to fill 256 CUs and then pays
// 4 x M x N f32 atomics (memory-side, 1.3 TB/s chip-wide: ~48 us per launch).  Together they are 192 tiles with the
// whole K each: no split, no atomics, a plain read-modify-write epilogue.
struct pgca_group_param {
  pgca_gemm_args a[4];
  int start[5];  // first workgroup of problem p; start[count..4] = total
  int ntm[4], ntn[4];
};

__global__ __launch_bounds__(512, 2) void gemm256_group_tn_kernel(const pgca_group_param gp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem2[];
  // Tile placement.  Workgroup b runs on XCD b % 8, and every XCD has its own 4 MiB L2: the tiles are laid out problem
  // after problem with the SHORTER tile dimension running fastest, and XCD x takes a contiguous run of that order - a
  // compact rectangle of (mostly) one problem, so the 24 tiles an XCD holds for a GPT-2-M block stream ~11 operand panels
  // through its L2 instead of ~24 when every problem is spread over all eight XCDs.
  const int b = xcd_remap(blockIdx.x, gp.start[4]);
  int p = 0;
  if (b >= gp.start[1]) p = 1;
  if (b >= gp.start[2]) p = 2;
  if (b >= gp.start[3]) p = 3;
  // field-by-field selection with constant indices keeps everything in SGPRs (a dynamically indexed by-value
  // aggregate would be spilled to scratch and come back in VGPRs, which the LDS-DMA asm cannot take)
#define PGCA_SEL(F) (p == 0 ? gp.a[0].F : p == 1 ? gp.a[1].F : p == 2 ? gp.a[2].F : gp.a[3].F)
  pgca_gemm_args a = {};
  a.A = PGCA_SEL(A);
  a.B = PGCA_SEL(B);
  a.M = PGCA_SEL(M);
  a.N = PGCA_SEL(N);
  a.K = PGCA_SEL(K);
  a.lda = PGCA_SEL(lda);
  a.ldb = PGCA_SEL(ldb);
  a.out_f32 = PGCA_SEL(out_f32);
  a.ld_out_f32 = PGCA_SEL(ld_out_f32);
  a.alpha = PGCA_SEL(alpha);
  a.accumulate = PGCA_SEL(accumulate);
  a.layout = PGCA_TN;
  a.epilogue = PGCA_EPI_NONE;
#undef PGCA_SEL
  const int ntm = p == 0 ? gp.ntm[0] : p == 1 ? gp.ntm[1] : p == 2 ? gp.ntm[2] : gp.ntm[3];
  const int ntn = p == 0 ? gp.ntn[0] : p == 1 ? gp.ntn[1] : p == 2 ? gp.ntn[2] : gp.ntn[3];
  const int st = p == 0 ? gp.start[0] : p == 1 ? gp.start[1] : p == 2 ? gp.start[2] : gp.start[3];
  const int l = b - st;
  int tm, tn;
  if (ntm <= ntn) {
    tn = l / ntm;
    tm = l - tn * ntm;
  } else {
    tm = l / ntn;
    tn = l - tm * ntn;
  }
  gemm256_body<1, 1, true>(a, ntm, ntn, a.K / BK, tm * ntn + tn, 0, smem2);
}

constexpr size_t GEMM256_LDS = 4 * TILE2_BYTES;  // 128 KiB

// Schedule of the 256^2 tile: 0 = gemm256_kernel (2-stage BK=64 loop), 6 = gemm256s_kernel (gemm_phase.hip: phase-staggered
// wave groups, 4-stage BK=32 ring).  Schedules that did not pay (BK=32 ring with plain barriers, phased halves, a 4-wave
// 128x128-per-wave asm pipeline, a 256x128 two-workgroups-per-CU tile) were measured, documented in DESIGN.md section 5 and
// removed from the library.
int plan_variant(const pgca_gemm_args& a) {
  const int forced = gemm_tuning().schedule;
  if (forced >= 0) return forced == 6 ? 6 : 0;
  // K-contiguous A (forward, data gradients, LM head): the phase-staggered loop is 3-12 % faster; the K-strided
  // weight-gradient layout pays two transposed LDS reads per fragment in the load phases and stays on the 2-stage loop.
  return a.layout == PGCA_TN ? 0 : 6;
}

}  // namespace

namespace pgca {
GemmTuning& gemm_tuning() {
  static GemmTuning t = [] {
    auto env = [](const char* name, int dflt) {
      const char* e = getenv(name);
      return e ? atoi(e) : dflt;
    };
    GemmTuning v;
    v.tile = env("PGCA_GEMM_TILE", 0);
    v.schedule = env("PGCA_GEMM_RING", -1);
    v.group = env("PGCA_GEMM_NO_GROUP", 0) ? 0 : 1;
    v.stagger = env("PGCA_GEMM_STAGGER", 0);
    v.pair_order = 0;
    return v;
  }();
  return t;
}

// Kernel choice: big, K-aligned problems take the 256^2 LDS-DMA kernels, everything else the general 128^2
// one.  Gradient-accumulating GEMMs with few output tiles but a long K (weight gradients: K = tokens) are split
// along K so the 256^2 kernel still fills the chip; partials meet through f32 atomics.
GemmPlan plan_gemm(const pgca_gemm_args& a) {
  GemmPlan p;
  p.ncols = a.epilogue == PGCA_EPI_DLOGITS ? a.out_cols : a.N;
  const int ntm2 = (a.M + BM2 - 1) / BM2, ntn2 = (p.ncols + BN2 - 1) / BN2;
  const int force = gemm_tuning().tile;
  const int nk_total = a.K / BK;
  int splits = 1;
  const bool splittable = a.epilogue == PGCA_EPI_NONE && a.accumulate && a.out_f32 && !a.out_bf16 && !a.bias &&
                          !a.residual;
  if (splittable && ntm2 * ntn2 > 0 && ntm2 * ntn2 < 192) {  // no output tiles: nothing to divide by (check_gemm_args rejects the shape)
    splits = 256 / (ntm2 * ntn2);
    if (splits > nk_total / 8) splits = nk_total / 8;
    if (splits > 16) splits = 16;
    if (splits < 1) splits = 1;
  }
  const bool want256 = force ? force == 256 : (ntm2 * ntn2 * splits >= 192);
  if ((a.K % BK) == 0 && want256 && a.M >= 8 && p.ncols >= 8) {
    p.tile = 256;
    p.variant = plan_variant(a);
    p.splits = splits;
    p.ntm = ntm2;
    p.ntn = ntn2;
    p.nk_per_split = (nk_total + splits - 1) / splits;
    p.grid_y = (nk_total + p.nk_per_split - 1) / p.nk_per_split;
  } else {
    p.tile = 128;
    p.variant = 0;
    p.splits = p.grid_y = 1;
    p.ntm = (a.M + BM - 1) / BM;
    p.ntn = (p.ncols + BN - 1) / BN;
    p.nk_per_split = (a.K + BK - 1) / BK;
  }
  return p;
}
}  // namespace pgca

extern "C" int pgca_set_option(const char* name, int32_t value) {
  if (!name) {
    set_error("pgca_set_option: null name");
    return PGCA_ERR_INVALID;
  }
  GemmTuning& t = gemm_tuning();
  const std::string n(name);
  if (n == "gemm_tile" && (value == 0 || value == 128 || value == 256)) t.tile = value;
  else if (n == "gemm_schedule" && (value == -1 || value == 0 || value == 6)) t.schedule = value;
  else if (n == "gemm_group" && (value == 0 || value == 1)) t.group = value;
  else if (n == "gemm_stagger" && value >= 0 && value <= 64) t.stagger = value;
  else if (n == "gemm_pair_order" && (value == 0 || value == 1)) t.pair_order = value;
  else {
    set_error("pgca_set_option: unknown option or value out of range (%s = %d)", name, value);
    return PGCA_ERR_INVALID;
  }
  return PGCA_OK;
}

extern "C" int pgca_gemm_plan(const pgca_gemm_args* args) {
  const GemmPlan p = plan_gemm(*args);
  if (p.tile != 256) return 12801;
  return p.variant * 1000000 + 25600 + p.splits;
}

// Argument checks of pgca_gemm_bf16, shared with the paired launch.
static int check_gemm_args(const pgca_gemm_args& a) {
  if (!a.A || !a.B || a.M <= 0 || a.N <= 0 || a.K <= 0) {
    set_error("pgca_gemm_bf16: null operand or empty shape (M=%d N=%d K=%d)", a.M, a.N, a.K);
    return PGCA_ERR_INVALID;
  }
  if ((a.lda & 7) || (a.ldb & 7) || ((uintptr_t)a.A & 15) || ((uintptr_t)a.B & 15)) {
    set_error("pgca_gemm_bf16: lda/ldb must be multiples of 8 and operands 16-B aligned (lda=%d ldb=%d)", a.lda,
              a.ldb);
    return PGCA_ERR_INVALID;
  }
  const bool a_kcontig = a.layout != PGCA_TN, b_kcontig = a.layout == PGCA_NT;
  if ((a_kcontig || b_kcontig) && (a.K & 7)) {
    set_error("pgca_gemm_bf16: K=%d must be a multiple of 8 for K-contiguous operands", a.K);
    return PGCA_ERR_INVALID;
  }
  if (a_kcontig ? a.lda < a.K : a.lda < ((a.M + 7) & ~7)) {
    set_error("pgca_gemm_bf16: lda=%d too small", a.lda);
    return PGCA_ERR_INVALID;
  }
  if (b_kcontig ? a.ldb < a.K : a.ldb < ((a.N + 7) & ~7)) {
    set_error("pgca_gemm_bf16: ldb=%d too small", a.ldb);
    return PGCA_ERR_INVALID;
  }
  if (a.epilogue == PGCA_EPI_ROWSTATS) {
    if (!a.stat_max || !a.stat_sum || a.stat_ld < 2 * ((a.N + BN - 1) / BN)) {
      set_error("pgca_gemm_bf16: ROWSTATS needs stat buffers with stat_ld >= %d", 2 * ((a.N + BN - 1) / BN));
      return PGCA_ERR_INVALID;
    }
  } else if (a.epilogue == PGCA_EPI_DLOGITS) {
    if (!a.row_lse || !a.row_scale || !a.targets || !a.out_bf16 || a.out_cols < a.N || a.ld_out_bf16 < a.out_cols) {
      set_error("pgca_gemm_bf16: DLOGITS needs row_lse,row_scale,targets,out_bf16 and out_cols >= N");
      return PGCA_ERR_INVALID;
    }
  } else {
    if (!a.out_bf16 && !a.out_f32) {
      set_error("pgca_gemm_bf16: no output buffer");
      return PGCA_ERR_INVALID;
    }
    if (((a.epilogue >= PGCA_EPI_DGELU_NEW && a.epilogue <= PGCA_EPI_DTANH) || a.epilogue == PGCA_EPI_DQUICK_GELU ||
         a.epilogue == PGCA_EPI_MUL_AUX) &&
        !a.aux_in) {
      set_error("pgca_gemm_bf16: derivative epilogue needs aux_in");
      return PGCA_ERR_INVALID;
    }
  }
  if (a.colsum_part && ((a.epilogue != PGCA_EPI_DGELU_NEW && a.epilogue != PGCA_EPI_MUL_AUX) || a.ld_colsum < a.N ||
                        a.accumulate == 2)) {
    set_error("pgca_gemm_bf16: colsum_part needs the DGELU_NEW / MUL_AUX epilogue, ld_colsum >= N and no split-K");
    return PGCA_ERR_INVALID;
  }
  return PGCA_OK;
}

extern "C" int pgca_gemm_bf16(const pgca_gemm_args* args, void* stream) {
  const pgca_gemm_args& a = *args;
  if (const int rc = check_gemm_args(a)) return rc;
  const GemmPlan p = plan_gemm(a);
  hipStream_t s = (hipStream_t)stream;
  if (p.tile == 128)
    return with_layout(a.layout, [&](auto la, auto lb) {
      hipLaunchKernelGGL((gemm_kernel<decltype(la)::value, decltype(lb)::value>), dim3(p.ntm * p.ntn), dim3(256), 0, s,
                         a, p.ntm, p.ntn);
      return check_launch("pgca_gemm_bf16");
    });
  pgca_gemm_args b = a;
  if (p.splits > 1) b.accumulate = 2;
  if (p.variant == 6) return launch_gemm256s(b, p, stream);
  return with_layout(a.layout, [&](auto la, auto lb) {
    constexpr auto kernel = gemm256_kernel<decltype(la)::value, decltype(lb)::value>;
    if (raise_lds_limit<kernel>(GEMM256_LDS, "gemm256")) return (int)PGCA_ERR_LAUNCH;
    hipLaunchKernelGGL(kernel, dim3(p.ntm * p.ntn, p.grid_y), dim3(512), GEMM256_LDS, s, b, p.ntm, p.ntn,
                       p.nk_per_split);
    return check_launch("pgca_gemm_bf16(256)");
  });
}

extern "C" int pgca_gemm_bf16_grouped(const pgca_gemm_args* args, int32_t count, void* stream) {
  if (!args || count <= 0) {
    set_error("pgca_gemm_bf16_grouped: no problems");
    return PGCA_ERR_INVALID;
  }
  // Two NT or two NN problems of one shape that would each run the phase-staggered 256^2 kernel unsplit: one grid.
  if (count == 2 && gemm_tuning().group) {
    const pgca_gemm_args &a = args[0], &b = args[1];
    const bool alike = (a.layout == PGCA_NT || a.layout == PGCA_NN) && b.layout == a.layout && a.M == b.M &&
                       a.N == b.N && a.K == b.K && a.epilogue != PGCA_EPI_DLOGITS && b.epilogue != PGCA_EPI_DLOGITS;
    const GemmPlan pa = alike ? plan_gemm(a) : GemmPlan{}, pb = alike ? plan_gemm(b) : GemmPlan{};
    if (alike && pa.tile == 256 && pb.tile == 256 && pa.splits == 1 && pb.splits == 1 && pa.variant == 6 &&
        pb.variant == 6) {
      for (int i = 0; i < 2; ++i) {
        const int rc = check_gemm_args(args[i]);
        if (rc) return rc;
      }
      return launch_gemm256s_pair(a, b, pa, stream);
    }
  }
  bool groupable = count <= 4 && gemm_tuning().group;
  for (int i = 0; i < count && groupable; ++i) {
    const pgca_gemm_args& a = args[i];
    // what the grouped kernel needs beyond valid arguments: whole 64-deep K tiles, the plain accumulate-or-store epilogue
    groupable = a.layout == PGCA_TN && (a.K % BK) == 0 && a.M >= 8 && a.N >= 8 && a.epilogue == PGCA_EPI_NONE &&
                a.out_f32 && !a.out_bf16 && !a.bias && !a.residual && !a.drop_threshold &&
                check_gemm_args(a) == PGCA_OK;
  }
  if (!groupable) {  // anything else: the ordinary path, one launch per problem
    for (int i = 0; i < count; ++i) {
      const int rc = pgca_gemm_bf16(&args[i], stream);
      if (rc) return rc;
    }
    return PGCA_OK;
  }
  if (raise_lds_limit<gemm256_group_tn_kernel>(GEMM256_LDS, "gemm256")) return PGCA_ERR_LAUNCH;
  pgca_group_param gp;
  int total = 0;
  for (int i = 0; i < 4; ++i) {
    if (i < count) {
      gp.a[i] = args[i];
      gp.ntm[i] = (args[i].M + BM2 - 1) / BM2;
      gp.ntn[i] = (args[i].N + BN2 - 1) / BN2;
      gp.start[i] = total;
      total += gp.ntm[i] * gp.ntn[i];
    } else {
      gp.a[i] = args[count - 1];
      gp.ntm[i] = gp.ntn[i] = 1;
      gp.start[i] = 0x7fffffff;
    }
  }
  gp.start[4] = total;
  hipLaunchKernelGGL(gemm256_group_tn_kernel, dim3(total), dim3(512), GEMM256_LDS, (hipStream_t)stream, gp);
  return check_launch("pgca_gemm_bf16_grouped");
}

extern "C" int pgca_rowstats_combine(const float* stat_max, const float* stat_sum, int32_t stat_ld, int32_t nparts,
                                     const float* target_val, int32_t M, float* lse, float* out_logprob,
                                     void* stream) {
  if (!stat_max || !stat_sum || M <= 0 || nparts <= 0 || (out_logprob && !target_val)) {
    set_error("pgca_rowstats_combine: bad arguments");
    return PGCA_ERR_INVALID;
  }
  hipLaunchKernelGGL(rowstats_combine_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, stat_max,
                     stat_sum, stat_ld, nparts, target_val, M, lse, out_logprob);
  return check_launch("pgca_rowstats_combine");
}
