// The fused GEMM epilogues (included from gemm_device.h): one 64 x 64 accumulator block of one wave -> global memory.
//   fetch   two strategies: the fast path requests every global operand of the block up front in 16-byte vectors, the
//           general path masks and loads 8 columns at a time;
//   maths   epilogue_math8, written once: alpha, bias, the activation / derivative / DLOGITS form, dropout;
//   store   epilogue_put8, written once: side values, residual, column sums, the outputs.
// Accumulator element acc[mi][ni][r] of the block with origin (mb, cb) is C[mb + mi*16 + (lane>>4)*4 + r]
//                                                                           [cb + ni*16 + (lane&15)].
#pragma once
#include "common.h"

namespace {

// max / sum over the 16 lanes of a DPP row (the 16 columns a 16x16 MFMA tile gives one output row), every lane gets
// the result.  quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror: four VALU ops, no LDS crossbar
// (`__shfl_xor` compiles to ds_bpermute: ~10x the latency, and the LM-head epilogue does 32 reductions per block).
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, dpp_f<0xB1>(v));
  v = fmaxf(v, dpp_f<0x4E>(v));
  v = fmaxf(v, dpp_f<0x141>(v));
  v = fmaxf(v, dpp_f<0x140>(v));
  return v;
}
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_f<0xB1>(v);
  v += dpp_f<0x4E>(v);
  v += dpp_f<0x141>(v);
  v += dpp_f<0x140>(v);
  return v;
}

__device__ __forceinline__ void epilogue_rowstats(const pgca_gemm_args& a, f32x4 (&acc)[4][4], int mb, int cb, int lane) {
  const int rbase = mb + (lane >> 4) * 4;
  const int cbase = cb + (lane & 15);
  const int part = cb >> 6;  // one partial per 64-column strip
  // The stat_ld contract is 2 * ceil(N / 128) partials per row, the 128^2 tile's count.  A 256^2 tile writes four strips,
  // so its last column tile can reach two strips further when N mod 256 is in 1..128: those would land on parts 0 and 1 of
  // the next row (and past the buffer on the last row).  Strips wholly past N but inside the range still write (-inf, 0).
  const bool part_ok = part < 2 * ((a.N + 127) >> 7);
  // the 16 target ids of this lane's rows, requested before anything depends on them (one round trip, not 16)
  long long tg[4][4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = rbase + mi * 16 + r;
      tg[mi][r] = (row < a.M && a.targets) ? a.targets[row] : -1;
    }
  float bs[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) bs[ni] = (a.bias && cbase + ni * 16 < a.N) ? a.bias[cbase + ni * 16] : 0.f;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = rbase + mi * 16 + r;
      const long long tgt = tg[mi][r];
      float x[4];
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const int col = cbase + ni * 16;
        const float t = a.alpha * acc[mi][ni][r] + bs[ni];
        if (col == tgt && a.target_val) a.target_val[row] = t;
        x[ni] = col < a.N ? t : -INFINITY;
      }
      const float mx = row16_max(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])));
      float sm = 0.f;
      if (mx > -INFINITY) sm = __expf(x[0] - mx) + __expf(x[1] - mx) + __expf(x[2] - mx) + __expf(x[3] - mx);
      sm = row16_sum(sm);
      if ((lane & 15) == 0 && row < a.M && part_ok) {
        a.stat_max[(size_t)row * a.stat_ld + part] = mx;
        a.stat_sum[(size_t)row * a.stat_ld + part] = sm;
      }
    }
  }
}

__device__ __forceinline__ bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---- 8 consecutive elements of one row, f32 or bf16 <-> 8 floats ---------------------------------------
// 16-byte vector accesses when all 8 are valid and p is 16-B aligned (VEC: the caller has established both for the whole
// block), else the first nv elements one by one (nv <= 0: none); elements not loaded read as 0.
template <bool VEC>
__device__ __forceinline__ bool vec8(const void* p, int nv) { return VEC || (nv == 8 && al16(p)); }
__device__ __forceinline__ void unpack8(const float4& c0, const float4& c1, float (&x)[8]) {
  x[0] = c0.x; x[1] = c0.y; x[2] = c0.z; x[3] = c0.w; x[4] = c1.x; x[5] = c1.y; x[6] = c1.z; x[7] = c1.w;
}
__device__ __forceinline__ void unpack8(const bf16x8& t, float (&x)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = bf2f(t[j]);
}
template <bool VEC>
__device__ __forceinline__ void ld8(const float* p, int nv, float (&x)[8]) {
  if (vec8<VEC>(p, nv)) {
    unpack8(*reinterpret_cast<const float4*>(p), *reinterpret_cast<const float4*>(p + 4), x);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = j < nv ? p[j] : 0.f;
  }
}
template <bool VEC>
__device__ __forceinline__ void ld8(const bf16_t* p, int nv, float (&x)[8]) {
  if (vec8<VEC>(p, nv)) {
    unpack8(*reinterpret_cast<const bf16x8*>(p), x);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = j < nv ? bf2f(p[j]) : 0.f;
  }
}
template <bool VEC>
__device__ __forceinline__ void st8(float* p, int nv, const float (&v)[8]) {
  if (vec8<VEC>(p, nv)) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) if (j < nv) p[j] = v[j];
  }
}
template <bool VEC>
__device__ __forceinline__ void st8(bf16_t* p, int nv, const float (&v)[8]) {
  if (vec8<VEC>(p, nv)) {
    bf16x8 t;
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = f2bf(v[j]);
    *reinterpret_cast<bf16x8*>(p) = t;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) if (j < nv) p[j] = f2bf(v[j]);
  }
}

// ---- what each form reads and writes besides the outputs --------------------------------------------------
constexpr bool epi_reads_aux(int e) {  // aux_in: the activation saved by the forward
  return e == PGCA_EPI_DGELU_NEW || e == PGCA_EPI_DRELU || e == PGCA_EPI_DTANH || e == PGCA_EPI_DQUICK_GELU ||
         e == PGCA_EPI_MUL_AUX;
}
constexpr bool epi_writes_side(int e) {  // aux_out: a side value of the maths (DLOGITS writes its own, see epilogue_put8)
  return e == PGCA_EPI_GELU_NEW || e == PGCA_EPI_QUICK_GELU || e == PGCA_EPI_TANH || e == PGCA_EPI_GELU_NEW_D;
}
constexpr bool epi_colsum(int e) { return e == PGCA_EPI_DGELU_NEW || e == PGCA_EPI_MUL_AUX; }  // colsum_part

// ---- maths ------------------------------------------------------------------------------------------------
// Everything that happens in registers to 8 consecutive output columns (col .. col + 7) of one row, in this order:
// alpha, bias, the form, dropout.  v: the accumulator values in, the results out (before residual / accumulate);
// x: the saved activation (forms that read aux_in); lse / rscale / tgt: the row's DLOGITS operands; drow: the row the
// dropout hash is keyed on; side: what the form leaves for aux_out (epi_writes_side).
template <int EPI>
__device__ __forceinline__ void epilogue_math8(const pgca_gemm_args& a, float (&v)[8], bool has_bias, const float (&b)[8],
                                               const float (&x)[8], float lse, float rscale, long long tgt,
                                               unsigned drow, int col, float (&side)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] *= a.alpha;
  if (has_bias) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] += b[j];
  }
  if (EPI == PGCA_EPI_GELU_NEW_D) {  // side: gelu_new'(pre), operand of MUL_AUX in the backward
#pragma unroll
    for (int j = 0; j < 8; ++j) gelu_new_both(v[j], v[j], side[j]);
  } else if (EPI == PGCA_EPI_GELU_NEW || EPI == PGCA_EPI_QUICK_GELU) {  // side: the pre-activation
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      side[j] = v[j];
      v[j] = EPI == PGCA_EPI_GELU_NEW ? gelu_new(v[j]) : quick_gelu(v[j]);
    }
  } else if (EPI == PGCA_EPI_RELU) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = fmaxf(v[j], 0.f);
  } else if (EPI == PGCA_EPI_TANH) {  // side: undropped tanh, operand of DTANH in the backward
#pragma unroll
    for (int j = 0; j < 8; ++j) side[j] = v[j] = fast_tanh(v[j]);
  } else if (epi_reads_aux(EPI)) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (EPI == PGCA_EPI_DGELU_NEW) v[j] *= dgelu_new(x[j]);
      else if (EPI == PGCA_EPI_MUL_AUX) v[j] *= x[j];
      else if (EPI == PGCA_EPI_DQUICK_GELU) v[j] *= dquick_gelu(x[j]);
      else if (EPI == PGCA_EPI_DRELU) v[j] = x[j] > 0.f ? v[j] : 0.f;
      else v[j] *= 1.f - x[j] * x[j];
    }
  } else if (EPI == PGCA_EPI_DLOGITS) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      v[j] = (col + j) < a.N ? rscale * (__expf(v[j] - lse) - ((col + j) == tgt ? 1.f : 0.f)) : 0.f;
  }
  if (a.drop_threshold) {
    const Drop d{a.drop_seed, a.drop_threshold, a.drop_scale};
    const unsigned base = drow * (unsigned)a.N + (unsigned)col;
    float m0[4], m1[4];
    d.mul4(base, m0);
    d.mul4(base + 4u, m1);
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] *= m0[j]; v[j + 4] *= m1[j]; }
  }
}
// row the dropout hash is keyed on (pgca_gemm_args::drop_rows - packed rows: hash of the padded position)
__device__ __forceinline__ unsigned drop_row(const pgca_gemm_args& a, int row) {
  return (a.drop_threshold && a.drop_rows) ? (unsigned)a.drop_rows[row] : (unsigned)row;
}

// ---- store ------------------------------------------------------------------------------------------------
// What follows the maths for the first nv of those 8 columns: the side values, the residual (res, fetched by the caller),
// the column sums, the outputs (old: the caller's copy of out_f32 when it accumulates) and the DLOGITS low half.
template <int EPI, bool VEC>
__device__ __forceinline__ void epilogue_put8(const pgca_gemm_args& a, int row, int col, int nv, float (&v)[8],
                                              const float (&side)[8], bool has_res, const float (&res)[8], bool has_old,
                                              const float (&old)[8], float (&cs)[8]) {
  auto aux = [&] { return reinterpret_cast<bf16_t*>(a.aux_out) + (size_t)row * a.ld_aux + col; };
  if (epi_writes_side(EPI) && a.aux_out) st8<VEC>(aux(), nv, side);
  if (has_res) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] += res[j];
  }
  if constexpr (epi_colsum(EPI)) {
#pragma unroll
    for (int j = 0; j < 8; ++j) cs[j] += j < nv ? v[j] : 0.f;
  }
  if (a.out_f32) {
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = has_old ? v[j] + old[j] : v[j];
    st8<VEC>(a.out_f32 + (size_t)row * a.ld_out_f32 + col, nv, o);
  }
  if (a.out_bf16) st8<VEC>(reinterpret_cast<bf16_t*>(a.out_bf16) + (size_t)row * a.ld_out_bf16 + col, nv, v);
  if (EPI == PGCA_EPI_DLOGITS && a.aux_out) {  // low half of the hi/lo bf16 split of the result (NT-Xent: f32-grade G)
    float lo[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) lo[j] = v[j] - bf2f(f2bf(v[j]));
    st8<VEC>(aux(), nv, lo);
  }
}

// Column sums of one 64 x 64 block (pgca_gemm_args::colsum_part): every lane holds the sums of its 8 columns over the
// rows it handled; the eight lanes that share those columns (lane bits 3..5 = row within the slab) are folded with three
// DPP-free shuffles and lane-row 0 writes row `brow` of the partial matrix.
__device__ __forceinline__ void colsum_flush(const pgca_gemm_args& a, float (&cs)[8], int brow, int col, int ncols,
                                             int lane) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    cs[j] += __shfl_xor(cs[j], 8);
    cs[j] += __shfl_xor(cs[j], 16);
    cs[j] += __shfl_xor(cs[j], 32);
  }
  if ((lane >> 3) == 0 && brow * 64 < a.M) {
    float* p = a.colsum_part + (size_t)brow * a.ld_colsum + col;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (col + j < ncols) p[j] = cs[j];
  }
}

// ---- wave-private staging slab -------------------------------------------------------------------------
// The accumulator block crosses LDS one 16-row MFMA tile row at a time: a slab of 16 x 64 f32 = 4 KiB per wave (32 KiB
// for the eight waves - ONE stage of the 256^2 operand ring, so a persistent kernel can keep the other three stages filled
// with the next tile's operands while it stores).  No padding: float4 group q of row r sits at group q ^ (r & 7), which makes
// the b32 writes of the MFMA layout (two rows x 16 columns per 32 lanes: bit 4 of the column differs) and the b128 row reads
// (the 16-lane service groups touch 16 distinct groups) conflict-free.
constexpr int CB_LD = 64, CB_ROWS = 16;
constexpr int CB_WAVE_FLOATS = CB_LD * CB_ROWS;  // 1024 floats = 4 KiB
__device__ __forceinline__ int cb_idx(int row, int col) { return row * CB_LD + (col ^ ((row & 7) << 2)); }
// slab <- tile row mi of the block (rows mi*16 .. mi*16+15)
__device__ __forceinline__ void cb_write(float* cbuf, const f32x4 (&acc)[4][4], int mi, int lane) {
#pragma unroll
  for (int ni = 0; ni < 4; ++ni)
#pragma unroll
    for (int r = 0; r < 4; ++r) cbuf[cb_idx((lane >> 4) * 4 + r, ni * 16 + (lane & 15))] = acc[mi][ni][r];
}
// 8 consecutive columns (lane & 7) * 8 .. +7 of slab row lr
__device__ __forceinline__ void cb_read8(const float* cbuf, int lr, int lane, float (&v)[8]) {
  const int q = (lane & 7) * 2, x = lr & 7;
  unpack8(*reinterpret_cast<const float4*>(cbuf + lr * CB_LD + ((q ^ x) << 2)),
          *reinterpret_cast<const float4*>(cbuf + lr * CB_LD + (((q + 1) ^ x) << 2)), v);
}

// ---- fast path --------------------------------------------------------------------------------------
// Interior, 16-B-aligned 64 x 64 blocks (all of the hot path).  What the general path below costs is not
// arithmetic but LATENCY: it loads the bias / residual stream / saved activation of 8 rows, waits, finishes them,
// stores, and only then loads the next 8 rows - 16 dependent HBM round trips per 64 x 64 block pair, with the
// matrix pipe idle (s_memtime: 35-66k clocks of epilogue against 52k of main loop at K = 1024).  Here every
// global operand of the whole block is requested up front (one round trip), no lane predicates, no block barriers
// (the staging buffer is private to the wave and a wave's LDS operations execute in order).
enum { PF_NONE = 0, PF_RES = 1, PF_ACC = 2 };  // what is prefetched besides the form's operands: residual / old out_f32

template <int EPI, int PF>
__device__ __forceinline__ void epilogue_store_fast(const pgca_gemm_args& a, f32x4 (&acc)[4][4], float* cbuf, int mb,
                                                    int cb, int lane) {
  constexpr bool AUXIN = epi_reads_aux(EPI), DL = EPI == PGCA_EPI_DLOGITS;
  const int r8 = lane >> 3;
  const int col = cb + (lane & 7) * 8;
  float b[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (a.bias) ld8<true>(a.bias + col, 8, b);
  float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float4 pre[PF != PF_NONE ? 8 : 1][2];
  bf16x8 ax[AUXIN ? 8 : 1];
  float lse[DL ? 8 : 1] = {}, rsc[DL ? 8 : 1] = {};  // the one-element forms are passed on unread: keep them defined
  long long tgt[DL ? 8 : 1] = {};
  unsigned drow[8];  // dead code without dropout
#pragma unroll
  for (int i8 = 0; i8 < 8; ++i8) {
    const int row = mb + i8 * 8 + r8;
    drow[i8] = drop_row(a, row);
    if (PF != PF_NONE) {
      const float* p = PF == PF_RES ? a.residual + (size_t)row * a.ld_res + col
                                    : a.out_f32 + (size_t)row * a.ld_out_f32 + col;
      pre[PF != PF_NONE ? i8 : 0][0] = *reinterpret_cast<const float4*>(p);
      pre[PF != PF_NONE ? i8 : 0][1] = *reinterpret_cast<const float4*>(p + 4);
    }
    if (AUXIN)
      ax[AUXIN ? i8 : 0] =
          *reinterpret_cast<const bf16x8*>(reinterpret_cast<const bf16_t*>(a.aux_in) + (size_t)row * a.ld_aux + col);
    if (DL) {
      lse[DL ? i8 : 0] = a.row_lse[row];
      rsc[DL ? i8 : 0] = a.row_scale[row];
      tgt[DL ? i8 : 0] = a.targets[row];
    }
  }
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    cb_write(cbuf, acc, mi, lane);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int i8 = mi * 2 + it;
      const int lr = it * 8 + r8;
      float v[8], x[8] = {}, side[8], pf[8] = {};
      cb_read8(cbuf, lr, lane, v);
      if (AUXIN) unpack8(ax[AUXIN ? i8 : 0], x);
      if (PF != PF_NONE) unpack8(pre[PF != PF_NONE ? i8 : 0][0], pre[PF != PF_NONE ? i8 : 0][1], pf);
      epilogue_math8<EPI>(a, v, true, b, x, lse[DL ? i8 : 0], rsc[DL ? i8 : 0], tgt[DL ? i8 : 0], drow[i8], col, side);
      epilogue_put8<EPI, true>(a, mb + mi * 16 + lr, col, 8, v, side, PF == PF_RES, pf, PF == PF_ACC, pf, cs);
    }
  }
  if constexpr (epi_colsum(EPI)) {
    if (a.colsum_part) colsum_flush(a, cs, mb >> 6, col, a.N, lane);
  }
}

// Uniform (per wave) test for the fast path: block inside the matrix, every pointer it touches 16-B aligned.
template <int EPI>
__device__ __forceinline__ bool epilogue_fast_ok(const pgca_gemm_args& a, int mb, int cb) {
  const int ncols = EPI == PGCA_EPI_DLOGITS ? a.out_cols : a.N;
  if (a.accumulate == 2 || mb + 64 > a.M || cb + 64 > ncols) return false;
  if (a.residual && a.out_f32 && a.accumulate) return false;
  bool ok = true;
  if (a.bias) ok = ok && al16(a.bias);
  if (a.residual) ok = ok && al16(a.residual) && !(a.ld_res & 3);
  if (a.out_f32) ok = ok && al16(a.out_f32) && !(a.ld_out_f32 & 3);
  if (a.out_bf16) ok = ok && al16(a.out_bf16) && !(a.ld_out_bf16 & 7);
  if (a.aux_out) ok = ok && al16(a.aux_out) && !(a.ld_aux & 7);
  if (a.aux_in) ok = ok && al16(a.aux_in) && !(a.ld_aux & 7);
  return ok;
}

// One 64 x 64 accumulator block (origin mb, cb) through the wave-private slab, 16 rows at a time, so every global access
// of the epilogue (bias, saved activations, residual stream, outputs) is a 16-byte vector op on 128..256 contiguous bytes
// per row.  No block barriers anywhere: the slab is private to the wave and a wave's LDS operations execute in order (the
// caller guarantees every wave has left the main loop's LDS before the first epilogue starts).
template <int EPI>
__device__ __forceinline__ void epilogue_store(const pgca_gemm_args& a, f32x4 (&acc)[4][4], unsigned char* smem, int mb,
                                               int cb, int lane, int wave) {
  float* cbuf = reinterpret_cast<float*>(smem) + wave * CB_WAVE_FLOATS;
  // residual / accumulate prefetch modes exist for the plain epilogue only (where the hot path uses them)
  const bool rmw = a.residual || (a.out_f32 && a.accumulate);
  if ((EPI == PGCA_EPI_NONE || !rmw) && epilogue_fast_ok<EPI>(a, mb, cb)) {  // wave-uniform
    if (EPI == PGCA_EPI_NONE && a.residual) epilogue_store_fast<PGCA_EPI_NONE, PF_RES>(a, acc, cbuf, mb, cb, lane);
    else if (EPI == PGCA_EPI_NONE && rmw) epilogue_store_fast<PGCA_EPI_NONE, PF_ACC>(a, acc, cbuf, mb, cb, lane);
    else epilogue_store_fast<EPI, PF_NONE>(a, acc, cbuf, mb, cb, lane);
    return;
  }
  // ---- general path: edge blocks, unaligned buffers, split-K partials
  const int ncols = EPI == PGCA_EPI_DLOGITS ? a.out_cols : a.N;
  const int col = cb + (lane & 7) * 8;
  float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    cb_write(cbuf, acc, mi, lane);
    if (EPI == PGCA_EPI_NONE && a.accumulate == 2) {
      // split-K partial: f32 atomic adds, one 256-byte row segment of the tile per wave-instruction
      // (the access shape at which global_atomic_add_f32 runs at its full memory-side rate)
      if (cb + lane < a.N) {
        for (int lr = 0; lr < CB_ROWS; ++lr) {
          const int row = mb + mi * 16 + lr;
          if (row < a.M) atomicAdd(a.out_f32 + (size_t)row * a.ld_out_f32 + cb + lane, a.alpha * cbuf[cb_idx(lr, lane)]);
        }
      }
    } else {
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        const int lr = it * 8 + (lane >> 3);
        const int row = mb + mi * 16 + lr;
        float v[8];
        cb_read8(cbuf, lr, lane, v);
        if (row < a.M && col < ncols) {
          const int nv = ncols - col < 8 ? ncols - col : 8;
          const bool has_old = a.out_f32 && a.accumulate;
          float b[8] = {}, x[8] = {}, res[8] = {}, old[8] = {}, side[8], lse = 0.f, rscale = 0.f;
          long long tgt = -1;
          if (a.bias) ld8<false>(a.bias + col, a.N - col < nv ? a.N - col : nv, b);
          if (epi_reads_aux(EPI)) ld8<false>(reinterpret_cast<const bf16_t*>(a.aux_in) + (size_t)row * a.ld_aux + col, nv, x);
          if (EPI == PGCA_EPI_DLOGITS) {
            lse = a.row_lse[row];
            rscale = a.row_scale[row];
            tgt = a.targets[row];
          }
          if (a.residual) ld8<false>(a.residual + (size_t)row * a.ld_res + col, nv, res);
          if (has_old) ld8<false>(a.out_f32 + (size_t)row * a.ld_out_f32 + col, nv, old);
          epilogue_math8<EPI>(a, v, a.bias != nullptr, b, x, lse, rscale, tgt, drop_row(a, row), col, side);
          epilogue_put8<EPI, false>(a, row, col, nv, v, side, a.residual != nullptr, res, has_old, old, cs);
        }
      }
    }
  }
  if constexpr (epi_colsum(EPI)) {
    if (a.colsum_part) colsum_flush(a, cs, mb >> 6, col, ncols, lane);
  }
}

// Runtime epilogue selection for one 64 x 64 accumulator block with origin (mb, cb).
__device__ __forceinline__ void run_epilogue(const pgca_gemm_args& a, f32x4 (&acc)[4][4], unsigned char* smem, int mb,
                                             int cb, int lane, int wave) {
  switch (a.epilogue) {
    case PGCA_EPI_ROWSTATS: epilogue_rowstats(a, acc, mb, cb, lane); break;
    case PGCA_EPI_GELU_NEW: epilogue_store<PGCA_EPI_GELU_NEW>(a, acc, smem, mb, cb, lane, wave); break;
    case PGCA_EPI_QUICK_GELU: epilogue_store<PGCA_EPI_QUICK_GELU>(a, acc, smem, mb, cb, lane, wave); break;
    case PGCA_EPI_RELU: epilogue_store<PGCA_EPI_RELU>(a, acc, smem, mb, cb, lane, wave); break;
    case PGCA_EPI_TANH: epilogue_store<PGCA_EPI_TANH>(a, acc, smem, mb, cb, lane, wave); break;
    case PGCA_EPI_DGELU_NEW: epilogue_store<PGCA_EPI_DGELU_NEW>(a, acc, smem, mb, cb, lane, wave); break;
    case PGCA_EPI_DRELU: epilogue_store<PGCA_EPI_DRELU>(a, acc, smem, mb, cb, lane, wave); break;
    case PGCA_EPI_DTANH: epilogue_store<PGCA_EPI_DTANH>(a, acc, smem, mb, cb, lane, wave); break;
    case PGCA_EPI_DLOGITS: epilogue_store<PGCA_EPI_DLOGITS>(a, acc, smem, mb, cb, lane, wave); break;
    case PGCA_EPI_DQUICK_GELU: epilogue_store<PGCA_EPI_DQUICK_GELU>(a, acc, smem, mb, cb, lane, wave); break;
    case PGCA_EPI_GELU_NEW_D: epilogue_store<PGCA_EPI_GELU_NEW_D>(a, acc, smem, mb, cb, lane, wave); break;
    case PGCA_EPI_MUL_AUX: epilogue_store<PGCA_EPI_MUL_AUX>(a, acc, smem, mb, cb, lane, wave); break;
    default: epilogue_store<PGCA_EPI_NONE>(a, acc, smem, mb, cb, lane, wave); break;
  }
}

}  // namespace
