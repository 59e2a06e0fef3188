// Building blocks shared by the GEMM translation units (gemm.hip, gemm_phase.hip, gemm_pair.hip): the launch plan and
// the host-side launch helpers, the tile order, operand staging geometry, MFMA fragment readers, the LDS-DMA issue
// helper and (gemm_epilogue.h) the fused epilogues.  Everything in the unnamed namespace has internal linkage; the
// cross-TU symbols are pgca::launch_gemm256s (gemm_phase.hip), pgca::launch_gemm256s_pair (gemm_pair.hip) and
// pgca::gemm_tuning / pgca::plan_gemm (gemm.hip).
#pragma once
#include <stdlib.h>

#include <type_traits>

#include "common.h"

namespace pgca {
// What pgca_gemm_bf16 launches for one problem; pgca_gemm_plan reports it, the paired launch reads it.
struct GemmPlan {
  int tile;          // 128 = register-staged 128^2 kernel, 256 = LDS-DMA 256^2 kernels
  int variant;       // schedule of the 256^2 tile: 0 = 2-stage BK=64 loop (gemm.hip), 6 = phase-staggered (gemm_phase.hip)
  int splits;        // planned split-K factor (> 1: partials meet through f32 atomics, accumulate == 2)
  int ntm, ntn;      // tiles along M and along the output columns
  int nk_per_split;  // 64-deep K tiles per split
  int grid_y;        // splits that own at least one K tile: ceil(K tiles / nk_per_split) <= splits
  int ncols;         // output columns: N, or out_cols for DLOGITS
};
GemmPlan plan_gemm(const pgca_gemm_args& a);
// 256 x 256, 8 waves, phase-staggered wave groups, 4-stage BK=32 ring (gemm_phase.hip).
int launch_gemm256s(const pgca_gemm_args& a, const GemmPlan& p, void* stream);
// Two NT or two NN problems of one shape and plan `p` (whole K, no split) as ONE grid of that kernel's tiles (gemm_pair.hip).
int launch_gemm256s_pair(const pgca_gemm_args& a0, const pgca_gemm_args& a1, const GemmPlan& p, void* stream);

// Process-wide dispatch knobs (pgca_set_option / environment, read ONCE): nothing on the launch path calls getenv.
struct GemmTuning {
  int tile;      // 0 = automatic, 128 / 256 = force that kernel family      (PGCA_GEMM_TILE)
  int schedule;  // -1 = automatic, 0 = 2-stage BK=64 loop, 6 = phase-staggered (PGCA_GEMM_RING)
  int group;     // 1 = grouped launches: the four weight gradients of a block, the forward pair of two trunks
                 //                                                              (PGCA_GEMM_NO_GROUP inverts)
  int pair_order;  // tile order of the paired launch: 0 = problem after problem, 1 = alternating by GROUP_M group
  int stagger;   // start delay step of the first wave of workgroups, in units of 1024 clocks (PGCA_GEMM_STAGGER)
};
GemmTuning& gemm_tuning();
}  // namespace pgca

using namespace pgca;

namespace {

// ---- host-side launch helpers ---------------------------------------------------------------------
// pgca_gemm_args::layout -> <LA, LB>, the K-strided flags of A and B: f(integral_constant<LA>, integral_constant<LB>).
template <typename F>
int with_layout(int layout, F&& f) {
  using S0 = std::integral_constant<int, 0>;
  using S1 = std::integral_constant<int, 1>;
  switch (layout) {
    case PGCA_NT: return f(S0{}, S0{});
    case PGCA_NN: return f(S0{}, S1{});
    case PGCA_TN: return f(S1{}, S1{});
    default: set_error("pgca_gemm_bf16: unknown layout %d", layout); return PGCA_ERR_INVALID;
  }
}

// Raises KERNEL's dynamic-LDS limit to `bytes`, once per kernel (initialisation of the local static is thread-safe).
template <auto KERNEL>
int raise_lds_limit(size_t bytes, const char* what) {
  static const bool ok = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)bytes) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    set_error("%s: cannot raise dynamic LDS limit", what);
    return PGCA_ERR_LAUNCH;
  }
  return PGCA_OK;
}

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int TILE_BYTES = 128 * 64 * 2;
constexpr int BM2 = 256, BN2 = 256;
constexpr int TILE2_BYTES = 256 * 64 * 2;
constexpr unsigned OOB = 0x80000000u;

// ---- tile order -----------------------------------------------------------------------------------
// Workgroup b runs on XCD b % 8: XCD x walks a contiguous run of the `total` places, so an XCD's resident blocks share
// operand panels in its private L2.
__device__ __forceinline__ int xcd_remap(int b, int total) {
  const int xcd = b & 7, q = total >> 3, r = total & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
}
// ... and inside that run tiles are visited in groups of GROUP_M tile rows, M fastest within a group: the ~64 blocks an
// XCD holds at once cover an 8 x 8 patch of tiles, so each A and B panel is fetched into its L2 once per 8 uses.
constexpr int GROUP_M = 8;
__device__ __forceinline__ void group_m_tile(int bid, int ntm, int ntn, int& tm, int& tn) {
  const int per_group = GROUP_M * ntn;
  const int group = bid / per_group;
  const int first_m = group * GROUP_M;
  const int gsize = min(GROUP_M, ntm - first_m);
  const int in_group = bid - group * per_group;
  tm = first_m + in_group % gsize;
  tn = in_group / gsize;
}

// ---- in-kernel clocks (diagnostic builds) -----------------------------------------------------------
// -DPGCA_GEMM_TIMING: main-loop / epilogue clocks per workgroup; -DPGCA_GEMM_TIMING2 adds per-phase clocks of the
// phase-staggered loop (tools/gemm_bench.py --timing reads them from the stat_max / stat_sum buffers).  Stamps cost a
// lgkmcnt(0) each; the product build defines neither.
#define PGCA_CLOCK(insn, v) asm volatile(insn " %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v)::"memory")
#ifdef PGCA_GEMM_TIMING
#define TSTAMP(v) PGCA_CLOCK("s_memtime", v)
#define TSTAMP_REAL(v) PGCA_CLOCK("s_memrealtime", v)  // constant 100 MHz
#else
#define TSTAMP(v)
#define TSTAMP_REAL(v)
#endif
#ifdef PGCA_GEMM_TIMING2
#define PSTAMP(v) PGCA_CLOCK("s_memtime", v)
#else
#define PSTAMP(v)
#endif

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0x7ffffff0, 0x00020000);
}

// ---- per-thread staging geometry of one operand tile -----------------------------------------
// KS = 0: operand is [rows, K] (K contiguous); tile image [128 rows][64 k], 128-B rows,
//         16-B chunk c of row r stored at chunk (c ^ (r & 7)).
// KS = 1: operand is [K, cols] (K strided);   tile image [64 k][128 cols], 256-B rows,
//         32-B slot s of row k stored at slot (s ^ h(k)), h(k) = (k&3) | ((k>>3)&1)<<2.
template <int KS>
struct Stage {
  unsigned goff[4];   // byte offset of this thread's 4 chunks relative to the tile base pointer
  unsigned loff[4];   // byte offset in the LDS image
  bool vspace[4];     // row (KS=0) / column (KS=1) inside the matrix
  int kpos[4];        // k offset inside the tile of each chunk (for the K-edge test)

  __device__ __forceinline__ void init(int t, int ld, int origin, int extent) {
    if (KS == 0) {
      const int r = t >> 3, c = t & 7;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = r + 32 * i;
        goff[i] = (unsigned)(row * ld + c * 8) * 2u;
        loff[i] = (unsigned)(row * 128 + ((c ^ (row & 7)) << 4));
        vspace[i] = (origin + row) < extent;
        kpos[i] = c * 8;
      }
    } else {
      const int kr = t >> 4, c16 = t & 15;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = kr + 16 * i;
        const int h = (k & 3) | (((k >> 3) & 1) << 2);
        goff[i] = (unsigned)(k * ld + c16 * 8) * 2u;
        loff[i] = (unsigned)(k * 256 + (((c16 >> 1) ^ h) << 5) + ((c16 & 1) << 4));
        vspace[i] = (origin + c16 * 8) < extent;
        kpos[i] = k;
      }
    }
  }
  __device__ __forceinline__ void load(const bf16_t* base, int krem, u32x4 (&r)[4]) const {
    __amdgpu_buffer_rsrc_t rs = make_rsrc(base);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool ok = vspace[i] && (kpos[i] < krem);
      r[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, ok ? goff[i] : OOB, 0, 0);
    }
  }
  __device__ __forceinline__ void store(unsigned char* lds, const u32x4 (&r)[4]) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4*>(lds + loff[i]) = r[i];
  }
};

// ---- fragment readers ---------------------------------------------------------------------------
// Returns the MFMA 16x16x32 operand fragment of 16-row (or 16-col) sub-tile `sub` of the wave's
// 64-wide strip starting at `wbase`, k-step kk (0,1) of the 64-deep tile.
template <int KS, int KSTRIDE = 256>
__device__ __forceinline__ bf16x8 read_frag(const unsigned char* lds, int wbase, int sub, int kk, int lane) {
  if (KS == 0) {
    const int row = wbase + sub * 16 + (lane & 15);
    const int c = kk * 4 + (lane >> 4);
    return *reinterpret_cast<const bf16x8*>(lds + row * 128 + ((c ^ (lane & 7)) << 4));
  } else {
    const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
    const int k = kk * 32 + 8 * g + q;
    const int h = q | ((g & 1) << 2);
    const int s32 = (wbase >> 4) + sub;
    const unsigned char* a0 = lds + k * KSTRIDE + ((s32 ^ h) << 5) + 8 * p;
    return tr_frag(a0, a0 + 4 * KSTRIDE);
  }
}

}  // namespace

#include "gemm_epilogue.h"

namespace {

// ---- LDS-DMA of one operand tile of the 256^2 kernels ------------------------------------------------
// The image of a 256 x BKT tile (BKT = 64: 32 KiB, gemm.hip; BKT = 32: 16 KiB, gemm_phase_body.h) is copied in 1-KiB
// pieces, BKT / 16 per wave.  The LDS image of each DMA instruction is lane-linear, so the XOR swizzles are applied to the
// SOURCE address (same involutions as the fragment readers).
__device__ __forceinline__ int swz4p(int q) { return (0x78 >> (2 * q)) & 3; }  // {0,2,3,1}

template <int KS, int BKT>
struct Dma {
  static constexpr int NP = BKT / 16;
  unsigned goff[NP];
  __device__ __forceinline__ void init(int lane, int wave, int ld, int origin, int extent) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int j = wave * NP + i;  // piece of the tile image
      if (KS == 0) {
        // [256 rows][64 k]: piece = 8 rows x 128 B, chunk c of row r at c ^ (r & 7)
        // [256 rows][32 k]: piece = 16 rows x 64 B, chunk c of row r at c ^ swz4p((r>>2)&3)
        const int r = BKT == 64 ? 8 * j + (lane >> 3) : 16 * j + (lane >> 2);
        const int c = BKT == 64 ? (lane & 7) ^ (lane >> 3) : (lane & 3) ^ swz4p((lane >> 4) & 3);
        const int rg = min(origin + r, extent - 1) - origin;
        goff[i] = (unsigned)(rg * ld + c * 8) * 2u;
      } else {  // [BKT k][256 cols]: piece = 2 k-rows x 512 B
        const int k = 2 * j + (lane >> 5);
        const int c16 = lane & 31;
        const int h = (k & 3) | (((k >> 3) & 1) << 2);
        const int col = (((c16 >> 1) ^ h) << 4) + ((c16 & 1) << 3);
        const int cg = min(origin + col, extent - 8) - origin;
        goff[i] = (unsigned)(k * ld + cg) * 2u;
      }
    }
  }
  // The DMA is issued from inline asm on purpose: hipcc tracks a builtin LDS-DMA as a pending LDS write and
  // drains it (s_waitcnt vmcnt(0)) in front of the next ds_read, which would serialise the copy of tile t+1 with
  // the MFMAs of tile t.  Untracked, it stays in flight across the whole compute phase; dma_wait() retires it
  // right before the barrier that hands the buffer to the readers.  (M0 = LDS byte address of lane 0's 16 bytes.)
  __device__ __forceinline__ void issue(const bf16_t* base, unsigned char* tile, int wave) const {
    const unsigned long long b = (unsigned long long)base;
    u32x4 rs;
    rs[0] = (unsigned)b;
    rs[1] = (unsigned)(b >> 32) & 0xffffu;
    rs[2] = 0x7ffffff0u;
    rs[3] = 0x00020000u;
    const unsigned lds0 = (unsigned)(size_t)LDS_PTR(tile) + (unsigned)wave * (NP * 1024u);
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      if constexpr (BKT == 64) {
        asm volatile("s_nop 4\n\ts_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds"
                     :
                     : "s"(lds0 + i * 1024u), "v"(goff[i]), "s"(rs)
                     : "memory");
      } else {
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds"
                     :
                     : "s"(lds0 + i * 1024u), "v"(goff[i]), "s"(rs)
                     : "memory");
      }
    }
  }
};

__device__ __forceinline__ void dma_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

template <int LA>
__device__ __forceinline__ void mma_half(const unsigned char* la, int row0, int kk, int lane, const bf16x8 (&fb)[4],
                                         f32x4 (&acc)[4][4]) {
  bf16x8 fa[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) fa[i] = read_frag<LA, 512>(la, row0, i, kk, lane);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
}

}  // namespace
