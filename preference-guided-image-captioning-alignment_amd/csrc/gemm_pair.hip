// Two problems in one grid of the phase-staggered 256 x 256 GEMM (main loop: gemm_phase_body.h).
#include "gemm_phase_body.h"

namespace {

// Two problems of the same layout and shape in ONE grid of 2 x ntm x ntn workgroups: the forward GEMMs of the policy
// and of the frozen reference policy.  Launched alone each ends on a part-filled last round of the 256 CUs (1144 tiles
// = 4.47 rounds for the N = 1024 projections); together the two tails share one round.  Every workgroup runs
// gemm256s_body on the arguments of its problem - the same k order and the same epilogue code as a single launch, so
// each tile's output is bit-identical to that launch's.
struct pgca_pair_param {
  pgca_gemm_args a[2];
  int ntm, ntn, nk, stagger;
  int order;  // 0: problem 0's tiles, then problem 1's; 1: the problems alternate by GROUP_M group of row tiles
};

template <int LA, int LB>
__global__ __launch_bounds__(512, 2) void gemm256s_pair_kernel(const pgca_pair_param gp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smems[];
  const int ntm = gp.ntm, ntn = gp.ntn, nwg = ntm * ntn;
  // the XCD split is applied to the total: an XCD's run lies in one problem (or crosses the seam once), so its L2 holds
  // the panels of one weight matrix at a time
  const int b = xcd_remap(blockIdx.x, 2 * nwg);
  int p, bid;
  if (gp.order == 0) {
    p = b >= nwg;
    bid = b - (p ? nwg : 0);
  } else {
    // every GROUP_M group before the one that holds b is full, so the division finds the group for the short last one too
    const int per_group = GROUP_M * ntn;
    const int g = b / (2 * per_group);
    const int size = min(GROUP_M, ntm - g * GROUP_M) * ntn;
    const int rem = b - g * 2 * per_group;
    p = rem >= size;
    bid = g * per_group + rem - (p ? size : 0);
  }
  // p and bid depend on blockIdx.x alone; the divisions above run on the vector unit, so bring both back to SGPRs
  // (left in VGPRs, everything derived from bid - the tile origin, live into the epilogue - stays there too)
  p = __builtin_amdgcn_readfirstlane(p);
  bid = __builtin_amdgcn_readfirstlane(bid);
  // p is wave-uniform.  The problem's arguments are copied from the kernel argument segment at a[p] (gp is the only
  // explicit argument: offset 0) by scalar loads, into the SGPRs where the single launch holds its by-value
  // pgca_gemm_args: 100 SGPRs, 256 VGPRs, no scratch, like gemm256s_kernel.  (Selecting field by field between a[0] and
  // a[1] keeps both candidates live across the main loop: 106 SGPRs and spills.)
  const char* kernarg = (const char*)__builtin_amdgcn_kernarg_segment_ptr();
  const pgca_gemm_args a = *(const pgca_gemm_args*)(kernarg + offsetof(pgca_pair_param, a) +
                                                    (p ? sizeof(pgca_gemm_args) : 0));
  // Forward epilogues only: launch_gemm256s_pair admits nothing else, so the derivative, ROWSTATS and DLOGITS cases of
  // run_epilogue are dead code here.
  if (a.epilogue > PGCA_EPI_TANH && a.epilogue != PGCA_EPI_GELU_NEW_D) return;
  gemm256s_body<LA, LB>(a, ntm, ntn, gp.nk, gp.stagger, bid, smems);
}

}  // namespace

int pgca::launch_gemm256s_pair(const pgca_gemm_args& a0, const pgca_gemm_args& a1, const GemmPlan& p, void* stream) {
  // the paired kernel carries the forward epilogues only; any other kind runs as the two single launches
  // pgca_gemm_bf16 makes of these problems (256^2 tile, whole K)
  auto forward_epilogue = [](int e) { return (e >= PGCA_EPI_NONE && e <= PGCA_EPI_TANH) || e == PGCA_EPI_GELU_NEW_D; };
  if (!forward_epilogue(a0.epilogue) || !forward_epilogue(a1.epilogue)) {
    const int rc = launch_gemm256s(a0, p, stream);
    return rc ? rc : launch_gemm256s(a1, p, stream);
  }
  pgca_pair_param gp;
  gp.a[0] = a0;
  gp.a[1] = a1;
  gp.ntm = p.ntm;
  gp.ntn = p.ntn;
  gp.nk = p.nk_per_split;  // in BK = 64 units: the whole K, no split
  gp.stagger = 2 * p.ntm * p.ntn >= 3 * 256 ? gemm_tuning().stagger : 0;
  gp.order = gemm_tuning().pair_order;
  auto launch = [&](auto lb) {  // A is K-contiguous in both layouts the caller pairs (NT, NN)
    constexpr auto kernel = gemm256s_pair_kernel<0, decltype(lb)::value>;
    if (raise_lds_limit<kernel>(GEMM256S_LDS, "gemm256s pair")) return (int)PGCA_ERR_LAUNCH;
    hipLaunchKernelGGL(kernel, dim3(2 * p.ntm * p.ntn), dim3(512), GEMM256S_LDS, (hipStream_t)stream, gp);
    return check_launch("pgca_gemm_bf16_grouped(256 phase-staggered pair)");
  };
  return a0.layout == PGCA_NT ? launch(std::integral_constant<int, 0>{}) : launch(std::integral_constant<int, 1>{});
}
