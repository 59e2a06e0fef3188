// Phase-staggered 256 x 256 GEMM, one problem per launch: the kernel around gemm256s_body (gemm_phase_body.h, where the
// schedule is described) and its launcher.
#include "gemm_phase_body.h"

namespace {

template <int LA, int LB>
__global__ __launch_bounds__(512, 2) void gemm256s_kernel(const pgca_gemm_args a, int ntm, int ntn, int nk_per_split,
                                                          int stagger) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smems[];
  gemm256s_body<LA, LB>(a, ntm, ntn, nk_per_split, stagger, xcd_remap(blockIdx.x, ntm * ntn), smems);
}

}  // namespace

int pgca::launch_gemm256s(const pgca_gemm_args& a, const GemmPlan& p, void* stream) {
  return with_layout(a.layout, [&](auto la, auto lb) {
    constexpr auto kernel = gemm256s_kernel<decltype(la)::value, decltype(lb)::value>;
    if (raise_lds_limit<kernel>(GEMM256S_LDS, "gemm256s")) return (int)PGCA_ERR_LAUNCH;
    // stagger only where it can pay: >= 3 rounds of workgroups over the 256 CUs
    const int stagger = (p.ntm * p.ntn >= 3 * 256 && p.grid_y == 1) ? gemm_tuning().stagger : 0;
    hipLaunchKernelGGL(kernel, dim3(p.ntm * p.ntn, p.grid_y), dim3(512), GEMM256S_LDS, (hipStream_t)stream, a, p.ntm,
                       p.ntn, p.nk_per_split, stagger);
    return check_launch("pgca_gemm_bf16(256 phase-staggered)");
  });
}
