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

template <int LA, int LB>
int launch_s(const pgca_gemm_args& a, int ntm, int ntn, int nkps, int nsplit, hipStream_t s) {
  static const bool attr_ok = hipFuncSetAttribute((const void*)gemm256s_kernel<LA, LB>,
                                                  hipFuncAttributeMaxDynamicSharedMemorySize,
                                                  (int)GEMM256S_LDS) == hipSuccess;  // once, thread-safe
  if (!attr_ok) {
    (void)hipGetLastError();
    set_error("gemm256s: cannot raise dynamic LDS limit");
    return PGCA_ERR_LAUNCH;
  }
  // stagger only where it can pay: >= 3 rounds of workgroups over the 256 CUs
  const int stagger = (ntm * ntn >= 3 * 256 && nsplit == 1) ? gemm_tuning().stagger : 0;
  hipLaunchKernelGGL((gemm256s_kernel<LA, LB>), dim3(ntm * ntn, nsplit), dim3(512), GEMM256S_LDS, s, a, ntm, ntn, nkps,
                     stagger);
  return check_launch("pgca_gemm_bf16(256 phase-staggered)");
}

}  // namespace

int pgca::launch_gemm256s(const pgca_gemm_args& a, int ntm, int ntn, int nk_per_split, int nsplit, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  switch (a.layout) {
    case PGCA_NT: return launch_s<0, 0>(a, ntm, ntn, nk_per_split, nsplit, s);
    case PGCA_NN: return launch_s<0, 1>(a, ntm, ntn, nk_per_split, nsplit, s);
    case PGCA_TN: return launch_s<1, 1>(a, ntm, ntn, nk_per_split, nsplit, s);
    default: set_error("pgca_gemm_bf16: unknown layout %d", a.layout); return PGCA_ERR_INVALID;
  }
}
