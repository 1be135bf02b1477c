// mlp_deep_multi.hpp -- M = 2..4 state rollouts per action sequence for the residual MLP with TWO hidden layers
// (models.MLPResidual2, mlp_deep.hpp) on the matrix cores: rollout_mlp_deep_multi.hip, the arithmetic, operand placement and
// pipeline of rollout_mlp_deep.hip with the work split, process-noise draw and cost exchange of mlp_split_multi.hpp (one wave
// per rollout copy).  Its own header for the reason mlp_deep.hpp gives: dispatch.hpp and include/mppi_amd.h are in the include
// closure of the units whose counter passes are committed (tests/test_lookup_evidence.py).
#pragma once
#include <cstddef>
#include <cstdint>
#include "mlp_split_multi.hpp"

namespace mppi {
constexpr size_t DEEP_MULTI_LDS_MAX = 160 * 1024;

// floats of the action tables in front of the hidden layer's bias and planes (Ue | Um | G), padded to 16 bytes
__host__ __device__ inline int deep_multi_table_floats(int J) { return (3 * J + 3) & ~3; }
// dynamic LDS of a launch: tables | hidden->hidden bias (H) | its planes (H/16 x H/32 x 2 planes x 64 lanes x 16 B) | the copies'
// exchange | the minima of a chunk's two halves
inline size_t deep_multi_lds_bytes(int J, int hidden) {
  const int HT = hidden / 16;
  return (size_t)(deep_multi_table_floats(J) + hidden + MULTI_XCHG_FLOATS + 2) * sizeof(float) + (size_t)HT * (HT / 2) * 2 * 64 * 16;
}

// The heavy model has no per-lane form at M > 1, so what the launcher serves is a STATIC promise: the (nx, nu) of the M = 1
// kernel, hidden in {32, 64, 128}, M in 2..PROCESS_NOISE_MM, tables of a (T, nu) sequence within the LDS limit, one environment.
bool mlp_deep_multi_supported(int nx, int nu, int hidden, int M, int T, int n_env);
// 0 / hipError_t; MPPI_E_UNSUPPORTED outside the promise above, for rows the kernel does not read (generated inside K1,
// (K,T,nu)) and for a full Sigma in any form (uncoloured rows, coloured rows, KMPPI's raw actions): the host promises the
// kernel a diagonal Sigma (forms._fused_multi_ok).  Serves `a.states` (M,K,T,nx) itself.
int rollout_mlp_deep_multi(const KArgs<float>& a, hipStream_t st);
}  // namespace mppi

// Not in include/mppi_amd.h yet (they join the header, and _native.SYMBOLS, at the next ABI bump; until then
// pytorch_mppi_amd/_native.py binds them beside the header's symbols): the promise above, and the successful launches of
// rollout_mlp_deep_multi_kernel in this process
extern "C" int mppi_mlp_deep_multi_supported(int32_t nx, int32_t nu, int32_t hidden, int32_t M, int32_t T, int32_t num_envs);
extern "C" int64_t mppi_stat_mlp_deep_multi_launches(void);
