// mlp_split32_multi.hpp -- M = 2..4 state rollouts per action sequence for the 2-layer residual MLP with 16 < nx <= 32 states
// (models.MLPResidual, mlp_split32.hpp) on the matrix cores: rollout_mlp_split32_multi.hip, the arithmetic, operand placement
// and slot pipeline of rollout_mlp_split32.hip with the work split, process-noise draw units and cost exchange of
// mlp_split_multi.hpp (one wave per rollout copy).  Its own header for the reason mlp_split32.hpp gives: dispatch.hpp and
// include/mppi_amd.h are in the include closure of the units whose counter passes are committed
// (tests/test_lookup_evidence.py).
#pragma once
#include <cstddef>
#include <cstdint>
#include "mlp_split_multi.hpp"

namespace mppi {
constexpr size_t SPLIT32_MULTI_LDS_MAX = 160 * 1024;

// floats of the action tables in front of the layer-1 planes (Ue | Um | G), padded to 16 bytes
__host__ __device__ inline int split32_multi_table_floats(int J) { return (3 * J + 3) & ~3; }
// dynamic LDS of a launch: tables | ONE copy of the layer-1 planes for the four copy-waves (H/16 hidden tiles x 2 k-steps x
// 3 planes x 64 lanes x 16 B: 96 KB at H = 256) | the copies' exchange | the minima of a chunk's two halves
inline size_t split32_multi_lds_bytes(int J, int hidden) {
  return (size_t)(split32_multi_table_floats(J) + MULTI_XCHG_FLOATS + 2) * sizeof(float) + (size_t)(hidden / 16) * 2 * 3 * 64 * 16;
}

// The model has no per-lane form at M > 1 beyond 16 states (rollout_mlp.hip MlpModelRolled), so what the launcher serves is a
// STATIC promise: the (nx, nu) pairs of the M = 1 kernel, the hidden widths whose instantiations hold their registers (see
// rollout_mlp_split32_multi.hip), M in 2..PROCESS_NOISE_MM, one environment, the tables of a (T, nu) sequence beside the planes
// and the exchange within the LDS limit.
bool mlp_split32_multi_supported(int nx, int nu, int hidden, int M, int T, int n_env);
// 0 / hipError_t; MPPI_E_UNSUPPORTED outside the promise above, for rows the kernel does not read (generated inside K1,
// (K,T,nu)) and for a Sigma that is not diagonal (generator-coloured rows carry their own diagonal form).  Serves `a.states`
// (M,K,T,nx) itself.
int rollout_mlp_split32_multi(const KArgs<float>& a, hipStream_t st);
}  // namespace mppi

// Not in include/mppi_amd.h yet (they join the header, and _native.SYMBOLS, at the next ABI bump; until then
// pytorch_mppi_amd/_native.py binds them beside the header's symbols): the promise above, and the successful launches of
// rollout_mlp_split32_multi_kernel in this process
extern "C" int mppi_mlp_split32_multi_supported(int32_t nx, int32_t nu, int32_t hidden, int32_t M, int32_t T, int32_t num_envs);
extern "C" int64_t mppi_stat_mlp_split32_multi_launches(void);
