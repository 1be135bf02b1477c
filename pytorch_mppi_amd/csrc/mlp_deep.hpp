// mlp_deep.hpp -- the residual MLP with TWO hidden layers (models.MLPResidual2):
//   x' = x + s * (W3 tanh(W2 tanh(W1 [x;u] + b1) + b2) + b3),   cost = sum qx x^2 + sum qu u^2
// Model id, parameter blob and entry points of its matrix-core kernel (rollout_mlp_deep.hip) and of its per-lane form
// (rollout_mlp2.hip).  Its own header because include/mppi_amd.h, dispatch.hpp and models.hpp are in the include closure of the
// units whose counter passes are committed (tests/test_lookup_evidence.py): the id and the symbol join the public header at the
// next ABI bump; until then pytorch_mppi_amd/_native.py binds them beside the header's.
#pragma once
#include <cstdint>
#include "common.hpp"

#define MPPI_MODEL_MLP2 5   /* beside MPPI_MODEL_MLP = 4 (include/mppi_amd.h) */

namespace mppi {
// Parameter blob.  Both hidden layers have ONE width H = MppiProblem.hidden (the host zero-pads the narrower one; a padding unit
// has zero weights in and out and zero bias, tanh(0) * 0 contributes nothing).  The hidden->hidden matrix is stored TRANSPOSED:
// row k of W2T holds what layer-1 unit k contributes to every layer-2 unit, which is what the per-lane form streams; the output
// matrix is transposed for the same reason (row m = what layer-2 unit m contributes to every state: one contiguous scalar load).
//   W1 (H, nx+nu) | b1 (H) | W2T (H, H), W2T[k][m] = W2[m][k] | b2 (H) | W3T (H, nx) | b3 (nx) | s (1) | qx (nx) | qu (nu)
__host__ __device__ inline int64_t mlp2_blob_elems(int nx, int nu, int H) {
  return (int64_t)H * (nx + nu) + H + (int64_t)H * H + H + (int64_t)nx * H + nx + 1 + nx + nu;
}

// matrix-core kernel: (nx, nu) of its instantiations, hidden in {32, 64, 128}
bool mlp_deep_supported(int nx, int nu, int hidden);
// 0 / hipError_t; MPPI_E_UNSUPPORTED for rows it does not read (generated inside K1, a full Sigma coloured in the lane, (K,T,nu)),
// visited states, M > 1 and where the action tables plus the hidden layer's planes exceed the CU's 160 KB of LDS
int rollout_mlp_deep(const KArgs<float>& a, hipStream_t st);

// the model's dispatcher (matrix cores where they serve the problem, else per lane) and the engine's static promise
int rollout_mlp2(const KArgs<float>& a, hipStream_t st);
int rollout_mlp2(const KArgs<double>& a, hipStream_t st);
bool supported_mlp2(int nx, int nu, int hidden);
}  // namespace mppi

// successful launches of rollout_mlp_deep_kernel in this process
extern "C" int64_t mppi_stat_mlp_deep_launches(void);
