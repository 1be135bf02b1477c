// mlp_relu.hpp -- the residual MLP with one hidden layer of ReLU units (models.MLPResidual(..., activation="relu")):
//   x' = x + s * (W2 relu(W1 [x;u] + b1) + b2),   cost = sum qx x^2 + sum qu u^2
// Model id and entry points of its matrix-core kernel (rollout_mlp_relu.hip), the model's ONLY fused form: models.hpp, where a
// per-lane functor would live, is in the include closure of the units whose counter passes are committed
// (tests/test_lookup_evidence.py), and so are include/mppi_amd.h and dispatch.hpp -- the id joins the public header at the next ABI
// bump; until then pytorch_mppi_amd/_native.py binds it beside the header's.  What the kernel does not serve (fp64, M > 1,
// visited states, other shapes) the host keeps on the callback loop, decided statically through mppi_model_supported.
#pragma once
#include <cstdint>
#include "common.hpp"

#define MPPI_MODEL_MLP_RELU 6   /* beside MPPI_MODEL_MLP = 4 (include/mppi_amd.h) and MPPI_MODEL_MLP2 = 5 (mlp_deep.hpp) */

namespace mppi {
// Parameter blob: MPPI_MODEL_MLP's layout, unchanged.  The host zero-pads the hidden axis to the kernel's width (a padding unit
// has zero weights in and out and zero bias: relu(0) * 0 contributes nothing).
//   W1 (H, nx+nu) | b1 (H) | W2 (nx, H) | b2 (nx) | s (1) | qx (nx) | qu (nu)
__host__ __device__ inline int64_t mlp_relu_blob_elems(int nx, int nu, int H) {
  return (int64_t)H * (nx + nu) + H + (int64_t)nx * H + nx + 1 + nx + nu;
}

// the engine's static promise (fp32 only: capi.hip asks the dtype): the (nx, nu) of the kernel's instantiations, hidden in {64, 128, 256}
bool supported_mlp_relu(int nx, int nu, int hidden);
// 0 / hipError_t; MPPI_E_UNSUPPORTED for rows it does not read (generated inside K1, a full Sigma coloured in the lane, (K,T,nu)),
// KMPPI's fused interpolation (the caller's two-launch form hands it raw action rows), visited states, M > 1 and action tables
// beyond the CU's LDS beside the layer-2 planes
int rollout_mlp_relu(const KArgs<float>& a, hipStream_t st);
}  // namespace mppi

// successful launches of rollout_mlp_relu_kernel in this process
extern "C" int64_t mppi_stat_mlp_relu_launches(void);
