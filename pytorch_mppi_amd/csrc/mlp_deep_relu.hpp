// mlp_deep_relu.hpp -- the residual MLP with TWO hidden layers of ReLU units (models.MLPResidual2(..., activation="relu")):
//   x' = x + s * (W3 relu(W2 relu(W1 [x;u] + b1) + b2) + b3),   cost = sum qx x^2 + sum qu u^2
// Model id and entry points of its matrix-core kernel (rollout_mlp_deep_relu.hip), the model's ONLY fused form.  Its own header
// for the reason mlp_deep.hpp and mlp_relu.hpp give: include/mppi_amd.h, dispatch.hpp and models.hpp are in the include closure
// of the units whose counter passes are committed (tests/test_lookup_evidence.py) -- the id joins the public header at the next
// ABI bump; until then pytorch_mppi_amd/_native.py binds it beside the header's.  What the kernel does not serve (fp64, M > 1,
// visited states, other shapes) the host keeps on the callback loop, decided statically through mppi_model_supported.
#pragma once
#include <cstdint>
#include "common.hpp"
#include "mlp_deep.hpp"   // the parameter blob: MPPI_MODEL_MLP2's layout, unchanged (mlp2_blob_elems)

#define MPPI_MODEL_MLP2_RELU 7   /* beside MPPI_MODEL_MLP2 = 5 (mlp_deep.hpp) and MPPI_MODEL_MLP_RELU = 6 (mlp_relu.hpp) */

namespace mppi {
// Parameter blob: mlp2_blob_elems(nx, nu, H), both hidden layers zero-padded by the host to the kernel's width H (a padding unit
// has zero weights in and out and zero bias: relu(0) * 0 contributes nothing).

// the engine's static promise (fp32 only: capi.hip asks the dtype): the (nx, nu) of the kernel's instantiations, hidden in {64, 128}
bool supported_mlp2_relu(int nx, int nu, int hidden);
// 0 / hipError_t; MPPI_E_UNSUPPORTED for rows it does not read (generated inside K1, a full Sigma coloured in the lane, (K,T,nu)),
// KMPPI's fused interpolation (the caller's two-launch form hands it raw action rows), visited states, M > 1 and action tables
// beyond the CU's 160 KB of LDS beside the hidden layer's planes (96 KB at H = 128)
int rollout_mlp_deep_relu(const KArgs<float>& a, hipStream_t st);
}  // namespace mppi

// successful launches of rollout_mlp_deep_relu_kernel in this process
extern "C" int64_t mppi_stat_mlp_deep_relu_launches(void);
