// mlp_split32.hpp -- entry points of the two-output-tile split-operand MLP kernel (rollout_mlp_split32.hip): 16 < nx <= 32.
// Its own header because dispatch.hpp is in the include closure of the units whose counter passes are committed
// (tests/test_lookup_evidence.py).
#pragma once
#include <cstdint>
#include "common.hpp"

namespace mppi {
bool mlp_split32_supported(int nx, int nu, int hidden);
// 0 / hipError_t; MPPI_E_UNSUPPORTED for rows it does not read (generated inside K1, a full Sigma coloured in the lane, (K,T,nu))
// and where the LDS tables plus the layer-1 weights exceed the CU's 160 KB (long horizons): the per-lane kernel takes those
int rollout_mlp_split32(const KArgs<float>& a, hipStream_t st);
}  // namespace mppi

// successful launches of the kernel in this process.  Not in include/mppi_amd.h yet: it joins the header (and
// _native.SYMBOLS) at the next ABI bump; until then pytorch_mppi_amd/_native.py binds it beside the header's symbols.
extern "C" int64_t mppi_stat_mlp_split32_launches(void);
