// mlp_split_multi.hpp -- M > 1 state rollouts per action sequence on the split-operand matrix-core MLP kernel
// (rollout_mlp_split_multi.hip: nx <= 16, nu <= 8, one wave per rollout copy), and the three pieces of it that do not depend
// on the network: the process-noise draw cut into pipeline units, the copies' cost exchange through LDS, the discounted
// variance.  Its own header because dispatch.hpp is in the include closure of the units whose counter passes are committed
// (tests/test_lookup_evidence.py).
#pragma once
#include <cstdint>
#include "common.hpp"

namespace mppi {
bool mlp_split_multi_supported(int nx, int nu, int hidden);
// 0 / hipError_t; MPPI_E_UNSUPPORTED for what the kernel does not serve (M outside 2..PROCESS_NOISE_MM, `states`, more than
// one environment, (K,T,nu) rows, nu != 4 with rows generated in K1 or coloured by a full Sigma in the lane, tables beyond the
// launcher's LDS limit): the per-lane kernel takes those
int rollout_mlp_split_multi(const KArgs<float>& a, hipStream_t st);

constexpr int MULTI_CH = 8;          // timesteps per exchange of the copies' costs
constexpr int MULTI_SAMPLES = 32;    // samples a copy-wave rolls at a time (two MFMA column tiles of 16)
// floats of the exchange: [2 buffers][MULTI_CH][PROCESS_NOISE_MM wave slots][MULTI_SAMPLES] step costs + [slots][samples] totals
constexpr int MULTI_XCHG_FLOATS = (2 * MULTI_CH + 1) * PROCESS_NOISE_MM * MULTI_SAMPLES;

#if defined(__HIPCC__)
// One philox_normal4 call of the process-noise stream (common.hpp: key seed ^ PROCESS_NOISE_KEY_TAG, counter (sample,
// (t MM + m) ceil(nx/4) + block, command)), cut into UNITS so that a hand-placed pipeline can put one unit between two
// matrix instructions: unit 0 = counter + round 0, units 1..9 = one round each (7..9 fall away for Philox4x32-7), units 10
// and 11 = one Box-Muller pair each.  The same functions in the same order as philox_normal4: the same bits.
struct ProcNoiseDraw {
  static constexpr int UNITS = 12;
  U4 c;
  unsigned k0, k1;
  template <int UNIT>
  __device__ __forceinline__ void unit(unsigned long long seed, unsigned long long call, long long kg, long long jb,
                                       const bool seven, float (&w)[4]) {
    static_assert(MPPI_PHILOX_ROUNDS == 10, "units 7..9 are the three rounds beyond Philox4x32-7");
    if constexpr (UNIT == 0) {
      const unsigned long long key = seed ^ PROCESS_NOISE_KEY_TAG;
      c = U4{(unsigned)kg, (unsigned)jb, (unsigned)call, (unsigned)(call >> 32) ^ (unsigned)(kg >> 32)};
      k0 = (unsigned)key;
      k1 = (unsigned)(key >> 32);
      philox_round(c, k0, k1, true);
    } else if constexpr (UNIT < 7) {
      philox_round(c, k0, k1, false);
    } else if constexpr (UNIT < 10) {
      if (!seven) philox_round(c, k0, k1, false);
    } else if constexpr (UNIT == 10) {
      box_muller(c.x, c.y, w[0], w[1]);
    } else {
      box_muller(c.z, c.w, w[2], w[3]);
    }
  }
};

// What the copies owe each other: one step cost per (timestep, copy, sample), in chunks of MULTI_CH timesteps, double-buffered
// (one barrier per chunk: nobody writes a half again before everybody has passed the NEXT barrier, i.e. has read it).
// `slot` = the writing wave's index in the workgroup; a sample group's copies sit in consecutive slots.
__device__ __forceinline__ float& multi_cost_slot(float* xch, int buf, int q, int slot, int sample) {
  return xch[((buf * MULTI_CH + q) * PROCESS_NOISE_MM + slot) * MULTI_SAMPLES + sample];
}
__device__ __forceinline__ float& multi_total_slot(float* xch, int slot, int sample) {
  return xch[(2 * MULTI_CH * PROCESS_NOISE_MM + slot) * MULTI_SAMPLES + sample];
}
// cvar += sum over the chunk's nt timesteps of var_m(c_m(t)) dpow, dpow *= var_disc -- the arithmetic and the order of
// rollout_stream_multi (rollout.hpp; mppi.py:363-364), one sample per calling lane
__device__ __forceinline__ void multi_variance_chunk(float* xch, int buf, int nt, int slot0, int M, int sample, float var_disc,
                                                     float& cvar, float& dpow) {
  const float inv_M = 1.0f / (float)M, inv_Mm1 = 1.0f / (float)(M - 1);
  for (int q = 0; q < nt; ++q) {
    float cm[PROCESS_NOISE_MM], mean = 0.f;
#pragma unroll
    for (int mm = 0; mm < PROCESS_NOISE_MM; ++mm) {
      cm[mm] = mm < M ? multi_cost_slot(xch, buf, q, slot0 + mm, sample) : 0.f;
      mean += cm[mm];
    }
    mean *= inv_M;
    float var = 0.f;
#pragma unroll
    for (int mm = 0; mm < PROCESS_NOISE_MM; ++mm) {
      const float d = cm[mm] - mean;
      if (mm < M) var = fmaf(d, d, var);
    }
    cvar = fmaf(var * inv_Mm1, dpow, cvar);
    dpow *= var_disc;
  }
}
#endif
}  // namespace mppi

// successful launches of the kernel in this process.  Not in include/mppi_amd.h yet: it joins the header (and
// _native.SYMBOLS) at the next ABI bump; until then pytorch_mppi_amd/_native.py binds it beside the header's symbols.
extern "C" int64_t mppi_stat_mlp_split_multi_launches(void);
