// K1 for the 2-layer MLP residual model with process noise and M = 2..4 state rollouts per action sequence
// (rollout_samples, mppi.py:334-373) on the 16-bit matrix cores: the split-operand arithmetic and the slot pipeline of
// rollout_mlp_split.hip (mlp_split_ops.hpp), ONE WAVE PER ROLLOUT COPY.
//
//   x' = x + s * (W2 tanh(W1 [x;u] + b1) + b2) + sd (.) n,   c_m(t) = sum qx x^2 + sum qu u^2   on the noisy state
//   total = mean_m sum_t c_m(t) + var_cost sum_t var_disc^t var_m(c_m(t)) + smoothness (once) + action cost (once)
// -- the quantities, conventions and process-noise counters of rollout_stream_multi (rollout.hpp), which this kernel replaces
// for nx <= 16 (there every copy is one more per-lane MLP step in the same lane).
//
// Arithmetic, operand layout and register budget are the M = 1 kernel's: layer 1 bf16 x 3 (six piece products), layer 2
// fp16 x 2 (three), transposed chain with the samples on the MFMA column axis, lane (g, s) owns state rows 4g..4g+3 and
// control(s) g (, g + 4), all weights resident (layer 1 in the AGPRs), two 16-sample tiles per wave.
//
// Work split.  The four waves of a workgroup hold the same weights, each in its own registers, and roll DIFFERENT COPIES of
// the SAME 32 samples.  A chunk is 64 consecutive samples (one block_min slot):
//   M = 3 | 4   the workgroup walks the chunk's two 32-sample halves one after the other, wave m = copy m (M = 3: the fourth
//               wave only keeps the barriers company);
//   M = 2       waves (0, 1) take half 0 and waves (2, 3) half 1 at the same time.
// Process noise.  Lane group g owns exactly Philox block q = g of the stream (its four state rows): one draw per tile and
// timestep, counter ((t MM + m) ceil(nx/4) + g).  The draw does not depend on the state, so its ~110 VALU instructions are cut
// into 12 units per tile (mlp_split_multi.hpp) and laid between the 24 matrix instructions of layer 1 of the FIRST hidden
// pair, where the M = 1 pipeline has nothing to overlap; the four normals wait in registers for the state update at the end of
// the timestep.  Lane groups beyond the model's nx carry sd = 0 (their draw is never used: x stays 0).
// What the copies owe each other is c_m(t): the lane's partial (its state rows + its control-effort term) is summed over the
// four lane groups and exchanged through LDS in chunks of 8 timesteps, double-buffered, one barrier per chunk; the first 32
// lanes of the sample group's first wave accumulate the discounted variance (one sample each), add the copies' totals in copy
// order and write cost, pert and the minimum.  Action cost and smoothness cost belong to the action sequence: counted once.
#include <hip/hip_ext.h>
#include <atomic>
#include <cstdlib>
#include "actions.hpp"
#include "dispatch.hpp"
#include "mlp_split_multi.hpp"
#include "mlp_split_ops.hpp"

namespace mppi {
using namespace split_ops;

namespace {
constexpr int SM_NT = 2;               // sample tiles (of 16) per wave
constexpr int SM_VPU = 2;              // hidden activations per VALU unit of the software pipeline
constexpr int SM_THREADS = 256;        // 4 waves = one per SIMD
constexpr int SM_CHUNK = 64;           // samples per workgroup chunk = one block_min slot
constexpr size_t SM_LDS_MAX = 60 * 1024;
static_assert(SM_NT * 16 == MULTI_SAMPLES && SM_THREADS / WAVE == PROCESS_NOISE_MM, "one wave per copy, two tiles per wave");

// component g (lane-dependent) of a row held in registers, as two levels of v_cndmask with the operands pinned in VGPRs (left
// alone, hipcc indexes the row dynamically, i.e. through scratch memory)
__device__ __forceinline__ float pick4_lane(const float (&z)[4], int g) {
  float a0 = z[0], a1 = z[1], a2 = z[2], a3 = z[3];
  asm volatile("" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3));
  const float lo = (g & 1) ? a1 : a0, hi = (g & 1) ? a3 : a2;
  return (g & 2) ? hi : lo;
}
}  // namespace

template <int HT /* hidden / 16 */, int NOISE, bool DIAG, int NX, int NU>
__global__ void __launch_bounds__(SM_THREADS, 1) rollout_mlp_split_multi_kernel(const KArgs<float> a) {
  static_assert(HT % 2 == 0, "layer 2 consumes hidden tiles in pairs");
  static_assert(NX >= 1 && NX <= 16 && NU >= 1 && NU <= 8, "one 16-state output tile, one 32-slot layer-1 k-step");
  constexpr int NC = NU > 4 ? 2 : 1, BIAS_E = 4 + NC, NI = NX + NU, NXB = (NX + 3) / 4;
  constexpr int NT = SM_NT, H = HT * 16, HP = HT / 2, MM = PROCESS_NOISE_MM, CH = MULTI_CH;
  // rows that are not one row-of-4 per timestep (nu != 4) are read component-wise only: external rows, diagonal / coloured form
  constexpr bool ROW1 = NOISE != MPPI_NOISE_PHILOX && (DIAG || NOISE == MPPI_NOISE_ACTIONS);
  static_assert(NU == 4 || ROW1, "nu != 4: component-wise rows only");
  stamp_entry(a.tstamp);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* Ue = reinterpret_cast<float*>(smem_raw);   // [J]
  float* Um = Ue + a.J;                             // [J]
  float* G = Um + a.J;                              // [J]
  float* fac = G + a.J;                             // [2*NU*NU]
  float* xch = fac + 2 * NU * NU;                   // [MULTI_XCHG_FLOATS] the copies' step costs and totals
  float* red = xch + MULTI_XCHG_FLOATS;             // [2] the minima of the chunk's two halves

  // (the wave index as a scalar: copy, sample half and the `mine` / `lead` branches below are wave-uniform)
  const int lane = threadIdx.x & (WAVE - 1), wv = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int g = lane >> 4, s = lane & 15;
  const int M = a.M;
  const bool pairs = M == 2;                        // two sample groups of two copy-waves | one group of up to four
  const int m = pairs ? (wv & 1) : wv;              // this wave's copy
  const int slot0 = pairs ? (wv & 2) : 0;           // first exchange slot of this wave's sample group
  const bool mine = m < M, lead = wv == slot0;
  const int npass = pairs ? 1 : 2;

  // ---- parameters: blob = W1 (H,nx+nu) | b1 (H) | W2 (nx,H) | b2 (nx) | res_scale | qx (nx) | qu (nu) ----
  const float* __restrict__ W1 = a.mp;
  const float* __restrict__ b1 = W1 + H * NI;
  const float* __restrict__ W2 = b1 + H;
  const float* __restrict__ b2 = W2 + NX * H;
  const float rs = b2[NX];
  float qx4[4], sd4[4];
  const bool noisy = a.proc_sd != nullptr;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    qx4[r] = 4 * g + r < NX ? b2[NX + 1 + 4 * g + r] : 0.f;
    sd4[r] = (noisy && 4 * g + r < NX) ? a.proc_sd[4 * g + r] : 0.f;
  }
  bool own[NC];
  float qu_c[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    own[c] = g + 4 * c < NU;
    qu_c[c] = own[c] ? b2[NX + 1 + NX + g + 4 * c] : 0.f;
  }

  // A fragments, resident for the whole launch (every wave its own: the copies share nothing but the exchange)
  Planes A1[HT];
  PlanesH A2[HP];
#pragma unroll
  for (int mt = 0; mt < HT; ++mt) {
    const float* __restrict__ row = W1 + (16 * mt + s) * NI;       // hidden unit 16 mt + s
    float v[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = 4 * g + e < NX ? EXP2_SCALE * row[4 * g + e] : 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) v[4 + c] = own[c] ? EXP2_SCALE * row[NX + g + 4 * c] : 0.f;
    v[BIAS_E] = g == 0 ? EXP2_SCALE * b1[16 * mt + s] : 0.f;       // bias column (B1 holds 1 there)
#pragma unroll
    for (int e = BIAS_E + 1; e < 8; ++e) v[e] = 0.f;
    A1[mt] = split_pack8(v);
  }
  float rowsum = 0.f;                                              // of row s of W2, this lane's quarter
#pragma unroll
  for (int j = 0; j < HP; ++j) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float w = s < NX ? W2[s * H + 16 * (2 * j + (e >> 2)) + 4 * g + (e & 3)] : 0.f;   // state row s, hidden h(j,g,e)
      rowsum += w;
      v[e] = -2.0f * w;
    }
    A2[j] = split_pack8_h(v);
  }
  // the 192 layer-1 weight registers live in the accumulation registers: an MFMA reads its A operand from an AGPR directly
#pragma unroll
  for (int mt = 0; mt < HT; ++mt) {
    asm volatile("" : "+a"(A1[mt].h));
    asm volatile("" : "+a"(A1[mt].m));
    asm volatile("" : "+a"(A1[mt].l));
  }
  rowsum += __shfl_xor(rowsum, 16, WAVE);
  rowsum += __shfl_xor(rowsum, 32, WAVE);
  float b2r[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) b2r[r] = (4 * g + r < NX ? b2[4 * g + r] : 0.f) + __shfl(rowsum, 4 * g + r, WAVE);   // D rows are 4g+r

  ActionConsts<float, NU> ac;
  ac.load(a, DIAG ? nullptr : fac);
  // Ue = the sequence the noise is added to and measured from (SMPPI: the host's base A + U dt); the action cost table G is
  // built from the lifted nominal U itself (u_eff) either way
  const bool smppi = a.B != nullptr;
  for (int j = threadIdx.x; j < a.J; j += SM_THREADS) Ue[j] = u_base(a, j);
  __syncthreads();
  for (int j = threadIdx.x; j < a.J; j += SM_THREADS) {
    const int n = j % NU, t0 = j - n;
    const float uj = Ue[j];
    Um[j] = a.coloured ? uj : uj + a.mu[n];
    float gg;
    if constexpr (DIAG) {
      if (a.coloured && !a.diag) {          // generator-coloured full Sigma: whole-row G from global
        gg = 0.f;
        for (int q = 0; q < NU; ++q) gg = fmaf(a.sinv[n * NU + q], smppi ? u_eff(a, t0 + q) : Ue[t0 + q], gg);
      } else {
        gg = (smppi ? u_eff(a, j) : uj) * a.sinv[n * NU + n];
      }
    } else {
      gg = 0.f;
      for (int q = 0; q < NU; ++q) gg = fmaf(ac.Sm[n * NU + q], smppi ? u_eff(a, t0 + q) : Ue[t0 + q], gg);
    }
    G[j] = a.lambda_ * gg;
  }
  __syncthreads();
  float sd_c[NC], lo_c[NC], hi_c[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int n = own[c] ? g + 4 * c : 0;
    sd_c[c] = a.coloured ? 1.f : a.L[n * NU + n];
    lo_c[c] = a.umin[n];
    hi_c[c] = a.umax[n];
  }
  float Lrow[NU];
  if constexpr (!DIAG) {
#pragma unroll
    for (int q = 0; q < NU; ++q) Lrow[q] = ac.Lm[g * NU + q];
  }
  const unsigned long long pn_seed = a.seed, pn_call = a.call;
  const bool seven = a.seven != 0;
  const float inv_M = 1.0f / (float)M;

  // ---- persistent over 64-sample chunks: the 288 weight registers are loaded once per wave ----
  const int nchunks = (a.K + SM_CHUNK - 1) / SM_CHUNK;
  for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    for (int pass = 0; pass < npass; ++pass) {
      const int half = pairs ? (wv >> 1) : pass;
      const int kbase = chunk * SM_CHUNK + half * MULTI_SAMPLES;
      int kk[NT], orow[NT];
      bool act[NT];
      float x[NT][4], cs[NT], ppart[NT], spart[NT], vprev[NT][NC];
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        const int kraw = kbase + 16 * i + s;
        act[i] = kraw < a.K;
        kk[i] = act[i] ? kraw : a.K - 1;
        orow[i] = overwrite_row(a, a.k_offset + kk[i]);
        const float* __restrict__ s0 = a.state_per_sample ? a.state + (long long)kk[i] * NX : a.state;
#pragma unroll
        for (int r = 0; r < 4; ++r) x[i][r] = 4 * g + r < NX ? s0[4 * g + r] : 0.f;
        cs[i] = 0.f;
        ppart[i] = 0.f;
        spart[i] = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) vprev[i][c] = 0.f;
      }
      float cvar = 0.f, dpow = 1.f;          // (lead wave, lanes 0..31: sample `lane` of the group)
      int buf = 0, t_done = 0;               // exchange half in use; timesteps whose variance has been accumulated

      float zc[NT][4], zn[NT][4];
      auto fetch = [&](int t, float (&dst)[NT][4]) {
#pragma unroll
        for (int i = 0; i < NT; ++i) {
          if constexpr (ROW1) {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
              const int j = t * NU + (own[c] ? g + 4 * c : 0);
              dst[i][c] = a.z[((long long)(j >> 2) * a.zp + kk[i]) * 4 + (j & 3)];
            }
          } else {
            noise4<float, NOISE == MPPI_NOISE_ACTIONS ? MPPI_NOISE_TNK4 : NOISE>(a, t, kk[i], dst[i]);
          }
        }
      };
      if (mine) fetch(0, zn);

      for (int t = 0; t < a.Tn; ++t) {
        if (mine) {
#pragma unroll
          for (int i = 0; i < NT; ++i) {
#pragma unroll
            for (int c = 0; c < (ROW1 ? NC : 4); ++c) zc[i][c] = zn[i][c];
          }
          if constexpr (NOISE == MPPI_NOISE_PHILOX) {
            // every copy-wave regenerates the row; copy 0 stores it
            if (a.z != nullptr && g == 0 && m == 0) {
#pragma unroll
              for (int i = 0; i < NT; ++i)
                if (act[i]) store4<float>(const_cast<float*>(a.z), a.zp, t, kk[i], zc[i]);
            }
          }
          fetch(t + 1 < a.Tn ? t + 1 : t, zn);   // prefetch the next step's rows

          // ---- actions (as in the M = 1 kernel): lane (g,s) owns control dimension g (and g + 4 where nu > 4); every copy-wave
          // makes them for itself ----
          float Ut[NC], Umt[NC], Gt[NC], cstep[NT];
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            const int jn = t * NU + (own[c] ? g + 4 * c : 0);
            Ut[c] = Ue[jn]; Umt[c] = Um[jn]; Gt[c] = own[c] ? G[jn] : 0.f;
          }
          Planes B1[NT];
#pragma unroll
          for (int i = 0; i < NT; ++i) {
            float uu[NC];
            cstep[i] = 0.f;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
              float v;
              if constexpr (NOISE == MPPI_NOISE_ACTIONS) {
                v = zc[i][c];                                   // ROW1: the lane's component was loaded
              } else if constexpr (DIAG) {
                const float zg = ROW1 ? zc[i][c] : pick4_lane(zc[i], g);
                v = fmaf(zg, sd_c[c], Umt[c]);
              } else {
                float acc = Umt[c];
#pragma unroll
                for (int q = 0; q < NU; ++q) acc = fmaf(zc[i][q], Lrow[q], acc);
                v = acc;
              }
              if (orow[i] == -1) v = 0.f;
              else if (orow[i] >= 0) v = a.sampler[((long long)orow[i] * a.Tn + t) * NU + (own[c] ? g + 4 * c : 0)];
              v = clampT(v, lo_c[c], hi_c[c]);
              if (NU != 4 && NU != 8) v = own[c] ? v : 0.f;                         // a lane group without a control of its own
              const float e = (v - Ut[c]) * ac.e_scale;                             // e_scale = 1 | 1/dt (SMPPI)
              ppart[i] = fmaf(Gt[c], ac.abs_cost ? fabsf(e) : e, ppart[i]);
              if (a.smooth_w != 0.f) {
                // SMPPI smoothness cost w |v[t] - v[t-1]|^2: of the action sequence, not of a copy -- its own sum
                const float d = v - vprev[i][c];
                if (t > 0) spart[i] = fmaf(a.smooth_w * d, d, spart[i]);
                vprev[i][c] = v;
              }
              uu[c] = a.u_scale * v;
              cstep[i] = fmaf(qu_c[c] * uu[c], uu[c], cstep[i]);                    // control effort (qu = 0: + 0)
            }
            float in[8] = {x[i][0], x[i][1], x[i][2], x[i][3], uu[0], 0.f, 0.f, 0.f};
            if constexpr (NC == 2) in[5] = uu[1];
            in[BIAS_E] = g == 0 ? 1.0f : 0.0f;
            B1[i] = split_pack8(in);
          }

          // ---- the two layers as the explicit software pipeline of rollout_mlp_split.hip (see there for the cycle budget and
          // the two rules: no dependent MFMAs back to back; pair j's activation work between the MFMAs of A(j+1) and C(j-1)) ----
          f32x4 Os[NT], Om[NT], Ob[NT];
          f32x4 Hc[2][2][NT];                      // [buffer][hidden tile of the pair][sample tile]
          float rr[NT][8];                         // r = 1/(2^h+1) of the pair's 8 hidden units per lane
          PlanesH B2[2][NT];                       // [buffer][sample tile]: fp16 hi | fp16 residual
          const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
          static_assert(NT == 2, "slot decoding assumes two sample tiles per wave");
          auto layer1_slot = [&](auto jn_c, auto slot_c) {             // slot 0..23 of pair jn: A(jn)
            constexpr int jn = decltype(jn_c)::value, slot = decltype(slot_c)::value;
            constexpr int pr = slot >> 2, q = (slot >> 1) & 1, i = slot & 1, buf1 = jn & 1;
            Hc[buf1][q][i] = mfma_bf(plane(A1[2 * jn + q], plane_a(pr)), plane(B1[i], plane_b(pr)), pr == 0 ? zero4 : Hc[buf1][q][i]);
          };
          auto layer2_slot = [&](auto jc_c, auto slot_c) {             // slot 0..5 of k-step jc: C(jc)
            constexpr int jc = decltype(jc_c)::value, slot = decltype(slot_c)::value;
            constexpr int pr = slot >> 1, i = slot & 1, buf2 = jc & 1;
            if constexpr (pr == 0) Ob[i] = mfma_h(A2[jc].h, B2[buf2][i].h, jc == 0 ? zero4 : Ob[i]);
            else if constexpr (pr == 1) Om[i] = mfma_h(A2[jc].h, B2[buf2][i].m, jc == 0 ? zero4 : Om[i]);
            else Os[i] = mfma_h(A2[jc].m, B2[buf2][i].h, jc == 0 ? zero4 : Os[i]);
          };
          constexpr int VPU = SM_VPU, NUNIT = 2 * (16 / VPU);
          float minus_one = -1.0f;
          asm volatile("" : "+v"(minus_one));
          auto valu_unit = [&](auto j_c, auto unit_c) {
            constexpr int j = decltype(j_c)::value, unit = decltype(unit_c)::value;
            constexpr int grp = unit >> 1, phase = unit & 1, bufv = j & 1;
            constexpr int v0 = grp * VPU;                              // first of the unit's values: v = 8 i + e
            if constexpr (phase == 0) {
#pragma unroll
              for (int v = v0; v < v0 + VPU; ++v) {
                const int i = v >> 3, e = v & 7;
                rr[i][e] = sigm2(Hc[bufv][e >> 2][i][e & 3]);
              }
            } else {
#pragma unroll
              for (int v = v0; v < v0 + VPU; v += 2) {
                const int i = v >> 3, e0 = v & 7, q = e0 >> 1;
                unsigned hp, mp;
                split_pair_h(rr[i][e0], rr[i][e0 + 1], minus_one, hp, mp);
                B2[bufv][i].h[q] = hp;
                B2[bufv][i].m[q] = mp;
              }
            }
          };
          // A(0): layer 1 of the first pair -- and this timestep's process-noise draw: unit (slot >> 1) of tile (slot & 1)
          // behind every matrix instruction
          float wn[NT][4];
          ProcNoiseDraw draw[NT];
          static_assert(2 * ProcNoiseDraw::UNITS == 24, "one draw unit per layer-1 slot of the first pair");
          static_for<0, 24>([&](auto sc) {
            constexpr int sl = decltype(sc)::value;
            layer1_slot(std::integral_constant<int, 0>{}, sc);
            if (noisy) {
              constexpr int i = sl & 1;
              draw[i].template unit<(sl >> 1)>(pn_seed, pn_call, a.k_offset + kk[i], ((long long)t * MM + m) * NXB + g, seven, wn[i]);
            }
            __builtin_amdgcn_sched_barrier(0);
          });
          static_for<0, HP>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            constexpr bool hasA = j + 1 < HP, hasC = j >= 1;
            constexpr int nA = hasA ? 24 : 0, nC = hasC ? 6 : 0, N = nA + nC;   // MFMA slots of this iteration
            static_for<0, N>([&](auto sc) {
              constexpr int sl = decltype(sc)::value;
              // the nC layer-2 slots spread evenly among the nA layer-1 slots
              constexpr int c_before = (sl * nC) / N, c_after = ((sl + 1) * nC) / N;
              if constexpr (c_after > c_before) layer2_slot(std::integral_constant<int, (j >= 1 ? j - 1 : 0)>{},
                                                            std::integral_constant<int, c_before>{});
              else layer1_slot(std::integral_constant<int, (hasA ? j + 1 : 0)>{}, std::integral_constant<int, sl - c_before>{});
              // B(j)'s VALU units spread evenly over the N slots
              static_for<(sl * NUNIT) / N, ((sl + 1) * NUNIT) / N>([&](auto uc) { valu_unit(jc, uc); });
              __builtin_amdgcn_sched_barrier(0);
            });
          });
          // C(HP-1): the last k-step of layer 2
          static_for<0, 6>([&](auto sc) {
            layer2_slot(std::integral_constant<int, HP - 1>{}, sc);
            __builtin_amdgcn_sched_barrier(0);
          });
          // ---- state update, process noise, this copy's step cost ----
#pragma unroll
          for (int i = 0; i < NT; ++i) {
            const f32x4 O = (Ob[i] + Om[i]) + MID_UNSCALE * Os[i];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              x[i][r] = fmaf(rs, O[r] + b2r[r], x[i][r]);
              if (noisy) x[i][r] = fmaf(sd4[r], wn[i][r], x[i][r]);
              cstep[i] = fmaf(qx4[r] * x[i][r], x[i][r], cstep[i]);
            }
            float c = cstep[i];
            c += __shfl_xor(c, 16, WAVE);
            c += __shfl_xor(c, 32, WAVE);
            cs[i] += c;
            if (g == 0) multi_cost_slot(xch, buf, t - t_done, wv, 16 * i + s) = c;
          }
        }
        // ---- a chunk of step costs is complete: the discounted variance across the copies, one sample per lane ----
        if (t - t_done == CH - 1 || t == a.Tn - 1) {
          __syncthreads();
          if (lead && lane < MULTI_SAMPLES) multi_variance_chunk(xch, buf, t - t_done + 1, slot0, M, lane, a.var_disc, cvar, dpow);
          t_done = t + 1;
          buf ^= 1;
        }
      }

      // ---- the copies' totals meet: the group's first wave adds them in copy order ----
      float p[NT], sm[NT];
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        p[i] = ppart[i]; sm[i] = spart[i];
        p[i] += __shfl_xor(p[i], 16, WAVE); p[i] += __shfl_xor(p[i], 32, WAVE);
        sm[i] += __shfl_xor(sm[i], 16, WAVE); sm[i] += __shfl_xor(sm[i], 32, WAVE);
        if (mine && g == 0) multi_total_slot(xch, wv, 16 * i + s) = cs[i];
      }
      __syncthreads();
      if (lead) {
        float total = inf_v<float>();
        if (lane < MULTI_SAMPLES) {                       // lane (g, s), g < 2 = sample tile g, column s
          float tot = 0.f;
#pragma unroll
          for (int mm = 0; mm < MM; ++mm)
            if (mm < M) tot += multi_total_slot(xch, slot0 + mm, lane);
          const float pert = g == 0 ? p[0] : p[1];
          const float rollout = tot * inv_M + a.var_cost * cvar + (g == 0 ? sm[0] : sm[1]);
          const bool on = g == 0 ? act[0] : act[1];
          const int k = g == 0 ? kk[0] : kk[1];
          if (on) {
            total = rollout + pert;
            a.cost[k] = total;
            if (a.pert != nullptr) a.pert[k] = pert;
          }
        }
        total = wave_min(total);
        if (lane == 0) red[half] = total;
      }
      // (the next pass writes the exchange only behind this barrier, and its totals only behind a later one)
    }
    __syncthreads();
    if (threadIdx.x == 0 && chunk < a.nb1) a.block_min[chunk] = fminf(red[0], red[1]);   // one minimum per 64 samples
  }
  if (a.tstamp != nullptr) {
    __syncthreads();
    stamp_exit(a.tstamp);
  }
}

template <int HT, int NX, int NU>
static int launch_sm(const KArgs<float>& a_in, hipStream_t st) {
  KArgs<float> a = a_in;
  const bool diag = a.diag != 0 || a.coloured != 0;
  const size_t smem = (size_t)(3 * a.J + 2 * NU * NU + MULTI_XCHG_FLOATS + 2) * sizeof(float);
  if (smem > SM_LDS_MAX) return MPPI_E_UNSUPPORTED;
  if (!(a.noise_src == MPPI_NOISE_PHILOX || a.noise_src == MPPI_NOISE_ACTIONS || a.noise_src == MPPI_NOISE_TNK4)) return MPPI_E_UNSUPPORTED;
  // nu != 4: the rows are read component-wise -- external rows in the diagonal (or coloured) form only
  if (NU != 4 && (a.noise_src == MPPI_NOISE_PHILOX || !(diag || a.noise_src == MPPI_NOISE_ACTIONS))) return MPPI_E_UNSUPPORTED;
  const int nchunks = (a.K + SM_CHUNK - 1) / SM_CHUNK;
  static const int n_cu = [] {
    int dev = 0, n = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    return n > 0 ? n : 256;
  }();
  const dim3 grid(nchunks < n_cu ? nchunks : n_cu), block(SM_THREADS);      // one workgroup per CU, persistent over its chunks
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  profile_next_events(&ev0, &ev1, &a.tstamp);
#define MPPI_LAUNCH1(KERNEL)                                                                         \
  do {                                                                                               \
    if (ev1 != nullptr) hipExtLaunchKernelGGL(KERNEL, grid, block, smem, st, ev0, ev1, 0, a);        \
    else hipLaunchKernelGGL(KERNEL, grid, block, smem, st, a);                                       \
  } while (0)
  if constexpr (NU == 4) {
#define MPPI_LAUNCH(NOISE_)                                                                          \
  do {                                                                                               \
    if (diag) MPPI_LAUNCH1((rollout_mlp_split_multi_kernel<HT, NOISE_, true, NX, NU>));             \
    else MPPI_LAUNCH1((rollout_mlp_split_multi_kernel<HT, NOISE_, false, NX, NU>));                 \
  } while (0)
    if (a.noise_src == MPPI_NOISE_PHILOX) MPPI_LAUNCH(MPPI_NOISE_PHILOX);
    else if (a.noise_src == MPPI_NOISE_ACTIONS) MPPI_LAUNCH(MPPI_NOISE_ACTIONS);
    else MPPI_LAUNCH(MPPI_NOISE_TNK4);
#undef MPPI_LAUNCH
  } else {
    if (a.noise_src == MPPI_NOISE_ACTIONS) MPPI_LAUNCH1((rollout_mlp_split_multi_kernel<HT, MPPI_NOISE_ACTIONS, true, NX, NU>));
    else MPPI_LAUNCH1((rollout_mlp_split_multi_kernel<HT, MPPI_NOISE_TNK4, true, NX, NU>));
  }
#undef MPPI_LAUNCH1
  return (int)hipGetLastError();
}

// The (nx, nu) pairs of the M = 1 kernel (rollout_mlp_split.hip), two translation units (MPPI_SPLIT_MULTI_GROUP, set by
// _build.py): 0 = (16, 4) with every noise form, 1 = the further shapes (external rows only, see launch_sm)
#ifndef MPPI_SPLIT_MULTI_GROUP
#define MPPI_SPLIT_MULTI_GROUP 0
#endif
#define MPPI_SPLIT_MULTI_DIMS_0(X) X(16, 4)
#define MPPI_SPLIT_MULTI_DIMS_1(X) X(8, 2) X(12, 6) X(16, 8)

template <int NX, int NU>
static int launch_sm_h(const KArgs<float>& a, hipStream_t st) {
  if (a.hidden == 64) return launch_sm<4, NX, NU>(a, st);
  if (a.hidden == 128) return launch_sm<8, NX, NU>(a, st);
  return launch_sm<16, NX, NU>(a, st);
}

#if MPPI_SPLIT_MULTI_GROUP == 0
int rollout_mlp_split_multi_g1(const KArgs<float>& a, hipStream_t st);

bool mlp_split_multi_supported(int nx, int nu, int hidden) {
  if (!(hidden == 64 || hidden == 128 || hidden == 256)) return false;
#define X(NX, NU) if (nx == NX && nu == NU) return true;
  MPPI_SPLIT_MULTI_DIMS_0(X) MPPI_SPLIT_MULTI_DIMS_1(X)
#undef X
  return false;
}

static std::atomic<long long> g_split_multi_launches{0};

int rollout_mlp_split_multi(const KArgs<float>& a, hipStream_t st) {
  if (a.mp == nullptr) return MPPI_E_BADARG;
  if (!mlp_split_multi_supported(a.nx, a.nu, a.hidden) || a.M < 2 || a.M > PROCESS_NOISE_MM || a.states != nullptr ||
      a.n_env > 1 || a.W != nullptr || a.Tn < 1)
    return MPPI_E_UNSUPPORTED;
  int r = MPPI_E_UNSUPPORTED;
#define X(NX, NU) if (a.nx == NX && a.nu == NU) r = launch_sm_h<NX, NU>(a, st); else
  MPPI_SPLIT_MULTI_DIMS_0(X)
#undef X
  r = rollout_mlp_split_multi_g1(a, st);
  if (r == 0) ++g_split_multi_launches;
  return r;
}
}  // namespace mppi

extern "C" int64_t mppi_stat_mlp_split_multi_launches(void) { return (int64_t)mppi::g_split_multi_launches.load(); }
#else
int rollout_mlp_split_multi_g1(const KArgs<float>& a, hipStream_t st) {
#define X(NX, NU) if (a.nx == NX && a.nu == NU) return launch_sm_h<NX, NU>(a, st);
  MPPI_SPLIT_MULTI_DIMS_1(X)
#undef X
  return MPPI_E_UNSUPPORTED;
}
}  // namespace mppi
#endif
