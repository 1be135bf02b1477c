// K1 for the 2-layer MLP residual model with 16 < nx <= 32 states (nu <= 8) on the 16-bit matrix cores with fp32-level
// accuracy: the split-operand arithmetic of rollout_mlp_split.hip (mlp_split_ops.hpp), widened to TWO 16-state output
// tiles of layer 2 and TWO 32-slot k-steps of layer 1.
//
//   x' = x + s * (W2 tanh(W1 [x;u] + b1) + b2),   cost = sum qx x^2 + sum qu u^2
//
// Transposed chain, samples on the MFMA column axis, no lane permutes or LDS round trips between layers or timesteps.
// Lane l = (g = l >> 4, s = l & 15).
//   layer 2   O_o^T (16 states x 16 samples) = sum_j A2[o][j] (16 x 32) . B2[j] (32 x 16),  o = 0, 1,  j = 0..H/32-1
//       output tile o holds state rows 16 o + 4g + r (r = 0..3) at lane (g, s); k-slot (g, e) of step j = hidden unit
//       16 (2j + (e >> 2)) + 4g + (e & 3) = the lane's accumulator registers of hidden tiles 2j and 2j + 1
//   layer 1   H^T (16 hidden x 16 samples) = sum_o A1[m][o] (16 x 32) . B1[o] (32 x 16)          per hidden tile m
//       k-step o, slot (g, e):  e < 4 -> state x[16 o + 4g + e] = what output tile o left in this very lane
//       k-step 0 only: e = 4 -> control u[g], (nu > 4:) e = 5 -> control u[g + 4], the next e at g = 0 -> constant 1 (b1)
//   Rows and slots beyond the model's nx / nu are zero in the weights and in the inputs.
//
// Where the weights live.  Per timestep the wave issues 60 MFMAs per pair of hidden tiles (6 products x 2 k-steps x 2 hidden
// tiles x 2 sample tiles of layer 1, 3 products x 2 output tiles x 2 sample tiles of layer 2): 480 at H = 256, 7680 cycles
// of its SIMD's matrix pipe.  The layer-1 fragments alone would be 16 x 2 x 3 x 4 = 384 registers, so
//   * the layer-1 planes stay in LDS for the whole launch, [hidden tile][k-step][plane][lane] as 16-byte elements (one
//     conflict-free ds_read_b128 per fragment plane, 96 KB at H = 256), each read once per timestep and used for both
//     sample tiles of the wave: 96 reads x 1 KB x 4 waves = ~3100 LDS cycles per CU and timestep, under the MFMAs.  A
//     plane is read one product (8 MFMA slots) ahead of its first use, inside the slot pipeline;
//   * the layer-2 planes (H/32 x 2 tiles x 2 planes x 4 = 128 registers at H = 256) are pinned in the AGPRs, and so are the
//     48 registers of the timestep's layer-1 B operand: an MFMA reads either operand from an AGPR directly.
// One workgroup of 4 waves per CU, persistent over 128-sample chunks, two sample tiles per wave -- as the 16-state kernel.
#include <hip/hip_ext.h>
#include <atomic>
#include "actions.hpp"
#include "dispatch.hpp"
#include "mlp_split32.hpp"
#include "mlp_split_ops.hpp"

namespace mppi {
using namespace split_ops;

namespace {
constexpr int S32_NT = 2;                                        // sample tiles (of 16) per wave
constexpr int S32_VPU = 2;                                       // hidden activations per VALU unit of the software pipeline
constexpr int S32_THREADS = 256;                                 // 4 waves = one per SIMD
constexpr int S32_SAMPLES = (S32_THREADS / WAVE) * S32_NT * 16;  // samples per workgroup chunk (128)
constexpr size_t S32_LDS_MAX = 160 * 1024;

// floats of the action tables in front of the layer-1 planes (Ue | Um | G), padded to 16 bytes
__host__ __device__ inline int s32_table_floats(int J) { return (3 * J + 3) & ~3; }
}  // namespace

template <int HT /* hidden / 16 */, int NOISE, int NX, int NU>
__global__ void __launch_bounds__(S32_THREADS, 1) rollout_mlp_split32_kernel(const KArgs<float> a_in) {
  static_assert(HT % 2 == 0, "layer 2 consumes hidden tiles in pairs");
  static_assert(NX > 16 && NX <= 32 && NU >= 1 && NU <= 8, "two 16-state output tiles, controls and bias in k-step 0");
  static_assert(NOISE == MPPI_NOISE_TNK4 || NOISE == MPPI_NOISE_ACTIONS, "rows from memory, read component-wise");
  constexpr int NC = NU > 4 ? 2 : 1, BIAS_E = 4 + NC, NI = NX + NU;
  constexpr int NT = S32_NT, H = HT * 16, HP = HT / 2;
  const KArgs<float> a = env_view(a_in);
  stamp_entry(a.tstamp);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* Ue = reinterpret_cast<float*>(smem_raw);   // [J]
  float* Um = Ue + a.J;                             // [J]
  float* G = Um + a.J;                              // [J]
  u32x4* A1s = reinterpret_cast<u32x4*>(Ue + s32_table_floats(a.J));   // [HT][2][3][64]

  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  const int g = lane >> 4, s = lane & 15;

  // ---- parameters: blob = W1 (H,nx+nu) | b1 (H) | W2 (nx,H) | b2 (nx) | res_scale | qx (nx) | qu (nu) ----
  const float* __restrict__ W1 = a.mp;
  const float* __restrict__ b1 = W1 + H * NI;
  const float* __restrict__ W2 = b1 + H;
  const float* __restrict__ b2 = W2 + NX * H;
  const float rs = b2[NX];
  float qx4[2][4];
#pragma unroll
  for (int o = 0; o < 2; ++o) {
#pragma unroll
    for (int r = 0; r < 4; ++r) qx4[o][r] = 16 * o + 4 * g + r < NX ? b2[NX + 1 + 16 * o + 4 * g + r] : 0.f;
  }
  bool own[NC];
  float qu_c[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    own[c] = g + 4 * c < NU;
    qu_c[c] = own[c] ? b2[NX + 1 + NX + g + 4 * c] : 0.f;
  }

  // ---- layer-1 planes into LDS: fragment f = 2 m + o of hidden tile m, k-step o; the four waves share the work ----
  for (int f = wv; f < 2 * HT; f += S32_THREADS / WAVE) {
    const int m = f >> 1, o = f & 1;
    const float* __restrict__ row = W1 + (16 * m + s) * NI;        // hidden unit 16m + s
    float v[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = 16 * o + 4 * g + e < NX ? EXP2_SCALE * row[16 * o + 4 * g + e] : 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) v[4 + c] = (o == 0 && own[c]) ? EXP2_SCALE * row[NX + g + 4 * c] : 0.f;
    v[BIAS_E] = (o == 0 && g == 0) ? EXP2_SCALE * b1[16 * m + s] : 0.f;   // bias column (B1 holds 1 there)
#pragma unroll
    for (int e = BIAS_E + 1; e < 8; ++e) v[e] = 0.f;
    const Planes p = split_pack8(v);
    A1s[(f * 3 + 0) * WAVE + lane] = p.h;
    A1s[(f * 3 + 1) * WAVE + lane] = p.m;
    A1s[(f * 3 + 2) * WAVE + lane] = p.l;
  }

  // ---- layer-2 planes: resident in the accumulation registers ----
  PlanesH A2[2][HP];
  float b2r[2][4];
#pragma unroll
  for (int o = 0; o < 2; ++o) {
    float rowsum = 0.f;                                            // of row 16 o + s of W2, this lane's quarter
#pragma unroll
    for (int j = 0; j < HP; ++j) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float w = 16 * o + s < NX ? W2[(16 * o + s) * H + 16 * (2 * j + (e >> 2)) + 4 * g + (e & 3)] : 0.f;
        rowsum += w;
        v[e] = -2.0f * w;
      }
      A2[o][j] = split_pack8_h(v);
    }
    rowsum += __shfl_xor(rowsum, 16, WAVE);
    rowsum += __shfl_xor(rowsum, 32, WAVE);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      b2r[o][r] = (16 * o + 4 * g + r < NX ? b2[16 * o + 4 * g + r] : 0.f) + __shfl(rowsum, 4 * g + r, WAVE);   // D rows are 4g+r
  }
#pragma unroll
  for (int o = 0; o < 2; ++o) {
#pragma unroll
    for (int j = 0; j < HP; ++j) {
      asm volatile("" : "+a"(A2[o][j].h));
      asm volatile("" : "+a"(A2[o][j].m));
    }
  }

  ActionConsts<float, NU> ac;
  ac.load(a, nullptr);
  // Ue = the sequence the noise is added to and measured from (SMPPI: the host's base A + U dt); the action cost table G is
  // built from the lifted nominal U itself (u_eff) either way
  const bool smppi = a.B != nullptr;
  for (int j = threadIdx.x; j < a.J; j += S32_THREADS) Ue[j] = u_base(a, j);
  __syncthreads();                                   // (the layer-1 planes are complete behind this barrier, too)
  for (int j = threadIdx.x; j < a.J; j += S32_THREADS) {
    const int n = j % NU, t0 = j - n;
    const float uj = Ue[j];
    Um[j] = a.coloured ? uj : uj + a.mu[n];
    float gg;
    if (a.coloured && !a.diag) {            // generator-coloured full Sigma: whole-row G from global
      gg = 0.f;
      for (int m = 0; m < NU; ++m) gg = fmaf(a.sinv[n * NU + m], smppi ? u_eff(a, t0 + m) : Ue[t0 + m], gg);
    } else {
      gg = (smppi ? u_eff(a, j) : uj) * a.sinv[n * NU + n];
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

  // ---- persistent over 128-sample chunks: the weights are laid out once per workgroup ----
  const int nchunks = (a.K + S32_SAMPLES - 1) / S32_SAMPLES;
  for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int kbase = chunk * S32_SAMPLES + wv * (NT * 16);
    int kk[NT], orow[NT];
    bool act[NT];
    float x[NT][2][4], cpart[NT], ppart[NT], vprev[NT][NC];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int kraw = kbase + 16 * i + s;
      act[i] = kraw < a.K;
      kk[i] = act[i] ? kraw : a.K - 1;
      orow[i] = overwrite_row(a, a.k_offset + kk[i]);
      const float* __restrict__ s0 = a.state_per_sample ? a.state + (long long)kk[i] * NX : a.state;
#pragma unroll
      for (int o = 0; o < 2; ++o) {
#pragma unroll
        for (int r = 0; r < 4; ++r) x[i][o][r] = 16 * o + 4 * g + r < NX ? s0[16 * o + 4 * g + r] : 0.f;
      }
      cpart[i] = 0.f;
      ppart[i] = 0.f;
#pragma unroll
      for (int c = 0; c < NC; ++c) vprev[i][c] = 0.f;
    }

    // the lane's component(s) n = g (, g + 4) of timestep t are element t nu + n of the sample's flat (T nu) sequence =
    // component (t nu + n) & 3 of row (t nu + n) >> 2
    float zc[NT][NC], zn[NT][NC];
    auto fetch = [&](int t, float (&dst)[NT][NC]) {
#pragma unroll
      for (int i = 0; i < NT; ++i) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int j = t * NU + (own[c] ? g + 4 * c : 0);
          dst[i][c] = a.z[((long long)(j >> 2) * a.zp + kk[i]) * 4 + (j & 3)];
        }
      }
    };
    fetch(0, zn);

    for (int t = 0; t < a.Tn; ++t) {
      // this lane's element of every layer-1 plane; opaque per timestep, so that the 96 reads of a timestep stay where the
      // slot pipeline below puts them (they are loop-invariant: hoisted, they would be 384 registers)
      int a1_lane = lane;
      asm volatile("" : "+v"(a1_lane));
      auto lds_plane = [&](int m, int o, int which) -> u32x4 { return A1s[((2 * m + o) * 3 + which) * WAVE + a1_lane]; };
      u32x4 Ah[2][2], Am[2][2], Al[2][2];        // [hidden tile of the pair][k-step]: the planes of the pair in flight
#pragma unroll
      for (int q = 0; q < 2; ++q) {
#pragma unroll
        for (int o = 0; o < 2; ++o) Al[q][o] = lds_plane(q, o, 2);      // l of pair 0: needed first (product l.h)
      }

#pragma unroll
      for (int i = 0; i < NT; ++i) {
#pragma unroll
        for (int c = 0; c < NC; ++c) zc[i][c] = zn[i][c];
      }
      fetch(t + 1 < a.Tn ? t + 1 : t, zn);   // prefetch the next step's rows (compute >> latency here)

      // ---- actions (as in the 16-state kernel): lane (g,s) owns control dimension g (and g + 4 where nu > 4) ----
      float Ut[NC], Umt[NC], Gt[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int jn = t * NU + (own[c] ? g + 4 * c : 0);
        Ut[c] = Ue[jn]; Umt[c] = Um[jn]; Gt[c] = own[c] ? G[jn] : 0.f;
      }
      Planes B1[NT][2];
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        float uu[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          float v;
          if constexpr (NOISE == MPPI_NOISE_ACTIONS) v = zc[i][c];
          else v = fmaf(zc[i][c], sd_c[c], Umt[c]);
          if (orow[i] == -1) v = 0.f;
          else if (orow[i] >= 0) v = a.sampler[((long long)orow[i] * a.Tn + t) * NU + (own[c] ? g + 4 * c : 0)];
          v = clampT(v, lo_c[c], hi_c[c]);
          if (NU != 4 && NU != 8) v = own[c] ? v : 0.f;                           // a lane group without a control of its own
          const float e = (v - Ut[c]) * ac.e_scale;                               // e_scale = 1 | 1/dt (SMPPI)
          ppart[i] = fmaf(Gt[c], ac.abs_cost ? fabsf(e) : e, ppart[i]);
          if (a.smooth_w != 0.f) {
            // SMPPI smoothness cost w |v[t] - v[t-1]|^2, this lane's control dimension(s); the dimensions of a sample meet in
            // the reduction over g at the end of the chunk
            const float d = v - vprev[i][c];
            if (t > 0) cpart[i] = fmaf(a.smooth_w * d, d, cpart[i]);
            vprev[i][c] = v;
          }
          uu[c] = a.u_scale * v;
          cpart[i] = fmaf(qu_c[c] * uu[c], uu[c], cpart[i]);                      // control effort (qu = 0: + 0)
        }
        float in0[8] = {x[i][0][0], x[i][0][1], x[i][0][2], x[i][0][3], uu[0], 0.f, 0.f, 0.f};
        if constexpr (NC == 2) in0[5] = uu[1];
        in0[BIAS_E] = g == 0 ? 1.0f : 0.0f;
        const float in1[8] = {x[i][1][0], x[i][1][1], x[i][1][2], x[i][1][3], 0.f, 0.f, 0.f, 0.f};
        B1[i][0] = split_pack8(in0);
        B1[i][1] = split_pack8(in1);
#pragma unroll
        for (int o = 0; o < 2; ++o) {
          asm volatile("" : "+a"(B1[i][o].h));
          asm volatile("" : "+a"(B1[i][o].m));
          asm volatile("" : "+a"(B1[i][o].l));
        }
      }

      // ---- the two layers as one software pipeline (the scheme of the 16-state kernel, twice the MFMA slots) ----
      // A dependent MFMA (same accumulator) cannot issue until its predecessor has drained: layer 1 round-robins the
      // 2 hidden tiles x 2 sample tiles of a pair inside each (product, k-step), so an accumulator comes up every 4th slot;
      // layer 2 keeps three accumulators per (output tile, sample tile), one per magnitude class of the products (small:
      // Wm.rh, 2^11-scaled | middle: Wh.rm | big: Wh.rh), each touched once per k-step and summed once per timestep.
      // Pair j's activation work B(j) runs between the MFMAs of layer 1 of pair j+1, A(j+1), and of layer 2 of pair j-1,
      // C(j-1); Hc and B2 are double-buffered.  The layer-1 planes of a pair come from LDS at the product boundaries:
      // h at slot 0 (first used by product 1), m at slot 8 (product 2), l of the NEXT pair at slot 24 (its product 0).
      // sched_barrier(0) after every slot keeps hipcc's scheduler from re-clustering the slots.
      f32x4 Os[2][NT], Om[2][NT], Ob[2][NT];   // [output tile][sample tile]
      f32x4 Hc[2][2][NT];                      // [buffer][hidden tile of the pair][sample tile]
      float rr[NT][8];                         // r = 1/(2^h+1) of the pair's 8 hidden units per lane
      PlanesH B2[2][NT];                       // [buffer][sample tile]: fp16 hi | fp16 residual
      const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
      static_assert(NT == 2, "slot decoding assumes two sample tiles per wave");
      auto layer1_slot = [&](auto jn_c, auto slot_c) {             // slot 0..47 of pair jn: A(jn)
        constexpr int jn = decltype(jn_c)::value, slot = decltype(slot_c)::value;
        constexpr int pr = slot >> 3, o = (slot >> 2) & 1, q = (slot >> 1) & 1, i = slot & 1, buf = jn & 1;
        if constexpr (slot == 0 || slot == 8 || (slot == 24 && jn + 1 < HP)) {
#pragma unroll
          for (int q2 = 0; q2 < 2; ++q2) {
#pragma unroll
            for (int o2 = 0; o2 < 2; ++o2) {
              if constexpr (slot == 0) Ah[q2][o2] = lds_plane(2 * jn + q2, o2, 0);
              else if constexpr (slot == 8) Am[q2][o2] = lds_plane(2 * jn + q2, o2, 1);
              else Al[q2][o2] = lds_plane(2 * (jn + 1) + q2, o2, 2);
            }
          }
        }
        constexpr int pa = plane_a(pr);
        const u32x4& wa = pa == 0 ? Ah[q][o] : (pa == 1 ? Am[q][o] : Al[q][o]);
        Hc[buf][q][i] = mfma_bf(wa, plane(B1[i][o], plane_b(pr)), (pr == 0 && o == 0) ? zero4 : Hc[buf][q][i]);
      };
      auto layer2_slot = [&](auto jc_c, auto slot_c) {             // slot 0..11 of k-step jc: C(jc)
        constexpr int jc = decltype(jc_c)::value, slot = decltype(slot_c)::value;
        constexpr int pr = slot >> 2, o = (slot >> 1) & 1, i = slot & 1, buf = jc & 1;
        if constexpr (pr == 0) Ob[o][i] = mfma_h(A2[o][jc].h, B2[buf][i].h, jc == 0 ? zero4 : Ob[o][i]);
        else if constexpr (pr == 1) Om[o][i] = mfma_h(A2[o][jc].h, B2[buf][i].m, jc == 0 ? zero4 : Om[o][i]);
        else Os[o][i] = mfma_h(A2[o][jc].m, B2[buf][i].h, jc == 0 ? zero4 : Os[o][i]);
      };
      // B(j) = activation work of the pair's 16 hidden values per lane, in units of VPU values x 2 phases
      // (phase 0: r = 1/(2^h + 1); phase 1: fp16 split + pack)
      constexpr int VPU = S32_VPU, NUNIT = 2 * (16 / VPU);
      float minus_one = -1.0f;
      asm volatile("" : "+v"(minus_one));
      auto valu_unit = [&](auto j_c, auto unit_c) {
        constexpr int j = decltype(j_c)::value, unit = decltype(unit_c)::value;
        constexpr int grp = unit >> 1, phase = unit & 1, buf = j & 1;
        constexpr int v0 = grp * VPU;                              // first of the unit's values: v = 8 i + e
        if constexpr (phase == 0) {
#pragma unroll
          for (int v = v0; v < v0 + VPU; ++v) {
            const int i = v >> 3, e = v & 7;
            rr[i][e] = sigm2(Hc[buf][e >> 2][i][e & 3]);
          }
        } else {
#pragma unroll
          for (int v = v0; v < v0 + VPU; v += 2) {
            const int i = v >> 3, e0 = v & 7, q = e0 >> 1;
            unsigned hp, mp;
            split_pair_h(rr[i][e0], rr[i][e0 + 1], minus_one, hp, mp);
            B2[buf][i].h[q] = hp;
            B2[buf][i].m[q] = mp;
          }
        }
      };
      // A(0): layer 1 of the first pair, nothing to overlap it with
      static_for<0, 48>([&](auto sc) {
        layer1_slot(std::integral_constant<int, 0>{}, sc);
        __builtin_amdgcn_sched_barrier(0);
      });
      static_for<0, HP>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        constexpr bool hasA = j + 1 < HP, hasC = j >= 1;
        constexpr int nA = hasA ? 48 : 0, nC = hasC ? 12 : 0, N = nA + nC;   // MFMA slots of this iteration
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
      static_for<0, 12>([&](auto sc) {
        layer2_slot(std::integral_constant<int, HP - 1>{}, sc);
        __builtin_amdgcn_sched_barrier(0);
      });
#pragma unroll
      for (int i = 0; i < NT; ++i) {
#pragma unroll
        for (int o = 0; o < 2; ++o) {
          const f32x4 O = (Ob[o][i] + Om[o][i]) + MID_UNSCALE * Os[o][i];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            x[i][o][r] = fmaf(rs, O[r] + b2r[o][r], x[i][o][r]);
            cpart[i] = fmaf(qx4[o][r] * x[i][o][r], x[i][o][r], cpart[i]);
          }
        }
      }
    }

    // ---- per-sample totals: sum the 4 lane groups ----
    float bm = inf_v<float>();
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      float c = cpart[i], p = ppart[i];
      c += __shfl_xor(c, 16, WAVE); c += __shfl_xor(c, 32, WAVE);
      p += __shfl_xor(p, 16, WAVE); p += __shfl_xor(p, 32, WAVE);
      const float total = c + p;
      if (act[i] && g == 0) {
        a.cost[kk[i]] = total;
        if (a.pert != nullptr) a.pert[kk[i]] = p;
      }
      if (act[i]) bm = fminf(bm, total);
    }
    // minima are kept per 64 consecutive samples: this wave's 32 samples are half of slot kbase/64; the two waves sharing
    // a slot combine through LDS
    bm = wave_min(bm);
    __shared__ float red[S32_THREADS / WAVE];
    __syncthreads();
    if (lane == 0) red[wv] = bm;
    __syncthreads();
    if (lane == 0 && (wv & 1) == 0) {
      const int slot = kbase / WAVE;
      if (slot < a.nb1) a.block_min[slot] = fminf(red[wv], red[wv + 1]);
    }
  }
  if (a.tstamp != nullptr) {
    __syncthreads();
    stamp_exit(a.tstamp);
  }
}

template <int HT, int NX, int NU>
static int launch_s32(const KArgs<float>& a_in, hipStream_t st) {
  KArgs<float> a = a_in;
  // the rows are read component-wise: external rows (TNK4 / raw actions) in the diagonal (or coloured) form only
  if (!(a.noise_src == MPPI_NOISE_TNK4 || a.noise_src == MPPI_NOISE_ACTIONS)) return MPPI_E_UNSUPPORTED;
  if (!(a.diag != 0 || a.coloured != 0 || a.noise_src == MPPI_NOISE_ACTIONS)) return MPPI_E_UNSUPPORTED;
  const size_t smem = (size_t)s32_table_floats(a.J) * sizeof(float) + (size_t)HT * 2 * 3 * WAVE * 16;
  if (smem + 64 > S32_LDS_MAX) return MPPI_E_UNSUPPORTED;      // (+ the kernel's static reduction slots) long horizons: per lane
  const int nchunks = (a.K + S32_SAMPLES - 1) / S32_SAMPLES;
  static const int n_cu = [] {
    int dev = 0, n = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    return n > 0 ? n : 256;
  }();
  int gx = nchunks;
  const int cap = n_cu / (a.n_env > 1 ? a.n_env : 1);
  if (gx > (cap > 1 ? cap : 1)) gx = cap > 1 ? cap : 1;       // one workgroup per CU, persistent over its chunks
  const dim3 grid(gx, 1, a.n_env), block(S32_THREADS);
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  profile_next_events(&ev0, &ev1, &a.tstamp);
#define MPPI_LAUNCH1(KERNEL)                                                                                   \
  do {                                                                                                         \
    if (smem > 64 * 1024) (void)hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem); \
    if (ev1 != nullptr) hipExtLaunchKernelGGL(KERNEL, grid, block, smem, st, ev0, ev1, 0, a);                  \
    else hipLaunchKernelGGL(KERNEL, grid, block, smem, st, a);                                                 \
  } while (0)
  if (a.noise_src == MPPI_NOISE_ACTIONS) MPPI_LAUNCH1((rollout_mlp_split32_kernel<HT, MPPI_NOISE_ACTIONS, NX, NU>));
  else MPPI_LAUNCH1((rollout_mlp_split32_kernel<HT, MPPI_NOISE_TNK4, NX, NU>));
#undef MPPI_LAUNCH1
  return (int)hipGetLastError();
}

// the (nx, nu) pairs with an instantiation; (24, 6) exercises every nx / nu guard
#define MPPI_SPLIT32_DIMS(X) X(32, 8) X(24, 6)

bool mlp_split32_supported(int nx, int nu, int hidden) {
  if (!(hidden == 64 || hidden == 128 || hidden == 256)) return false;
#define X(NX, NU) if (nx == NX && nu == NU) return true;
  MPPI_SPLIT32_DIMS(X)
#undef X
  return false;
}

static std::atomic<long long> g_split32_launches{0};

int rollout_mlp_split32(const KArgs<float>& a, hipStream_t st) {
  if (a.mp == nullptr) return MPPI_E_BADARG;
  if (!mlp_split32_supported(a.nx, a.nu, a.hidden) || a.states != nullptr || a.M != 1) return MPPI_E_UNSUPPORTED;
  int r = MPPI_E_UNSUPPORTED;
#define X(NX, NU)                                                         \
  if (a.nx == NX && a.nu == NU)                                           \
    r = a.hidden == 64 ? launch_s32<4, NX, NU>(a, st) : (a.hidden == 128 ? launch_s32<8, NX, NU>(a, st) : launch_s32<16, NX, NU>(a, st));
  MPPI_SPLIT32_DIMS(X)
#undef X
  if (r == 0) ++g_split32_launches;
  return r;
}

}  // namespace mppi

extern "C" int64_t mppi_stat_mlp_split32_launches(void) { return (int64_t)mppi::g_split32_launches.load(); }
