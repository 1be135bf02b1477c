// K1 for the residual MLP with TWO hidden layers (mlp_deep.hpp; nx <= 16, nu <= 8, both hidden layers padded to one width
// H in {32, 64, 128}) on the 16-bit matrix cores with fp32-level accuracy: the split-operand arithmetic of the one-hidden-layer
// kernels (mlp_split_ops.hpp) with a hidden->hidden layer between them.
//
//   x' = x + s * (W3 tanh(W2 tanh(W1 [x;u] + b1) + b2) + b3),   cost = sum qx x^2 + sum qu u^2
//
// Transposed chain, samples on the MFMA column axis, no lane permutes or LDS round trips between layers or timesteps.
// Lane l = (g = l >> 4, s = l & 15); tanh = 1 - 2 r with r = 1 / (2^h + 1), the affine parts folded into the NEXT layer's weights.
//   layer 1   H1^T (16 units x 16 samples) = A1[m] (16 x 32) . B1 (32 x 16)     per hidden tile m, bf16 x 3, six products
//       k-slot (g, e):  e < 4 -> state x[4g + e] = what the output tile left in this very lane;  e = 4 -> control u[g],
//       (nu > 4:) e = 5 -> control u[g + 4], the next e at g = 0 -> constant 1 (b1).  A1 = 2 log2(e) W1.
//   hidden    H2^T (16 units x 16 samples) = sum_j A2[m][j] (16 x 32) . R1[j] (32 x 16)      per hidden tile m, fp16 x 2
//       k-slot (g, e) of step j = layer-1 unit 16 (2j + (e >> 2)) + 4g + (e & 3) = the lane's accumulator registers of layer-1
//       tiles 2j and 2j + 1: layer 1's D layout IS this layer's B layout.  A2 = -2 (2 log2 e) W2 = fp16 hi + 2^-11 fp16 residual;
//       three products Wh.rm, Wh.rh (one accumulator, started from the bias 2 log2 e (b2 + rowsum W2) as the C operand of the
//       tile's first MFMA) and Wm.rh (2^11-scaled, its own accumulator).
//   output    O^T (16 states x 16 samples) = sum_j A3[j] (16 x 32) . R2[j] (32 x 16),  A3 = -2 W3, same three products
//   Rows and slots beyond the model's nx / nu and units beyond its widths are zero in the weights.
//
// Where the weights live (H = 128: 312 MFMAs per wave and timestep, 96 + 192 + 24):
//   * layer 1 (8 tiles x 3 planes x 4 = 96 registers) and the output layer (4 k-steps x 2 planes x 4 = 32) are pinned in AGPRs,
//     and so are the timestep's layer-1 B operand (24) and the r planes of the whole first hidden vector (4 k-steps x 2 planes x
//     4 x 2 sample tiles = 64), which only MFMAs read: an MFMA takes either operand from an AGPR directly;
//   * the hidden layer's planes (8 x 4 x 2 planes x 1 KB = 64 KB) stay in LDS for the whole launch, [tile][k-step][plane][lane]
//     as 16-byte elements: one conflict-free ds_read_b128 per plane, read once per timestep for both sample tiles of the wave.
//     The hi plane (two products) is double-buffered and read one k-step (12 MFMA slots) ahead, the residual plane 8 slots ahead;
//   * the hidden layer's bias: H floats in LDS, one broadcast ds_read_b128 per tile.
// The software pipeline has three stages (the hidden layer needs ALL of layer 1's activations before any of its tiles completes):
//   stage 1  layer 1 pair by pair (24 slots); pair p - 1's activation VALU work between pair p's MFMAs
//   stage 2  hidden layer, output-tile pair by pair (12 H/32 slots); between pair p's MFMAs run the activations of pair p - 1
//            (for p = 0: of layer 1's last pair, ahead of the k-step that consumes them) and the 6 slots of the output layer's
//            k-step p - 2
//   tail     the last pair's activations around the output layer's last two k-steps
// One persistent workgroup of 4 waves per CU over 128-sample chunks, two sample tiles per wave -- as the one-hidden-layer kernels.
// TWIN: rollout_mlp_deep_multi.hip (M = 2..4, one wave per rollout copy) restates dp_interleave, the plane packing, the slot
// lambdas and act_unit of this file: a fix to the pipeline here is a fix there, too (to be shared through a header).
#include <hip/hip_ext.h>
#include <atomic>
#include "actions.hpp"
#include "dispatch.hpp"
#include "mlp_deep.hpp"
#include "mlp_split_ops.hpp"

namespace mppi {
using namespace split_ops;

namespace {
constexpr int DP_NT = 2;                                         // sample tiles (of 16) per wave
constexpr int DP_VPU = 2;                                        // hidden activations per VALU unit of the software pipeline
constexpr int DP_THREADS = 256;                                  // 4 waves = one per SIMD
constexpr int DP_SAMPLES = (DP_THREADS / WAVE) * DP_NT * 16;     // samples per workgroup chunk (128)
constexpr size_t DP_LDS_MAX = 160 * 1024;

// floats of the action tables in front of the hidden layer's bias and planes (Ue | Um | G), padded to 16 bytes
__host__ __device__ inline int dp_table_floats(int J) { return (3 * J + 3) & ~3; }

// NS MFMA slots, each followed by its share of NUN VALU units spread evenly over the first SPAN slots (SPAN = 0: all of them in
// front).  sched_barrier(0) after every slot keeps hipcc's scheduler from re-clustering the slots.
template <int NS, int SPAN, int NUN, class FS, class FU>
__device__ __forceinline__ void dp_interleave(FS&& slot, FU&& unit) {
  if constexpr (SPAN == 0 && NUN > 0) {
    static_for<0, NUN>(unit);
    __builtin_amdgcn_sched_barrier(0);
  }
  static_for<0, NS>([&](auto sc) {
    constexpr int sl = decltype(sc)::value;
    slot(sc);
    if constexpr (sl < SPAN) static_for<(sl * NUN) / SPAN, ((sl + 1) * NUN) / SPAN>(unit);
    __builtin_amdgcn_sched_barrier(0);
  });
}
template <int V> using ic = std::integral_constant<int, V>;
}  // namespace

template <int HT /* hidden / 16 */, int NOISE, int NX, int NU>
__global__ void __launch_bounds__(DP_THREADS, 1) rollout_mlp_deep_kernel(const KArgs<float> a_in) {
  static_assert(HT % 2 == 0, "a k-step of the 16-bit layers consumes hidden tiles in pairs");
  static_assert(NX >= 1 && NX <= 16 && NU >= 1 && NU <= 8, "one 16-state output tile, controls and bias in the layer-1 k-step");
  static_assert(NOISE == MPPI_NOISE_TNK4 || NOISE == MPPI_NOISE_ACTIONS, "rows from memory, read component-wise");
  constexpr int NC = NU > 4 ? 2 : 1, BIAS_E = 4 + NC, NI = NX + NU;
  constexpr int NT = DP_NT, H = HT * 16, HP = HT / 2;
  const KArgs<float> a = env_view(a_in);
  stamp_entry(a.tstamp);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* Ue = reinterpret_cast<float*>(smem_raw);   // [J]
  float* Um = Ue + a.J;                             // [J]
  float* G = Um + a.J;                              // [J]
  float* bias2 = Ue + dp_table_floats(a.J);         // [H]
  u32x4* A2s = reinterpret_cast<u32x4*>(bias2 + H); // [HT][HP][2][64]

  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  const int g = lane >> 4, s = lane & 15;

  // ---- parameters (mlp_deep.hpp): W1 (H,nx+nu) | b1 (H) | W2T (H,H) | b2 (H) | W3T (H,nx) | b3 (nx) | res_scale | qx | qu ----
  const float* __restrict__ W1 = a.mp;
  const float* __restrict__ b1 = W1 + H * NI;
  const float* __restrict__ W2T = b1 + H;
  const float* __restrict__ b2 = W2T + H * H;
  const float* __restrict__ W3T = b2 + H;
  const float* __restrict__ b3 = W3T + NX * H;
  const float rs = b3[NX];
  float qx4[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) qx4[r] = 4 * g + r < NX ? b3[NX + 1 + 4 * g + r] : 0.f;
  bool own[NC];
  float qu_c[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    own[c] = g + 4 * c < NU;
    qu_c[c] = own[c] ? b3[NX + 1 + NX + g + 4 * c] : 0.f;
  }

  // ---- hidden-layer planes into LDS: fragment f = m HP + j of output tile m, k-step j; the four waves share the work ----
  for (int f = wv; f < HT * HP; f += DP_THREADS / WAVE) {
    const int m = f / HP, j = f % HP;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (-2.0f * EXP2_SCALE) * W2T[(16 * (2 * j + (e >> 2)) + 4 * g + (e & 3)) * H + 16 * m + s];
    const PlanesH p = split_pack8_h(v);
    A2s[(f * 2 + 0) * WAVE + lane] = p.h;
    A2s[(f * 2 + 1) * WAVE + lane] = p.m;
  }
  // ... and its bias 2 log2(e) (b2 + rowsum W2): the "1" of tanh = 1 - 2 r.  One unit per thread, summed in fp64
  for (int u = threadIdx.x; u < H; u += DP_THREADS) {
    double sum = (double)b2[u];
    for (int k = 0; k < H; ++k) sum += (double)W2T[k * H + u];
    bias2[u] = (float)((double)EXP2_SCALE * sum);
  }

  // ---- layer-1 and output-layer planes: resident in the accumulation registers ----
  Planes A1[HT];
#pragma unroll
  for (int m = 0; m < HT; ++m) {
    const float* __restrict__ row = W1 + (16 * m + s) * NI;        // hidden unit 16m + s
    float v[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = 4 * g + e < NX ? EXP2_SCALE * row[4 * g + e] : 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) v[4 + c] = own[c] ? EXP2_SCALE * row[NX + g + 4 * c] : 0.f;
    v[BIAS_E] = g == 0 ? EXP2_SCALE * b1[16 * m + s] : 0.f;         // bias column (B1 holds 1 there)
#pragma unroll
    for (int e = BIAS_E + 1; e < 8; ++e) v[e] = 0.f;
    A1[m] = split_pack8(v);
  }
  PlanesH A3[HP];
  float b3r[4];
  {
    float rowsum = 0.f;                                            // of row s of W3, this lane's quarter
#pragma unroll
    for (int j = 0; j < HP; ++j) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float w = s < NX ? W3T[(16 * (2 * j + (e >> 2)) + 4 * g + (e & 3)) * NX + s] : 0.f;
        rowsum += w;
        v[e] = -2.0f * w;
      }
      A3[j] = split_pack8_h(v);
    }
    rowsum += __shfl_xor(rowsum, 16, WAVE);
    rowsum += __shfl_xor(rowsum, 32, WAVE);
#pragma unroll
    for (int r = 0; r < 4; ++r) b3r[r] = (4 * g + r < NX ? b3[4 * g + r] : 0.f) + __shfl(rowsum, 4 * g + r, WAVE);   // D rows are 4g+r
  }
#pragma unroll
  for (int m = 0; m < HT; ++m) {
    asm volatile("" : "+a"(A1[m].h));
    asm volatile("" : "+a"(A1[m].m));
    asm volatile("" : "+a"(A1[m].l));
  }
#pragma unroll
  for (int j = 0; j < HP; ++j) {
    asm volatile("" : "+a"(A3[j].h));
    asm volatile("" : "+a"(A3[j].m));
  }

  ActionConsts<float, NU> ac;
  ac.load(a, nullptr);
  // Ue = the sequence the noise is added to and measured from (SMPPI: the host's base A + U dt); the action cost table G is
  // built from the lifted nominal U itself (u_eff) either way
  const bool smppi = a.B != nullptr;
  for (int j = threadIdx.x; j < a.J; j += DP_THREADS) Ue[j] = u_base(a, j);
  __syncthreads();                                   // (the hidden layer's planes and bias are complete behind this barrier, too)
  for (int j = threadIdx.x; j < a.J; j += DP_THREADS) {
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
  const int nchunks = (a.K + DP_SAMPLES - 1) / DP_SAMPLES;
  for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int kbase = chunk * DP_SAMPLES + wv * (NT * 16);
    int kk[NT], orow[NT];
    bool act[NT];
    float x[NT][4], cpart[NT], ppart[NT], vprev[NT][NC];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int kraw = kbase + 16 * i + s;
      act[i] = kraw < a.K;
      kk[i] = act[i] ? kraw : a.K - 1;
      orow[i] = overwrite_row(a, a.k_offset + kk[i]);
      const float* __restrict__ s0 = a.state_per_sample ? a.state + (long long)kk[i] * NX : a.state;
#pragma unroll
      for (int r = 0; r < 4; ++r) x[i][r] = 4 * g + r < NX ? s0[4 * g + r] : 0.f;
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
      // this lane's element of every hidden-layer plane; opaque per timestep, so that the reads of a timestep stay where the
      // slot pipeline below puts them (they are loop-invariant: hoisted, they would be 256 registers at H = 128)
      int a2_lane = lane, b2_lane = 4 * g;
      asm volatile("" : "+v"(a2_lane));
      asm volatile("" : "+v"(b2_lane));
      auto lds_plane = [&](int m, int j, int which) -> u32x4 { return A2s[((m * HP + j) * 2 + which) * WAVE + a2_lane]; };
      auto lds_bias = [&](int m) -> f32x4 { return *reinterpret_cast<const f32x4*>(bias2 + 16 * m + b2_lane); };
      // hidden-layer planes in flight.  Step n = p HP + j (pair p of output tiles, k-step j): hi [n & 1][tile of the pair], read at
      // the first slot of step n - 1; residual [tile of the pair], read at the first slot of its own step (used from slot 8)
      u32x4 Wh[2][2], Wm[2];
      f32x4 bias[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        Wh[0][q] = lds_plane(q, 0, 0);
        bias[q] = lds_bias(q);
      }

#pragma unroll
      for (int i = 0; i < NT; ++i) {
#pragma unroll
        for (int c = 0; c < NC; ++c) zc[i][c] = zn[i][c];
      }
      fetch(t + 1 < a.Tn ? t + 1 : t, zn);   // prefetch the next step's rows (compute >> latency here)

      // ---- actions (as in the one-hidden-layer kernels): lane (g,s) owns control dimension g (and g + 4 where nu > 4) ----
      float Ut[NC], Umt[NC], Gt[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int jn = t * NU + (own[c] ? g + 4 * c : 0);
        Ut[c] = Ue[jn]; Umt[c] = Um[jn]; Gt[c] = own[c] ? G[jn] : 0.f;
      }
      Planes B1[NT];
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
        float in0[8] = {x[i][0], x[i][1], x[i][2], x[i][3], uu[0], 0.f, 0.f, 0.f};
        if constexpr (NC == 2) in0[5] = uu[1];
        in0[BIAS_E] = g == 0 ? 1.0f : 0.0f;
        B1[i] = split_pack8(in0);
        asm volatile("" : "+a"(B1[i].h));
        asm volatile("" : "+a"(B1[i].m));
        asm volatile("" : "+a"(B1[i].l));
      }

      // ---- the three layers as one software pipeline ----
      // A dependent MFMA (same accumulator) cannot issue until its predecessor has drained: every layer round-robins the 2 tiles
      // x 2 sample tiles of a pair inside each product, so an accumulator comes up every 4th slot.
      f32x4 Hc[2][2][NT];                      // layer 1 [buffer][hidden tile of the pair][sample tile]
      PlanesH R1[HP][NT];                      // r planes of the whole first hidden vector [k-step][sample tile]
      f32x4 Ab[2][2][NT], As[2][2][NT];        // hidden layer [buffer][tile of the pair][sample tile]: Wh.r | 2^11 Wm.rh
      PlanesH R2[2][NT];                       // r planes of the second hidden vector [buffer][sample tile]
      f32x4 Ob[NT], Os[NT];                    // output layer
      float rr[NT][8];                         // r = 1/(2^h+1) of a pair's 8 hidden units per lane
      const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
      static_assert(NT == 2, "slot decoding assumes two sample tiles per wave");
      auto layer1_slot = [&](auto p_c, auto slot_c) {              // slot 0..23 of pair p
        constexpr int p = decltype(p_c)::value, slot = decltype(slot_c)::value;
        constexpr int pr = slot >> 2, q = (slot >> 1) & 1, i = slot & 1, buf = p & 1;
        Hc[buf][q][i] = mfma_bf(plane(A1[2 * p + q], plane_a(pr)), plane(B1[i], plane_b(pr)), pr == 0 ? zero4 : Hc[buf][q][i]);
      };
      auto hidden_slot = [&](auto p_c, auto slot_c) {              // slot 0..12 HP - 1 of output-tile pair p
        constexpr int p = decltype(p_c)::value, slot = decltype(slot_c)::value;
        constexpr int j = slot / 12, w = slot % 12, pr = w >> 2, q = (w >> 1) & 1, i = w & 1, buf = p & 1, n = p * HP + j;
        if constexpr (w == 0) {
#pragma unroll
          for (int q2 = 0; q2 < 2; ++q2) {
            Wm[q2] = lds_plane(2 * p + q2, j, 1);
            if constexpr (n + 1 < HP * HP) Wh[(n + 1) & 1][q2] = lds_plane(2 * ((n + 1) / HP) + q2, (n + 1) % HP, 0);
          }
        }
        if constexpr (w == 4 && j == HP - 1 && p + 1 < HP) {       // the next pair's bias, behind this pair's last use of it
#pragma unroll
          for (int q2 = 0; q2 < 2; ++q2) bias[q2] = lds_bias(2 * (p + 1) + q2);
        }
        if constexpr (pr == 0) Ab[buf][q][i] = mfma_h(Wh[n & 1][q], R1[j][i].m, j == 0 ? bias[q] : Ab[buf][q][i]);
        else if constexpr (pr == 1) Ab[buf][q][i] = mfma_h(Wh[n & 1][q], R1[j][i].h, Ab[buf][q][i]);
        else As[buf][q][i] = mfma_h(Wm[q], R1[j][i].h, j == 0 ? zero4 : As[buf][q][i]);
      };
      auto output_slot = [&](auto jc_c, auto slot_c) {             // slot 0..5 of k-step jc
        constexpr int jc = decltype(jc_c)::value, slot = decltype(slot_c)::value;
        constexpr int pr = slot >> 1, i = slot & 1, buf = jc & 1;
        if constexpr (pr == 0) Ob[i] = mfma_h(A3[jc].h, R2[buf][i].m, jc == 0 ? zero4 : Ob[i]);
        else if constexpr (pr == 1) Ob[i] = mfma_h(A3[jc].h, R2[buf][i].h, Ob[i]);
        else Os[i] = mfma_h(A3[jc].m, R2[buf][i].h, jc == 0 ? zero4 : Os[i]);
      };
      // activation work of a pair's 16 hidden values per lane, in units of VPU values x 2 phases
      // (phase 0: r = 1/(2^h + 1); phase 1: fp16 split + pack).  LAYER 1: Hc of pair idx -> R1[idx] (then pinned in AGPRs);
      // LAYER 2: Ab + 2^-11 As of pair idx -> R2[idx & 1]
      constexpr int VPU = DP_VPU, NUNIT = 2 * (16 / VPU);
      float minus_one = -1.0f;
      asm volatile("" : "+v"(minus_one));
      auto act_unit = [&](auto layer_c, auto idx_c, auto unit_c) {
        constexpr int layer = decltype(layer_c)::value, idx = decltype(idx_c)::value, unit = decltype(unit_c)::value;
        constexpr int grp = unit >> 1, phase = unit & 1, buf = idx & 1;
        constexpr int v0 = grp * VPU;                              // first of the unit's values: v = 8 i + e
        if constexpr (phase == 0) {
#pragma unroll
          for (int v = v0; v < v0 + VPU; ++v) {
            const int i = v >> 3, e = v & 7;
            if constexpr (layer == 1) rr[i][e] = sigm2(Hc[buf][e >> 2][i][e & 3]);
            else rr[i][e] = sigm2(__builtin_fmaf(As[buf][e >> 2][i][e & 3], MID_UNSCALE, Ab[buf][e >> 2][i][e & 3]));
          }
        } else {
#pragma unroll
          for (int v = v0; v < v0 + VPU; v += 2) {
            const int i = v >> 3, e0 = v & 7, q = e0 >> 1;
            unsigned hp, mp;
            split_pair_h(rr[i][e0], rr[i][e0 + 1], minus_one, hp, mp);
            if constexpr (layer == 1) { R1[idx][i].h[q] = hp; R1[idx][i].m[q] = mp; }
            else { R2[buf][i].h[q] = hp; R2[buf][i].m[q] = mp; }
          }
        }
        if constexpr (layer == 1 && unit == NUNIT - 1) {
#pragma unroll
          for (int i = 0; i < NT; ++i) {
            asm volatile("" : "+a"(R1[idx][i].h));
            asm volatile("" : "+a"(R1[idx][i].m));
          }
        }
      };
      // stage 1: layer 1, the activations of pair p - 1 between the MFMAs of pair p
      static_for<0, HP>([&](auto pc) {
        constexpr int p = decltype(pc)::value, pv = p >= 1 ? p - 1 : 0;
        dp_interleave<24, (p >= 1 ? 24 : 0), (p >= 1 ? NUNIT : 0)>(
            [&](auto sc) { layer1_slot(pc, sc); }, [&](auto uc) { act_unit(ic<1>{}, ic<pv>{}, uc); });
      });
      // stage 2: the hidden layer; the output layer's k-step p - 2 spread evenly among pair p's slots
      static_for<0, HP>([&](auto pc) {
        constexpr int p = decltype(pc)::value;
        constexpr int nH = 12 * HP, nC = p >= 2 ? 6 : 0, N = nH + nC;
        auto slot = [&](auto sc) {
          constexpr int sl = decltype(sc)::value;
          constexpr int c_before = (sl * nC) / N, c_after = ((sl + 1) * nC) / N;
          if constexpr (c_after > c_before) output_slot(ic<(p >= 2 ? p - 2 : 0)>{}, ic<c_before>{});
          else hidden_slot(pc, ic<sl - c_before>{});
        };
        // pair 0 carries the activations of layer 1's last pair: complete before k-step HP - 1 consumes them
        if constexpr (p == 0) dp_interleave<N, 12 * (HP - 1), NUNIT>(slot, [&](auto uc) { act_unit(ic<1>{}, ic<HP - 1>{}, uc); });
        else dp_interleave<N, N, NUNIT>(slot, [&](auto uc) { act_unit(ic<2>{}, ic<(p >= 1 ? p - 1 : 0)>{}, uc); });
      });
      // tail: the activations of the last pair, the output layer's last two k-steps
      dp_interleave<(HP >= 2 ? 6 : 0), (HP >= 2 ? 6 : 0), NUNIT>(
          [&](auto sc) { output_slot(ic<(HP >= 2 ? HP - 2 : 0)>{}, sc); }, [&](auto uc) { act_unit(ic<2>{}, ic<HP - 1>{}, uc); });
      dp_interleave<6, 0, 0>([&](auto sc) { output_slot(ic<HP - 1>{}, sc); }, [&](auto) {});
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        const f32x4 O = Ob[i] + MID_UNSCALE * Os[i];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          x[i][r] = fmaf(rs, O[r] + b3r[r], x[i][r]);
          cpart[i] = fmaf(qx4[r] * x[i][r], x[i][r], cpart[i]);
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
    __shared__ float red[DP_THREADS / WAVE];
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
static int launch_deep(const KArgs<float>& a_in, hipStream_t st) {
  KArgs<float> a = a_in;
  // the rows are read component-wise: external rows (TNK4 / raw actions) in the diagonal (or coloured) form only
  if (!(a.noise_src == MPPI_NOISE_TNK4 || a.noise_src == MPPI_NOISE_ACTIONS)) return MPPI_E_UNSUPPORTED;
  if (!(a.diag != 0 || a.coloured != 0 || a.noise_src == MPPI_NOISE_ACTIONS)) return MPPI_E_UNSUPPORTED;
  const size_t smem = (size_t)(dp_table_floats(a.J) + HT * 16) * sizeof(float) + (size_t)HT * (HT / 2) * 2 * WAVE * 16;
  if (smem + 64 > DP_LDS_MAX) return MPPI_E_UNSUPPORTED;       // (+ the kernel's static reduction slots) long horizons: per lane
  const int nchunks = (a.K + DP_SAMPLES - 1) / DP_SAMPLES;
  static const int n_cu = [] {
    int dev = 0, n = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    return n > 0 ? n : 256;
  }();
  int gx = nchunks;
  const int cap = n_cu / (a.n_env > 1 ? a.n_env : 1);
  if (gx > (cap > 1 ? cap : 1)) gx = cap > 1 ? cap : 1;       // one workgroup per CU, persistent over its chunks
  const dim3 grid(gx, 1, a.n_env), block(DP_THREADS);
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  profile_next_events(&ev0, &ev1, &a.tstamp);
#define MPPI_LAUNCH1(KERNEL)                                                                                   \
  do {                                                                                                         \
    if (smem > 64 * 1024) (void)hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem); \
    if (ev1 != nullptr) hipExtLaunchKernelGGL(KERNEL, grid, block, smem, st, ev0, ev1, 0, a);                  \
    else hipLaunchKernelGGL(KERNEL, grid, block, smem, st, a);                                                 \
  } while (0)
  if (a.noise_src == MPPI_NOISE_ACTIONS) MPPI_LAUNCH1((rollout_mlp_deep_kernel<HT, MPPI_NOISE_ACTIONS, NX, NU>));
  else MPPI_LAUNCH1((rollout_mlp_deep_kernel<HT, MPPI_NOISE_TNK4, NX, NU>));
#undef MPPI_LAUNCH1
  return (int)hipGetLastError();
}

// the (nx, nu) pairs with an instantiation; (12, 6) exercises every nx / nu guard, (2, 1) is the pendulum-sized net
#define MPPI_DEEP_DIMS(X) X(16, 4) X(12, 6) X(2, 1)

bool mlp_deep_supported(int nx, int nu, int hidden) {
  if (!(hidden == 32 || hidden == 64 || hidden == 128)) return false;
#define X(NX, NU) if (nx == NX && nu == NU) return true;
  MPPI_DEEP_DIMS(X)
#undef X
  return false;
}

static std::atomic<long long> g_deep_launches{0};

int rollout_mlp_deep(const KArgs<float>& a, hipStream_t st) {
  if (a.mp == nullptr) return MPPI_E_BADARG;
  if (!mlp_deep_supported(a.nx, a.nu, a.hidden) || a.states != nullptr || a.M != 1) return MPPI_E_UNSUPPORTED;
  int r = MPPI_E_UNSUPPORTED;
#define X(NX, NU)                                                         \
  if (a.nx == NX && a.nu == NU)                                           \
    r = a.hidden == 32 ? launch_deep<2, NX, NU>(a, st) : (a.hidden == 64 ? launch_deep<4, NX, NU>(a, st) : launch_deep<8, NX, NU>(a, st));
  MPPI_DEEP_DIMS(X)
#undef X
  if (r == 0) ++g_deep_launches;
  return r;
}

}  // namespace mppi

extern "C" int64_t mppi_stat_mlp_deep_launches(void) { return (int64_t)mppi::g_deep_launches.load(); }
