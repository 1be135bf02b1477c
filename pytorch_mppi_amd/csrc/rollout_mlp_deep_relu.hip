// K1 for the residual MLP with TWO hidden layers of ReLU units (mlp_deep_relu.hpp; the (nx, nu) of rollout_mlp_deep.hip, both
// hidden layers padded to one width H in {64, 128}) on the 16-bit matrix cores with fp32-level accuracy and NO limit on the
// weights or the activations.
//
//   x' = x + s * (W3 relu(W2 relu(W1 [x;u] + b1) + b2) + b3),   cost = sum qx x^2 + sum qu u^2
//
// relu(h) is unbounded, so ALL THREE layers run on bf16 x 3 (fp32's exponent range in every piece), as the two layers of
// rollout_mlp_relu.hip do:
//   v = hi + mid + lo exactly by truncation (8 + 8 + 8 significant bits), six of the nine piece products on
//   v_mfma_f32_16x16x32_bf16, smallest first:  l.h  h.l  m.m | m.h  h.m | h.h  -- dropping m.l, l.m, l.l <= 2^-23 relative.
//   Nothing is folded into the weights: b1 rides in the constant-1 k-slot of layer 1, b2 is the C operand of a hidden tile's first
//   MFMA, b3 is added in fp32.
//
// Transposed chain, samples on the MFMA column axis, no lane permutes or LDS round trips between layers or timesteps.
// Lane l = (g = l >> 4, s = l & 15); A[i][k] and B[k][j] hold k = 8g + e (e = 0..7) at i = j = s, D[i][j] holds i = 4g + r at j = s.
//   layer 1   H1^T (16 units x 16 samples) = A1[m] (16 x 32) . B1 (32 x 16)     per hidden tile m
//       k-slot (g, e):  e < 4 -> state x[4g+e]   e = 4 -> control u[g]   (nu > 4: e = 5 -> control u[g+4])
//       the next e at g = 0 -> constant 1 (b1 rides in that column of A1)   the rest -> 0
//   hidden    H2^T (16 units x 16 samples) = b2 + sum_j A2[m][j] (16 x 32) . R1[j] (32 x 16)     per hidden tile m
//       k-slot (g, e) of step j = layer-1 unit 16 (2j + (e >> 2)) + 4g + (e & 3) = the lane's accumulator registers of layer-1
//       tiles 2j and 2j + 1: layer 1's D layout IS this layer's B layout.
//   output    O^T (16 states x 16 samples) = sum_j A3[j] (16 x 32) . R2[j] (32 x 16): the hidden layer's D layout is its B layout
//   Rows and slots beyond the model's nx / nu and units beyond its widths are zero in the weights.
//
// Where the operands live (H = 128: 528 MFMAs per wave and timestep, 96 + 384 + 48):
//   * AGPRs, which only MFMAs read (an MFMA takes either operand from there directly): layer 1 (8 tiles x 3 planes x 4 = 96
//     registers), the output layer (4 k-steps x 3 planes x 4 = 48) and the bf16 planes of the whole first hidden vector (4 k-steps x
//     3 planes x 4 x 2 sample tiles = 96) -- 240 of 256;
//   * the timestep's layer-1 B operand (24) stays in VGPRs: it is dead before the hidden layer's buffers come alive;
//   * the hidden layer's planes (8 tiles x 4 k-steps x 3 planes x 1 KB = 96 KB) stay in LDS for the whole launch,
//     [tile][k-step][plane][lane] as 16-byte elements: one conflict-free ds_read_b128 per plane, read once per timestep for both
//     sample tiles of the wave.  Each plane is read as soon as the registers of its predecessor are free: lo (one product, the
//     first) 20 MFMA slots ahead of its use, mid (products 3 and 4) 16 slots ahead; hi (three products, the last among them) is
//     double-buffered and read a whole k-step (24 slots) ahead;
//   * the hidden layer's bias: H floats in LDS, one broadcast ds_read_b128 per tile.
// The software pipeline has three stages (the hidden layer needs ALL of layer 1's activations before any of its tiles completes):
//   stage 1  layer 1 pair by pair (24 slots); pair p - 1's max-and-split VALU work between pair p's MFMAs
//   stage 2  hidden layer, output-tile pair by pair (24 H/32 slots); between pair p's MFMAs run the activations of pair p - 1
//            (for p = 0: of layer 1's last pair, ahead of the k-step that consumes them) and the 12 slots of the output layer's
//            k-step p - 2
//   tail     the last pair's activations around the output layer's last two k-steps
// Every layer round-robins the accumulators of a pair inside each product, so a dependent MFMA is four slots behind its
// predecessor.  The action and cost prologue and the chunk epilogue are rollout_mlp_relu.hip's.
// One persistent workgroup of 4 waves per CU over 128-sample chunks, two sample tiles per wave -- as the siblings.
#include <hip/hip_ext.h>
#include <atomic>
#include "actions.hpp"
#include "dispatch.hpp"
#include "mlp_deep_relu.hpp"
#include "mlp_split_ops.hpp"

namespace mppi {
using namespace split_ops;

namespace {
constexpr int DR_NT = 2;                                         // sample tiles (of 16) per wave
constexpr int DR_THREADS = 256;                                  // 4 waves = one per SIMD
constexpr int DR_SAMPLES = (DR_THREADS / WAVE) * DR_NT * 16;     // samples per workgroup chunk (128)
constexpr size_t DR_LDS_MAX = 160 * 1024;

// floats of the action tables in front of the hidden layer's bias and planes (Ue | Um | G), padded to 16 bytes
__host__ __device__ inline int dr_table_floats(int J) { return (3 * J + 3) & ~3; }
__host__ __device__ inline size_t dr_plane_bytes(int HT) { return (size_t)HT * (HT / 2) * 3 * WAVE * 16; }

// NS MFMA slots, each followed by its share of NUN VALU units spread evenly over the first SPAN slots.  sched_barrier(0) after
// every slot keeps hipcc's scheduler from re-clustering the slots.
template <int NS, int SPAN, int NUN, class FS, class FU>
__device__ __forceinline__ void dr_interleave(FS&& slot, FU&& unit) {
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
__global__ void __launch_bounds__(DR_THREADS, 1) rollout_mlp_deep_relu_kernel(const KArgs<float> a_in) {
  static_assert(HT % 2 == 0 && HT >= 4, "a k-step consumes hidden tiles in pairs; the three-stage pipeline needs two pairs");
  static_assert(NX >= 1 && NX <= 16 && NU >= 1 && NU <= 8, "one 16-state output tile, controls and bias in the layer-1 k-step");
  static_assert(NOISE == MPPI_NOISE_TNK4 || NOISE == MPPI_NOISE_ACTIONS, "rows from memory, read component-wise");
  constexpr int NC = NU > 4 ? 2 : 1, BIAS_E = 4 + NC, NI = NX + NU;
  constexpr int NT = DR_NT, H = HT * 16, HP = HT / 2;
  const KArgs<float> a = env_view(a_in);
  stamp_entry(a.tstamp);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* Ue = reinterpret_cast<float*>(smem_raw);   // [J]
  float* Um = Ue + a.J;                             // [J]
  float* G = Um + a.J;                              // [J]
  float* bias2 = Ue + dr_table_floats(a.J);         // [H]
  u32x4* A2s = reinterpret_cast<u32x4*>(bias2 + H); // [HT][HP][3][64]

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
  float qx4[4], b3r[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    qx4[r] = 4 * g + r < NX ? b3[NX + 1 + 4 * g + r] : 0.f;
    b3r[r] = 4 * g + r < NX ? b3[4 * g + r] : 0.f;                 // D rows are 4g + r
  }
  bool own[NC];
  float qu_c[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    own[c] = g + 4 * c < NU;
    qu_c[c] = own[c] ? b3[NX + 1 + NX + g + 4 * c] : 0.f;
  }

  // ---- hidden-layer planes into LDS: fragment f = m HP + j of output tile m, k-step j; the four waves share the work ----
  for (int f = wv; f < HT * HP; f += DR_THREADS / WAVE) {
    const int m = f / HP, j = f % HP;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = W2T[(16 * (2 * j + (e >> 2)) + 4 * g + (e & 3)) * H + 16 * m + s];
    const Planes p = split_pack8(v);
    A2s[(f * 3 + 0) * WAVE + lane] = p.h;
    A2s[(f * 3 + 1) * WAVE + lane] = p.m;
    A2s[(f * 3 + 2) * WAVE + lane] = p.l;
  }
  for (int u = threadIdx.x; u < H; u += DR_THREADS) bias2[u] = b2[u];

  // ---- layer-1 and output-layer planes: resident in the accumulation registers ----
  Planes A1[HT];
#pragma unroll
  for (int m = 0; m < HT; ++m) {
    const float* __restrict__ row = W1 + (16 * m + s) * NI;        // hidden unit 16m + s
    float v[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = 4 * g + e < NX ? row[4 * g + e] : 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) v[4 + c] = own[c] ? row[NX + g + 4 * c] : 0.f;
    v[BIAS_E] = g == 0 ? b1[16 * m + s] : 0.f;                     // bias column (B1 holds 1 there)
#pragma unroll
    for (int e = BIAS_E + 1; e < 8; ++e) v[e] = 0.f;
    A1[m] = split_pack8(v);
  }
  Planes A3[HP];
#pragma unroll
  for (int j = 0; j < HP; ++j) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = s < NX ? W3T[(16 * (2 * j + (e >> 2)) + 4 * g + (e & 3)) * NX + s] : 0.f;
    A3[j] = split_pack8(v);
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
    asm volatile("" : "+a"(A3[j].l));
  }

  ActionConsts<float, NU> ac;
  ac.load(a, nullptr);
  // Ue = the sequence the noise is added to and measured from (SMPPI: the host's base A + U dt); the action cost table G is
  // built from the lifted nominal U itself (u_eff) either way
  const bool smppi = a.B != nullptr;
  for (int j = threadIdx.x; j < a.J; j += DR_THREADS) Ue[j] = u_base(a, j);
  __syncthreads();                                   // (the hidden layer's planes and bias are complete behind this barrier, too)
  for (int j = threadIdx.x; j < a.J; j += DR_THREADS) {
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
  const int nchunks = (a.K + DR_SAMPLES - 1) / DR_SAMPLES;
  for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int kbase = chunk * DR_SAMPLES + wv * (NT * 16);
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
      // slot pipeline below puts them (they are loop-invariant: hoisted, they would be 384 registers at H = 128)
      int a2_lane = lane, b2_lane = 4 * g;
      asm volatile("" : "+v"(a2_lane));
      asm volatile("" : "+v"(b2_lane));
      auto lds_plane = [&](int m, int j, int which) -> u32x4 { return A2s[((m * HP + j) * 3 + which) * WAVE + a2_lane]; };
      auto lds_bias = [&](int m) -> f32x4 { return *reinterpret_cast<const f32x4*>(bias2 + 16 * m + b2_lane); };

#pragma unroll
      for (int i = 0; i < NT; ++i) {
#pragma unroll
        for (int c = 0; c < NC; ++c) zc[i][c] = zn[i][c];
      }
      fetch(t + 1 < a.Tn ? t + 1 : t, zn);   // prefetch the next step's rows (compute >> latency here)

      // ---- actions (as in the tanh kernels): lane (g,s) owns control dimension g (and g + 4 where nu > 4) ----
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
      }

      // ---- the three layers as one software pipeline ----
      // A dependent MFMA (same accumulator) cannot issue until its predecessor has drained: layer 1 and the hidden layer
      // round-robin the 2 tiles x 2 sample tiles of a pair inside each product (an accumulator comes up every 4th slot); the output
      // layer keeps two accumulators per sample tile (even | odd products), summed once per timestep.
      f32x4 Hc[2][2][NT];                      // layer 1 [buffer][hidden tile of the pair][sample tile]
      Planes R1[HP][NT];                       // bf16 planes of the whole first hidden vector [k-step][sample tile]
      f32x4 Ac[2][2][NT];                      // hidden layer [buffer][tile of the pair][sample tile]
      Planes R2[2][NT];                        // bf16 planes of the second hidden vector [buffer][sample tile]
      f32x4 O[2][NT];                          // output layer [parity of the product][sample tile]
      // hidden-layer planes in flight.  Step n = p HP + j (pair p of output tiles, k-step j), [tile of the pair]: hi [n & 1], read at
      // the first slot of step n - 1; lo and mid single-buffered, read behind their last use in step n - 1 (slots 4 and 16)
      u32x4 Wh[2][2], Wm[2], Wl[2];
      f32x4 bias[2];
      const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
      static_assert(NT == 2, "slot decoding assumes two sample tiles per wave");
      auto layer1_slot = [&](auto p_c, auto slot_c) {              // slot 0..23 of pair p
        constexpr int p = decltype(p_c)::value, slot = decltype(slot_c)::value;
        constexpr int pr = slot >> 2, q = (slot >> 1) & 1, i = slot & 1, buf = p & 1;
        if constexpr (p == HP - 1 && slot == 0) {                  // the hidden layer's first step, under layer 1's last pair
#pragma unroll
          for (int q2 = 0; q2 < 2; ++q2) {
            Wh[0][q2] = lds_plane(q2, 0, 0);
            Wm[q2] = lds_plane(q2, 0, 1);
            Wl[q2] = lds_plane(q2, 0, 2);
            bias[q2] = lds_bias(q2);
          }
        }
        Hc[buf][q][i] = mfma_bf(plane(A1[2 * p + q], plane_a(pr)), plane(B1[i], plane_b(pr)), pr == 0 ? zero4 : Hc[buf][q][i]);
      };
      auto hidden_slot = [&](auto p_c, auto slot_c) {              // slot 0..24 HP - 1 of output-tile pair p
        constexpr int p = decltype(p_c)::value, slot = decltype(slot_c)::value;
        constexpr int j = slot / 24, w = slot % 24, pr = w >> 2, q = (w >> 1) & 1, i = w & 1, buf = p & 1, n = p * HP + j;
        constexpr int pn = (n + 1) / HP, jn = (n + 1) % HP;        // the next step's pair and k-step
        if constexpr (n + 1 < HP * HP && (w == 0 || w == 4 || w == 16)) {
#pragma unroll
          for (int q2 = 0; q2 < 2; ++q2) {
            if constexpr (w == 0) Wh[(n + 1) & 1][q2] = lds_plane(2 * pn + q2, jn, 0);
            else if constexpr (w == 4) Wl[q2] = lds_plane(2 * pn + q2, jn, 2);       // behind product 0, lo's only use
            else Wm[q2] = lds_plane(2 * pn + q2, jn, 1);                               // behind products 2 and 3
          }
        }
        if constexpr (w == 4 && j == 0 && p + 1 < HP) {            // the next pair's bias, behind this pair's only use of it
#pragma unroll
          for (int q2 = 0; q2 < 2; ++q2) bias[q2] = lds_bias(2 * (p + 1) + q2);
        }
        constexpr int pa = plane_a(pr);
        const u32x4& wa = pa == 0 ? Wh[n & 1][q] : (pa == 1 ? Wm[q] : Wl[q]);
        Ac[buf][q][i] = mfma_bf(wa, plane(R1[j][i], plane_b(pr)), (j == 0 && pr == 0) ? bias[q] : Ac[buf][q][i]);
      };
      auto output_slot = [&](auto jc_c, auto slot_c) {             // slot 0..11 of k-step jc
        constexpr int jc = decltype(jc_c)::value, slot = decltype(slot_c)::value;
        constexpr int pr = slot >> 1, i = slot & 1, buf = jc & 1;
        O[pr & 1][i] = mfma_bf(plane(A3[jc], plane_a(pr)), plane(R2[buf][i], plane_b(pr)), (jc == 0 && pr < 2) ? zero4 : O[pr & 1][i]);
      };
      // activation work of a pair's 16 hidden values per lane, in units of two values (one register of each plane): max(h, 0),
      // the truncation split, the three packs.  LAYER 1: Hc of pair idx -> R1[idx] (then pinned in AGPRs); LAYER 2: Ac of pair
      // idx -> R2[idx & 1]
      constexpr int NUNIT = 8;
      auto relu_unit = [&](auto layer_c, auto idx_c, auto unit_c) {
        constexpr int layer = decltype(layer_c)::value, idx = decltype(idx_c)::value, unit = decltype(unit_c)::value;
        constexpr int v0 = 2 * unit, i = v0 >> 3, e0 = v0 & 7, q = e0 >> 1, buf = idx & 1;
        const f32x4& src = layer == 1 ? Hc[buf][e0 >> 2][i] : Ac[buf][e0 >> 2][i];
        const float ra = fmaxf(src[e0 & 3], 0.f), rb = fmaxf(src[(e0 & 3) + 1], 0.f);
        const Split3 sa = split3(ra), sb = split3(rb);
        Planes& dst = layer == 1 ? R1[idx][i] : R2[buf][i];
        dst.h[q] = pack_bf16(ra, rb);                              // truncation = the upper halves as they are
        dst.m[q] = pack_bf16(sa.m, sb.m);
        dst.l[q] = pack_bf16(sa.l, sb.l);
        if constexpr (layer == 1 && unit == NUNIT - 1) {
#pragma unroll
          for (int i2 = 0; i2 < NT; ++i2) {
            asm volatile("" : "+a"(R1[idx][i2].h));
            asm volatile("" : "+a"(R1[idx][i2].m));
            asm volatile("" : "+a"(R1[idx][i2].l));
          }
        }
      };
      // stage 1: layer 1, the activations of pair p - 1 between the MFMAs of pair p
      static_for<0, HP>([&](auto pc) {
        constexpr int p = decltype(pc)::value, pv = p >= 1 ? p - 1 : 0;
        dr_interleave<24, (p >= 1 ? 24 : 0), (p >= 1 ? NUNIT : 0)>(
            [&](auto sc) { layer1_slot(pc, sc); }, [&](auto uc) { relu_unit(ic<1>{}, ic<pv>{}, uc); });
      });
      // stage 2: the hidden layer; the output layer's k-step p - 2 spread evenly among pair p's slots
      static_for<0, HP>([&](auto pc) {
        constexpr int p = decltype(pc)::value;
        constexpr int nH = 24 * HP, nC = p >= 2 ? 12 : 0, N = nH + nC;
        auto slot = [&](auto sc) {
          constexpr int sl = decltype(sc)::value;
          constexpr int c_before = (sl * nC) / N, c_after = ((sl + 1) * nC) / N;
          if constexpr (c_after > c_before) output_slot(ic<(p >= 2 ? p - 2 : 0)>{}, ic<c_before>{});
          else hidden_slot(pc, ic<sl - c_before>{});
        };
        // pair 0 carries the activations of layer 1's last pair: complete before k-step HP - 1 consumes them
        if constexpr (p == 0) dr_interleave<N, 24 * (HP - 1), NUNIT>(slot, [&](auto uc) { relu_unit(ic<1>{}, ic<HP - 1>{}, uc); });
        else dr_interleave<N, N, NUNIT>(slot, [&](auto uc) { relu_unit(ic<2>{}, ic<(p >= 1 ? p - 1 : 0)>{}, uc); });
      });
      // tail: the activations of the last pair, the output layer's last two k-steps
      dr_interleave<12, 12, NUNIT>([&](auto sc) { output_slot(ic<HP - 2>{}, sc); },
                                   [&](auto uc) { relu_unit(ic<2>{}, ic<HP - 1>{}, uc); });
      dr_interleave<12, 0, 0>([&](auto sc) { output_slot(ic<HP - 1>{}, sc); }, [&](auto) {});
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        const f32x4 Ot = O[0][i] + O[1][i];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          x[i][r] = fmaf(rs, Ot[r] + b3r[r], x[i][r]);
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
    __shared__ float red[DR_THREADS / WAVE];
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
static int launch_deep_relu(const KArgs<float>& a_in, hipStream_t st) {
  KArgs<float> a = a_in;
  // the rows are read component-wise: external rows (TNK4 / raw actions) in the diagonal (or coloured) form only
  if (!(a.noise_src == MPPI_NOISE_TNK4 || a.noise_src == MPPI_NOISE_ACTIONS)) return MPPI_E_UNSUPPORTED;
  if (!(a.diag != 0 || a.coloured != 0 || a.noise_src == MPPI_NOISE_ACTIONS)) return MPPI_E_UNSUPPORTED;
  const size_t smem = (size_t)(dr_table_floats(a.J) + HT * 16) * sizeof(float) + dr_plane_bytes(HT);
  if (smem + 64 > DR_LDS_MAX) return MPPI_E_UNSUPPORTED;       // (+ the kernel's static reduction slots)
  const int nchunks = (a.K + DR_SAMPLES - 1) / DR_SAMPLES;
  static const int n_cu = [] {
    int dev = 0, n = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    return n > 0 ? n : 256;
  }();
  int gx = nchunks;
  const int cap = n_cu / (a.n_env > 1 ? a.n_env : 1);
  if (gx > (cap > 1 ? cap : 1)) gx = cap > 1 ? cap : 1;       // one workgroup per CU, persistent over its chunks
  const dim3 grid(gx, 1, a.n_env), block(DR_THREADS);
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  profile_next_events(&ev0, &ev1, &a.tstamp);
#define MPPI_LAUNCH1(KERNEL)                                                                                   \
  do {                                                                                                         \
    if (smem > 64 * 1024) (void)hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem); \
    if (ev1 != nullptr) hipExtLaunchKernelGGL(KERNEL, grid, block, smem, st, ev0, ev1, 0, a);                  \
    else hipLaunchKernelGGL(KERNEL, grid, block, smem, st, a);                                                 \
  } while (0)
  if (a.noise_src == MPPI_NOISE_ACTIONS) MPPI_LAUNCH1((rollout_mlp_deep_relu_kernel<HT, MPPI_NOISE_ACTIONS, NX, NU>));
  else MPPI_LAUNCH1((rollout_mlp_deep_relu_kernel<HT, MPPI_NOISE_TNK4, NX, NU>));
#undef MPPI_LAUNCH1
  return (int)hipGetLastError();
}

// the (nx, nu) pairs with an instantiation: those of the tanh kernel (rollout_mlp_deep.hip MPPI_DEEP_DIMS)
#define MPPI_DEEP_RELU_DIMS(X) X(16, 4) X(12, 6) X(2, 1)

bool supported_mlp2_relu(int nx, int nu, int hidden) {
  if (!(hidden == 64 || hidden == 128)) return false;
#define X(NX, NU) if (nx == NX && nu == NU) return true;
  MPPI_DEEP_RELU_DIMS(X)
#undef X
  return false;
}

static std::atomic<long long> g_deep_relu_launches{0};

int rollout_mlp_deep_relu(const KArgs<float>& a, hipStream_t st) {
  if (a.mp == nullptr) return MPPI_E_BADARG;
  // KMPPI's fused interpolation: the caller's two-launch form hands this kernel raw action rows
  if (!supported_mlp2_relu(a.nx, a.nu, a.hidden) || a.states != nullptr || a.M != 1 || a.W != nullptr) return MPPI_E_UNSUPPORTED;
  int r = MPPI_E_UNSUPPORTED;
#define X(NX, NU) \
  if (a.nx == NX && a.nu == NU) r = a.hidden == 64 ? launch_deep_relu<4, NX, NU>(a, st) : launch_deep_relu<8, NX, NU>(a, st);
  MPPI_DEEP_RELU_DIMS(X)
#undef X
  if (r == 0) ++g_deep_relu_launches;
  return r;
}

}  // namespace mppi

extern "C" int64_t mppi_stat_mlp_deep_relu_launches(void) { return (int64_t)mppi::g_deep_relu_launches.load(); }
