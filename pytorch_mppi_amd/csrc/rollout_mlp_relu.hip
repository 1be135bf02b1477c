// K1 for the residual MLP with one hidden layer of ReLU units (mlp_relu.hpp; the (nx, nu) of the split-operand kernel, hidden padded
// to H in {64, 128, 256}) on the 16-bit matrix cores with fp32-level accuracy and NO limit on the weights or the activations.
//
//   x' = x + s * (W2 relu(W1 [x;u] + b1) + b2),   cost = sum qx x^2 + sum qu u^2
//
// The tanh kernels (rollout_mlp_split.hip) feed layer 2 with r = 1 / (2^h + 1) in (0, 1), which two fp16 pieces hold; relu(h) is
// unbounded, so BOTH layers run on bf16 x 3 here (fp32's exponent range in every piece):
//   v = hi + mid + lo exactly by truncation (8 + 8 + 8 significant bits), six of the nine piece products on
//   v_mfma_f32_16x16x32_bf16, smallest first:  l.h  h.l  m.m | m.h  h.m | h.h  -- dropping m.l, l.m, l.l <= 2^-23 relative.
//   Nothing is folded into the weights: W1, b1 (through the constant-1 k-slot) and W2 are split as they are, b2 is added in fp32.
// Balance: per pair of hidden tiles and wave 24 + 12 MFMAs against ~6.5 plain VALU operations per activation (v_max, two
// v_and + v_sub, 1.5 v_perm) -- no transcendental: the matrix pipe (36 x 16 cycles) is the longer side, not VALU issue as in the
// tanh kernels (v_exp + v_rcp = 32 of their ~48 VALU cycles per activation).
//
// Transposed chain, samples on the MFMA column axis, no lane permutes or LDS round trips between layers or timesteps.
// Lane l = (g = l >> 4, s = l & 15); A[i][k] and B[k][j] hold k = 8g + e (e = 0..7) at i = j = s, D[i][j] holds i = 4g + r at j = s.
//   layer 1   H^T (16 hidden x 16 samples) = A1[m] (16 x 32) . B1 (32 x 16)    per hidden tile m
//       k-slot (g, e):  e < 4 -> state x[4g+e]   e = 4 -> control u[g]   (nu > 4: e = 5 -> control u[g+4])
//       the next e at g = 0 -> constant 1 (b1 rides in that column of A1)   the rest -> 0
//   layer 2   O^T (16 states x 16 samples) = sum_j A2[j] (16 x 32) . B2[j] (32 x 16),  j = 0..H/32-1
//       k-slot (g, e) of step j = hidden unit 16 (2j + (e >> 2)) + 4g + (e & 3) = the lane's accumulator registers of hidden
//       tiles 2j and 2j + 1: layer 1's D layout IS layer 2's B layout.
// Where the weights live: layer 1 (H/16 tiles x 3 planes x 4 = 192 registers at H = 256) is pinned in AGPRs -- an MFMA reads its A
// operand from there directly.  Three layer-2 planes per k-step would be 96 more, which does not fit beside the pipeline's VGPRs:
// they stay in LDS for the whole launch, [k-step][plane][lane] as 16-byte elements (H/32 x 3 x 1 KB = 24 KB at H = 256), one
// conflict-free ds_read_b128 per plane and k-step, shared by the four waves, double-buffered in registers and read one k-step
// ahead (under the previous k-step's MFMAs).  One layout for every width: at H <= 128 the reads cost 3 LDS instructions per 36 MFMAs.
// Software pipeline per timestep (as the siblings): iteration j issues layer 1 of pair j + 1 (24 slots) and layer 2 of k-step
// j - 1 (12 slots, spread evenly among them), with the max-and-split VALU work of pair j between those MFMAs; Hc and B2 are
// double-buffered.  Layer 2 keeps one accumulator per magnitude class of the products and sample tile, so a dependent MFMA is at
// least five slots behind its predecessor in the steady state.
// One persistent workgroup of 4 waves per CU over 128-sample chunks, two sample tiles per wave.
#include <hip/hip_ext.h>
#include <atomic>
#include "actions.hpp"
#include "dispatch.hpp"
#include "mlp_relu.hpp"
#include "mlp_split_ops.hpp"

namespace mppi {
using namespace split_ops;

namespace {
constexpr int RL_NT = 2;                                         // sample tiles (of 16) per wave
constexpr int RL_THREADS = 256;                                  // 4 waves = one per SIMD
constexpr int RL_SAMPLES = (RL_THREADS / WAVE) * RL_NT * 16;     // samples per workgroup chunk (128)
constexpr size_t RL_LDS_MAX = 160 * 1024;

// floats of the action tables in front of the layer-2 planes (Ue | Um | G), padded to 16 bytes
__host__ __device__ inline int rl_table_floats(int J) { return (3 * J + 3) & ~3; }
__host__ __device__ inline size_t rl_plane_bytes(int HT) { return (size_t)(HT / 2) * 3 * WAVE * 16; }

template <int V> using ic = std::integral_constant<int, V>;
}  // namespace

template <int HT /* hidden / 16 */, int NOISE, int NX, int NU>
__global__ void __launch_bounds__(RL_THREADS, 1) rollout_mlp_relu_kernel(const KArgs<float> a_in) {
  static_assert(HT % 2 == 0 && HT >= 4, "layer 2 consumes hidden tiles in pairs; the pipeline overlaps at least two pairs");
  static_assert(NX >= 1 && NX <= 16 && NU >= 1 && NU <= 8, "one 16-state output tile, controls and bias in the layer-1 k-step");
  static_assert(NOISE == MPPI_NOISE_TNK4 || NOISE == MPPI_NOISE_ACTIONS, "rows from memory, read component-wise");
  constexpr int NC = NU > 4 ? 2 : 1, BIAS_E = 4 + NC, NI = NX + NU;
  constexpr int NT = RL_NT, H = HT * 16, HP = HT / 2;
  const KArgs<float> a = env_view(a_in);
  stamp_entry(a.tstamp);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* Ue = reinterpret_cast<float*>(smem_raw);   // [J]
  float* Um = Ue + a.J;                             // [J]
  float* G = Um + a.J;                              // [J]
  u32x4* A2s = reinterpret_cast<u32x4*>(Ue + rl_table_floats(a.J));   // [HP][3][64]

  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  const int g = lane >> 4, s = lane & 15;

  // ---- parameters: blob = W1 (H,nx+nu) | b1 (H) | W2 (nx,H) | b2 (nx) | res_scale | qx (nx) | qu (nu) ----
  const float* __restrict__ W1 = a.mp;
  const float* __restrict__ b1 = W1 + H * NI;
  const float* __restrict__ W2 = b1 + H;
  const float* __restrict__ b2 = W2 + NX * H;
  const float rs = b2[NX];
  float qx4[4], b2r[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    qx4[r] = 4 * g + r < NX ? b2[NX + 1 + 4 * g + r] : 0.f;
    b2r[r] = 4 * g + r < NX ? b2[4 * g + r] : 0.f;                 // D rows are 4g + r
  }
  bool own[NC];
  float qu_c[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    own[c] = g + 4 * c < NU;
    qu_c[c] = own[c] ? b2[NX + 1 + NX + g + 4 * c] : 0.f;
  }

  // ---- layer-2 planes into LDS: k-step j, state row s, hidden unit h(j, g, e); the four waves share the work ----
  for (int j = wv; j < HP; j += RL_THREADS / WAVE) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = s < NX ? W2[s * H + 16 * (2 * j + (e >> 2)) + 4 * g + (e & 3)] : 0.f;
    const Planes p = split_pack8(v);
    A2s[(j * 3 + 0) * WAVE + lane] = p.h;
    A2s[(j * 3 + 1) * WAVE + lane] = p.m;
    A2s[(j * 3 + 2) * WAVE + lane] = p.l;
  }

  // ---- layer-1 planes: resident in the accumulation registers ----
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
#pragma unroll
  for (int m = 0; m < HT; ++m) {
    asm volatile("" : "+a"(A1[m].h));
    asm volatile("" : "+a"(A1[m].m));
    asm volatile("" : "+a"(A1[m].l));
  }

  ActionConsts<float, NU> ac;
  ac.load(a, nullptr);
  // Ue = the sequence the noise is added to and measured from (SMPPI: the host's base A + U dt); the action cost table G is
  // built from the lifted nominal U itself (u_eff) either way
  const bool smppi = a.B != nullptr;
  for (int j = threadIdx.x; j < a.J; j += RL_THREADS) Ue[j] = u_base(a, j);
  __syncthreads();                                   // (the layer-2 planes are complete behind this barrier, too)
  for (int j = threadIdx.x; j < a.J; j += RL_THREADS) {
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
  const int nchunks = (a.K + RL_SAMPLES - 1) / RL_SAMPLES;
  for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int kbase = chunk * RL_SAMPLES + wv * (NT * 16);
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
      // this lane's element of every layer-2 plane; opaque per timestep, so that the reads of a timestep stay where the slot
      // pipeline below puts them (they are loop-invariant: hoisted, they would be 96 registers at H = 256)
      int a2_lane = lane;
      asm volatile("" : "+v"(a2_lane));
      auto lds_planes = [&](int j) -> Planes {
        Planes p;
        p.h = A2s[(j * 3 + 0) * WAVE + a2_lane];
        p.m = A2s[(j * 3 + 1) * WAVE + a2_lane];
        p.l = A2s[(j * 3 + 2) * WAVE + a2_lane];
        return p;
      };
      Planes Wp[2];                            // layer-2 planes in flight: k-step j in [j & 1], read at the first slot of k-step j - 1
      Wp[0] = lds_planes(0);

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

      // ---- the two layers as one software pipeline ----
      // A dependent MFMA (same accumulator) cannot issue until its predecessor has drained: layer 1 round-robins the 2 hidden
      // tiles x 2 sample tiles of a pair inside each product (an accumulator comes up every 4th layer-1 slot); layer 2 keeps one
      // accumulator per magnitude class of the products (small: l.h h.l m.m | middle: m.h h.m | big: h.h) and sample tile,
      // summed once per timestep.
      f32x4 Hc[2][2][NT];                      // layer 1 [buffer][hidden tile of the pair][sample tile]
      Planes B2[2][NT];                        // bf16 planes of relu(h) [buffer][sample tile]
      f32x4 Os[NT], Om[NT], Ob[NT];
      const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
      static_assert(NT == 2, "slot decoding assumes two sample tiles per wave");
      auto layer1_slot = [&](auto p_c, auto slot_c) {              // slot 0..23 of pair p
        constexpr int p = decltype(p_c)::value, slot = decltype(slot_c)::value;
        constexpr int pr = slot >> 2, q = (slot >> 1) & 1, i = slot & 1, buf = p & 1;
        Hc[buf][q][i] = mfma_bf(plane(A1[2 * p + q], plane_a(pr)), plane(B1[i], plane_b(pr)), pr == 0 ? zero4 : Hc[buf][q][i]);
      };
      auto layer2_slot = [&](auto jc_c, auto slot_c) {             // slot 0..11 of k-step jc
        constexpr int jc = decltype(jc_c)::value, slot = decltype(slot_c)::value;
        constexpr int pr = slot >> 1, i = slot & 1, buf = jc & 1;
        if constexpr (slot == 0 && jc + 1 < HP) Wp[(jc + 1) & 1] = lds_planes(jc + 1);   // the next k-step's planes, under this one's MFMAs
        const u32x4& wa = plane(Wp[buf], plane_a(pr));
        const u32x4& hb = plane(B2[buf][i], plane_b(pr));
        if constexpr (pr <= 2) Os[i] = mfma_bf(wa, hb, (jc == 0 && pr == 0) ? zero4 : Os[i]);
        else if constexpr (pr <= 4) Om[i] = mfma_bf(wa, hb, (jc == 0 && pr == 3) ? zero4 : Om[i]);
        else Ob[i] = mfma_bf(wa, hb, jc == 0 ? zero4 : Ob[i]);
      };
      // activation work of pair j's 16 hidden values per lane, in units of two values (one register of each plane):
      // max(h, 0), the truncation split, the three packs
      constexpr int NUNIT = 8;
      auto relu_unit = [&](auto j_c, auto unit_c) {
        constexpr int j = decltype(j_c)::value, unit = decltype(unit_c)::value;
        constexpr int v0 = 2 * unit, i = v0 >> 3, e0 = v0 & 7, q = e0 >> 1, buf = j & 1;
        const float ra = fmaxf(Hc[buf][e0 >> 2][i][e0 & 3], 0.f), rb = fmaxf(Hc[buf][e0 >> 2][i][(e0 & 3) + 1], 0.f);
        const Split3 sa = split3(ra), sb = split3(rb);
        B2[buf][i].h[q] = pack_bf16(ra, rb);                       // truncation = the upper halves as they are
        B2[buf][i].m[q] = pack_bf16(sa.m, sb.m);
        B2[buf][i].l[q] = pack_bf16(sa.l, sb.l);
      };
      // layer 1 of the first pair, nothing to overlap it with
      static_for<0, 24>([&](auto sc) {
        layer1_slot(ic<0>{}, sc);
        __builtin_amdgcn_sched_barrier(0);
      });
      static_for<0, HP>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        constexpr bool hasA = j + 1 < HP, hasC = j >= 1;
        constexpr int nA = hasA ? 24 : 0, nC = hasC ? 12 : 0, N = nA + nC;   // MFMA slots of this iteration
        static_for<0, N>([&](auto sc) {
          constexpr int sl = decltype(sc)::value;
          // the nC layer-2 slots spread evenly among the nA layer-1 slots
          constexpr int c_before = (sl * nC) / N, c_after = ((sl + 1) * nC) / N;
          if constexpr (c_after > c_before) layer2_slot(ic<(j >= 1 ? j - 1 : 0)>{}, ic<c_before>{});
          else layer1_slot(ic<(hasA ? j + 1 : 0)>{}, ic<sl - c_before>{});
          // pair j's VALU units spread evenly over the N slots
          static_for<(sl * NUNIT) / N, ((sl + 1) * NUNIT) / N>([&](auto uc) { relu_unit(jc, uc); });
          __builtin_amdgcn_sched_barrier(0);
        });
      });
      // the last k-step of layer 2
      static_for<0, 12>([&](auto sc) {
        layer2_slot(ic<HP - 1>{}, sc);
        __builtin_amdgcn_sched_barrier(0);
      });
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        const f32x4 O = (Os[i] + Om[i]) + Ob[i];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          x[i][r] = fmaf(rs, O[r] + b2r[r], x[i][r]);
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
    __shared__ float red[RL_THREADS / WAVE];
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
static int launch_relu(const KArgs<float>& a_in, hipStream_t st) {
  KArgs<float> a = a_in;
  // the rows are read component-wise: external rows (TNK4 / raw actions) in the diagonal (or coloured) form only
  if (!(a.noise_src == MPPI_NOISE_TNK4 || a.noise_src == MPPI_NOISE_ACTIONS)) return MPPI_E_UNSUPPORTED;
  if (!(a.diag != 0 || a.coloured != 0 || a.noise_src == MPPI_NOISE_ACTIONS)) return MPPI_E_UNSUPPORTED;
  const size_t smem = (size_t)rl_table_floats(a.J) * sizeof(float) + rl_plane_bytes(HT);
  if (smem + 64 > RL_LDS_MAX) return MPPI_E_UNSUPPORTED;       // (+ the kernel's static reduction slots)
  const int nchunks = (a.K + RL_SAMPLES - 1) / RL_SAMPLES;
  static const int n_cu = [] {
    int dev = 0, n = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    return n > 0 ? n : 256;
  }();
  int gx = nchunks;
  const int cap = n_cu / (a.n_env > 1 ? a.n_env : 1);
  if (gx > (cap > 1 ? cap : 1)) gx = cap > 1 ? cap : 1;       // one workgroup per CU, persistent over its chunks
  const dim3 grid(gx, 1, a.n_env), block(RL_THREADS);
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  profile_next_events(&ev0, &ev1, &a.tstamp);
#define MPPI_LAUNCH1(KERNEL)                                                                                   \
  do {                                                                                                         \
    if (smem > 64 * 1024) (void)hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem); \
    if (ev1 != nullptr) hipExtLaunchKernelGGL(KERNEL, grid, block, smem, st, ev0, ev1, 0, a);                  \
    else hipLaunchKernelGGL(KERNEL, grid, block, smem, st, a);                                                 \
  } while (0)
  if (a.noise_src == MPPI_NOISE_ACTIONS) MPPI_LAUNCH1((rollout_mlp_relu_kernel<HT, MPPI_NOISE_ACTIONS, NX, NU>));
  else MPPI_LAUNCH1((rollout_mlp_relu_kernel<HT, MPPI_NOISE_TNK4, NX, NU>));
#undef MPPI_LAUNCH1
  return (int)hipGetLastError();
}

// the (nx, nu) pairs with an instantiation: those of the split-operand kernel (rollout_mlp_split.hip)
#define MPPI_RELU_DIMS(X) X(16, 4) X(8, 2) X(12, 6) X(16, 8)

bool supported_mlp_relu(int nx, int nu, int hidden) {
  if (!(hidden == 64 || hidden == 128 || hidden == 256)) return false;
#define X(NX, NU) if (nx == NX && nu == NU) return true;
  MPPI_RELU_DIMS(X)
#undef X
  return false;
}

static std::atomic<long long> g_relu_launches{0};

int rollout_mlp_relu(const KArgs<float>& a, hipStream_t st) {
  if (a.mp == nullptr) return MPPI_E_BADARG;
  // KMPPI's fused interpolation: the caller's two-launch form hands this kernel raw action rows
  if (!supported_mlp_relu(a.nx, a.nu, a.hidden) || a.states != nullptr || a.M != 1 || a.W != nullptr) return MPPI_E_UNSUPPORTED;
  int r = MPPI_E_UNSUPPORTED;
#define X(NX, NU)                                                         \
  if (a.nx == NX && a.nu == NU)                                           \
    r = a.hidden == 64 ? launch_relu<4, NX, NU>(a, st) : (a.hidden == 128 ? launch_relu<8, NX, NU>(a, st) : launch_relu<16, NX, NU>(a, st));
  MPPI_RELU_DIMS(X)
#undef X
  if (r == 0) ++g_relu_launches;
  return r;
}

}  // namespace mppi

extern "C" int64_t mppi_stat_mlp_relu_launches(void) { return (int64_t)mppi::g_relu_launches.load(); }
