// K1 for the residual MLP with TWO hidden layers (mlp_deep.hpp; nx <= 16, nu <= 8, H in {32, 64, 128}) with process noise and
// M = 2..4 state rollouts per action sequence (rollout_samples, mppi.py:334-373) on the 16-bit matrix cores.
//
//   x' = x + s * (W3 tanh(W2 tanh(W1 [x;u] + b1) + b2) + b3) + sd (.) n,   c_m(t) = sum qx x^2 + sum qu u^2   on the noisy state
//   total = mean_m sum_t c_m(t) + var_cost sum_t var_disc^t var_m(c_m(t)) + smoothness (once) + action cost (once)
// -- the quantities, conventions and process-noise counters of rollout_stream_multi (rollout.hpp) and of
// rollout_mlp_split_multi_kernel.  The model's per-lane form has no M > 1 instantiation (rollout_mlp2.hip), so this kernel is
// the only HIP form of such a command: it also serves the visited states.
//
// Arithmetic and operand placement are rollout_mlp_deep.hip's, see there: layer 1 bf16 x 3 with its planes (and the output
// layer's) in AGPRs, the hidden and output layers two-piece fp16, the hidden->hidden planes and their bias in LDS -- one copy
// for the workgroup, laid out once per launch --, the three-stage MFMA / activation pipeline, two 16-sample tiles per wave,
// lane (g, s) owns state rows 4g..4g+3 and control(s) g (, g + 4).
// Work split (rollout_mlp_split_multi.hip): ONE WAVE PER ROLLOUT COPY, the four waves of a workgroup roll different copies of
// the same 32 samples.  A chunk is 64 consecutive samples (one block_min slot):
//   M = 3 | 4   the workgroup walks the chunk's two 32-sample halves in turn, wave m = copy m (M = 3: the fourth wave only keeps
//               the barriers company);
//   M = 2       waves (0, 1) take half 0 and waves (2, 3) half 1 at the same time.
// Process noise: lane group g draws Philox block g of the stream (its own four state rows), counter ((t MM + m) ceil(nx/4) + g),
// as ProcNoiseDraw's 12 units per tile behind the 24 layer-1 MFMAs of the FIRST hidden pair of stage 1 -- the one stretch of the
// M = 1 pipeline without VALU work.  The normals wait for the state update at the end of the timestep; lane groups beyond nx
// carry sd = 0.  proc_sd == nullptr: a deterministic model, no draw.
// Cost exchange: multi_cost_slot / multi_total_slot / multi_variance_chunk (mlp_split_multi.hpp), chunks of MULTI_CH timesteps,
// double-buffered, one barrier per chunk; the first 32 lanes of the sample group's first wave finish cost, pert and minimum.
// Visited states: the lane that owns rows 4g..4g+3 of copy m stores them to (M,K,T,nx) behind a wave-uniform branch.
// Rows come from memory only (MPPI_NOISE_TNK4, MPPI_NOISE_ACTIONS), read component-wise, under a DIAGONAL Sigma only: the action
// cost table is one product per element.  A full Sigma (coloured rows or KMPPI's raw actions alike) keeps the callback loop.
// TWIN: dm_interleave, the plane packing, the slot lambdas and act_unit restate rollout_mlp_deep.hip (whose unit is left as it
// was measured): a fix to the pipeline there is a fix here, too (to be shared through a header).
#include <hip/hip_ext.h>
#include <atomic>
#include "actions.hpp"
#include "dispatch.hpp"
#include "mlp_deep.hpp"
#include "mlp_deep_multi.hpp"
#include "mlp_split_ops.hpp"

namespace mppi {
using namespace split_ops;

namespace {
constexpr int DM_NT = 2;               // sample tiles (of 16) per wave
constexpr int DM_VPU = 2;              // hidden activations per VALU unit of the software pipeline
constexpr int DM_THREADS = 256;        // 4 waves = one per SIMD = one per rollout copy
constexpr int DM_CHUNK = 64;           // samples per workgroup chunk = one block_min slot
static_assert(DM_NT * 16 == MULTI_SAMPLES && DM_THREADS / WAVE == PROCESS_NOISE_MM, "one wave per copy, two tiles per wave");

// NS MFMA slots, each followed by its share of NUN VALU units spread evenly over the first SPAN slots (SPAN = 0: all of them in
// front).  sched_barrier(0) after every slot keeps hipcc's scheduler from re-clustering the slots.
template <int NS, int SPAN, int NUN, class FS, class FU>
__device__ __forceinline__ void dm_interleave(FS&& slot, FU&& unit) {
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
__global__ void __launch_bounds__(DM_THREADS, 1) rollout_mlp_deep_multi_kernel(const KArgs<float> a) {
  static_assert(HT % 2 == 0, "a k-step of the 16-bit layers consumes hidden tiles in pairs");
  static_assert(NX >= 1 && NX <= 16 && NU >= 1 && NU <= 8, "one 16-state output tile, controls and bias in the layer-1 k-step");
  static_assert(NOISE == MPPI_NOISE_TNK4 || NOISE == MPPI_NOISE_ACTIONS, "rows from memory, read component-wise");
  constexpr int NC = NU > 4 ? 2 : 1, BIAS_E = 4 + NC, NI = NX + NU, NXB = (NX + 3) / 4;
  constexpr int NT = DM_NT, H = HT * 16, HP = HT / 2, MM = PROCESS_NOISE_MM, CH = MULTI_CH;
  stamp_entry(a.tstamp);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* Ue = reinterpret_cast<float*>(smem_raw);            // [J]
  float* Um = Ue + a.J;                                      // [J]
  float* G = Um + a.J;                                       // [J]
  float* bias2 = Ue + deep_multi_table_floats(a.J);          // [H]
  u32x4* A2s = reinterpret_cast<u32x4*>(bias2 + H);          // [HT][HP][2][64]
  float* xch = reinterpret_cast<float*>(A2s + HT * HP * 2 * WAVE);   // [MULTI_XCHG_FLOATS] the copies' step costs and totals
  float* red = xch + MULTI_XCHG_FLOATS;                      // [2] the minima of the chunk's two halves

  // (the wave index as a scalar: copy, sample half and the `mine` / `lead` branches below are wave-uniform)
  const int lane = threadIdx.x & (WAVE - 1), wv = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int g = lane >> 4, s = lane & 15;
  const int M = a.M;
  const bool pairs = M == 2;                        // two sample groups of two copy-waves | one group of up to four
  const int m = pairs ? (wv & 1) : wv;              // this wave's copy
  const int slot0 = pairs ? (wv & 2) : 0;           // first exchange slot of this wave's sample group
  const bool mine = m < M, lead = wv == slot0;
  const int npass = pairs ? 1 : 2;

  // ---- parameters (mlp_deep.hpp): W1 (H,nx+nu) | b1 (H) | W2T (H,H) | b2 (H) | W3T (H,nx) | b3 (nx) | res_scale | qx | qu ----
  const float* __restrict__ W1 = a.mp;
  const float* __restrict__ b1 = W1 + H * NI;
  const float* __restrict__ W2T = b1 + H;
  const float* __restrict__ b2 = W2T + H * H;
  const float* __restrict__ W3T = b2 + H;
  const float* __restrict__ b3 = W3T + NX * H;
  const float rs = b3[NX];
  const bool noisy = a.proc_sd != nullptr;
  float qx4[4], sd4[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    qx4[r] = 4 * g + r < NX ? b3[NX + 1 + 4 * g + r] : 0.f;
    sd4[r] = (noisy && 4 * g + r < NX) ? a.proc_sd[4 * g + r] : 0.f;
  }
  bool own[NC];
  float qu_c[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    own[c] = g + 4 * c < NU;
    qu_c[c] = own[c] ? b3[NX + 1 + NX + g + 4 * c] : 0.f;
  }

  // ---- hidden-layer planes into LDS: fragment f = mt HP + j of output tile mt, k-step j; the four waves share the work ----
  for (int f = wv; f < HT * HP; f += DM_THREADS / WAVE) {
    const int mt = f / HP, j = f % HP;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (-2.0f * EXP2_SCALE) * W2T[(16 * (2 * j + (e >> 2)) + 4 * g + (e & 3)) * H + 16 * mt + s];
    const PlanesH p = split_pack8_h(v);
    A2s[(f * 2 + 0) * WAVE + lane] = p.h;
    A2s[(f * 2 + 1) * WAVE + lane] = p.m;
  }
  // ... and its bias 2 log2(e) (b2 + rowsum W2): the "1" of tanh = 1 - 2 r.  One unit per thread, summed in fp64
  for (int u = threadIdx.x; u < H; u += DM_THREADS) {
    double sum = (double)b2[u];
    for (int k = 0; k < H; ++k) sum += (double)W2T[k * H + u];
    bias2[u] = (float)((double)EXP2_SCALE * sum);
  }

  // ---- layer-1 and output-layer planes: resident in the accumulation registers, every copy-wave its own ----
  Planes A1[HT];
#pragma unroll
  for (int mt = 0; mt < HT; ++mt) {
    const float* __restrict__ row = W1 + (16 * mt + s) * NI;       // hidden unit 16 mt + s
    float v[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = 4 * g + e < NX ? EXP2_SCALE * row[4 * g + e] : 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) v[4 + c] = own[c] ? EXP2_SCALE * row[NX + g + 4 * c] : 0.f;
    v[BIAS_E] = g == 0 ? EXP2_SCALE * b1[16 * mt + s] : 0.f;        // bias column (B1 holds 1 there)
#pragma unroll
    for (int e = BIAS_E + 1; e < 8; ++e) v[e] = 0.f;
    A1[mt] = split_pack8(v);
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
  for (int mt = 0; mt < HT; ++mt) {
    asm volatile("" : "+a"(A1[mt].h));
    asm volatile("" : "+a"(A1[mt].m));
    asm volatile("" : "+a"(A1[mt].l));
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
  for (int j = threadIdx.x; j < a.J; j += DM_THREADS) Ue[j] = u_base(a, j);
  __syncthreads();                                   // (the hidden layer's planes and bias are complete behind this barrier, too)
  for (int j = threadIdx.x; j < a.J; j += DM_THREADS) {
    const int n = j % NU;
    const float uj = Ue[j];
    Um[j] = uj + a.mu[n];
    G[j] = a.lambda_ * ((smppi ? u_eff(a, j) : uj) * a.sinv[n * NU + n]);     // (diagonal Sigma: launch_dm)
  }
  __syncthreads();
  float sd_c[NC], lo_c[NC], hi_c[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int n = own[c] ? g + 4 * c : 0;
    sd_c[c] = a.L[n * NU + n];
    lo_c[c] = a.umin[n];
    hi_c[c] = a.umax[n];
  }
  const unsigned long long pn_seed = a.seed, pn_call = a.call;
  const bool seven = a.seven != 0;
  const bool keep_states = a.states != nullptr;
  const float inv_M = 1.0f / (float)M;

  // ---- persistent over 64-sample chunks: the weights are laid out once per workgroup (LDS) and wave (AGPRs) ----
  const int nchunks = (a.K + DM_CHUNK - 1) / DM_CHUNK;
  for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    for (int pass = 0; pass < npass; ++pass) {
      const int half = pairs ? (wv >> 1) : pass;
      const int kbase = chunk * DM_CHUNK + half * MULTI_SAMPLES;
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
      if (mine) fetch(0, zn);

      for (int t = 0; t < a.Tn; ++t) {
        if (mine) {
          // this lane's element of every hidden-layer plane; opaque per timestep, so that the reads of a timestep stay where the
          // slot pipeline below puts them (they are loop-invariant: hoisted, they would be 256 registers at H = 128)
          int a2_lane = lane, b2_lane = 4 * g;
          asm volatile("" : "+v"(a2_lane));
          asm volatile("" : "+v"(b2_lane));
          auto lds_plane = [&](int mt, int j, int which) -> u32x4 { return A2s[((mt * HP + j) * 2 + which) * WAVE + a2_lane]; };
          auto lds_bias = [&](int mt) -> f32x4 { return *reinterpret_cast<const f32x4*>(bias2 + 16 * mt + b2_lane); };
          // hidden-layer planes in flight.  Step n = p HP + j (pair p of output tiles, k-step j): hi [n & 1][tile of the pair],
          // read at the first slot of step n - 1; residual [tile of the pair], read at the first slot of its own step
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
              if constexpr (NOISE == MPPI_NOISE_ACTIONS) v = zc[i][c];
              else v = fmaf(zc[i][c], sd_c[c], Umt[c]);
              if (orow[i] == -1) v = 0.f;
              else if (orow[i] >= 0) v = a.sampler[((long long)orow[i] * a.Tn + t) * NU + (own[c] ? g + 4 * c : 0)];
              v = clampT(v, lo_c[c], hi_c[c]);
              if (NU != 4 && NU != 8) v = own[c] ? v : 0.f;                           // a lane group without a control of its own
              const float e = (v - Ut[c]) * ac.e_scale;                               // e_scale = 1 | 1/dt (SMPPI)
              ppart[i] = fmaf(Gt[c], ac.abs_cost ? fabsf(e) : e, ppart[i]);
              if (a.smooth_w != 0.f) {
                // SMPPI smoothness cost w |v[t] - v[t-1]|^2: of the action sequence, not of a copy -- its own sum
                const float d = v - vprev[i][c];
                if (t > 0) spart[i] = fmaf(a.smooth_w * d, d, spart[i]);
                vprev[i][c] = v;
              }
              uu[c] = a.u_scale * v;
              cstep[i] = fmaf(qu_c[c] * uu[c], uu[c], cstep[i]);                      // control effort (qu = 0: + 0)
            }
            float in0[8] = {x[i][0], x[i][1], x[i][2], x[i][3], uu[0], 0.f, 0.f, 0.f};
            if constexpr (NC == 2) in0[5] = uu[1];
            in0[BIAS_E] = g == 0 ? 1.0f : 0.0f;
            B1[i] = split_pack8(in0);
            asm volatile("" : "+a"(B1[i].h));
            asm volatile("" : "+a"(B1[i].m));
            asm volatile("" : "+a"(B1[i].l));
          }

          // ---- the three layers as the software pipeline of rollout_mlp_deep.hip (see there for the slot decoding) ----
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
            constexpr int pr = slot >> 2, q = (slot >> 1) & 1, i = slot & 1, bf = p & 1;
            Hc[bf][q][i] = mfma_bf(plane(A1[2 * p + q], plane_a(pr)), plane(B1[i], plane_b(pr)), pr == 0 ? zero4 : Hc[bf][q][i]);
          };
          auto hidden_slot = [&](auto p_c, auto slot_c) {              // slot 0..12 HP - 1 of output-tile pair p
            constexpr int p = decltype(p_c)::value, slot = decltype(slot_c)::value;
            constexpr int j = slot / 12, w = slot % 12, pr = w >> 2, q = (w >> 1) & 1, i = w & 1, bf = p & 1, n = p * HP + j;
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
            if constexpr (pr == 0) Ab[bf][q][i] = mfma_h(Wh[n & 1][q], R1[j][i].m, j == 0 ? bias[q] : Ab[bf][q][i]);
            else if constexpr (pr == 1) Ab[bf][q][i] = mfma_h(Wh[n & 1][q], R1[j][i].h, Ab[bf][q][i]);
            else As[bf][q][i] = mfma_h(Wm[q], R1[j][i].h, j == 0 ? zero4 : As[bf][q][i]);
          };
          auto output_slot = [&](auto jc_c, auto slot_c) {             // slot 0..5 of k-step jc
            constexpr int jc = decltype(jc_c)::value, slot = decltype(slot_c)::value;
            constexpr int pr = slot >> 1, i = slot & 1, bf = jc & 1;
            if constexpr (pr == 0) Ob[i] = mfma_h(A3[jc].h, R2[bf][i].m, jc == 0 ? zero4 : Ob[i]);
            else if constexpr (pr == 1) Ob[i] = mfma_h(A3[jc].h, R2[bf][i].h, Ob[i]);
            else Os[i] = mfma_h(A3[jc].m, R2[bf][i].h, jc == 0 ? zero4 : Os[i]);
          };
          // activation work of a pair's 16 hidden values per lane, in units of VPU values x 2 phases
          // (phase 0: r = 1/(2^h + 1); phase 1: fp16 split + pack).  LAYER 1: Hc of pair idx -> R1[idx] (then pinned in AGPRs);
          // LAYER 2: Ab + 2^-11 As of pair idx -> R2[idx & 1]
          constexpr int VPU = DM_VPU, NUNIT = 2 * (16 / VPU);
          float minus_one = -1.0f;
          asm volatile("" : "+v"(minus_one));
          auto act_unit = [&](auto layer_c, auto idx_c, auto unit_c) {
            constexpr int layer = decltype(layer_c)::value, idx = decltype(idx_c)::value, unit = decltype(unit_c)::value;
            constexpr int grp = unit >> 1, phase = unit & 1, bf = idx & 1;
            constexpr int v0 = grp * VPU;                              // first of the unit's values: v = 8 i + e
            if constexpr (phase == 0) {
#pragma unroll
              for (int v = v0; v < v0 + VPU; ++v) {
                const int i = v >> 3, e = v & 7;
                if constexpr (layer == 1) rr[i][e] = sigm2(Hc[bf][e >> 2][i][e & 3]);
                else rr[i][e] = sigm2(__builtin_fmaf(As[bf][e >> 2][i][e & 3], MID_UNSCALE, Ab[bf][e >> 2][i][e & 3]));
              }
            } else {
#pragma unroll
              for (int v = v0; v < v0 + VPU; v += 2) {
                const int i = v >> 3, e0 = v & 7, q = e0 >> 1;
                unsigned hp, mp;
                split_pair_h(rr[i][e0], rr[i][e0 + 1], minus_one, hp, mp);
                if constexpr (layer == 1) { R1[idx][i].h[q] = hp; R1[idx][i].m[q] = mp; }
                else { R2[bf][i].h[q] = hp; R2[bf][i].m[q] = mp; }
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
          // stage 1: layer 1.  Behind the 24 MFMAs of the first pair this timestep's process-noise draw: unit (slot >> 1) of
          // tile (slot & 1); between the MFMAs of pair p >= 1 the activations of pair p - 1
          float wn[NT][4];
          ProcNoiseDraw draw[NT];
          static_assert(2 * ProcNoiseDraw::UNITS == 24, "one draw unit per layer-1 slot of the first pair");
          static_for<0, 24>([&](auto sc) {
            constexpr int sl = decltype(sc)::value;
            layer1_slot(ic<0>{}, sc);
            if (noisy) {
              constexpr int i = sl & 1;
              draw[i].template unit<(sl >> 1)>(pn_seed, pn_call, a.k_offset + kk[i], ((long long)t * MM + m) * NXB + g, seven, wn[i]);
            }
            __builtin_amdgcn_sched_barrier(0);
          });
          static_for<1, HP>([&](auto pc) {
            constexpr int p = decltype(pc)::value;
            dm_interleave<24, 24, NUNIT>([&](auto sc) { layer1_slot(pc, sc); }, [&](auto uc) { act_unit(ic<1>{}, ic<p - 1>{}, uc); });
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
            if constexpr (p == 0) dm_interleave<N, 12 * (HP - 1), NUNIT>(slot, [&](auto uc) { act_unit(ic<1>{}, ic<HP - 1>{}, uc); });
            else dm_interleave<N, N, NUNIT>(slot, [&](auto uc) { act_unit(ic<2>{}, ic<(p >= 1 ? p - 1 : 0)>{}, uc); });
          });
          // tail: the activations of the last pair, the output layer's last two k-steps
          dm_interleave<(HP >= 2 ? 6 : 0), (HP >= 2 ? 6 : 0), NUNIT>(
              [&](auto sc) { output_slot(ic<(HP >= 2 ? HP - 2 : 0)>{}, sc); }, [&](auto uc) { act_unit(ic<2>{}, ic<HP - 1>{}, uc); });
          dm_interleave<6, 0, 0>([&](auto sc) { output_slot(ic<HP - 1>{}, sc); }, [&](auto) {});

          // ---- state update, process noise, this copy's step cost (and its visited state) ----
#pragma unroll
          for (int i = 0; i < NT; ++i) {
            const f32x4 O = Ob[i] + MID_UNSCALE * Os[i];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              x[i][r] = fmaf(rs, O[r] + b3r[r], x[i][r]);
              if (noisy) x[i][r] = fmaf(sd4[r], wn[i][r], x[i][r]);
              cstep[i] = fmaf(qx4[r] * x[i][r], x[i][r], cstep[i]);
            }
            float c = cstep[i];
            c += __shfl_xor(c, 16, WAVE);
            c += __shfl_xor(c, 32, WAVE);
            cs[i] += c;
            if (g == 0) multi_cost_slot(xch, buf, t - t_done, wv, 16 * i + s) = c;
          }
          if (keep_states) {
#pragma unroll
            for (int i = 0; i < NT; ++i) {
              float* __restrict__ row = a.states + (((long long)m * a.K + kk[i]) * a.Tn + t) * NX + 4 * g;
              if constexpr (NX % 4 == 0) {
                if (act[i] && 4 * g < NX) *reinterpret_cast<f32x4*>(row) = f32x4{x[i][0], x[i][1], x[i][2], x[i][3]};
              } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                  if (act[i] && 4 * g + r < NX) row[r] = x[i][r];
              }
            }
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
static int launch_dm(const KArgs<float>& a_in, hipStream_t st) {
  KArgs<float> a = a_in;
  // the rows are read component-wise and the action cost is one product per element: external rows (TNK4 / raw actions) under a
  // diagonal Sigma only
  if (!(a.noise_src == MPPI_NOISE_TNK4 || a.noise_src == MPPI_NOISE_ACTIONS)) return MPPI_E_UNSUPPORTED;
  if (a.diag == 0 || a.coloured != 0) return MPPI_E_UNSUPPORTED;
  const size_t smem = deep_multi_lds_bytes(a.J, HT * 16);
  const int nchunks = (a.K + DM_CHUNK - 1) / DM_CHUNK;
  static const int n_cu = [] {
    int dev = 0, n = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    return n > 0 ? n : 256;
  }();
  const dim3 grid(nchunks < n_cu ? nchunks : n_cu), block(DM_THREADS);      // one workgroup per CU, persistent over its chunks
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  profile_next_events(&ev0, &ev1, &a.tstamp);
#define MPPI_LAUNCH1(KERNEL)                                                                                   \
  do {                                                                                                         \
    if (smem > 64 * 1024) (void)hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem); \
    if (ev1 != nullptr) hipExtLaunchKernelGGL(KERNEL, grid, block, smem, st, ev0, ev1, 0, a);                  \
    else hipLaunchKernelGGL(KERNEL, grid, block, smem, st, a);                                                 \
  } while (0)
  if (a.noise_src == MPPI_NOISE_ACTIONS) MPPI_LAUNCH1((rollout_mlp_deep_multi_kernel<HT, MPPI_NOISE_ACTIONS, NX, NU>));
  else MPPI_LAUNCH1((rollout_mlp_deep_multi_kernel<HT, MPPI_NOISE_TNK4, NX, NU>));
#undef MPPI_LAUNCH1
  return (int)hipGetLastError();
}

// The (nx, nu) pairs of the M = 1 kernel (rollout_mlp_deep.hip MPPI_DEEP_DIMS), one translation unit each
// (MPPI_DEEP_MULTI_GROUP, set by _build.py; chained like rollout_mlp2.hip)
#ifndef MPPI_DEEP_MULTI_GROUP
#define MPPI_DEEP_MULTI_GROUP 0
#endif
#define MPPI_DEEP_MULTI_DIMS_0(X) X(16, 4)
#define MPPI_DEEP_MULTI_DIMS_1(X) X(12, 6)
#define MPPI_DEEP_MULTI_DIMS_2(X) X(2, 1)

template <int NX, int NU>
static int launch_dm_h(const KArgs<float>& a, hipStream_t st) {
  if (a.hidden == 32) return launch_dm<2, NX, NU>(a, st);
  if (a.hidden == 64) return launch_dm<4, NX, NU>(a, st);
  return launch_dm<8, NX, NU>(a, st);
}

int rollout_mlp_deep_multi_g1(const KArgs<float>& a, hipStream_t st);
int rollout_mlp_deep_multi_g2(const KArgs<float>& a, hipStream_t st);

#if MPPI_DEEP_MULTI_GROUP == 0
bool mlp_deep_multi_supported(int nx, int nu, int hidden, int M, int T, int n_env) {
  if (!mlp_deep_supported(nx, nu, hidden) || M < 2 || M > PROCESS_NOISE_MM || T < 1 || n_env > 1) return false;
  if ((long long)T * nu > (1 << 20)) return false;
  return deep_multi_lds_bytes(T * nu, hidden) <= DEEP_MULTI_LDS_MAX;
}

static std::atomic<long long> g_deep_multi_launches{0};

int rollout_mlp_deep_multi(const KArgs<float>& a, hipStream_t st) {
  if (a.mp == nullptr) return MPPI_E_BADARG;
  if (!mlp_deep_multi_supported(a.nx, a.nu, a.hidden, a.M, a.Tn, a.n_env) || a.W != nullptr) return MPPI_E_UNSUPPORTED;
  int r;
#define X(NX, NU) if (a.nx == NX && a.nu == NU) r = launch_dm_h<NX, NU>(a, st); else
  MPPI_DEEP_MULTI_DIMS_0(X)
#undef X
  r = rollout_mlp_deep_multi_g1(a, st);
  if (r == 0) ++g_deep_multi_launches;
  return r;
}
}  // namespace mppi

extern "C" int mppi_mlp_deep_multi_supported(int32_t nx, int32_t nu, int32_t hidden, int32_t M, int32_t T, int32_t num_envs) {
  return mppi::mlp_deep_multi_supported(nx, nu, hidden, M, T, num_envs) ? 1 : 0;
}
extern "C" int64_t mppi_stat_mlp_deep_multi_launches(void) { return (int64_t)mppi::g_deep_multi_launches.load(); }
#elif MPPI_DEEP_MULTI_GROUP == 1
int rollout_mlp_deep_multi_g1(const KArgs<float>& a, hipStream_t st) {
#define X(NX, NU) if (a.nx == NX && a.nu == NU) return launch_dm_h<NX, NU>(a, st);
  MPPI_DEEP_MULTI_DIMS_1(X)
#undef X
  return rollout_mlp_deep_multi_g2(a, st);
}
}  // namespace mppi
#else
int rollout_mlp_deep_multi_g2(const KArgs<float>& a, hipStream_t st) {
#define X(NX, NU) if (a.nx == NX && a.nu == NU) return launch_dm_h<NX, NU>(a, st);
  MPPI_DEEP_MULTI_DIMS_2(X)
#undef X
  return MPPI_E_UNSUPPORTED;
}
}  // namespace mppi
#endif
