// K1 for the 2-layer MLP residual model with 16 < nx <= 32 states (nu <= 8), process noise and M = 2..4 state rollouts per
// action sequence (rollout_samples, mppi.py:334-373) on the 16-bit matrix cores.
//
//   x' = x + s * (W2 tanh(W1 [x;u] + b1) + b2) + sd (.) n,   c_m(t) = sum qx x^2 + sum qu u^2   on the noisy state
//   total = mean_m sum_t c_m(t) + var_cost sum_t var_disc^t var_m(c_m(t)) + smoothness (once) + action cost (once)
// -- the quantities, conventions and process-noise counters of rollout_stream_multi (rollout.hpp) and of
// rollout_mlp_split_multi_kernel.  The model's per-lane form has no M > 1 instantiation beyond 16 states (rollout_mlp.hip
// MlpModelRolled), so this kernel is the only HIP form of such a command: it also serves the visited states.
//
// Arithmetic, operand layout and slot pipeline are rollout_mlp_split32.hip's, see there: layer 1 bf16 x 3 (six piece products)
// over two 32-slot k-steps fed from the accumulators of the same lane, layer 2 fp16 x 2 (three products) into two 16-state output
// tiles, tile o = rows 16 o + 4g + r at lane (g, s); the layer-1 planes in LDS as [hidden tile][k-step][plane][lane] 16-byte
// elements, read one product ahead; the layer-2 planes and the timestep's layer-1 B operand pinned in AGPRs; no lane permutes.
// Work split (rollout_mlp_split_multi.hip): ONE WAVE PER ROLLOUT COPY, the four waves of a workgroup roll different copies of
// the same 32 samples.  A chunk is 64 consecutive samples (one block_min slot):
//   M = 3 | 4   the workgroup walks the chunk's two 32-sample halves in turn, wave m = copy m (M = 3: the fourth wave only keeps
//               the barriers company);
//   M = 2       waves (0, 1) take half 0 and waves (2, 3) half 1 at the same time.
// ONE copy of the layer-1 planes serves the four copy-waves (96 KB at H = 256: what makes a wave per copy affordable at this
// size); every wave pins its own layer-2 planes.
// Process noise.  Row 16 o + 4g + r lies in Philox block 4 o + g of the stream, so lane group g draws TWO blocks per sample tile
// and timestep, counter ((t MM + m) ceil(nx/4) + 4 o + g): four ProcNoiseDraw streams of 12 units (mlp_split_multi.hpp) = 48 units,
// one behind each of the 48 matrix instructions of layer 1 of the FIRST hidden pair, where the M = 1 pipeline has no VALU work.
// The two sample tiles' streams of one output tile run interleaved (two draw states alive), the output tiles one after the
// other; the 16 normals wait for the state update at the end of the timestep.  A block beyond the model's nx (24 states: tile 1,
// lane groups 2 and 3) carries sd = 0: x stays 0 there.  proc_sd == nullptr: a deterministic model, no draw.
// Cost exchange: the lane's partial (both output tiles' state rows + its control-effort terms) summed over the four lane groups,
// then multi_cost_slot / multi_total_slot / multi_variance_chunk (mlp_split_multi.hpp): chunks of MULTI_CH timesteps,
// double-buffered, one barrier per chunk; the first 32 lanes of the sample group's first wave finish cost, pert and minimum.
// Visited states: the lane that owns rows 16 o + 4g .. + 3 of copy m stores them to (M,K,T,nx) behind a wave-uniform branch.
// Rows come from memory only (MPPI_NOISE_TNK4, MPPI_NOISE_ACTIONS), read component-wise, under a DIAGONAL Sigma (generator-
// coloured rows included): the action cost table is one product per element.
// TWIN: the plane packing, the slot lambdas and valu_unit restate rollout_mlp_split32.hip (whose unit is left as it was measured):
// a fix to the pipeline there is a fix here, too.
#include <hip/hip_ext.h>
#include <atomic>
#include "actions.hpp"
#include "dispatch.hpp"
#include "mlp_split32.hpp"
#include "mlp_split32_multi.hpp"
#include "mlp_split_ops.hpp"

namespace mppi {
using namespace split_ops;

namespace {
constexpr int S32M_NT = 2;             // sample tiles (of 16) per wave
constexpr int S32M_VPU = 2;            // hidden activations per VALU unit of the software pipeline
constexpr int S32M_THREADS = 256;      // 4 waves = one per SIMD = one per rollout copy
constexpr int S32M_CHUNK = 64;         // samples per workgroup chunk = one block_min slot
static_assert(S32M_NT * 16 == MULTI_SAMPLES && S32M_THREADS / WAVE == PROCESS_NOISE_MM, "one wave per copy, two tiles per wave");
}  // namespace

template <int HT /* hidden / 16 */, int NOISE, int NX, int NU>
__global__ void __launch_bounds__(S32M_THREADS, 1) rollout_mlp_split32_multi_kernel(const KArgs<float> a) {
  static_assert(HT % 2 == 0, "layer 2 consumes hidden tiles in pairs");
  static_assert(NX > 16 && NX <= 32 && NU >= 1 && NU <= 8, "two 16-state output tiles, controls and bias in k-step 0");
  static_assert(NOISE == MPPI_NOISE_TNK4 || NOISE == MPPI_NOISE_ACTIONS, "rows from memory, read component-wise");
  constexpr int NC = NU > 4 ? 2 : 1, BIAS_E = 4 + NC, NI = NX + NU, NXB = (NX + 3) / 4;
  constexpr int NT = S32M_NT, H = HT * 16, HP = HT / 2, MM = PROCESS_NOISE_MM, CH = MULTI_CH;
  stamp_entry(a.tstamp);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* Ue = reinterpret_cast<float*>(smem_raw);   // [J]
  float* Um = Ue + a.J;                             // [J]
  float* G = Um + a.J;                              // [J]
  u32x4* A1s = reinterpret_cast<u32x4*>(Ue + split32_multi_table_floats(a.J));   // [HT][2][3][64]
  float* xch = reinterpret_cast<float*>(A1s + HT * 2 * 3 * WAVE);                // [MULTI_XCHG_FLOATS] the copies' step costs and totals
  float* red = xch + MULTI_XCHG_FLOATS;                                          // [2] the minima of the chunk's two halves

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
  const bool noisy = a.proc_sd != nullptr;
  float qx4[2][4], sd4[2][4];
#pragma unroll
  for (int o = 0; o < 2; ++o) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * o + 4 * g + r;
      qx4[o][r] = row < NX ? b2[NX + 1 + row] : 0.f;
      sd4[o][r] = (noisy && row < NX) ? a.proc_sd[row] : 0.f;
    }
  }
  bool own[NC];
  float qu_c[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    own[c] = g + 4 * c < NU;
    qu_c[c] = own[c] ? b2[NX + 1 + NX + g + 4 * c] : 0.f;
  }

  // ---- layer-1 planes into LDS, one copy for the four copy-waves: fragment f = 2 mt + o of hidden tile mt, k-step o ----
  for (int f = wv; f < 2 * HT; f += S32M_THREADS / WAVE) {
    const int mt = f >> 1, o = f & 1;
    const float* __restrict__ row = W1 + (16 * mt + s) * NI;       // hidden unit 16 mt + s
    float v[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = 16 * o + 4 * g + e < NX ? EXP2_SCALE * row[16 * o + 4 * g + e] : 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) v[4 + c] = (o == 0 && own[c]) ? EXP2_SCALE * row[NX + g + 4 * c] : 0.f;
    v[BIAS_E] = (o == 0 && g == 0) ? EXP2_SCALE * b1[16 * mt + s] : 0.f;   // bias column (B1 holds 1 there)
#pragma unroll
    for (int e = BIAS_E + 1; e < 8; ++e) v[e] = 0.f;
    const Planes p = split_pack8(v);
    A1s[(f * 3 + 0) * WAVE + lane] = p.h;
    A1s[(f * 3 + 1) * WAVE + lane] = p.m;
    A1s[(f * 3 + 2) * WAVE + lane] = p.l;
  }

  // ---- layer-2 planes: resident in the accumulation registers, every copy-wave its own ----
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
  for (int j = threadIdx.x; j < a.J; j += S32M_THREADS) Ue[j] = u_base(a, j);
  __syncthreads();                                   // (the layer-1 planes are complete behind this barrier, too)
  for (int j = threadIdx.x; j < a.J; j += S32M_THREADS) {
    const int n = j % NU;
    const float uj = Ue[j];
    Um[j] = a.coloured ? uj : uj + a.mu[n];
    G[j] = a.lambda_ * ((smppi ? u_eff(a, j) : uj) * a.sinv[n * NU + n]);     // (diagonal Sigma: launch_s32m)
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
  const unsigned long long pn_seed = a.seed, pn_call = a.call;
  const bool seven = a.seven != 0;
  const bool keep_states = a.states != nullptr;
  const float inv_M = 1.0f / (float)M;

  // ---- persistent over 64-sample chunks: the weights are laid out once per workgroup (LDS) and wave (AGPRs) ----
  const int nchunks = (a.K + S32M_CHUNK - 1) / S32M_CHUNK;
  for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    for (int pass = 0; pass < npass; ++pass) {
      const int half = pairs ? (wv >> 1) : pass;
      const int kbase = chunk * S32M_CHUNK + half * MULTI_SAMPLES;
      int kk[NT], orow[NT];
      bool act[NT];
      float x[NT][2][4], cs[NT], ppart[NT], spart[NT], vprev[NT][NC];
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
          // this lane's element of every layer-1 plane; opaque per timestep, so that the 96 reads of a timestep stay where the
          // slot pipeline below puts them (they are loop-invariant: hoisted, they would be 384 registers)
          int a1_lane = lane;
          asm volatile("" : "+v"(a1_lane));
          auto lds_plane = [&](int mt, int o, int which) -> u32x4 { return A1s[((2 * mt + o) * 3 + which) * WAVE + a1_lane]; };
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
          fetch(t + 1 < a.Tn ? t + 1 : t, zn);   // prefetch the next step's rows

          // ---- actions (as in the M = 1 kernel): lane (g,s) owns control dimension g (and g + 4 where nu > 4); every copy-wave
          // makes them for itself ----
          float Ut[NC], Umt[NC], Gt[NC], cstep[NT];
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            const int jn = t * NU + (own[c] ? g + 4 * c : 0);
            Ut[c] = Ue[jn]; Umt[c] = Um[jn]; Gt[c] = own[c] ? G[jn] : 0.f;
          }
          Planes B1[NT][2];
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

          // ---- the two layers as the software pipeline of rollout_mlp_split32.hip (see there for the slot decoding, the cycle
          // budget and the two rules: no dependent MFMAs back to back; pair j's activation work between the MFMAs of A(j+1) and
          // C(j-1); the layer-1 planes of a pair from LDS at the product boundaries) ----
          f32x4 Os[2][NT], Om[2][NT], Ob[2][NT];   // [output tile][sample tile]
          f32x4 Hc[2][2][NT];                      // [buffer][hidden tile of the pair][sample tile]
          float rr[NT][8];                         // r = 1/(2^h+1) of the pair's 8 hidden units per lane
          PlanesH B2[2][NT];                       // [buffer][sample tile]: fp16 hi | fp16 residual
          const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
          static_assert(NT == 2, "slot decoding assumes two sample tiles per wave");
          auto layer1_slot = [&](auto jn_c, auto slot_c) {             // slot 0..47 of pair jn: A(jn)
            constexpr int jn = decltype(jn_c)::value, slot = decltype(slot_c)::value;
            constexpr int pr = slot >> 3, o = (slot >> 2) & 1, q = (slot >> 1) & 1, i = slot & 1, bf = jn & 1;
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
            Hc[bf][q][i] = mfma_bf(wa, plane(B1[i][o], plane_b(pr)), (pr == 0 && o == 0) ? zero4 : Hc[bf][q][i]);
          };
          auto layer2_slot = [&](auto jc_c, auto slot_c) {             // slot 0..11 of k-step jc: C(jc)
            constexpr int jc = decltype(jc_c)::value, slot = decltype(slot_c)::value;
            constexpr int pr = slot >> 2, o = (slot >> 1) & 1, i = slot & 1, bf = jc & 1;
            if constexpr (pr == 0) Ob[o][i] = mfma_h(A2[o][jc].h, B2[bf][i].h, jc == 0 ? zero4 : Ob[o][i]);
            else if constexpr (pr == 1) Om[o][i] = mfma_h(A2[o][jc].h, B2[bf][i].m, jc == 0 ? zero4 : Om[o][i]);
            else Os[o][i] = mfma_h(A2[o][jc].m, B2[bf][i].h, jc == 0 ? zero4 : Os[o][i]);
          };
          // B(j) = activation work of the pair's 16 hidden values per lane, in units of VPU values x 2 phases
          // (phase 0: r = 1/(2^h + 1); phase 1: fp16 split + pack)
          constexpr int VPU = S32M_VPU, NUNIT = 2 * (16 / VPU);
          float minus_one = -1.0f;
          asm volatile("" : "+v"(minus_one));
          auto valu_unit = [&](auto j_c, auto unit_c) {
            constexpr int j = decltype(j_c)::value, unit = decltype(unit_c)::value;
            constexpr int grp = unit >> 1, phase = unit & 1, bf = j & 1;
            constexpr int v0 = grp * VPU;                              // first of the unit's values: v = 8 i + e
            if constexpr (phase == 0) {
#pragma unroll
              for (int v = v0; v < v0 + VPU; ++v) {
                const int i = v >> 3, e = v & 7;
                rr[i][e] = sigm2(Hc[bf][e >> 2][i][e & 3]);
              }
            } else {
#pragma unroll
              for (int v = v0; v < v0 + VPU; v += 2) {
                const int i = v >> 3, e0 = v & 7, q = e0 >> 1;
                unsigned hp, mp;
                split_pair_h(rr[i][e0], rr[i][e0 + 1], minus_one, hp, mp);
                B2[bf][i].h[q] = hp;
                B2[bf][i].m[q] = mp;
              }
            }
          };
          // A(0): layer 1 of the first pair -- and this timestep's process-noise draws.  Slots 0..23 carry Philox block g (output
          // tile 0), slots 24..47 block 4 + g (output tile 1): unit ((slot % 24) >> 1) of sample tile (slot & 1) behind every
          // matrix instruction, the two tiles' dependency chains interleaved
          float wn[NT][2][4];
          ProcNoiseDraw draw[NT];
          static_assert(4 * ProcNoiseDraw::UNITS == 48, "one draw unit per layer-1 slot of the first pair");
          static_for<0, 48>([&](auto sc) {
            constexpr int sl = decltype(sc)::value;
            layer1_slot(std::integral_constant<int, 0>{}, sc);
            if (noisy) {
              constexpr int i = sl & 1, o = sl / 24, unit = (sl % 24) >> 1;
              draw[i].template unit<unit>(pn_seed, pn_call, a.k_offset + kk[i], ((long long)t * MM + m) * NXB + 4 * o + g, seven, wn[i][o]);
            }
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

          // ---- state update, process noise, this copy's step cost (and its visited state) ----
#pragma unroll
          for (int i = 0; i < NT; ++i) {
#pragma unroll
            for (int o = 0; o < 2; ++o) {
              const f32x4 O = (Ob[o][i] + Om[o][i]) + MID_UNSCALE * Os[o][i];
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                x[i][o][r] = fmaf(rs, O[r] + b2r[o][r], x[i][o][r]);
                if (noisy) x[i][o][r] = fmaf(sd4[o][r], wn[i][o][r], x[i][o][r]);
                cstep[i] = fmaf(qx4[o][r] * x[i][o][r], x[i][o][r], cstep[i]);
              }
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
#pragma unroll
              for (int o = 0; o < 2; ++o) {
                float* __restrict__ row = a.states + (((long long)m * a.K + kk[i]) * a.Tn + t) * NX + 16 * o + 4 * g;
                if constexpr (NX % 4 == 0) {
                  if (act[i] && 16 * o + 4 * g < NX) *reinterpret_cast<f32x4*>(row) = f32x4{x[i][o][0], x[i][o][1], x[i][o][2], x[i][o][3]};
                } else {
#pragma unroll
                  for (int r = 0; r < 4; ++r)
                    if (act[i] && 16 * o + 4 * g + r < NX) row[r] = x[i][o][r];
                }
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
static int launch_s32m(const KArgs<float>& a_in, hipStream_t st) {
  KArgs<float> a = a_in;
  // the rows are read component-wise and the action cost is one product per element: external rows (TNK4 / raw actions) under a
  // diagonal Sigma only (generator-coloured rows of a diagonal Sigma included)
  if (!(a.noise_src == MPPI_NOISE_TNK4 || a.noise_src == MPPI_NOISE_ACTIONS)) return MPPI_E_UNSUPPORTED;
  if (a.diag == 0) return MPPI_E_UNSUPPORTED;
  const size_t smem = split32_multi_lds_bytes(a.J, HT * 16);
  const int nchunks = (a.K + S32M_CHUNK - 1) / S32M_CHUNK;
  static const int n_cu = [] {
    int dev = 0, n = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    return n > 0 ? n : 256;
  }();
  const dim3 grid(nchunks < n_cu ? nchunks : n_cu), block(S32M_THREADS);    // one workgroup per CU, persistent over its chunks
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  profile_next_events(&ev0, &ev1, &a.tstamp);
#define MPPI_LAUNCH1(KERNEL)                                                                                   \
  do {                                                                                                         \
    if (smem > 64 * 1024) (void)hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem); \
    if (ev1 != nullptr) hipExtLaunchKernelGGL(KERNEL, grid, block, smem, st, ev0, ev1, 0, a);                  \
    else hipLaunchKernelGGL(KERNEL, grid, block, smem, st, a);                                                 \
  } while (0)
  if (a.noise_src == MPPI_NOISE_ACTIONS) MPPI_LAUNCH1((rollout_mlp_split32_multi_kernel<HT, MPPI_NOISE_ACTIONS, NX, NU>));
  else MPPI_LAUNCH1((rollout_mlp_split32_multi_kernel<HT, MPPI_NOISE_TNK4, NX, NU>));
#undef MPPI_LAUNCH1
  return (int)hipGetLastError();
}

// The (nx, nu) pairs of the M = 1 kernel (rollout_mlp_split32.hip MPPI_SPLIT32_DIMS), one translation unit each
// (MPPI_SPLIT32_MULTI_GROUP, set by _build.py)
#ifndef MPPI_SPLIT32_MULTI_GROUP
#define MPPI_SPLIT32_MULTI_GROUP 0
#endif
#define MPPI_SPLIT32_MULTI_DIMS_0(X) X(32, 8)
#define MPPI_SPLIT32_MULTI_DIMS_1(X) X(24, 6)

template <int NX, int NU>
static int launch_s32m_h(const KArgs<float>& a, hipStream_t st) {
  if (a.hidden == 64) return launch_s32m<4, NX, NU>(a, st);
  if (a.hidden == 128) return launch_s32m<8, NX, NU>(a, st);
  return launch_s32m<16, NX, NU>(a, st);
}

int rollout_mlp_split32_multi_g1(const KArgs<float>& a, hipStream_t st);

#if MPPI_SPLIT32_MULTI_GROUP == 0
bool mlp_split32_multi_supported(int nx, int nu, int hidden, int M, int T, int n_env) {
  if (nx <= 16 || !mlp_split32_supported(nx, nu, hidden) || M < 2 || M > PROCESS_NOISE_MM || T < 1 || n_env > 1) return false;
  if ((long long)T * nu > (1 << 20)) return false;
  return split32_multi_lds_bytes(T * nu, hidden) <= SPLIT32_MULTI_LDS_MAX;
}

static std::atomic<long long> g_split32_multi_launches{0};

int rollout_mlp_split32_multi(const KArgs<float>& a, hipStream_t st) {
  if (a.mp == nullptr) return MPPI_E_BADARG;
  if (!mlp_split32_multi_supported(a.nx, a.nu, a.hidden, a.M, a.Tn, a.n_env) || a.W != nullptr) return MPPI_E_UNSUPPORTED;
  int r;
#define X(NX, NU) if (a.nx == NX && a.nu == NU) r = launch_s32m_h<NX, NU>(a, st); else
  MPPI_SPLIT32_MULTI_DIMS_0(X)
#undef X
  r = rollout_mlp_split32_multi_g1(a, st);
  if (r == 0) ++g_split32_multi_launches;
  return r;
}
}  // namespace mppi

extern "C" int mppi_mlp_split32_multi_supported(int32_t nx, int32_t nu, int32_t hidden, int32_t M, int32_t T, int32_t num_envs) {
  return mppi::mlp_split32_multi_supported(nx, nu, hidden, M, T, num_envs) ? 1 : 0;
}
extern "C" int64_t mppi_stat_mlp_split32_multi_launches(void) { return (int64_t)mppi::g_split32_multi_launches.load(); }
#else
int rollout_mlp_split32_multi_g1(const KArgs<float>& a, hipStream_t st) {
#define X(NX, NU) if (a.nx == NX && a.nu == NU) return launch_s32m_h<NX, NU>(a, st);
  MPPI_SPLIT32_MULTI_DIMS_1(X)
#undef X
  return MPPI_E_UNSUPPORTED;
}
}  // namespace mppi
#endif
