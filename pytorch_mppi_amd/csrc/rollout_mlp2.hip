// K1 instantiations of the residual MLP with two hidden layers (mlp_deep.hpp, models.MLPResidual2): the model's dispatcher and
// its per-lane VALU form -- fp32 and fp64, any rows, visited states, KMPPI, any common hidden width that is a multiple of 32.
// One translation unit per (nx, nu) pair (MPPI_MLP2_GROUP, set by _build.py; chained like rollout_mlp.hip).
#include <cstdlib>
#include "dispatch.hpp"
#include "mlp_deep.hpp"
#include "mlp_deep_multi.hpp"
#include "rollout.hpp"
namespace mppi {
#ifndef MPPI_MLP2_GROUP
#define MPPI_MLP2_GROUP 0
#endif
#define MPPI_MLP2_DIMS_0(X) X(16, 4)
#define MPPI_MLP2_DIMS_1(X) X(12, 6)
#define MPPI_MLP2_DIMS_2(X) X(2, 1)
#if MPPI_MLP2_GROUP == 0
#define MPPI_DIMS MPPI_MLP2_DIMS_0
#define MPPI_THIS rollout_mlp2_valu
#define MPPI_NEXT rollout_mlp2_valu_g1
#elif MPPI_MLP2_GROUP == 1
#define MPPI_DIMS MPPI_MLP2_DIMS_1
#define MPPI_THIS rollout_mlp2_valu_g1
#define MPPI_NEXT rollout_mlp2_valu_g2
#else
#define MPPI_DIMS MPPI_MLP2_DIMS_2
#define MPPI_THIS rollout_mlp2_valu_g2
#endif
#ifdef MPPI_NEXT
int MPPI_NEXT(const KArgs<float>& a, hipStream_t st);
int MPPI_NEXT(const KArgs<double>& a, hipStream_t st);
#endif

// A lane cannot index a hidden vector dynamically without scratch, and 2 x H activations do not fit its registers.  So the second
// hidden layer is produced in blocks of MB units (32 in fp32, 16 in fp64: the registers a lane has) whose pre-activations sit in a compile-time-indexed register array: for each
// block the loop over the layer-1 units k stays ROLLED -- tanh of unit k, then its contribution W2T[k][block] to the MB
// accumulators, fully unrolled -- and the block's tanh goes straight into the (unrolled) output layer.  Layer 1 is evaluated once
// per block (H / MB times per step): the price of holding nothing that is indexed at run time.  The weights are wave-uniform ->
// scalar loads; W2 is stored transposed in the blob so that a block's row is contiguous.
template <typename T, int NX_, int NU_>
struct Mlp2Model {
  static constexpr int NX = NX_, NU = NU_, NI = NX_ + NU_;
  static constexpr int MB = sizeof(T) == 4 ? 32 : 16;   // accumulators per block: layer 1 is evaluated H / MB times per step
  static constexpr bool NO_KMPPI_FUSE = true;
  // one rolled copy of the step, one state rollout per action sequence (rollout.hpp model_heavy): the unrolled streams and the
  // multi-rollout instantiations spill (40 VGPRs and 164 B of scratch at (16, 4)), so they are not built: rollout_samples > 1
  // is the matrix-core kernel's alone (rollout_mlp_deep_multi.hip), else the callback loop (models.MLPResidual2.heavy)
  static constexpr bool HEAVY = true;
  // (one base pointer and offsets worked out where they are used: eight resident pointers cost the scalar registers the rollout
  //  streams of rollout.hpp need for their own tables)
  const T* __restrict__ mp;
  int H;
  __device__ explicit Mlp2Model(const KArgs<T>& a) : mp(a.mp), H(a.hidden) {}
  __device__ __forceinline__ void step(T (&x)[NX], const T (&u)[NU], int) const {
    const T* __restrict__ W1 = mp;
    const T* __restrict__ b1 = W1 + (long long)H * NI;
    const T* __restrict__ W2T = b1 + H;
    const T* __restrict__ b2 = W2T + (long long)H * H;
    const T* __restrict__ W3T = b2 + H;
    const T* __restrict__ b3 = W3T + (long long)NX * H;
    T o[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) o[i] = b3[i];
#pragma clang loop unroll(disable)
    for (int mb = 0; mb < H; mb += MB) {
      T acc[MB];
#pragma unroll
      for (int m = 0; m < MB; ++m) acc[m] = b2[mb + m];
#pragma clang loop unroll(disable)
      for (int k = 0; k < H; ++k) {
        const T* __restrict__ w = W1 + (long long)k * NI;
        T h1 = b1[k];
#pragma unroll
        for (int i = 0; i < NX; ++i) h1 = m_fma(x[i], w[i], h1);
#pragma unroll
        for (int n = 0; n < NU; ++n) h1 = m_fma(u[n], w[NX + n], h1);
        const T th = m_tanh(h1);
        const T* __restrict__ w2 = W2T + (long long)k * H + mb;
#pragma unroll
        for (int m = 0; m < MB; ++m) acc[m] = m_fma(th, w2[m], acc[m]);
      }
#pragma unroll
      for (int m = 0; m < MB; ++m) {
        const T th2 = m_tanh(acc[m]);
        const T* __restrict__ w3 = W3T + (long long)(mb + m) * NX;
#pragma unroll
        for (int i = 0; i < NX; ++i) o[i] = m_fma(th2, w3[i], o[i]);
      }
    }
    const T s = b3[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = x[i] + s * o[i];
  }
  __device__ __forceinline__ T cost(const T (&x)[NX], const T (&u)[NU], int) const {
    const T* __restrict__ qx = mp + mlp2_blob_elems(NX, NU, H) - NX - NU;
    const T* __restrict__ qu = qx + NX;
    T c = (qx[0] * x[0]) * x[0];
#pragma unroll
    for (int i = 1; i < NX; ++i) c += (qx[i] * x[i]) * x[i];
#pragma unroll
    for (int n = 0; n < NU; ++n) c += (qu[n] * u[n]) * u[n];
    return c;
  }
  __device__ __forceinline__ T terminal(const T (&)[NX]) const { return T(0); }
};

// launch_rollout (rollout.hpp) for this model alone: the rolled streaming kernel on rows in the engine's layout, generated inside
// K1, or raw actions -- and nothing else.  Not built: the single-launch form of a small command (rollout_cost_kernel<..., FUSE>),
// whose instantiations for this model reserve a 36-byte stack frame (K1, K3 and K4 are then three launches, as behind the
// matrix-core kernel); the multi-rollout forms (see HEAVY above); KMPPI's fused form (NO_KMPPI_FUSE: the caller's two-launch form).
template <class Model, typename T>
static int launch_per_lane(const KArgs<T>& a_in, hipStream_t st) {
  constexpr int NU = Model::NU;
  KArgs<T> a = a_in;
  if (a.W != nullptr || a.noise_src == MPPI_NOISE_KTN || a.M > 1) return MPPI_E_UNSUPPORTED;   // the caller converts / falls back
  const bool diag = a.diag != 0 || a.coloured != 0;   // a coloured stream runs the diagonal instantiation
  const size_t smem = (size_t)(3 * a.J + BLOCK / WAVE + (a.diag != 0 ? 0 : 2 * NU * NU)) * sizeof(T);
  if (smem > 160 * 1024) return MPPI_E_UNSUPPORTED;   // T*nu beyond the LDS tables: not built
  const int nchunks = (a.K + K1_BLOCK - 1) / K1_BLOCK;
  static const int n_cu = [] {
    int dev = 0, n = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    return n > 0 ? n : 256;
  }();
  const int cap = n_cu / (a.n_env > 1 ? a.n_env : 1);
  const int gx = nchunks > (cap > 1 ? cap : 1) ? (cap > 1 ? cap : 1) : nchunks;   // persistent: one workgroup per CU
  const dim3 grid(gx, 1, a.n_env), block(K1_BLOCK);
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  profile_next_events(&ev0, &ev1, &a.tstamp);
#define MPPI_LAUNCH(NOISE_)                                                                                                     \
  do {                                                                                                                          \
    auto kernel = diag ? rollout_cost_kernel<Model, T, NOISE_, true> : rollout_cost_kernel<Model, T, NOISE_, false>;            \
    if (smem > 64 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem); \
    if (ev1 != nullptr) hipExtLaunchKernelGGL(kernel, grid, block, smem, st, ev0, ev1, 0, a);                                   \
    else hipLaunchKernelGGL(kernel, grid, block, smem, st, a);                                                                  \
  } while (0)
  if (a.noise_src == MPPI_NOISE_PHILOX) MPPI_LAUNCH(MPPI_NOISE_PHILOX);
  else if (a.noise_src == MPPI_NOISE_ACTIONS) MPPI_LAUNCH(MPPI_NOISE_ACTIONS);
  else MPPI_LAUNCH(MPPI_NOISE_TNK4);
#undef MPPI_LAUNCH
  return (int)hipGetLastError();
}

template <typename T> static int go(const KArgs<T>& a, hipStream_t st) {
  if (a.mp == nullptr || a.hidden <= 0 || a.hidden % 32 != 0) return MPPI_E_BADARG;
#define X(NX, NU) if (a.nx == NX && a.nu == NU) return launch_per_lane<Mlp2Model<T, NX, NU>, T>(a, st);
  MPPI_DIMS(X)
#undef X
#ifdef MPPI_NEXT
  return MPPI_NEXT(a, st);
#else
  return MPPI_E_UNSUPPORTED;
#endif
}
#if MPPI_MLP2_GROUP != 0
int MPPI_THIS(const KArgs<float>& a, hipStream_t st) { return go(a, st); }
int MPPI_THIS(const KArgs<double>& a, hipStream_t st) { return go(a, st); }
}  // namespace mppi
#else
bool supported_mlp2(int nx, int nu, int hidden) {
  if (hidden <= 0 || hidden % 32 != 0) return false;
#define X(NX, NU) if (nx == NX && nu == NU) return true;
  MPPI_MLP2_DIMS_0(X) MPPI_MLP2_DIMS_1(X) MPPI_MLP2_DIMS_2(X)
#undef X
  return false;
}
int rollout_mlp2(const KArgs<float>& a, hipStream_t st) {
  if (a.W != nullptr) return MPPI_E_UNSUPPORTED;   // KMPPI: the matrix-core kernel reads raw action rows (two-launch form)
  // fp32, hidden in {32, 64, 128}, one rollout per sequence, no visited states: the matrix-core kernel (rollout_mlp_deep.hip).
  // MPPI_MLP_VALU=1 (A/B measurements) and weights outside its fp16 operand range (MPPI_MODEL_FLAG_EXACT_FP32, set by the host)
  // select the per-lane form, and so does every problem the kernel itself refuses.
  const char* fv = getenv("MPPI_MLP_VALU");
  const bool force_valu = fv != nullptr && fv[0] == '1';
  const bool exact = (a.model_flags & MPPI_MODEL_FLAG_EXACT_FP32) != 0;
  // M = 2..4 rollouts per sequence: one wave per copy on the matrix cores (rollout_mlp_deep_multi.hip), which also writes the
  // visited states.  There is no per-lane form behind it (HEAVY above): what it refuses is refused (the host keeps such
  // commands on the callback loop, forms._fused_multi_ok).  MPPI_MLP_VALU has nothing to select here and is not read: the A/B
  // switch of this path is MPPI_MLP_MULTI=0, read by the host (back to the callback loop)
  if (a.M > 1) return exact || a.noise_src == MPPI_NOISE_KTN ? MPPI_E_UNSUPPORTED : rollout_mlp_deep_multi(a, st);
  if (!force_valu && !exact && a.M == 1 && a.states == nullptr && mlp_deep_supported(a.nx, a.nu, a.hidden)) {
    // the kernel reads the engine's own layout: ask the caller to convert a (K,T,nu) draw
    if (a.noise_src == MPPI_NOISE_KTN) return MPPI_E_UNSUPPORTED;
    const int r = rollout_mlp_deep(a, st);
    if (r != MPPI_E_UNSUPPORTED) return r;
  }
  return go(a, st);
}
int rollout_mlp2(const KArgs<double>& a, hipStream_t st) { return go(a, st); }
}  // namespace mppi
#endif
