// mlp_split_ops.hpp -- the split-operand arithmetic of the matrix-core MLP kernels, for rollout_mlp_split32.hip.
// (rollout_mlp_split.hip keeps its own copy in an anonymous namespace: that unit and its include closure are hashed
// against the committed counter passes, tests/test_lookup_evidence.py, so it does not include this header.)
//
//   layer 1: bf16 x 3 by truncation, v = hi + mid + lo exactly (8 + 8 + 8 significant bits), six of the nine piece
//            products on v_mfma_f32_16x16x32_bf16, smallest first:  l.h  h.l  m.m  m.h  h.m  h.h
//   layer 2: fp16 x 2, W' = Wh + 2^-11 Wm, r = rh + rm, three products on v_mfma_f32_16x16x32_f16:
//            Wh.rh  Wh.rm  (one magnitude class each)  2^-11 Wm.rh (its own accumulator)
//   tanh = 1 - 2r, r = 1 / (2^h + 1): the affine parts are folded into the weights
// Operand layout of the 16x16x32 instructions, lane l = (g = l >> 4, s = l & 15): A[i][k] and B[k][j] hold k = 8g + e
// (e = 0..7) at i = j = s; D[i][j] holds i = 4g + r (r = 0..3) at j = s.
#pragma once
#include <type_traits>
#include "common.hpp"

namespace mppi {
namespace split_ops {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

constexpr float EXP2_SCALE = 2.8853900817779268f;   // 2 * log2(e)
constexpr float MID_SCALE = 2048.0f, MID_UNSCALE = 1.0f / 2048.0f;

// one fp32 value -> its three bf16 pieces, each still an fp32 whose low 16 bits are zero
struct Split3 { float h, m, l; };
__device__ __forceinline__ Split3 split3(float v) {
  Split3 r;
  r.h = __uint_as_float(__float_as_uint(v) & 0xFFFF0000u);
  const float r1 = v - r.h;                              // exact
  r.m = __uint_as_float(__float_as_uint(r1) & 0xFFFF0000u);
  r.l = r1 - r.m;                                        // exact, <= 8 significant bits
  return r;
}
// bf16 pair (lo half = a, hi half = b) out of two fp32 whose bf16 truncation is wanted
__device__ __forceinline__ unsigned pack_bf16(float a, float b) {
  return __builtin_amdgcn_perm(__float_as_uint(b), __float_as_uint(a), 0x07060302u);
}
// eight fp32 -> three bf16x8 planes
struct Planes { u32x4 h, m, l; };
__device__ __forceinline__ Planes split_pack8(const float (&v)[8]) {
  Split3 s[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = split3(v[e]);
  Planes p;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    p.h[q] = pack_bf16(v[2 * q], v[2 * q + 1]);          // truncation = the upper halves as they are
    p.m[q] = pack_bf16(s[2 * q].m, s[2 * q + 1].m);
    p.l[q] = pack_bf16(s[2 * q].l, s[2 * q + 1].l);
  }
  return p;
}
__device__ __forceinline__ f32x4 mfma_bf(const u32x4& a, const u32x4& b, f32x4 acc) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
}
// product pr of the six: 0 l.h | 1 h.l | 2 m.m | 3 m.h | 4 h.m | 5 h.h   (a = weights, b = inputs): which plane of each
constexpr int plane_a(int pr) { return pr == 0 ? 2 : ((pr == 2 || pr == 3) ? 1 : 0); }   // 0 h | 1 m | 2 l
constexpr int plane_b(int pr) { return pr == 1 ? 2 : ((pr == 2 || pr == 4) ? 1 : 0); }
__device__ __forceinline__ const u32x4& plane(const Planes& p, int which) { return which == 0 ? p.h : (which == 1 ? p.m : p.l); }

struct PlanesH { u32x4 h, m; };
__device__ __forceinline__ unsigned cvt_pk_f16(f32x2 v) {       // v_cvt_pk_f16_f32, round to nearest even
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2_t));
}
__device__ __forceinline__ f32x2 f16pair_to_f32(unsigned p) {
  return __builtin_convertvector(__builtin_bit_cast(f16x2_t, p), f32x2);
}
__device__ __forceinline__ f32x4 mfma_h(const u32x4& a, const u32x4& b, f32x4 acc) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), acc, 0, 0, 0);
}
// eight fp32 weights -> {fp16 hi, fp16 of the 2^11-scaled residual}
__device__ __forceinline__ PlanesH split_pack8_h(const float (&v)[8]) {
  PlanesH p;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x2 w = {v[2 * q], v[2 * q + 1]};
    const unsigned hp = cvt_pk_f16(w);
    p.h[q] = hp;
    p.m[q] = cvt_pk_f16((w - f16pair_to_f32(hp)) * f32x2{MID_SCALE, MID_SCALE});
  }
  return p;
}
// two activations r -> the fp16 pair of their hi pieces and of their residuals (|r - hi - mid| <= 2^-25).  The residual is
// one v_fma_mix_f32 per value (fp16 source converted inside the instruction): hipcc selects it for an fma whose
// multiplier it cannot fold (`minus_one` opaque in a VGPR) when the SLP vectorizer is off (-fno-slp-vectorize, _build.py).
__device__ __forceinline__ void split_pair_h(float ra, float rb, float minus_one, unsigned& hi, unsigned& mid) {
  hi = cvt_pk_f16(f32x2{ra, rb});
  const f16x2_t hh = __builtin_bit_cast(f16x2_t, hi);
  const float r1a = __builtin_fmaf((float)hh.x, minus_one, ra);          // exact
  const float r1b = __builtin_fmaf((float)hh.y, minus_one, rb);
  mid = cvt_pk_f16(f32x2{r1a, r1b});
}

// r = 1 / (2^x + 1)
__device__ __forceinline__ float sigm2(float x_exp2_units) {
  return __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(x_exp2_units) + 1.0f);
}

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

}  // namespace split_ops
}  // namespace mppi
