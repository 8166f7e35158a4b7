// Shared device helpers for the gfx950 (MI355X / CDNA4) beta-VAE-GAN kernels.
// 64-wide wavefronts, fp32-input MFMA (v_mfma_f32_32x32x2_f32: exact fp32,
// bitwise a k-ordered fmaf chain), LDS-staged NCHW patches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define VG_WAVE 64

// Tuning knobs (forced tile variants, split targets ...): mutable process-globals exist ONLY in the tuning build
// (-DVG_TUNING -> libvaegan_hip_tuning.so, loaded by tests/ and scripts/ through _lib.load_tuning()); in the product
// library they are compile-time constants and the vg_debug_* setters are absent: it holds no global mutable state
// (include/vaegan_hip.h, "Conventions").
#ifdef VG_TUNING
#define VG_KNOB(type, name, value) type name = value
#else
#define VG_KNOB(type, name, value) constexpr type name = value
#endif

#define VG_CHECK_LAUNCH()                         \
  do {                                            \
    hipError_t e__ = hipGetLastError();           \
    if (e__ != hipSuccess) return (int)e__;       \
  } while (0)

// ---- a scheduled scalar -----------------------------------------------------------------------
// A hyperparameter that may change between the replays of a captured iteration -- beta, the KL capacity, FactorVAE's
// gamma, the augmentation's p, the GAN label -- reaches its kernel as ONE argument: a host float, or one fp32 word on the
// device that the kernel reads as it is when it runs.  An entry point and its `_dev` twin differ only in how they build
// it; the kernel reads it once, at the top, and the same fp32 value gives the same bits either way.
struct Word {
  float v;
  bool dev;            // built by word_at: `p` is what counts, NULL included (the host's view; the kernel looks at p alone)
  const float* p;
};
inline Word word(float v) { return {v, false, nullptr}; }
inline Word word_at(const float* p) { return {0.f, true, p}; }
// an entry that takes both in one signature (`target, target_dev`): the word where there is one
inline Word word_or(float v, const float* p) { return p ? word_at(p) : word(v); }
// what is checked of a float alone (a range, finiteness) asks this first: of a word the host knows no value
inline bool is_float(Word w) { return !w.dev; }
// a `_dev` entry given NULL for a word: every launcher refuses it (VG_ERR_BAD_ARG) before any launch, through this
template <class... W>
inline bool words_ok(W... w) { return ((!w.dev || w.p) && ...); }
__device__ __forceinline__ float read_word(Word w) { return w.p ? w.p[0] : w.v; }

// D(32x32) += A(32x2) * B(2x32).  Lane l supplies A[i=l&31][k=l>>5] and
// B[k=l>>5][j=l&31]; D register r of lane l is D[i=(r&3)+8*(r>>2)+4*(l>>5)][j=l&31].
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ int acc_row(int r, int lane) {
  return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
}

// Activation applied on load: identity (slope 1), ReLU (0), LeakyReLU (0.2).  One compare, one select, one multiply,
// no branch -- and a NaN stays a NaN, as in torch (fmaxf / fminf drop it: max(NaN, 0) = 0).
__device__ __forceinline__ float act_slope(float v, float slope) { return v * (v > 0.f ? 1.f : slope); }
// An operand read as act(v * scale[c] + shift[c]): the producing layer's BatchNorm and activation, applied on load
// (vg_conv_fusion semantics; the host side is affine_on_load_slope, conv_tile.hpp).
__device__ __forceinline__ float affine_act(float v, float sc, float sh, float slope) { return act_slope(fmaf(v, sc, sh), slope); }

template <int V> struct IntC { static constexpr int value = V; };      // a compile-time int as a (generic lambda) argument

// ---- split arithmetics of the convolution kernels -------------------------------------------
// An fp32 operand becomes NP 16-bit planes; the plane products whose indices sum to < NP go to the 16-bit MFMA with
// fp32 accumulation.  bf16 planes (F16 = false): each plane takes the leading 8 significand bits of what is left --
// 3 planes are the whole fp32 significand, full fp32 range, 6 products.  fp16 planes (F16 = true, NP = 2): hi + lo carry
// 11 + 11 significand bits (residual <= 2^-24 relative), 3 products; fp16 has 5 exponent bits, so the operand is first
// multiplied by an exact power of two that puts the tensor's largest magnitude just under 2^15 (f16_scale_of of an
// UPPER BOUND of max|x| read from device memory), and the product of the two operands' inverse scales is applied to
// the fp32 accumulators at the end.  Elements more than 2^-16 below the bound keep fewer than 22 bits (the lo plane
// runs into fp16's subnormals, which the MFMA honours: profiles/r04_mfma_f16.jsonl): their error is bounded by 2^-40
// of the tensor's bound instead of 2^-24 of themselves.
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

#define VG_PLANES_F16_FLAG 0x100      // == VG_PLANES_F16 of vaegan_hip.h

// A packed filter (conv_bf16split.hip, pack kernel) is nsteps K steps of planes x 2 k-blocks x CoutP units of 16 bytes,
// then VG_PACK_SPARE zero steps (the ring kernel's filter DMA runs up to VG_RING_SLOTS steps past the last one), then,
// with fp16 planes, a 16-byte trailer whose first float is the inverse of the filter's power-of-two scale.
constexpr int VG_PACK_SPARE = 6;
// 16-byte units in front of the trailer (host side; the pack kernel writes the same expression out)
constexpr size_t vg_pack_trailer_units(int nsteps, int planes, int CoutP) {
  return (size_t)(nsteps + VG_PACK_SPARE) * planes * 2 * CoutP;
}

// Statistics slots of the convolution epilogues (vg_conv_fusion.stats, [slot][Cout][2]): each slot is an fp32 sum of
// output values (and of their squares) in which no term goes through more than this many roundings (its square and
// every addition on its way to the slot: a per-lane fma chain, then the butterfly over 32 lanes).  Then a slot is within
// gamma_16 ~ 16 * 2^-24 of its exact value, relative to its sum of magnitudes, whatever the number of terms;
// vg_bn_finalize_stats relies on that (bn.hip, bn_act_bound).  A producer with deeper sums must raise it.
constexpr int VG_STATS_SLOT_DEPTH = 16;

// biased fp32 exponent of an upper bound `amax` >= 0, clamped so that both 2^(14 - E) and 2^(E - 14) are normal fp32
// numbers (amax = 0 or subnormal: the largest scale; inf / NaN: the smallest -- the data then carries the inf / NaN)
__device__ __forceinline__ unsigned f16_bound_exp(float amax) {
  const unsigned e = (__float_as_uint(amax) >> 23) & 0xffu;
  return min(max(e, 15u), 254u);
}
// amax in [2^E, 2^(E+1))  ->  2^(14 - E): the scaled tensor lies in (-2^15, 2^15), fp16's largest finite value is 65504
__device__ __forceinline__ float f16_scale_of(float amax) { return __uint_as_float((268u - f16_bound_exp(amax)) << 23); }
__device__ __forceinline__ float f16_unscale_of(float amax) { return __uint_as_float((f16_bound_exp(amax) - 14u) << 23); }

// One bf16 plane of v[8]: the leading 8 significand bits of every element; v keeps what is left.
__device__ __forceinline__ bf16x8 take_bf16_plane(float* v) {
  bf16x8 q;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const __bf16 h = (__bf16)v[j];
    q[j] = h;
    v[j] -= (float)h;
  }
  return q;
}
// v[8] -> NP bf16 planes hi, (mid,) lo, typed; v is consumed.  The kernels that feed the planes straight to the MFMA
// (conv_thin_*.hip) use this form: no bit casts on their fragments.
template <int NP>
__device__ __forceinline__ void split_bf16(float* v, bf16x8* out) {
#pragma unroll
  for (int p = 0; p < NP; ++p) out[p] = take_bf16_plane(v);
}

// The plane products of one MFMA step, index sum < NP, smallest terms first: f(IntC<pa>, IntC<pb>) for sum = NP - 1 .. 0,
// pa = sum .. 0, pb = sum - pa -- (2,0) (1,1) (0,2) (1,0) (0,1) (0,0) for three planes, (1,0) (0,1) (0,0) for two.
template <int NP, int SUM = NP - 1, int PA = SUM, class F>
__device__ __forceinline__ void for_plane_products(F&& f) {
  f(IntC<PA>{}, IntC<SUM - PA>{});
  if constexpr (PA > 0) for_plane_products<NP, SUM, PA - 1>(f);
  else if constexpr (SUM > 0) for_plane_products<NP, SUM - 1, SUM - 1>(f);
}

// v[8] (already scaled when F16) -> NP planes as raw 16-byte units; v is consumed
template <int NP, bool F16>
__device__ __forceinline__ void split_planes16(float* v, f32x4* out) {
  if constexpr (F16) {
    static_assert(NP == 2, "fp16 planes: hi + lo");
    // Two elements at a time, as 2-wide vectors: v_cvt_pk_f16_f32 (round to nearest even, two floats -> one packed
    // register, no separate pack), v_pk_add_f32 for the residual -- 2.5 VALU per element where the scalar form
    // (cvt, cvt back, sub, and a cvt_pk each for packing hi and lo) took 4.  Same roundings: same bits.
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
    f16x2 hi[4], lo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x2 v2 = {v[2 * j], v[2 * j + 1]};
      const f16x2 h = __builtin_convertvector(v2, f16x2);                 // |v - h| <= 2^-12 |v|
      hi[j] = h;
      lo[j] = __builtin_convertvector(v2 - __builtin_convertvector(h, f32x2), f16x2);   // exact difference, 11 more bits
    }
    struct P4 { f16x2 q[4]; };
    out[0] = __builtin_bit_cast(f32x4, P4{{hi[0], hi[1], hi[2], hi[3]}});
    out[1] = __builtin_bit_cast(f32x4, P4{{lo[0], lo[1], lo[2], lo[3]}});
  } else {
#pragma unroll
    for (int p = 0; p < NP; ++p) out[p] = __builtin_bit_cast(f32x4, take_bf16_plane(v));      // hi, (mid,) lo
  }
}

template <bool F16>
__device__ __forceinline__ f32x16 mfma_split16(bf16x8 a, bf16x8 b, f32x16 c) {
  if constexpr (F16)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// ---- wavefront / block reductions (64 lanes; no 32-lane idioms) -------------
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;  // valid in lane 0
}

template <typename T>
__device__ __forceinline__ T wave_allsum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Sum over a block of NT threads (NT multiple of 64); result valid in thread 0.
// `red` is LDS scratch of at least NT/64 elements.
template <int NT, typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wid] = v;
  __syncthreads();
  T t = 0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) t += red[i];
  }
  return t;
}

// Bound of max |x| for the fp16-plane arithmetic: bit pattern of |v| (integer order == float order for non-negative
// floats; NaN patterns sort above every number), and the workgroup's maximum added to a device word with ONE atomic
// (order-independent: deterministic).  Every thread of the NT-thread workgroup must call it.
__device__ __forceinline__ unsigned abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

template <int NT>
__device__ __forceinline__ void block_amax_atomic(unsigned m, unsigned* out) {
  __shared__ unsigned amax_red[NT / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) amax_red[wid] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 1; i < NT / 64; ++i) m = max(m, amax_red[i]);
    // most workgroups find the word already above their maximum: a relaxed load (possibly stale: then the atomic runs
    // anyway) keeps thousands of them from queueing on one address (16 384 atomics made a 20 us pass take 190)
    if (m > __hip_atomic_load(out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(out, m);
  }
}

// ---- the Adam element and the end of a step kernel, shared by adam.hip and the fused weight-gradient step of
// gemm_split.hip ------------------------------------------------------------------------------------------------------
// One element of the plain step with its roundings spelled out.  The plain kernel (adam.hip, adam_multi_kernel) is
// compiled under the default contraction, and the compiler forms v differently in its two loops: in the 16-byte body as
// ONE fma, fma(b2, v, (omb2 g) g), in the scalar loops as two rounded products and a rounded sum; m and p are an fma
// in both.  So this copy takes no contraction of its own and, per element, which of the two loops the plain kernel
// would have run it in.  tests/test_adam_ema_gpu.py compares the bits on every path.
__device__ __forceinline__ void adam_one_as(bool body, float& p, float g, float& m, float& v, float omb1, float b2,
                                            float omb2, float step_size, float bc2s, float eps) {
#pragma clang fp contract(off)
  m = __builtin_fmaf(omb1, g - m, m);
  const float gg = (omb2 * g) * g;
  const float b2v = b2 * v;
  v = body ? __builtin_fmaf(b2, v, gg) : b2v + gg;
  const float denom = sqrtf(v) / bc2s + eps;
  p = __builtin_fmaf(-step_size, m / denom, p);
}

constexpr unsigned VG_NONFINITE_BITS = 0x7f800000u;      // abs_bits(x) >= this: x is inf or NaN
constexpr unsigned VG_FLAG_GRAD = 1u, VG_FLAG_PARAM = 2u;      // == VG_NONFINITE_GRAD / VG_NONFINITE_PARAM of vaegan_hip.h

// ORs `bits` (this thread's non-finite findings) over the workgroup into *out: no memory traffic unless a bit is set.
// Every thread of the NT-thread workgroup must call it.
template <int NT>
__device__ __forceinline__ void block_flag_or(unsigned bits, unsigned* out) {
  __shared__ unsigned flag_red[NT / 64];
  const unsigned w = (__ballot(bits & VG_FLAG_GRAD) ? VG_FLAG_GRAD : 0u) | (__ballot(bits & VG_FLAG_PARAM) ? VG_FLAG_PARAM : 0u);
  if ((threadIdx.x & 63) == 0) flag_red[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned all = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) all |= flag_red[i];
    if (all) atomicOr(out, all);
  }
}

// The end of a step kernel: this thread's max |p| (`am`) and max |g| (`gm`), as bits, go into the tensor's amax word
// and flag word (either may be NULL; both pointers are uniform over the workgroup).  Every thread must call it.
template <int NT>
__device__ __forceinline__ void emit_amax_and_flags(unsigned am, unsigned gm, unsigned* amax, unsigned* flag) {
  if (amax) block_amax_atomic<NT>(am, amax);
  if (flag)
    block_flag_or<NT>((gm >= VG_NONFINITE_BITS ? VG_FLAG_GRAD : 0u) | (am >= VG_NONFINITE_BITS ? VG_FLAG_PARAM : 0u), flag);
}

__host__ __device__ constexpr int cdiv(int a, int b) { return (a + b - 1) / b; }

// cross-file internal entry points (not part of the C ABI)
int vg_internal_wgrad_reduce(const float* slabs, float* dw, int n, int splits, hipStream_t st, int accumulate = 0);
// (conv_ring.hip's entry points for conv_bf16split.hip: conv_tile.hpp)
#ifdef VG_TUNING
void vg_internal_ring_set_variant(int v);
void vg_internal_wx_set_th(int th);
int vg_internal_wgrad_reducer(const float* slabs, const float* dw, int n, int splits);   // conv_wgrad.hip: 0 / 1 / 2 / 3 = slab_sum4 / reduce<16> / reduce<4> / slab_sum1
#endif
int vg_internal_convT_s1_thin(const float* x, const float* w, const float* bias, float* y, int B, int Cin, int H,
                              int W, int Cout, hipStream_t st);
