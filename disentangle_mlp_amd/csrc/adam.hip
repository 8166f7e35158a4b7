// Adam step of the three optimizers (/root/reference/experiments/new_betavaegan.py:49-50:
// optim.Adam defaults -- betas (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad), SURVEY.md
// section 8 row a14: 182.9 M parameter updates per iteration, 28 bytes each -- purely HBM-bound.
//
//   m <- m + (1 - beta1) (g - m)             (torch: exp_avg.lerp_(grad, 1 - beta1))
//   v <- beta2 v + (1 - beta2) g g           (exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2))
//   p <- p - step_size * m / (sqrt(v) / bias_correction2_sqrt + eps)
//
// One launch updates up to VG_ADAM_MAX_TENSORS tensors: their pointers travel in the kernel
// arguments, a workgroup owns 8192 consecutive elements of one tensor (16-byte loads / stores when
// the four pointers allow it).  Bias corrections are computed on the host in double precision.
//
// Non-finite guard (vg_adam_step_checked / vg_adam_step_dev_checked): the step is the one pass that reads every gradient
// and writes every parameter, so it also notices an inf / NaN among them -- |x| as bits >= 0x7f800000 -- and ORs
// VG_NONFINITE_GRAD / VG_NONFINITE_PARAM into the tensor's caller-owned flag word: one wavefront / LDS reduction per
// workgroup, one atomicOr per workgroup that saw something, none in a clean step.  By itself it DETECTS, it does not
// skip the update: a skip needs a grid-wide answer before the first store -- which the opt-in norm pass below gives
// (vg_adam_step_clip with skip_nonfinite).  Without that opt-in, when a bit is up the weights are poisoned; recovery
// is the last good checkpoint.  The arithmetic that writes p, m, v and amax is the unchecked step's.
//
// Weight EMA (vg_adam_step_ema / vg_adam_step_dev_ema): the thread that has just formed an element's new p also moves
// the element's running average, e <- e + (1 - decay) (p_new - e) (torch's lerp form for weights below 0.5), from the
// value in its register: 8 more bytes per parameter instead of the 12 of a separate pass over p and e.  It is a
// compile-time variant with a pack of its own (AdamPackEma): the kernels of the entry points above are what they
// were.  An inf / NaN in p goes into e unfiltered; the guard reports it as before.
//
// Clipping by global norm / skipping a non-finite step (vg_grad_sumsq_multi, vg_grad_clip_finalize, vg_adam_step_clip /
// vg_adam_step_dev_clip): one deterministic pass over the gradients in front of the step -- fp64 squares and sums from
// the thread level on (the square of an fp32 number is exact in fp64, and no |g| overflows), one fp64 partial per
// workgroup in a slot of its own, no atomics -- and a one-workgroup kernel that adds the partials in a fixed order and
// writes a four-word record: the norm, the clip coefficient min(1, max_norm / (norm + 1e-6)) (clip_grad_norm_'s
// formula, formed in double, rounded once), a skip word and a running count of skips.  The clip variant of the step
// reads the record at its top and uses every gradient as gs = coef * g (one fp32 rounding, that of g.mul_(coef)), from
// registers: 4 more bytes per parameter instead of the 12 of torch's recipe.  With the skip word up it stores nothing to
// p, m, v or the EMA; it still emits max |p| (the bounds words were zeroed in front of the step) and flags the tensor
// that holds the inf / NaN.  It is a kernel and a pack of its own: the kernels of the entry points above are what
// they were.
//
// Weight decay and hyper-parameters on the device (vg_adam_prepare_dev, vg_adam_step_decay / vg_adam_step_dev_decay):
// the learning rate and the weight decay of a captured step live in a device pair [lr, weight_decay] the prepare kernel
// reads, so a schedule changes them between replays.  The decay step is the clip step with one more register operation
// per element in front of the update -- coupled (L2): gd = gs + (wd * p), a rounded product and a rounded sum;
// decoupled (AdamW): pd = p * s2 with s2 = (float)(1 - lr * wd) formed in double -- and no memory traffic of its own.
// With wd == 0 neither term is formed (no 0 * inf) and the bits are the clip step's.  Again a kernel and a pack of its
// own.
//
// EMA decay on the device (vg_adam_step_dev_ema_dev): the decay step with (float)(1 - decay) read from a device word
// instead of the pack -- an ordinary global load, uniform over the grid -- so a warm-up changes the decay between the
// replays of a captured step.  A compile-time variant of the decay kernel with a pack of its own; the word 1.0f
// ("follow the weights") stores p itself, since e + 1 (p - e) is not p in fp32.
#include "common.hpp"
#include "vaegan_hip.h"

#include <type_traits>

namespace {

constexpr int ANT = 256, ACHUNK = 8192, AMAX = 24;

struct AdamPack {
  float* p[AMAX];
  const float* g[AMAX];
  float* m[AMAX];
  float* v[AMAX];
  unsigned long long n[AMAX];
  unsigned* amax[AMAX];               // per tensor, may be NULL: max |p| after the update is added here (atomic max)
  unsigned* flag[AMAX];               // per tensor, may be NULL: VG_NONFINITE_* bits are ORed in here (never cleared)
  unsigned first_block[AMAX + 1];     // prefix sums of ceil(n / ACHUNK)
  int count;
};

// The pack of the EMA variant: e[t] may be NULL (that tensor is not averaged); omd = (float)(1 - decay).
struct AdamPackEma : AdamPack {
  float* e[AMAX];
  float omd;
};

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float omb1, float b2, float omb2,
                                         float step_size, float bc2s, float eps) {
  m = m + omb1 * (g - m);
  v = b2 * v + omb2 * g * g;
  const float denom = sqrtf(v) / bc2s + eps;
  p = p - step_size * (m / denom);
}

// adam_one for the EMA variant, which must give the bits of the kernels without EMA element by element -- wherever its
// own alignment rule (the EMA pointer counts) sends the element.  Those kernels are compiled under the default
// contraction, and the compiler forms v differently in their two loops: in the 16-byte body as ONE fma,
// fma(b2, v, (omb2 g) g), in the scalar loops as two rounded products and a rounded sum; m and p are an fma in both.
// So this copy spells the roundings out (no contraction of its own) and takes, per element, which of the two loops
// the step without EMA would have run it in.  tests/test_adam_ema_gpu.py compares the bits on every path.
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

__device__ __forceinline__ float ema_one(float e, float p, float omd) { return e + omd * (p - e); }

// One thread: the scalars of an optimizer step whose step count lives on the device (a step captured in a HIP graph
// cannot take them as kernel arguments: they change from replay to replay).  `advance`: the device counter is advanced
// by one and used (captured steps); otherwise `step_host` is used and, when there is a device counter, stored in it (an
// eager step between replays keeps the counter current).  Both ways the bias corrections are formed here, in double,
// from the same expression -- an eager step and a replayed one give the same bits.
__global__ void adam_prepare_kernel(double step_host, double* __restrict__ step_dev, int advance, double lr, double beta1,
                                    double beta2, float* __restrict__ scalars) {
  double step = step_host;
  if (advance) step = step_dev[0] + 1.0;
  if (step_dev) step_dev[0] = step;
  const double bc1 = 1.0 - pow(beta1, step);
  const double bc2 = 1.0 - pow(beta2, step);
  scalars[0] = (float)(lr / bc1);       // step_size
  scalars[1] = (float)sqrt(bc2);        // bias_correction2_sqrt
}

// s2 of the decoupled decay: 1 - lr * wd in double, a rounded product and a rounded difference (what Python's
// ``1 - lr * wd`` gives; contracted to one fma the host's and the device's value could differ in the last bit).
__host__ __device__ __forceinline__ float decoupled_factor(double lr, double wd) {
#pragma clang fp contract(off)
  const double prod = lr * wd;
  return (float)(1.0 - prod);
}

// adam_prepare_kernel with lr and the weight decay read from DEVICE memory (hyper = [lr, weight_decay]): a schedule
// changes them between the replays of a captured step.  scalars[0..1] by the expressions above (same lr, same bits);
// scalars[2] the decoupled factor (1 when there is nothing to decay), scalars[3] the coupled coefficient (0 likewise).
__global__ void adam_prepare_dev_kernel(double step_host, double* __restrict__ step_dev, int advance,
                                        const double* __restrict__ hyper, int decoupled, double beta1, double beta2,
                                        float* __restrict__ scalars) {
  double step = step_host;
  if (advance) step = step_dev[0] + 1.0;
  if (step_dev) step_dev[0] = step;
  const double lr = hyper[0], wd = hyper[1];
  const double bc1 = 1.0 - pow(beta1, step);
  const double bc2 = 1.0 - pow(beta2, step);
  scalars[0] = (float)(lr / bc1);       // step_size
  scalars[1] = (float)sqrt(bc2);        // bias_correction2_sqrt
  scalars[2] = (decoupled && wd != 0.0) ? decoupled_factor(lr, wd) : 1.f;
  scalars[3] = decoupled ? 0.f : (float)wd;
}

constexpr unsigned NONFINITE_BITS = 0x7f800000u;      // abs_bits(x) >= this: x is inf or NaN

// ORs `bits` (this thread's VG_NONFINITE_* findings) over the workgroup into *out: no memory traffic unless a bit is set.
// Every thread of the ANT-thread workgroup must call it.
__device__ __forceinline__ void block_flag_or(unsigned bits, unsigned* out) {
  __shared__ unsigned flag_red[ANT / 64];
  const unsigned w = (__ballot(bits & VG_NONFINITE_GRAD) ? (unsigned)VG_NONFINITE_GRAD : 0u) |
                     (__ballot(bits & VG_NONFINITE_PARAM) ? (unsigned)VG_NONFINITE_PARAM : 0u);
  if ((threadIdx.x & 63) == 0) flag_red[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned all = 0;
#pragma unroll
    for (int i = 0; i < ANT / 64; ++i) all |= flag_red[i];
    if (all) atomicOr(out, all);
  }
}

template <bool DEV, bool EMA>
__global__ __launch_bounds__(ANT) void adam_multi_kernel(std::conditional_t<EMA, AdamPackEma, AdamPack> A, float omb1,
                                                        float b2, float omb2, float step_size, float bc2s, float eps,
                                                        const float* __restrict__ scalars) {
  if constexpr (DEV) {
    step_size = scalars[0];
    bc2s = scalars[1];
  }
  int t = 0;
  while (t + 1 < A.count && blockIdx.x >= A.first_block[t + 1]) ++t;
  const unsigned long long n = A.n[t];
  const unsigned long long base = (unsigned long long)(blockIdx.x - A.first_block[t]) * ACHUNK;
  const unsigned long long end = min(base + (unsigned long long)ACHUNK, n);
  float* __restrict__ p = A.p[t];
  const float* __restrict__ g = A.g[t];
  float* __restrict__ m = A.m[t];
  float* __restrict__ v = A.v[t];
  bool vec = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0);
  [[maybe_unused]] const bool vec_step = vec;      // what the step without EMA decides for this tensor (adam_one_as)
  float* __restrict__ e = nullptr;      // (uniform over the workgroup, like t)
  float omd = 0.f;
  if constexpr (EMA) {
    e = A.e[t];
    omd = A.omd;
    vec = vec && (((uintptr_t)e & 15) == 0);      // NULL passes: the choice of a tensor without an average is unchanged
  }
  // bound of max |p| for the fp16-plane GEMMs that read this weight next (VgAdamTensor::amax): the step that changes the
  // weight is the one pass that sees every new value anyway -- no separate 134 MB read per weight and iteration
  unsigned am = 0;
  unsigned gm = 0;      // max |g| as bits, of the gradients read: the non-finite guard's half of the same bookkeeping
  if (vec) {
    const unsigned long long end4 = base + ((end - base) & ~3ULL);
    for (unsigned long long i = base + 4ULL * threadIdx.x; i < end4; i += 4ULL * ANT) {
      f32x4 pv = *reinterpret_cast<f32x4*>(p + i), mv = *reinterpret_cast<f32x4*>(m + i);
      f32x4 vv = *reinterpret_cast<f32x4*>(v + i);
      const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pj = pv[j], mj = mv[j], vj = vv[j];
        if constexpr (EMA)
          adam_one_as(true, pj, gv[j], mj, vj, omb1, b2, omb2, step_size, bc2s, eps);
        else
          adam_one(pj, gv[j], mj, vj, omb1, b2, omb2, step_size, bc2s, eps);
        pv[j] = pj; mv[j] = mj; vv[j] = vj;
        am = max(am, abs_bits(pj));
        gm = max(gm, abs_bits(gv[j]));
      }
      *reinterpret_cast<f32x4*>(p + i) = pv;
      *reinterpret_cast<f32x4*>(m + i) = mv;
      *reinterpret_cast<f32x4*>(v + i) = vv;
      if constexpr (EMA) {
        if (e) {
          f32x4 ev = *reinterpret_cast<f32x4*>(e + i);
#pragma unroll
          for (int j = 0; j < 4; ++j) ev[j] = ema_one(ev[j], pv[j], omd);
          *reinterpret_cast<f32x4*>(e + i) = ev;
        }
      }
    }
    for (unsigned long long i = end4 + threadIdx.x; i < end; i += ANT) {
      const float gi = g[i];
      if constexpr (EMA) {
        float pi = p[i];      // the average below takes the new p from this register
        adam_one_as(false, pi, gi, m[i], v[i], omb1, b2, omb2, step_size, bc2s, eps);
        p[i] = pi;
        if (e) e[i] = ema_one(e[i], pi, omd);
        am = max(am, abs_bits(pi));
      } else {
        adam_one(p[i], gi, m[i], v[i], omb1, b2, omb2, step_size, bc2s, eps);
        am = max(am, abs_bits(p[i]));
      }
      gm = max(gm, abs_bits(gi));
    }
  } else {
    [[maybe_unused]] const unsigned long long end4 = base + ((end - base) & ~3ULL);
    for (unsigned long long i = base + threadIdx.x; i < end; i += ANT) {
      const float gi = g[i];
      if constexpr (EMA) {
        float pi = p[i];      // the average below takes the new p from this register
        adam_one_as(vec_step && i < end4, pi, gi, m[i], v[i], omb1, b2, omb2, step_size, bc2s, eps);
        p[i] = pi;
        if (e) e[i] = ema_one(e[i], pi, omd);
        am = max(am, abs_bits(pi));
      } else {
        adam_one(p[i], gi, m[i], v[i], omb1, b2, omb2, step_size, bc2s, eps);
        am = max(am, abs_bits(p[i]));
      }
      gm = max(gm, abs_bits(gi));
    }
  }
  if (A.amax[t]) block_amax_atomic<ANT>(am, A.amax[t]);      // (t is uniform over the workgroup)
  if (A.flag[t])
    block_flag_or((gm >= NONFINITE_BITS ? (unsigned)VG_NONFINITE_GRAD : 0u) |
                      (am >= NONFINITE_BITS ? (unsigned)VG_NONFINITE_PARAM : 0u),
                  A.flag[t]);
}

// ---- clipping by global norm, skipping a non-finite step --------------------------------------------------------------
// The record vg_grad_clip_finalize writes and the clip step reads: four 32-bit words.
constexpr int REC_NORM = 0, REC_COEF = 1, REC_SKIP = 2, REC_SKIPPED = 3;

struct SumsqPack {
  const float* g[AMAX];
  unsigned long long n[AMAX];
  unsigned first_block[AMAX + 1];     // prefix sums of ceil(n / ACHUNK) within this launch
  int count;
};

// One workgroup: the sum of squares, in fp64, of its ACHUNK elements of one tensor -> partials[blockIdx.x] (`partials`
// already points at this launch's first slot).  Every thread adds its elements in index order, the wavefronts and the
// workgroup reduce in a fixed tree: the same bits run to run.
__global__ __launch_bounds__(ANT) void grad_sumsq_multi_kernel(SumsqPack A, double* __restrict__ partials) {
  __shared__ double red[ANT / 64];
  int t = 0;
  while (t + 1 < A.count && blockIdx.x >= A.first_block[t + 1]) ++t;
  const unsigned long long n = A.n[t];
  const unsigned long long base = (unsigned long long)(blockIdx.x - A.first_block[t]) * ACHUNK;
  const unsigned long long end = min(base + (unsigned long long)ACHUNK, n);
  const float* __restrict__ g = A.g[t];
  double s = 0.0;
  unsigned long long tail = base;
  if (((uintptr_t)g & 15) == 0) {      // (base is a multiple of ACHUNK: g + base is aligned when g is)
    const unsigned long long end4 = base + ((end - base) & ~3ULL);
    for (unsigned long long i = base + 4ULL * threadIdx.x; i < end4; i += 4ULL * ANT) {
      const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double d = (double)gv[j];
        s += d * d;
      }
    }
    tail = end4;
  }
  for (unsigned long long i = tail + threadIdx.x; i < end; i += ANT) {
    const double d = (double)g[i];
    s += d * d;
  }
  s = block_sum<ANT, double>(s, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// One workgroup: norm = sqrt(sum of the partials), added in a fixed order in fp64, and the record.
__global__ __launch_bounds__(ANT) void grad_clip_finalize_kernel(const double* __restrict__ partials,
                                                                 unsigned long long n_partials, double max_norm,
                                                                 int skip_nonfinite, float* __restrict__ record) {
  __shared__ double red[ANT / 64];
  double s = 0.0;
  for (unsigned long long i = threadIdx.x; i < n_partials; i += ANT) s += partials[i];
  s = block_sum<ANT, double>(s, red);
  if (threadIdx.x == 0) {
    const double norm = sqrt(s);
    const bool finite = isfinite(norm);
    double coef = 1.0;
    if (max_norm > 0.0) {
      // torch: clamp(max_norm / (total_norm + 1e-6), max=1.0) -- a NaN stays a NaN (fmin would drop it)
      const double c = max_norm / (norm + 1e-6);
      coef = c < 1.0 ? c : (c != c ? c : 1.0);
    }
    const unsigned skip = (!finite && skip_nonfinite) ? 1u : 0u;
    if (skip) coef = 0.0;
    unsigned* const words = reinterpret_cast<unsigned*>(record);
    record[REC_NORM] = (float)norm;
    record[REC_COEF] = (float)coef;
    words[REC_SKIP] = skip;
    words[REC_SKIPPED] = words[REC_SKIPPED] + skip;
  }
}

// gs = coef * g, rounded once as g.mul_(coef) rounds it: kept from being fused into the m update that follows.
__device__ __forceinline__ float clip_scale(float coef, float g) {
#pragma clang fp contract(off)
  return coef * g;
}

// The step of adam_multi_kernel<DEV, true> with every gradient scaled by the record's coefficient, or -- the record's
// skip word up -- no step at all: p and g are read for max |p| and the flag words, nothing is stored to p, m, v, e.
// e[t] may be NULL as in the EMA variant; a launch without any average passes NULLs.  adam_one_as and its `body` rule
// give, element by element, the bits of the step without the feature on the scaled gradient.
template <bool DEV>
__global__ __launch_bounds__(ANT) void adam_clip_multi_kernel(AdamPackEma A, float omb1, float b2, float omb2,
                                                             float step_size, float bc2s, float eps,
                                                             const float* __restrict__ scalars,
                                                             const float* __restrict__ record) {
  if constexpr (DEV) {
    step_size = scalars[0];
    bc2s = scalars[1];
  }
  const float coef = record[REC_COEF];
  const bool skip = reinterpret_cast<const unsigned*>(record)[REC_SKIP] != 0u;      // (uniform over the grid)
  int t = 0;
  while (t + 1 < A.count && blockIdx.x >= A.first_block[t + 1]) ++t;
  const unsigned long long n = A.n[t];
  const unsigned long long base = (unsigned long long)(blockIdx.x - A.first_block[t]) * ACHUNK;
  const unsigned long long end = min(base + (unsigned long long)ACHUNK, n);
  float* __restrict__ p = A.p[t];
  const float* __restrict__ g = A.g[t];
  float* __restrict__ m = A.m[t];
  float* __restrict__ v = A.v[t];
  float* __restrict__ e = A.e[t];
  const float omd = A.omd;
  const bool vec_step = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0);
  const bool vec = vec_step && (((uintptr_t)e & 15) == 0);
  const unsigned long long end4 = base + ((end - base) & ~3ULL);
  unsigned am = 0, gm = 0;
  if (skip) {
    unsigned long long tail = base;
    if (vec_step) {
      for (unsigned long long i = base + 4ULL * threadIdx.x; i < end4; i += 4ULL * ANT) {
        const f32x4 pv = *reinterpret_cast<const f32x4*>(p + i);
        const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          am = max(am, abs_bits(pv[j]));
          gm = max(gm, abs_bits(gv[j]));
        }
      }
      tail = end4;
    }
    for (unsigned long long i = tail + threadIdx.x; i < end; i += ANT) {
      am = max(am, abs_bits(p[i]));
      gm = max(gm, abs_bits(g[i]));
    }
  } else if (vec) {
    for (unsigned long long i = base + 4ULL * threadIdx.x; i < end4; i += 4ULL * ANT) {
      f32x4 pv = *reinterpret_cast<f32x4*>(p + i), mv = *reinterpret_cast<f32x4*>(m + i);
      f32x4 vv = *reinterpret_cast<f32x4*>(v + i);
      const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pj = pv[j], mj = mv[j], vj = vv[j];
        const float gs = clip_scale(coef, gv[j]);
        adam_one_as(true, pj, gs, mj, vj, omb1, b2, omb2, step_size, bc2s, eps);
        pv[j] = pj; mv[j] = mj; vv[j] = vj;
        am = max(am, abs_bits(pj));
        gm = max(gm, abs_bits(gs));
      }
      *reinterpret_cast<f32x4*>(p + i) = pv;
      *reinterpret_cast<f32x4*>(m + i) = mv;
      *reinterpret_cast<f32x4*>(v + i) = vv;
      if (e) {
        f32x4 ev = *reinterpret_cast<f32x4*>(e + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) ev[j] = ema_one(ev[j], pv[j], omd);
        *reinterpret_cast<f32x4*>(e + i) = ev;
      }
    }
    for (unsigned long long i = end4 + threadIdx.x; i < end; i += ANT) {
      const float gs = clip_scale(coef, g[i]);
      float pi = p[i];
      adam_one_as(false, pi, gs, m[i], v[i], omb1, b2, omb2, step_size, bc2s, eps);
      p[i] = pi;
      if (e) e[i] = ema_one(e[i], pi, omd);
      am = max(am, abs_bits(pi));
      gm = max(gm, abs_bits(gs));
    }
  } else {
    for (unsigned long long i = base + threadIdx.x; i < end; i += ANT) {
      const float gs = clip_scale(coef, g[i]);
      float pi = p[i];
      adam_one_as(vec_step && i < end4, pi, gs, m[i], v[i], omb1, b2, omb2, step_size, bc2s, eps);
      p[i] = pi;
      if (e) e[i] = ema_one(e[i], pi, omd);
      am = max(am, abs_bits(pi));
      gm = max(gm, abs_bits(gs));
    }
  }
  if (A.amax[t]) block_amax_atomic<ANT>(am, A.amax[t]);
  if (A.flag[t])
    block_flag_or((gm >= NONFINITE_BITS ? (unsigned)VG_NONFINITE_GRAD : 0u) |
                      (am >= NONFINITE_BITS ? (unsigned)VG_NONFINITE_PARAM : 0u),
                  A.flag[t]);
}

// ---- weight decay inside the step -------------------------------------------------------------------------------------
// The pack of the decay variant: s2 / wdc are what vg_adam_prepare_dev leaves in scalars[2..3], formed on the host.
struct AdamPackDecay : AdamPackEma {
  float s2;       // decoupled: p is multiplied by this before the update; 1: not
  float wdc;      // coupled: this times p is added to the gradient; 0: not
};

// The pack of the variant that reads (float)(1 - decay) from device memory: omd is not used.
struct AdamPackDecayDev : AdamPackDecay {
  const float* omd_dev;
};

// wd * p and gs + (wd * p): a rounded product and a rounded sum (torch: p.mul(wd), then g.add_), never one fma.
__device__ __forceinline__ float decay_grad(float gs, float wdc, float p) {
#pragma clang fp contract(off)
  const float wp = wdc * p;
  return gs + wp;
}

// p * s2, one rounding (torch: p.mul_(1 - lr * wd)): kept from being fused into the update that follows.
__device__ __forceinline__ float decay_param(float p, float s2) {
#pragma clang fp contract(off)
  return p * s2;
}

// adam_clip_multi_kernel with the weights decayed in registers in front of the update.  `record` may be NULL here (no
// clipping, nothing skipped: gs = g).  l2 / dec are uniform over the grid; with neither, every element takes the clip
// step's operations and nothing else.  The GRAD bit is judged on gs -- the gradient the caller handed in, scaled -- not
// on gd, which an inf WEIGHT would poison as well; amax and the PARAM bit on the final p.
// EDEV: (float)(1 - decay) comes from the device word A.omd_dev; 1.0f stores p itself, anything else takes ema_one.
template <bool DEV, bool EDEV = false>
__global__ __launch_bounds__(ANT) void adam_decay_multi_kernel(std::conditional_t<EDEV, AdamPackDecayDev, AdamPackDecay> A,
                                                              float omb1, float b2, float omb2, float step_size,
                                                              float bc2s, float eps, const float* __restrict__ scalars,
                                                              const float* __restrict__ record) {
  float s2 = A.s2, wdc = A.wdc;
  if constexpr (DEV) {
    step_size = scalars[0];
    bc2s = scalars[1];
    s2 = scalars[2];
    wdc = scalars[3];
  }
  const bool dec = s2 != 1.f, l2 = wdc != 0.f;
  const bool scale = record != nullptr;
  const float coef = scale ? record[REC_COEF] : 1.f;
  const bool skip = scale && reinterpret_cast<const unsigned*>(record)[REC_SKIP] != 0u;      // (uniform over the grid)
  int t = 0;
  while (t + 1 < A.count && blockIdx.x >= A.first_block[t + 1]) ++t;
  const unsigned long long n = A.n[t];
  const unsigned long long base = (unsigned long long)(blockIdx.x - A.first_block[t]) * ACHUNK;
  const unsigned long long end = min(base + (unsigned long long)ACHUNK, n);
  float* __restrict__ p = A.p[t];
  const float* __restrict__ g = A.g[t];
  float* __restrict__ m = A.m[t];
  float* __restrict__ v = A.v[t];
  float* __restrict__ e = A.e[t];
  float omd = A.omd;
  [[maybe_unused]] bool follow = false;      // (uniform over the grid)
  if constexpr (EDEV) {
    omd = A.omd_dev[0];
    follow = omd == 1.f;
  }
  // one element of the average from the p just formed
  auto avg = [&](float ej, float pj) {
    if constexpr (EDEV) {
      if (follow) return pj;
    }
    return ema_one(ej, pj, omd);
  };
  const bool vec_step = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0);
  const bool vec = vec_step && (((uintptr_t)e & 15) == 0);
  const unsigned long long end4 = base + ((end - base) & ~3ULL);
  unsigned am = 0, gm = 0;
  // one element: (p, g as read) -> the new p; m and v in place
  auto one = [&](bool body, float& pj, float gj, float& mj, float& vj) {
    const float gs = scale ? clip_scale(coef, gj) : gj;
    gm = max(gm, abs_bits(gs));
    const float gd = l2 ? decay_grad(gs, wdc, pj) : gs;
    if (dec) pj = decay_param(pj, s2);
    adam_one_as(body, pj, gd, mj, vj, omb1, b2, omb2, step_size, bc2s, eps);
    am = max(am, abs_bits(pj));
  };
  if (skip) {
    unsigned long long tail = base;
    if (vec_step) {
      for (unsigned long long i = base + 4ULL * threadIdx.x; i < end4; i += 4ULL * ANT) {
        const f32x4 pv = *reinterpret_cast<const f32x4*>(p + i);
        const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          am = max(am, abs_bits(pv[j]));
          gm = max(gm, abs_bits(gv[j]));
        }
      }
      tail = end4;
    }
    for (unsigned long long i = tail + threadIdx.x; i < end; i += ANT) {
      am = max(am, abs_bits(p[i]));
      gm = max(gm, abs_bits(g[i]));
    }
  } else if (vec) {
    for (unsigned long long i = base + 4ULL * threadIdx.x; i < end4; i += 4ULL * ANT) {
      f32x4 pv = *reinterpret_cast<f32x4*>(p + i), mv = *reinterpret_cast<f32x4*>(m + i);
      f32x4 vv = *reinterpret_cast<f32x4*>(v + i);
      const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pj = pv[j], mj = mv[j], vj = vv[j];
        one(true, pj, gv[j], mj, vj);
        pv[j] = pj; mv[j] = mj; vv[j] = vj;
      }
      *reinterpret_cast<f32x4*>(p + i) = pv;
      *reinterpret_cast<f32x4*>(m + i) = mv;
      *reinterpret_cast<f32x4*>(v + i) = vv;
      if (e) {
        f32x4 ev = *reinterpret_cast<f32x4*>(e + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) ev[j] = avg(ev[j], pv[j]);
        *reinterpret_cast<f32x4*>(e + i) = ev;
      }
    }
    for (unsigned long long i = end4 + threadIdx.x; i < end; i += ANT) {
      float pi = p[i];
      one(false, pi, g[i], m[i], v[i]);
      p[i] = pi;
      if (e) e[i] = avg(e[i], pi);
    }
  } else {
    for (unsigned long long i = base + threadIdx.x; i < end; i += ANT) {
      float pi = p[i];
      one(vec_step && i < end4, pi, g[i], m[i], v[i]);
      p[i] = pi;
      if (e) e[i] = avg(e[i], pi);
    }
  }
  if (A.amax[t]) block_amax_atomic<ANT>(am, A.amax[t]);
  if (A.flag[t])
    block_flag_or((gm >= NONFINITE_BITS ? (unsigned)VG_NONFINITE_GRAD : 0u) |
                      (am >= NONFINITE_BITS ? (unsigned)VG_NONFINITE_PARAM : 0u),
                  A.flag[t]);
}

}  // namespace

namespace {
template <bool EMA>
int adam_launch(const VgAdamTensor* tensors, unsigned* const* flags, int count, double beta1, double beta2, double eps,
                float step_size, float bc2s, const float* scalars, hipStream_t st, float* const* ema = nullptr,
                double ema_decay = 0.0, const float* clip_record = nullptr) {
  const float omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2);
  int i = 0;
  while (i < count) {
    std::conditional_t<EMA, AdamPackEma, AdamPack> A;
    if constexpr (EMA) A.omd = (float)(1.0 - ema_decay);
    A.count = 0;
    unsigned blocks = 0;
    while (i < count && A.count < AMAX) {
      unsigned* const flag = flags ? flags[i] : nullptr;
      float* ema_i = nullptr;
      if constexpr (EMA) ema_i = ema ? ema[i] : nullptr;      // (ema == NULL: the clip step without an average)
      const VgAdamTensor& T = tensors[i++];
      if (T.n == 0) continue;      // (its flag word is left untouched)
      if (!T.p || !T.g || !T.m || !T.v) return VG_ERR_BAD_ARG;
      const unsigned long long nb = (T.n + ACHUNK - 1) / ACHUNK;
      if (nb > 0x3fffffffULL - blocks) return VG_ERR_BAD_ARG;
      const int k = A.count++;
      A.p[k] = T.p; A.g[k] = T.g; A.m[k] = T.m; A.v[k] = T.v; A.n[k] = T.n;
      A.amax[k] = reinterpret_cast<unsigned*>(T.amax);
      A.flag[k] = flag;
      if constexpr (EMA) A.e[k] = ema_i;
      A.first_block[k] = blocks;
      blocks += (unsigned)nb;
    }
    if (A.count == 0) break;
    A.first_block[A.count] = blocks;
    if constexpr (EMA) {
      if (clip_record) {
        if (scalars)
          hipLaunchKernelGGL((adam_clip_multi_kernel<true>), dim3(blocks), dim3(ANT), 0, st, A, omb1, (float)beta2, omb2,
                             0.f, 0.f, (float)eps, scalars, clip_record);
        else
          hipLaunchKernelGGL((adam_clip_multi_kernel<false>), dim3(blocks), dim3(ANT), 0, st, A, omb1, (float)beta2, omb2,
                             step_size, bc2s, (float)eps, (const float*)nullptr, clip_record);
        VG_CHECK_LAUNCH();
        continue;
      }
    }
    if (scalars)
      hipLaunchKernelGGL((adam_multi_kernel<true, EMA>), dim3(blocks), dim3(ANT), 0, st, A, omb1, (float)beta2, omb2, 0.f,
                         0.f, (float)eps, scalars);
    else
      hipLaunchKernelGGL((adam_multi_kernel<false, EMA>), dim3(blocks), dim3(ANT), 0, st, A, omb1, (float)beta2, omb2,
                         step_size, bc2s, (float)eps, (const float*)nullptr);
    VG_CHECK_LAUNCH();
  }
  return 0;
}
}  // namespace

extern "C" int vg_adam_step_checked(const VgAdamTensor* tensors, int count, double lr, double beta1, double beta2,
                                    double eps, double bias_correction1, double bias_correction2_sqrt,
                                    unsigned* const* nonfinite, void* stream) {
  if (count < 0 || (count > 0 && !tensors) || !(bias_correction1 > 0.0) || !(bias_correction2_sqrt > 0.0))
    return VG_ERR_BAD_ARG;
  // scalars are formed in double and rounded once, as torch does with its Python-side hyper-parameters
  return adam_launch<false>(tensors, nonfinite, count, beta1, beta2, eps, (float)(lr / bias_correction1),
                            (float)bias_correction2_sqrt, nullptr, (hipStream_t)stream);
}

extern "C" int vg_adam_step_ema(const VgAdamTensor* tensors, int count, double lr, double beta1, double beta2, double eps,
                                double bias_correction1, double bias_correction2_sqrt, unsigned* const* nonfinite,
                                float* const* ema, double ema_decay, void* stream) {
  if (count < 0 || (count > 0 && !tensors) || !(bias_correction1 > 0.0) || !(bias_correction2_sqrt > 0.0) || !ema ||
      !(ema_decay > 0.0 && ema_decay < 1.0))
    return VG_ERR_BAD_ARG;
  return adam_launch<true>(tensors, nonfinite, count, beta1, beta2, eps, (float)(lr / bias_correction1),
                           (float)bias_correction2_sqrt, nullptr, (hipStream_t)stream, ema, ema_decay);
}

extern "C" int vg_adam_step(const VgAdamTensor* tensors, int count, double lr, double beta1, double beta2, double eps,
                            double bias_correction1, double bias_correction2_sqrt, void* stream) {
  return vg_adam_step_checked(tensors, count, lr, beta1, beta2, eps, bias_correction1, bias_correction2_sqrt, nullptr,
                              stream);
}

extern "C" int vg_adam_prepare(double step, double* step_dev, int advance_device_counter, double lr, double beta1,
                               double beta2, float* scalars, void* stream) {
  if (!scalars || (advance_device_counter ? !step_dev : !(step >= 1.0)) || !(beta1 >= 0.0 && beta1 < 1.0) ||
      !(beta2 >= 0.0 && beta2 < 1.0))
    return VG_ERR_BAD_ARG;
  hipLaunchKernelGGL(adam_prepare_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step, step_dev,
                     advance_device_counter ? 1 : 0, lr, beta1, beta2, scalars);
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int vg_adam_step_dev_checked(const VgAdamTensor* tensors, int count, double beta1, double beta2, double eps,
                                        const float* scalars, unsigned* const* nonfinite, void* stream) {
  if (count < 0 || (count > 0 && !tensors) || !scalars) return VG_ERR_BAD_ARG;
  return adam_launch<false>(tensors, nonfinite, count, beta1, beta2, eps, 0.f, 0.f, scalars, (hipStream_t)stream);
}

extern "C" int vg_adam_step_dev_ema(const VgAdamTensor* tensors, int count, double beta1, double beta2, double eps,
                                    const float* scalars, unsigned* const* nonfinite, float* const* ema,
                                    double ema_decay, void* stream) {
  if (count < 0 || (count > 0 && !tensors) || !scalars || !ema || !(ema_decay > 0.0 && ema_decay < 1.0))
    return VG_ERR_BAD_ARG;
  return adam_launch<true>(tensors, nonfinite, count, beta1, beta2, eps, 0.f, 0.f, scalars, (hipStream_t)stream, ema,
                           ema_decay);
}

extern "C" int vg_adam_step_dev(const VgAdamTensor* tensors, int count, double beta1, double beta2, double eps,
                                const float* scalars, void* stream) {
  return vg_adam_step_dev_checked(tensors, count, beta1, beta2, eps, scalars, nullptr, stream);
}

// ---- clipping by global norm / skipping a non-finite step: the entry points --------------------------------------------
extern "C" size_t vg_grad_sumsq_partials(const size_t* n, int count) {
  size_t slots = 0;
  if (!n) return 0;
  for (int i = 0; i < count; ++i) slots += (n[i] + ACHUNK - 1) / ACHUNK;
  return slots;
}

extern "C" int vg_grad_sumsq_multi(const float* const* grads, const size_t* n, int count, double* partials,
                                   size_t capacity, void* stream) {
  if (count < 0 || (count > 0 && (!grads || !n)) || !partials) return VG_ERR_BAD_ARG;
  if (vg_grad_sumsq_partials(n, count) > capacity) return VG_ERR_BAD_ARG;
  for (int i = 0; i < count; ++i)
    if (n[i] && (!grads[i] || (n[i] + ACHUNK - 1) / ACHUNK > 0x3fffffffULL)) return VG_ERR_BAD_ARG;
  size_t first = 0;      // this launch's first slot
  int i = 0;
  while (i < count) {
    SumsqPack A;
    A.count = 0;
    unsigned blocks = 0;
    while (i < count && A.count < AMAX) {
      const unsigned long long nb = (n[i] + ACHUNK - 1) / ACHUNK;
      if (nb == 0) { ++i; continue; }
      if (nb > 0x3fffffffULL - blocks) break;      // (a launch of its own for what does not fit this grid)
      const int k = A.count++;
      A.g[k] = grads[i];
      A.n[k] = n[i];
      A.first_block[k] = blocks;
      blocks += (unsigned)nb;
      ++i;
    }
    if (A.count == 0) break;
    A.first_block[A.count] = blocks;
    hipLaunchKernelGGL(grad_sumsq_multi_kernel, dim3(blocks), dim3(ANT), 0, (hipStream_t)stream, A, partials + first);
    VG_CHECK_LAUNCH();
    first += blocks;
  }
  return 0;
}

extern "C" int vg_grad_clip_finalize(const double* partials, size_t n_partials, double max_norm, int skip_nonfinite,
                                     float* record, void* stream) {
  if (!partials || !record || max_norm != max_norm) return VG_ERR_BAD_ARG;
  hipLaunchKernelGGL(grad_clip_finalize_kernel, dim3(1), dim3(ANT), 0, (hipStream_t)stream, partials,
                     (unsigned long long)n_partials, max_norm, skip_nonfinite ? 1 : 0, record);
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int vg_adam_step_clip(const VgAdamTensor* tensors, int count, double lr, double beta1, double beta2, double eps,
                                 double bias_correction1, double bias_correction2_sqrt, unsigned* const* nonfinite,
                                 float* const* ema, double ema_decay, const float* clip_record, void* stream) {
  if (count < 0 || (count > 0 && !tensors) || !(bias_correction1 > 0.0) || !(bias_correction2_sqrt > 0.0) ||
      !clip_record || (ema && !(ema_decay > 0.0 && ema_decay < 1.0)))
    return VG_ERR_BAD_ARG;
  return adam_launch<true>(tensors, nonfinite, count, beta1, beta2, eps, (float)(lr / bias_correction1),
                           (float)bias_correction2_sqrt, nullptr, (hipStream_t)stream, ema, ema ? ema_decay : 0.5,
                           clip_record);
}

extern "C" int vg_adam_step_dev_clip(const VgAdamTensor* tensors, int count, double beta1, double beta2, double eps,
                                     const float* scalars, unsigned* const* nonfinite, float* const* ema,
                                     double ema_decay, const float* clip_record, void* stream) {
  if (count < 0 || (count > 0 && !tensors) || !scalars || !clip_record ||
      (ema && !(ema_decay > 0.0 && ema_decay < 1.0)))
    return VG_ERR_BAD_ARG;
  return adam_launch<true>(tensors, nonfinite, count, beta1, beta2, eps, 0.f, 0.f, scalars, (hipStream_t)stream, ema,
                           ema ? ema_decay : 0.5, clip_record);
}

// ---- weight decay inside the step, hyper-parameters on the device: the entry points -----------------------------------
namespace {
// EDEV (with `scalars` only): (float)(1 - decay) is read from the device word `ema_omd`, ema_decay is not used.
template <bool EDEV = false>
int adam_decay_launch(const VgAdamTensor* tensors, unsigned* const* flags, int count, double beta1, double beta2,
                      double eps, float step_size, float bc2s, float s2, float wdc, const float* scalars, hipStream_t st,
                      float* const* ema, double ema_decay, const float* clip_record, const float* ema_omd = nullptr) {
  const float omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2);
  int i = 0;
  while (i < count) {
    std::conditional_t<EDEV, AdamPackDecayDev, AdamPackDecay> A;
    A.omd = (float)(1.0 - ema_decay);
    if constexpr (EDEV) A.omd_dev = ema_omd;
    A.s2 = s2;
    A.wdc = wdc;
    A.count = 0;
    unsigned blocks = 0;
    while (i < count && A.count < AMAX) {
      unsigned* const flag = flags ? flags[i] : nullptr;
      float* const ema_i = ema ? ema[i] : nullptr;
      const VgAdamTensor& T = tensors[i++];
      if (T.n == 0) continue;      // (its flag word is left untouched)
      if (!T.p || !T.g || !T.m || !T.v) return VG_ERR_BAD_ARG;
      const unsigned long long nb = (T.n + ACHUNK - 1) / ACHUNK;
      if (nb > 0x3fffffffULL - blocks) return VG_ERR_BAD_ARG;
      const int k = A.count++;
      A.p[k] = T.p; A.g[k] = T.g; A.m[k] = T.m; A.v[k] = T.v; A.n[k] = T.n;
      A.amax[k] = reinterpret_cast<unsigned*>(T.amax);
      A.flag[k] = flag;
      A.e[k] = ema_i;
      A.first_block[k] = blocks;
      blocks += (unsigned)nb;
    }
    if (A.count == 0) break;
    A.first_block[A.count] = blocks;
    if constexpr (EDEV)
      hipLaunchKernelGGL((adam_decay_multi_kernel<true, true>), dim3(blocks), dim3(ANT), 0, st, A, omb1, (float)beta2,
                         omb2, 0.f, 0.f, (float)eps, scalars, clip_record);
    else if (scalars)
      hipLaunchKernelGGL((adam_decay_multi_kernel<true>), dim3(blocks), dim3(ANT), 0, st, A, omb1, (float)beta2, omb2, 0.f,
                         0.f, (float)eps, scalars, clip_record);
    else
      hipLaunchKernelGGL((adam_decay_multi_kernel<false>), dim3(blocks), dim3(ANT), 0, st, A, omb1, (float)beta2, omb2,
                         step_size, bc2s, (float)eps, (const float*)nullptr, clip_record);
    VG_CHECK_LAUNCH();
  }
  return 0;
}
}  // namespace

extern "C" int vg_adam_prepare_dev(double step, double* step_dev, int advance_device_counter, const double* hyper,
                                   int decoupled, double beta1, double beta2, float* scalars, void* stream) {
  if (!hyper || !scalars || (advance_device_counter ? !step_dev : !(step >= 1.0)) || !(beta1 >= 0.0 && beta1 < 1.0) ||
      !(beta2 >= 0.0 && beta2 < 1.0))
    return VG_ERR_BAD_ARG;
  hipLaunchKernelGGL(adam_prepare_dev_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step, step_dev,
                     advance_device_counter ? 1 : 0, hyper, decoupled ? 1 : 0, beta1, beta2, scalars);
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int vg_adam_step_decay(const VgAdamTensor* tensors, int count, double lr, double beta1, double beta2,
                                  double eps, double bias_correction1, double bias_correction2_sqrt,
                                  unsigned* const* nonfinite, float* const* ema, double ema_decay,
                                  const float* clip_record, double weight_decay, int decoupled, void* stream) {
  if (count < 0 || (count > 0 && !tensors) || !(bias_correction1 > 0.0) || !(bias_correction2_sqrt > 0.0) ||
      (ema && !(ema_decay > 0.0 && ema_decay < 1.0)) || !(weight_decay >= 0.0))      // (a NaN fails the comparison)
    return VG_ERR_BAD_ARG;
  // the two words vg_adam_prepare_dev would leave in scalars[2..3]
  const float s2 = (decoupled && weight_decay != 0.0) ? decoupled_factor(lr, weight_decay) : 1.f;
  const float wdc = decoupled ? 0.f : (float)weight_decay;
  return adam_decay_launch(tensors, nonfinite, count, beta1, beta2, eps, (float)(lr / bias_correction1),
                           (float)bias_correction2_sqrt, s2, wdc, nullptr, (hipStream_t)stream, ema,
                           ema ? ema_decay : 0.5, clip_record);
}

extern "C" int vg_adam_step_dev_decay(const VgAdamTensor* tensors, int count, double beta1, double beta2, double eps,
                                      const float* scalars, unsigned* const* nonfinite, float* const* ema,
                                      double ema_decay, const float* clip_record, void* stream) {
  if (count < 0 || (count > 0 && !tensors) || !scalars || (ema && !(ema_decay > 0.0 && ema_decay < 1.0)))
    return VG_ERR_BAD_ARG;
  return adam_decay_launch(tensors, nonfinite, count, beta1, beta2, eps, 0.f, 0.f, 1.f, 0.f, scalars,
                           (hipStream_t)stream, ema, ema ? ema_decay : 0.5, clip_record);
}

extern "C" int vg_adam_step_dev_ema_dev(const VgAdamTensor* tensors, int count, double beta1, double beta2, double eps,
                                        const float* scalars, unsigned* const* nonfinite, float* const* ema,
                                        const float* ema_omd, const float* clip_record, void* stream) {
  if (count < 0 || (count > 0 && !tensors) || !scalars || !ema || !ema_omd) return VG_ERR_BAD_ARG;
  return adam_decay_launch<true>(tensors, nonfinite, count, beta1, beta2, eps, 0.f, 0.f, 1.f, 0.f, scalars,
                                 (hipStream_t)stream, ema, 0.5, clip_record, ema_omd);
}
