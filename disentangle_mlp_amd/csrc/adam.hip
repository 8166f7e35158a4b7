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
// the pointers allow it).  Bias corrections are computed on the host in double precision, or by a one-thread prepare
// kernel from a device step counter (steps captured in a HIP graph).
//
// Two step kernels stand behind the entry points; both emit max |p| into the tensor's amax word and OR
// VG_NONFINITE_GRAD / VG_NONFINITE_PARAM -- |x| as bits >= 0x7f800000 among the gradients read / the parameters
// written -- into the tensor's caller-owned flag word (one wavefront / LDS reduction per workgroup, one atomicOr per
// workgroup that saw something, none in a clean step), where the caller hands such words in.
//
// The plain kernel (adam_multi_kernel<DEV>; vg_adam_step, _checked, _dev, _dev_checked): the step above and nothing
// else.  It is the default path and the yardstick: compiled under the default contraction, its bits are what the tests
// root every other entry point in.  By itself it DETECTS an inf / NaN, it does not skip the update -- a skip needs a
// grid-wide answer before the first store; once a bit is up the weights are poisoned and the last good checkpoint is
// the way back.
//
// The feature kernel (adam_multi_feature_kernel; every other entry point): the same step, element by element the plain
// kernel's bits (adam_one_as), with four features that are each a uniform run-time test and cost nothing when off:
//
//   weight EMA      e[t] != NULL: the thread that has just formed an element's new p also moves the element's running
//                   average, e <- e + (1 - decay) (p_new - e) (torch's lerp form for weights below 0.5), from the value
//                   in its register: 8 more bytes per parameter instead of the 12 of a separate pass.  An inf / NaN in p
//                   goes into e unfiltered.  (1 - decay) is a host float in the pack, or -- omd_dev != NULL -- a device
//                   word a warm-up changes between the replays of a captured step; the device word 1.0f ("follow the
//                   weights") stores p itself, since e + 1 (p - e) is not p in fp32.
//   clip / skip     record != NULL: every gradient is used as gs = coef * g (one fp32 rounding, that of g.mul_(coef)),
//                   4 more bytes per parameter instead of the 12 of torch's recipe.  With the record's skip word up
//                   nothing is stored to p, m, v or an average; max |p| and the flag of the tensor that holds the
//                   inf / NaN are still emitted.  The record comes from one deterministic pass over the gradients in
//                   front of the step (vg_grad_sumsq_multi: fp64 squares and sums from the thread level on, one partial
//                   per workgroup in a slot of its own, no atomics) and a one-workgroup kernel that adds the partials in
//                   a fixed order (vg_grad_clip_finalize: norm, coefficient min(1, max_norm / (norm + 1e-6)) formed in
//                   double, skip word, running count of skips).
//   weight decay    one more register operation per element in front of the update, no memory traffic: coupled (L2),
//                   wdc != 0: gd = gs + (wdc * p), a rounded product and a rounded sum; decoupled (AdamW), s2 != 1:
//                   pd = p * s2 with s2 = (float)(1 - lr * wd) formed in double.  With wd == 0 neither term is formed
//                   (no 0 * inf).  s2 / wdc are host floats in the pack, or -- decay_dev -- scalars[2..3] as
//                   vg_adam_prepare_dev leaves them from a device pair [lr, weight_decay] a schedule changes between
//                   replays.
//
//   entry point                 scalars             EMA                       record      decay
//   vg_adam_step_ema            host                required, host decay      --          --
//   vg_adam_step_dev_ema        device, 2 words     required, host decay      --          --
//   vg_adam_step_clip           host                optional, host decay      required    --
//   vg_adam_step_dev_clip       device, 2 words     optional, host decay      required    --
//   vg_adam_step_decay          host                optional, host decay      optional    host (weight_decay, decoupled)
//   vg_adam_step_dev_decay      device, 4 words     optional, host decay      optional    scalars[2..3]
//   vg_adam_step_dev_ema_dev    device, 4 words     required, device word     optional    scalars[2..3]
#include "common.hpp"
#include "vaegan_hip.h"

namespace {

constexpr int ANT = 256, ACHUNK = 8192, AMAX = 24;
constexpr unsigned long long MAX_GRID = 0x3fffffffULL;      // workgroups of one launch
static_assert(VG_FLAG_GRAD == VG_NONFINITE_GRAD && VG_FLAG_PARAM == VG_NONFINITE_PARAM, "common.hpp's flag bits");

__host__ __device__ constexpr unsigned long long chunks_of(unsigned long long n) { return (n + ACHUNK - 1) / ACHUNK; }

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

// The pack of the feature kernel.
struct AdamFeaturePack : AdamPack {
  float* e[AMAX];           // per tensor, may be NULL: that tensor is not averaged
  float omd;                // (float)(1 - decay) formed on the host; used when omd_dev == NULL
  const float* omd_dev;     // NULL, or the device word that holds (float)(1 - decay)
  float s2;                 // decoupled decay: p is multiplied by this before the update; 1: not
  float wdc;                // coupled decay: this times p is added to the gradient; 0: not
  int decay_dev;            // s2 / wdc are read from scalars[2..3] (vg_adam_prepare_dev wrote them) instead
};

// The workgroup's tensor and its ACHUNK elements [base, end) of it (uniform over the workgroup).
struct Chunk {
  int t;
  unsigned long long base, end;
};

template <typename Pack>
__device__ __forceinline__ Chunk chunk_of_block(const Pack& A) {
  int t = 0;
  while (t + 1 < A.count && blockIdx.x >= A.first_block[t + 1]) ++t;
  const unsigned long long n = A.n[t];
  const unsigned long long base = (unsigned long long)(blockIdx.x - A.first_block[t]) * ACHUNK;
  return {t, base, min(base + (unsigned long long)ACHUNK, n)};
}

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float omb1, float b2, float omb2,
                                         float step_size, float bc2s, float eps) {
  m = m + omb1 * (g - m);
  v = b2 * v + omb2 * g * g;
  const float denom = sqrtf(v) / bc2s + eps;
  p = p - step_size * (m / denom);
}

// adam_one for the feature kernel, which must give the bits of the plain kernel element by element -- wherever its
// own alignment rule (the EMA pointer counts) sends the element: adam_one_as of common.hpp.

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

// (block_flag_or and emit_amax_and_flags, the end of both step kernels: common.hpp)

// ---- the plain step ----------------------------------------------------------------------------------------------------
// Its three loops are the reference bits of every other entry point (adam_one_as names the compiler's choices in them).
template <bool DEV>
__global__ __launch_bounds__(ANT) void adam_multi_kernel(AdamPack A, float omb1, float b2, float omb2, float step_size,
                                                        float bc2s, float eps, const float* __restrict__ scalars) {
  if constexpr (DEV) {
    step_size = scalars[0];
    bc2s = scalars[1];
  }
  const Chunk c = chunk_of_block(A);
  const int t = c.t;
  const unsigned long long base = c.base, end = c.end;
  float* __restrict__ p = A.p[t];
  const float* __restrict__ g = A.g[t];
  float* __restrict__ m = A.m[t];
  float* __restrict__ v = A.v[t];
  const bool vec = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0);
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
        adam_one(pj, gv[j], mj, vj, omb1, b2, omb2, step_size, bc2s, eps);
        pv[j] = pj; mv[j] = mj; vv[j] = vj;
        am = max(am, abs_bits(pj));
        gm = max(gm, abs_bits(gv[j]));
      }
      *reinterpret_cast<f32x4*>(p + i) = pv;
      *reinterpret_cast<f32x4*>(m + i) = mv;
      *reinterpret_cast<f32x4*>(v + i) = vv;
    }
    for (unsigned long long i = end4 + threadIdx.x; i < end; i += ANT) {
      const float gi = g[i];
      adam_one(p[i], gi, m[i], v[i], omb1, b2, omb2, step_size, bc2s, eps);
      am = max(am, abs_bits(p[i]));
      gm = max(gm, abs_bits(gi));
    }
  } else {
    for (unsigned long long i = base + threadIdx.x; i < end; i += ANT) {
      const float gi = g[i];
      adam_one(p[i], gi, m[i], v[i], omb1, b2, omb2, step_size, bc2s, eps);
      am = max(am, abs_bits(p[i]));
      gm = max(gm, abs_bits(gi));
    }
  }
  emit_amax_and_flags<ANT>(am, gm, A.amax[t], A.flag[t]);      // (t is uniform over the workgroup)
}

// ---- clipping by global norm, skipping a non-finite step --------------------------------------------------------------
// The record vg_grad_clip_finalize writes and the feature kernel reads: four 32-bit words.
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
  const Chunk c = chunk_of_block(A);
  const unsigned long long base = c.base, end = c.end;
  const float* __restrict__ g = A.g[c.t];
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

// ---- the step with features -------------------------------------------------------------------------------------------
// gs = coef * g, rounded once as g.mul_(coef) rounds it: kept from being fused into the m update that follows.
__device__ __forceinline__ float clip_scale(float coef, float g) {
#pragma clang fp contract(off)
  return coef * g;
}

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

// The plain step with the weight EMA, the clip record and the weight decay, each a test that is uniform over the grid
// (per tensor for e): `scalars` NULL -- step_size / bc2s are the arguments; `record` NULL -- gs = g, nothing is
// skipped; s2 == 1 and wdc == 0 -- nothing decays; e[t] NULL -- the tensor is not averaged.  With everything off an
// element takes the plain kernel's operations and nothing else: adam_one_as and its `body` rule give the plain
// kernel's bits on (p, g) as this kernel has prepared them.  With the record's skip word up p and g are read for
// max |p| and the flag words, nothing is stored to p, m, v, e.  The GRAD bit is judged on gs -- the gradient the caller
// handed in, scaled (unscaled in a skipped step) -- not on gd, which an inf WEIGHT would poison as well; amax and the
// PARAM bit on the final p.
__global__ __launch_bounds__(ANT) void adam_multi_feature_kernel(AdamFeaturePack A, float omb1, float b2, float omb2,
                                                                float step_size, float bc2s, float eps,
                                                                const float* __restrict__ scalars,
                                                                const float* __restrict__ record) {
  float s2 = A.s2, wdc = A.wdc;
  if (scalars) {
    step_size = scalars[0];
    bc2s = scalars[1];
  }
  // scalars[2..3] exist only behind vg_adam_prepare_dev: vg_adam_prepare leaves a two-word buffer
  if (A.decay_dev) {
    s2 = scalars[2];
    wdc = scalars[3];
  }
  const bool dec = s2 != 1.f, l2 = wdc != 0.f;
  const bool scale = record != nullptr;
  const float coef = scale ? record[REC_COEF] : 1.f;
  const bool skip = scale && reinterpret_cast<const unsigned*>(record)[REC_SKIP] != 0u;
  const Chunk c = chunk_of_block(A);
  const int t = c.t;
  const unsigned long long base = c.base, end = c.end;
  float* __restrict__ p = A.p[t];
  const float* __restrict__ g = A.g[t];
  float* __restrict__ m = A.m[t];
  float* __restrict__ v = A.v[t];
  float* __restrict__ e = A.e[t];
  const float omd = A.omd_dev ? A.omd_dev[0] : A.omd;
  // "follow the weights" is the DEVICE word's 1.0f alone: a host (float)(1 - decay) that rounds to 1 takes ema_one
  const bool follow = A.omd_dev && omd == 1.f;
  // one element of the average from the p just formed
  auto avg = [&](float ej, float pj) { return follow ? pj : ema_one(ej, pj, omd); };
  const bool vec_step = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0);      // the plain kernel's choice
  const bool vec = vec_step && (((uintptr_t)e & 15) == 0);      // NULL passes
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
      float pi = p[i];      // the average takes the new p from this register
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
  emit_amax_and_flags<ANT>(am, gm, A.amax[t], A.flag[t]);
}

// ---- packing and launching -------------------------------------------------------------------------------------------
// What an entry point asks for.  The first block is every step's; `feature` and what follows select the feature
// kernel and what it turns on (the defaults turn everything off).
struct StepArgs {
  const VgAdamTensor* tensors;
  int count;
  unsigned* const* flags;               // NULL, or `count` flag words
  double beta1, beta2, eps;
  float step_size, bc2s;                // host scalars; not read when `scalars` is given
  const float* scalars;                 // NULL, or the device scalars
  hipStream_t st;
  bool feature = false;
  float* const* ema = nullptr;          // NULL (no average at all), or `count` averages
  double ema_decay = 0.5;               // (0.5: a placeholder where nothing is averaged, or the decay is on the device)
  const float* ema_omd = nullptr;       // the device word with (float)(1 - decay): ema_decay is not used
  const float* clip_record = nullptr;
  float s2 = 1.f, wdc = 0.f;            // the two words vg_adam_prepare_dev would leave in scalars[2..3]
  bool decay_dev = false;               // ... or those of `scalars` themselves
};

StepArgs host_step(const VgAdamTensor* tensors, int count, unsigned* const* flags, double lr, double beta1, double beta2,
                   double eps, double bias_correction1, double bias_correction2_sqrt, void* stream) {
  // scalars are formed in double and rounded once, as torch does with its Python-side hyper-parameters
  return {tensors, count, flags, beta1, beta2, eps, (float)(lr / bias_correction1), (float)bias_correction2_sqrt,
          nullptr, (hipStream_t)stream};
}

StepArgs dev_step(const VgAdamTensor* tensors, int count, unsigned* const* flags, double beta1, double beta2, double eps,
                  const float* scalars, void* stream) {
  return {tensors, count, flags, beta1, beta2, eps, 0.f, 0.f, scalars, (hipStream_t)stream};
}

int adam_launch(const StepArgs& S) {
  const float omb1 = (float)(1.0 - S.beta1), b2 = (float)S.beta2, omb2 = (float)(1.0 - S.beta2), eps = (float)S.eps;
  int i = 0;
  while (i < S.count) {
    AdamFeaturePack A;
    A.omd = (float)(1.0 - S.ema_decay);
    A.omd_dev = S.ema_omd;
    A.s2 = S.s2;
    A.wdc = S.wdc;
    A.decay_dev = S.decay_dev ? 1 : 0;
    A.count = 0;
    unsigned blocks = 0;
    while (i < S.count && A.count < AMAX) {
      unsigned* const flag = S.flags ? S.flags[i] : nullptr;
      float* const ema_i = S.ema ? S.ema[i] : nullptr;
      const VgAdamTensor& T = S.tensors[i++];
      if (T.n == 0) continue;      // (its flag word is left untouched)
      if (!T.p || !T.g || !T.m || !T.v) return VG_ERR_BAD_ARG;
      const unsigned long long nb = chunks_of(T.n);
      if (nb > MAX_GRID - blocks) return VG_ERR_BAD_ARG;
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
    if (S.feature)
      hipLaunchKernelGGL(adam_multi_feature_kernel, dim3(blocks), dim3(ANT), 0, S.st, A, omb1, b2, omb2, S.step_size,
                         S.bc2s, eps, S.scalars, S.clip_record);
    else if (S.scalars)      // (the plain kernels take the pack's base)
      hipLaunchKernelGGL(adam_multi_kernel<true>, dim3(blocks), dim3(ANT), 0, S.st, static_cast<const AdamPack&>(A), omb1,
                         b2, omb2, 0.f, 0.f, eps, S.scalars);
    else
      hipLaunchKernelGGL(adam_multi_kernel<false>, dim3(blocks), dim3(ANT), 0, S.st, static_cast<const AdamPack&>(A), omb1,
                         b2, omb2, S.step_size, S.bc2s, eps, (const float*)nullptr);
    VG_CHECK_LAUNCH();
  }
  return 0;
}

bool bad_tensors(const VgAdamTensor* tensors, int count) { return count < 0 || (count > 0 && !tensors); }
bool bad_decay(double ema_decay) { return !(ema_decay > 0.0 && ema_decay < 1.0); }      // (a NaN is bad)

}  // namespace

extern "C" int vg_adam_step_checked(const VgAdamTensor* tensors, int count, double lr, double beta1, double beta2,
                                    double eps, double bias_correction1, double bias_correction2_sqrt,
                                    unsigned* const* nonfinite, void* stream) {
  if (bad_tensors(tensors, count) || !(bias_correction1 > 0.0) || !(bias_correction2_sqrt > 0.0)) return VG_ERR_BAD_ARG;
  return adam_launch(
      host_step(tensors, count, nonfinite, lr, beta1, beta2, eps, bias_correction1, bias_correction2_sqrt, stream));
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
  if (bad_tensors(tensors, count) || !scalars) return VG_ERR_BAD_ARG;
  return adam_launch(dev_step(tensors, count, nonfinite, beta1, beta2, eps, scalars, stream));
}

extern "C" int vg_adam_step_dev(const VgAdamTensor* tensors, int count, double beta1, double beta2, double eps,
                                const float* scalars, void* stream) {
  return vg_adam_step_dev_checked(tensors, count, beta1, beta2, eps, scalars, nullptr, stream);
}

// ---- weight EMA: the entry points --------------------------------------------------------------------------------------
extern "C" int vg_adam_step_ema(const VgAdamTensor* tensors, int count, double lr, double beta1, double beta2, double eps,
                                double bias_correction1, double bias_correction2_sqrt, unsigned* const* nonfinite,
                                float* const* ema, double ema_decay, void* stream) {
  if (bad_tensors(tensors, count) || !(bias_correction1 > 0.0) || !(bias_correction2_sqrt > 0.0) || !ema ||
      bad_decay(ema_decay))
    return VG_ERR_BAD_ARG;
  StepArgs S = host_step(tensors, count, nonfinite, lr, beta1, beta2, eps, bias_correction1, bias_correction2_sqrt, stream);
  S.feature = true;
  S.ema = ema;
  S.ema_decay = ema_decay;
  return adam_launch(S);
}

extern "C" int vg_adam_step_dev_ema(const VgAdamTensor* tensors, int count, double beta1, double beta2, double eps,
                                    const float* scalars, unsigned* const* nonfinite, float* const* ema,
                                    double ema_decay, void* stream) {
  if (bad_tensors(tensors, count) || !scalars || !ema || bad_decay(ema_decay)) return VG_ERR_BAD_ARG;
  StepArgs S = dev_step(tensors, count, nonfinite, beta1, beta2, eps, scalars, stream);
  S.feature = true;
  S.ema = ema;
  S.ema_decay = ema_decay;
  return adam_launch(S);
}

// ---- clipping by global norm / skipping a non-finite step: the entry points --------------------------------------------
extern "C" size_t vg_grad_sumsq_partials(const size_t* n, int count) {
  size_t slots = 0;
  if (!n) return 0;
  for (int i = 0; i < count; ++i) slots += chunks_of(n[i]);
  return slots;
}

extern "C" int vg_grad_sumsq_multi(const float* const* grads, const size_t* n, int count, double* partials,
                                   size_t capacity, void* stream) {
  if (count < 0 || (count > 0 && (!grads || !n)) || !partials) return VG_ERR_BAD_ARG;
  if (vg_grad_sumsq_partials(n, count) > capacity) return VG_ERR_BAD_ARG;
  for (int i = 0; i < count; ++i)
    if (n[i] && (!grads[i] || chunks_of(n[i]) > MAX_GRID)) return VG_ERR_BAD_ARG;
  size_t first = 0;      // this launch's first slot
  int i = 0;
  while (i < count) {
    SumsqPack A;
    A.count = 0;
    unsigned blocks = 0;
    while (i < count && A.count < AMAX) {
      const unsigned long long nb = chunks_of(n[i]);
      if (nb == 0) { ++i; continue; }
      if (nb > MAX_GRID - blocks) break;      // (a launch of its own for what does not fit this grid)
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
  if (bad_tensors(tensors, count) || !(bias_correction1 > 0.0) || !(bias_correction2_sqrt > 0.0) || !clip_record ||
      (ema && bad_decay(ema_decay)))
    return VG_ERR_BAD_ARG;
  StepArgs S = host_step(tensors, count, nonfinite, lr, beta1, beta2, eps, bias_correction1, bias_correction2_sqrt, stream);
  S.feature = true;
  S.ema = ema;
  S.ema_decay = ema ? ema_decay : 0.5;
  S.clip_record = clip_record;
  return adam_launch(S);
}

extern "C" int vg_adam_step_dev_clip(const VgAdamTensor* tensors, int count, double beta1, double beta2, double eps,
                                     const float* scalars, unsigned* const* nonfinite, float* const* ema,
                                     double ema_decay, const float* clip_record, void* stream) {
  if (bad_tensors(tensors, count) || !scalars || !clip_record || (ema && bad_decay(ema_decay))) return VG_ERR_BAD_ARG;
  StepArgs S = dev_step(tensors, count, nonfinite, beta1, beta2, eps, scalars, stream);
  S.feature = true;
  S.ema = ema;
  S.ema_decay = ema ? ema_decay : 0.5;
  S.clip_record = clip_record;
  return adam_launch(S);
}

// ---- weight decay inside the step, hyper-parameters on the device: the entry points -----------------------------------
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
  if (bad_tensors(tensors, count) || !(bias_correction1 > 0.0) || !(bias_correction2_sqrt > 0.0) ||
      (ema && bad_decay(ema_decay)) || !(weight_decay >= 0.0))      // (a NaN fails the comparison)
    return VG_ERR_BAD_ARG;
  StepArgs S = host_step(tensors, count, nonfinite, lr, beta1, beta2, eps, bias_correction1, bias_correction2_sqrt, stream);
  S.feature = true;
  S.ema = ema;
  S.ema_decay = ema ? ema_decay : 0.5;
  S.clip_record = clip_record;
  S.s2 = (decoupled && weight_decay != 0.0) ? decoupled_factor(lr, weight_decay) : 1.f;
  S.wdc = decoupled ? 0.f : (float)weight_decay;
  return adam_launch(S);
}

extern "C" int vg_adam_step_dev_decay(const VgAdamTensor* tensors, int count, double beta1, double beta2, double eps,
                                      const float* scalars, unsigned* const* nonfinite, float* const* ema,
                                      double ema_decay, const float* clip_record, void* stream) {
  if (bad_tensors(tensors, count) || !scalars || (ema && bad_decay(ema_decay))) return VG_ERR_BAD_ARG;
  StepArgs S = dev_step(tensors, count, nonfinite, beta1, beta2, eps, scalars, stream);
  S.feature = true;
  S.ema = ema;
  S.ema_decay = ema ? ema_decay : 0.5;
  S.clip_record = clip_record;
  S.decay_dev = true;
  return adam_launch(S);
}

extern "C" int vg_adam_step_dev_ema_dev(const VgAdamTensor* tensors, int count, double beta1, double beta2, double eps,
                                        const float* scalars, unsigned* const* nonfinite, float* const* ema,
                                        const float* ema_omd, const float* clip_record, void* stream) {
  if (bad_tensors(tensors, count) || !scalars || !ema || !ema_omd) return VG_ERR_BAD_ARG;
  StepArgs S = dev_step(tensors, count, nonfinite, beta1, beta2, eps, scalars, stream);
  S.feature = true;
  S.ema = ema;
  S.ema_omd = ema_omd;
  S.clip_record = clip_record;
  S.decay_dev = true;
  return adam_launch(S);
}
