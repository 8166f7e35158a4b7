// BatchNorm (2-D and 1-D) fused with ReLU / LeakyReLU(0.2): train mode forward and backward, eval mode on the running
// statistics, the coefficients from a convolution's statistics slots, plus the per-channel sum used for convolution bias
// gradients.
// HBM-bound kernels: float4 coalesced streams over NCHW planes, fp64 partial sums
// reduced with 64-lane wavefront shuffles, deterministic two-stage reductions.
//
// Replaces F.batch_norm(training=True) + activation reached from
// /root/reference/models/model.py:451-458 (encoder), :462,468 (heads), :492
// (decoder preprocess), :496-505 (decoder), :390-400 (discriminator), and nn.BatchNorm*.eval() of the same modules.
//
// Every formula, walk and reduction is stated once, in the first section; the kernels below call them.  Order of the file:
// shared helpers -- train forward (with the two passes the backward shares) -- train backward (one pass, team, the plan)
// -- coefficients from slots -- eval -- the C entry points.
#include <atomic>

#include "common.hpp"
#include "vaegan_hip.h"

namespace {

// ---- shared helpers -------------------------------------------------------------------------------------------------
constexpr int NT = 256;
constexpr int NS_MAX = 64;   // slices per channel in the two-stage reductions

bool act_ok(int act) { return act >= VG_ACT_NONE && act <= VG_ACT_LRELU; }

__device__ __forceinline__ float act_fwd(float v, int act) {
  // compare + select with the NaN on the "keep v" side: a NaN stays a NaN, as in torch (v > 0 ? v : 0 made it 0, and a
  // channel whose batch mean is NaN left BatchNorm + ReLU as zeros); -inf and -0 still give +0, finite values their bits
  if (act == VG_ACT_RELU) return v <= 0.f ? 0.f : v;
  if (act == VG_ACT_LRELU) return v > 0.f ? v : 0.2f * v;
  return v;
}

// gy * act'(pre), in two forms that differ ONLY in a NaN pre-activation under ReLU / LeakyReLU: the train-mode form takes
// it for "not positive" (the gradient is 0, or 0.2 g), the eval-mode form has no derivative there and returns the NaN.
// (Train mode meets a NaN pre-activation only in a channel whose statistics are NaN, where c1 / c2 make gx NaN anyway;
// with frozen coefficients nothing else would carry it.)  Making them agree changes results: not done here.
__device__ __forceinline__ float act_grad(float pre, float g, int act) {
  if (act == VG_ACT_RELU) return pre > 0.f ? g : 0.f;
  if (act == VG_ACT_LRELU) return pre > 0.f ? g : 0.2f * g;
  return g;
}
__device__ __forceinline__ float act_slope_of(int act) { return act == VG_ACT_RELU ? 0.f : act == VG_ACT_LRELU ? 0.2f : 1.f; }
// a multiplication by 1 or by the slope (a NaN gradient stays a NaN, as act_slope keeps a NaN value)
__device__ __forceinline__ float eval_act_grad(float pre, float g, float slope) {
  const float d = pre > 0.f ? 1.f : slope;
  return (pre != pre && slope != 1.f) ? pre : g * d;
}

// Mean and biased variance of `count` values from their fp64 sums; cancellation can leave the difference below 0: clamped.
__device__ __forceinline__ void mean_and_variance(double s1, double s2, double count, double& m, double& var) {
  m = s1 / count;
  var = s2 / count - m * m;
  if (var < 0.0) var = 0.0;
}

// A channel's coefficients from its sums over `count` values (fp64): m, var (biased, clamped at 0) for the bound and the
// running statistics; mu, invstd saved for the backward; scale = gamma * invstd, shift = beta - mu * scale.
struct Coeffs {
  double m, var;
  float mu, invstd, scale, shift;
};
__device__ __forceinline__ Coeffs channel_coefficients(double s1, double s2, double count, float eps, float gamma,
                                                       float beta) {
  Coeffs k;
  mean_and_variance(s1, s2, count, k.m, k.var);
  k.mu = (float)k.m;
  k.invstd = (float)(1.0 / sqrt(k.var + (double)eps));
  k.scale = gamma * k.invstd;
  k.shift = beta - k.mu * k.scale;
  return k;
}
// ... and the running statistics they update (either may be NULL): the variance enters unbiased
__device__ __forceinline__ void update_running(float* running_mean, float* running_var, int c, const Coeffs& k, double count,
                                               float momentum) {
  if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * k.mu;
  if (running_var) {
    const double unb = count > 1.0 ? k.var * count / (count - 1.0) : k.var;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unb;
  }
}

// What a train-mode backward knows of its channel: the saved statistics and the forward's coefficients again.
struct Saved {
  float mu, is, sc, sh;
};
__device__ __forceinline__ Saved saved_coefficients(const float* mean, const float* invstd, const float* gamma,
                                                    const float* beta, int c) {
  Saved k;
  k.mu = mean[c];
  k.is = invstd[c];
  k.sc = gamma[c] * k.is;
  k.sh = beta[c] - k.mu * k.sc;
  return k;
}

// The backward's terms: xhat; the two fp64 sums of g_pre (dbeta) and g_pre * xhat (dgamma) -- the product is rounded to
// fp32 before it is added; gx = sc * (g_pre - c1 - xhat * c2), c1 = sum(g_pre) / N, c2 = sum(g_pre * xhat) / N.
__device__ __forceinline__ float bn_xhat(float x, float mu, float is) { return (x - mu) * is; }
__device__ __forceinline__ void add_grad_sums(double& s1, double& s2, float g, float x, float mu, float is) {
  s1 += g;
  s2 += (double)(g * bn_xhat(x, mu, is));
}
__device__ __forceinline__ float bn_gx(float g, float x, const Saved& k, float c1, float c2) {
  return k.sc * (g - c1 - bn_xhat(x, k.mu, k.is) * c2);
}

// dbeta / dgamma of channel c (either may be NULL) from the two sums; accumulate: added to what is there (a layer used
// twice before one backward: no add launch)
__device__ __forceinline__ void store_param_grads(float* dgamma, float* dbeta, int c, double t1, double t2, int accumulate) {
  if (dbeta) dbeta[c] = (float)t1 + (accumulate ? dbeta[c] : 0.f);
  if (dgamma) dgamma[c] = (float)t2 + (accumulate ? dgamma[c] : 0.f);
}

// The two-stage partials part[c][ns][2] (fp64): a slice's pair, and a channel's pairs added in slice order.
__device__ __forceinline__ void store_partial(double* part, int c, int ns, int k, double t1, double t2) {
  part[((size_t)c * ns + k) * 2 + 0] = t1;
  part[((size_t)c * ns + k) * 2 + 1] = t2;
}
__device__ __forceinline__ void sum_partials(const double* part, int c, int ns, double& s1, double& s2) {
  for (int k = 0; k < ns; ++k) {               // fixed order
    s1 += part[((size_t)c * ns + k) * 2];
    s2 += part[((size_t)c * ns + k) * 2 + 1];
  }
}

// Where virtual element v = b * HW + hw of channel c lies in NCHW; hw_shift >= 0: power-of-two planes, no division per load
// (64-bit in the walk, 32-bit in the register tile).
__device__ __forceinline__ int hw_shift_of(int HW) { return (HW & (HW - 1)) == 0 ? __builtin_ctz(HW) : -1; }
template <typename I>
__device__ __forceinline__ size_t plane_offset(I v, int C, int HW, int hw_shift, int c) {
  const I b = hw_shift >= 0 ? (v >> hw_shift) : v / HW, hw = v - b * HW;
  return ((size_t)b * C + c) * HW + hw;
}

// The plane walk: slice k of channel c is the virtual elements v = b * HW + hw in [k * per, (k + 1) * per) of its B planes;
// a workgroup of NT threads goes through them 16 bytes (vec) or one element per lane at a time and calls one(x, gy) on
// each (gy = 0 without HAS_G); with WRITE what it returns is stored to `out` at the same place.
// vec: four elements of a plane per 16-byte load -- the host's decision (streams_vec below): HW % 4 == 0 AND every streamed
// tensor on a 16-byte boundary.  A contiguous view at an odd offset takes the scalar loop; the one-pass backward, which
// has no scalar form, is not launched for it.
template <bool HAS_G, bool WRITE, typename F>
__device__ __forceinline__ void plane_walk(const float* x, const float* gy, float* out, int B, int C, int HW, int c, int k,
                                           long per, int vec, F one) {
  const long total = (long)B * HW;
  const long v0 = (long)k * per, v1 = min(v0 + per, total);
  const int hw_shift = hw_shift_of(HW);
  if (vec) {
    for (long v = v0 + 4L * threadIdx.x; v < v1; v += 4L * NT) {
      const size_t off = plane_offset(v, C, HW, hw_shift, c);
      const float4 xv = *reinterpret_cast<const float4*>(x + off);
      float4 gv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (HAS_G) gv = *reinterpret_cast<const float4*>(gy + off);
      if constexpr (WRITE) {
        float4 o;
        o.x = one(xv.x, gv.x);
        o.y = one(xv.y, gv.y);
        o.z = one(xv.z, gv.z);
        o.w = one(xv.w, gv.w);
        *reinterpret_cast<float4*>(out + off) = o;
      } else {
        one(xv.x, gv.x);
        one(xv.y, gv.y);
        one(xv.z, gv.z);
        one(xv.w, gv.w);
      }
    }
  } else {
    for (long v = v0 + threadIdx.x; v < v1; v += NT) {
      const size_t off = plane_offset(v, C, HW, hw_shift, c);
      if constexpr (WRITE)
        out[off] = one(x[off], HAS_G ? gy[off] : 0.f);
      else
        one(x[off], HAS_G ? gy[off] : 0.f);
    }
  }
}

// CH columns (channels) x KL lanes, thread = kl * CH + cl: every thread brings a pair of fp64 sums, the KL pairs of a
// column are added through LDS in a fixed order and are valid, on return, in the threads with kl == 0.  The order is a
// compile-time choice: serial 0 .. KL - 1, or (TREE) KL / 8 lanes that each add 8 consecutive ones, then those serially.
// Every thread of the workgroup must call it.
template <int CH, int KL, bool TREE>
__device__ __forceinline__ void column_sums(double& s1, double& s2) {
  __shared__ double r1[KL][CH], r2[KL][CH];
  const int cl = threadIdx.x % CH, kl = threadIdx.x / CH;
  r1[kl][cl] = s1;
  r2[kl][cl] = s2;
  __syncthreads();
  constexpr int LAST = TREE ? KL / 8 : KL;
  if constexpr (TREE) {
    if (kl < LAST) {
      s1 = 0.0;
      s2 = 0.0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        s1 += r1[kl * 8 + k][cl];
        s2 += r2[kl * 8 + k][cl];
      }
    }
    __syncthreads();
    if (kl < LAST) {
      r1[kl][cl] = s1;
      r2[kl][cl] = s2;
    }
    __syncthreads();
  }
  if (kl == 0) {
    s1 = 0.0;
    s2 = 0.0;
#pragma unroll
    for (int k = 0; k < LAST; ++k) {
      s1 += r1[k][cl];
      s2 += r2[k][cl];
    }
  }
}

// The same over partial sums in memory: pair k of channel c at part[(c * cs + k * ks) * 2 + {0, 1}] -- a convolution's
// fp32 statistics slots [slot][C][2] (cs = 1, ks = C; PAIR: read as one 8-byte load) or fp64 partials [c][n][2] (cs = n,
// ks = 1).  Lane kl adds every KL-th pair of [k0, k1), then column_sums.
template <int CH, int KL, bool TREE, bool PAIR, typename T>
__device__ __forceinline__ void slot_sums(const T* part, long cs, long ks, int k0, int k1, int c, int C, double& s1,
                                          double& s2) {
  static_assert(!PAIR || sizeof(T) == sizeof(float), "8-byte pairs: fp32 slots");
  const int kl = threadIdx.x / CH;
  s1 = 0.0;
  s2 = 0.0;
  if (c < C)
    for (int k = k0 + kl; k < k1; k += KL) {
      const T* p = part + ((size_t)c * cs + (size_t)k * ks) * 2;
      if constexpr (PAIR) {
        const float2 v = *reinterpret_cast<const float2*>(p);
        s1 += (double)v.x;
        s2 += (double)v.y;
      } else {
        s1 += (double)p[0];
        s2 += (double)p[1];
      }
    }
  column_sums<CH, KL, TREE>(s1, s2);
}

struct Slicing {
  int ns;        // slices per channel
  long per;      // virtual elements (b*HW+hw) per slice, multiple of 4 when HW%4==0
};
Slicing make_slicing(int B, int C, int HW) {
  const long total = (long)B * HW;
  long ns = 2048 / C;
  if (ns < 1) ns = 1;
  if (ns > NS_MAX) ns = NS_MAX;
  long per = (total + ns - 1) / ns;
  if (per < 1024) per = 1024;
  per = (per + 3) / 4 * 4;
  ns = (total + per - 1) / per;
  Slicing s;
  s.ns = (int)ns;
  s.per = per;
  return s;
}

// slices of the apply pass: >= 4096 elements per workgroup so that the per-workgroup prologue (partials
// reduction + barrier) is amortised, but enough workgroups to fill the chip
Slicing make_apply_slicing(int B, int C, int HW) {
  const long total = (long)B * HW;
  long ns = 4096 / C;
  if (ns < 1) ns = 1;
  long per = (total + ns - 1) / ns;
  if (per < 4096) per = 4096;
  per = (per + 3) / 4 * 4;
  Slicing s;
  s.per = per;
  s.ns = (int)((total + per - 1) / per);
  return s;
}

// The 16-byte loops are taken only when four elements of a plane share a load (HW % 4 == 0) and every tensor that is
// streamed starts on a 16-byte boundary (pass nullptr for one that is not there); otherwise the scalar loops.
int streams_vec(int HW, const void* a, const void* b = nullptr, const void* c = nullptr) {
  return (HW & 3) == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

// Upper bound of max |act(x * sc + sh)| over a channel of n = count values, from its sums alone (act_amax of the
// finalize kernels: what an fp16-plane convolution that applies sc / sh on load scales its input by).
//   s2, m, var: the channel's sum of x^2, mean and clamped variance (s2 / n - m^2, >= 0) as the finalize kernel computed
//   them in fp64; mu = (float)m, sc, beta: the coefficients it wrote (sh = beta - mu * sc).
//   delta: relative error of the sums -- |S2 - T2| <= delta T2 and |S1 - T1| <= delta sum |x|, T1 / T2 the exact sums.
// Samuelson: every x satisfies |x - T1/n| <= sigma sqrt(n - 1), sigma^2 = T2/n - (T1/n)^2 the EXACT variance.  `var` is
// not that: when |mean| >> sigma, S2/n - m^2 cancels, the computed variance can be ~0 while sigma is not, 1/std then
// goes up to 1/sqrt(eps), and a bound from `var` alone falls far below the data.  With q = S2/n:
//   T2/n <= q / (1 - delta),  |m - T1/n| <= delta sum|x| / n <= delta sqrt(T2/n)          (Cauchy-Schwarz)
//   sigma^2 - (q - m^2) = (T2/n - q) + (m - T1/n)(m + T1/n) <= (delta + delta (2 + delta)) T2/n <= 3.01 delta q
// (delta <= 1e-3), plus fp64 rounding of q - m^2 (< 2^-50 q); so var_up = var + (3.01 delta + 2^-50) q >= sigma^2, and
//   |x - mu| <= sqrt(var_up (n - 1)) + |T1/n - m| + |m - mu| <= sqrt(var_up (n - 1)) + 1.01 delta sqrt(q) + 2^-23 |m|.
// |x sc + sh| <= |sc| |x - mu| + |beta| + (rounding of sh: <= 2^-23 (|beta| + |mu sc|)); the consumer's fmaf and the
// final fp64 -> fp32 conversion round by 2^-24 each: (1 + 2^-20).  ReLU / LeakyReLU(0.2) only shrink magnitudes.
// Where the sums are accurate (|mean| <= 8 sigma, the slots' delta) this stays within 0.1 % of the former
// |gamma| sqrt(n) + |beta|; under cancellation it grows with sqrt(delta) |mean| instead of falling below the data.
__device__ __forceinline__ float bn_act_bound(double s2, double m, double var, double count, double delta, float mu,
                                              float sc, float beta) {
  const double q = s2 / count;
  const double var_up = var + (3.01 * delta + 0x1p-50) * q;
  const double dev = sqrt(var_up * fmax(count - 1.0, 0.0)) + 1.01 * delta * sqrt(q) + 0x1p-23 * fabs(m);
  const double asc = fabs((double)sc), ab = fabs((double)beta);
  const double b = asc * dev + ab + 0x1p-23 * (ab + asc * fabs((double)mu));
  return (float)(b * (1.0 + 0x1p-20));
}

// delta of bn_act_bound for sums made of fp32 statistics slots (each an fp32 sum in which a term goes through at most
// D = VG_STATS_SLOT_DEPTH roundings: within gamma_D <= (D + 0.01) 2^-24 of the exact sum, relative to the sum of
// magnitudes -- for the squares that is T2 itself) added in fp64 over nslots slots (and NS_MAX partials):
// (nslots + 2 NS_MAX) 2^-53 more
double slot_sums_delta(int nslots) { return (VG_STATS_SLOT_DEPTH + 1) * 0x1p-24 + (nslots + 2.0 * NS_MAX) * 0x1p-53; }

// ... and for fp64 sums of fp32 values (bn_partial_kernel<0>: x^2 is exact in fp64): count + partials additions
double fp64_sums_delta(double count) { return (count + 2.0 * NS_MAX + NT) * 0x1p-53; }

// ---- train forward, and the two passes that the backward shares with it ---------------------------------------------
// First pass.  MODE 0: sum x, sum x^2.   MODE 1: sum g_pre, sum g_pre*xhat (backward).   MODE 2: sum x only.
template <int MODE>
__global__ __launch_bounds__(NT) void bn_partial_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                        const float* __restrict__ gamma,
                                                        const float* __restrict__ beta,
                                                        const float* __restrict__ mean,
                                                        const float* __restrict__ invstd, double* __restrict__ part,
                                                        int B, int C, int HW, long per, int ns, int act, int vec) {
  __shared__ double red[NT / 64];
  const int c = blockIdx.x, k = blockIdx.y;
  double s1 = 0.0, s2 = 0.0;
  Saved co = {0.f, 0.f, 0.f, 0.f};
  if (MODE == 1) co = saved_coefficients(mean, invstd, gamma, beta, c);
  plane_walk<MODE == 1, false>(x, gy, nullptr, B, C, HW, c, k, per, vec, [&](float xv, float gv) {
    if (MODE == 0) {
      s1 += xv;
      s2 += (double)xv * xv;
    } else if (MODE == 2) {
      s1 += xv;
    } else {
      add_grad_sums(s1, s2, act_grad(fmaf(xv, co.sc, co.sh), gv, act), xv, co.mu, co.is);
    }
  });
  const double t1 = block_sum<NT>(s1, red);
  const double t2 = block_sum<NT>(s2, red);
  if (threadIdx.x == 0) store_partial(part, c, ns, k, t1, t2);
}

__global__ __launch_bounds__(NT) void channel_sum_finalize_kernel(const double* __restrict__ part, int ns, int C,
                                                                  float* __restrict__ out) {
  const int c = blockIdx.x * NT + threadIdx.x;
  if (c >= C) return;
  double s1 = 0.0, s2 = 0.0;
  sum_partials(part, c, ns, s1, s2);
  out[c] = (float)s1;
}

// Normalise (FWD) or input-gradient (BWD) pass with the per-channel finalisation folded in: a
// workgroup owns one slice of ONE channel, re-derives that channel's coefficients from the
// (<= 64) fp64 partial sums in a fixed order -- no separate finalize launch, no coefficient
// table, coefficients live in registers -- and streams its slice as float4.  The slice-0
// workgroup of a channel also writes the saved / running statistics (FWD) or dgamma / dbeta (BWD).
//   FWD: y  = act(x*sc + sh)            BWD: gx = bn_gx(g_pre, x)
template <bool BWD>
__global__ __launch_bounds__(NT) void bn_apply_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                      const double* __restrict__ part, int ns,
                                                      const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float* __restrict__ mean_io,
                                                      float* __restrict__ invstd_io,
                                                      float* __restrict__ running_mean,
                                                      float* __restrict__ running_var, float* __restrict__ dgamma,
                                                      float* __restrict__ dbeta, float* __restrict__ out, int B,
                                                      int C, int HW, long per, float eps, float momentum, int act,
                                                      int accp, unsigned* __restrict__ out_amax, int vec) {
  // vec: x, gy and out are streamed
  // out_amax (backward, may be NULL): max |gx| is added to it (common.hpp block_amax_atomic) -- the bound the fp16-plane
  // convolutions that consume gx scale it by, emitted here instead of by a pass of its own
  // `per`: elements of this channel per workgroup of THIS pass (independent of the partial pass)
  __shared__ float s_co[4];
  // slices in descending order: the sums pass before this one went through the channel's slices in ascending order (same
  // channel -> same XCD in both launches), so the end of the channel is what its L2 still holds
  const int c = blockIdx.x, k = (int)gridDim.y - 1 - (int)blockIdx.y;
  const double count = (double)B * HW;
  if (threadIdx.x < 64) {   // wavefront 0: fixed-order reduction of the slice partials
    double s1 = 0.0, s2 = 0.0;
    for (int j = threadIdx.x; j < ns; j += 64) {
      s1 += part[((size_t)c * ns + j) * 2];
      s2 += part[((size_t)c * ns + j) * 2 + 1];
    }
    s1 = wave_allsum(s1);
    s2 = wave_allsum(s2);
    if (threadIdx.x == 0) {
      if (!BWD) {
        const Coeffs co = channel_coefficients(s1, s2, count, eps, gamma[c], beta[c]);
        s_co[0] = co.scale;
        s_co[1] = co.shift;
        if (k == 0) {
          mean_io[c] = co.mu;
          invstd_io[c] = co.invstd;
          update_running(running_mean, running_var, c, co, count, momentum);
        }
      } else {
        const Saved co = saved_coefficients(mean_io, invstd_io, gamma, beta, c);
        s_co[0] = co.sc;
        s_co[1] = co.sh;
        s_co[2] = (float)(s1 / count);
        s_co[3] = (float)(s2 / count);
        if (k == 0) store_param_grads(dgamma, dbeta, c, s1, s2, accp);
      }
    }
  }
  __syncthreads();
  Saved co = {0.f, 0.f, s_co[0], s_co[1]};
  float c1 = 0.f, c2 = 0.f;
  if (BWD) {
    c1 = s_co[2];
    c2 = s_co[3];
    co.mu = mean_io[c];
    co.is = invstd_io[c];
  }
  unsigned am = 0;
  plane_walk<BWD, true>(x, gy, out, B, C, HW, c, k, per, vec, [&](float xv, float gv) -> float {
    const float pre = fmaf(xv, co.sc, co.sh);
    const float r = BWD ? bn_gx(act_grad(pre, gv, act), xv, co, c1, c2) : act_fwd(pre, act);
    am = max(am, abs_bits(r));
    return r;
  });
  if (out_amax) block_amax_atomic<NT>(am, out_amax);      // wave-uniform condition
}

// BatchNorm1d: x [B][C].  A workgroup owns 32 consecutive channels (128-byte coalesced rows);
// its 8 row-slices (threads 32*s .. 32*s+31) each sum every 8th batch row in fp64 and combine
// through LDS in a fixed order (column_sums); the normalise / gradient pass re-reads the rows from L2.
constexpr int B1_CH = 32, B1_SL = 8;

__global__ __launch_bounds__(NT) void bn1d_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float* __restrict__ y,
                                                      float* __restrict__ running_mean,
                                                      float* __restrict__ running_var, float* __restrict__ save_mean,
                                                      float* __restrict__ save_invstd, int B, int C, float eps,
                                                      float momentum, int act) {
  __shared__ float s_sc[B1_CH], s_sh[B1_CH];
  const int cl = threadIdx.x % B1_CH, sl = threadIdx.x / B1_CH;
  const int c = blockIdx.x * B1_CH + cl;
  const bool cok = c < C;
  double s1 = 0.0, s2 = 0.0;
  if (cok)
    for (int b = sl; b < B; b += B1_SL) {
      const float v = x[(size_t)b * C + c];
      s1 += v;
      s2 += (double)v * v;
    }
  column_sums<B1_CH, B1_SL, false>(s1, s2);
  if (sl == 0 && cok) {
    const Coeffs co = channel_coefficients(s1, s2, (double)B, eps, gamma[c], beta[c]);
    save_mean[c] = co.mu;
    save_invstd[c] = co.invstd;
    update_running(running_mean, running_var, c, co, (double)B, momentum);
    s_sc[cl] = co.scale;
    s_sh[cl] = co.shift;
  }
  __syncthreads();
  if (cok) {
    const float sc = s_sc[cl], sh = s_sh[cl];
    for (int b = sl; b < B; b += B1_SL) {
      const size_t o = (size_t)b * C + c;
      y[o] = act_fwd(fmaf(x[o], sc, sh), act);
    }
  }
}

constexpr int AA_U = 4;
// y = act(x * scale[c] + shift[c]): the normalise pass with given coefficients (layers whose consumer cannot apply
// them while it loads)
// hw4_shift >= 0: H*W/4 is a power of two (every layer of the reference) -- the channel is a shift and a 32-bit remainder;
// the 64-bit division per thread that this replaces made the pass run at 0.8 TB/s (20 us for 16 MB).
__global__ __launch_bounds__(NT) void affine_act_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, float* __restrict__ y, int C,
                                                        int HW, size_t n4, int act, int hw4_shift,
                                                        unsigned* __restrict__ y_amax) {
  // A workgroup walks chunks of NT * AA_U units of 16 bytes, grid-stride (<= 2048 workgroups: one maximum and one atomic
  // per workgroup, not per 4 KB); within a chunk a thread's AA_U units are NT apart (contiguous per round, all loads of
  // a chunk in flight together).
  unsigned am = 0;
  for (size_t base = (size_t)blockIdx.x * (NT * AA_U) + threadIdx.x; base < n4 + threadIdx.x;
       base += (size_t)gridDim.x * (NT * AA_U)) {
    float4 v[AA_U];
    float sc[AA_U], sh[AA_U];
#pragma unroll
    for (int u = 0; u < AA_U; ++u) {
      const size_t i0 = base + (size_t)u * NT;
      const size_t i = i0 < n4 ? i0 : n4 - 1;               // past the end: the last unit again (not stored)
      // HW % 4 == 0: the four elements share a channel
      const int c = hw4_shift >= 0 ? (int)((unsigned)(i >> hw4_shift) % (unsigned)C) : (int)(((4 * i) / HW) % C);
      sc[u] = scale[c];
      sh[u] = shift[c];
      v[u] = *reinterpret_cast<const float4*>(x + 4 * i);
    }
#pragma unroll
    for (int u = 0; u < AA_U; ++u) {
      const size_t i0 = base + (size_t)u * NT;
      float4 o;
      o.x = act_fwd(fmaf(v[u].x, sc[u], sh[u]), act);
      o.y = act_fwd(fmaf(v[u].y, sc[u], sh[u]), act);
      o.z = act_fwd(fmaf(v[u].z, sc[u], sh[u]), act);
      o.w = act_fwd(fmaf(v[u].w, sc[u], sh[u]), act);
      if (i0 < n4) *reinterpret_cast<float4*>(y + 4 * i0) = o;
      am = max(max(am, abs_bits(o.x)), max(max(abs_bits(o.y), abs_bits(o.z)), abs_bits(o.w)));
    }
  }
  if (y_amax) block_amax_atomic<NT>(am, y_amax);      // max |y| for an fp16-plane consumer (common.hpp)
}

// the same for H*W not a multiple of 4 (odd image sizes): one element per lane
__global__ __launch_bounds__(NT) void affine_act_scalar_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                               const float* __restrict__ shift, float* __restrict__ y,
                                                               int C, int HW, size_t n, int act,
                                                               unsigned* __restrict__ y_amax) {
  const size_t e0 = (size_t)blockIdx.x * NT + threadIdx.x;
  const size_t e = e0 < n ? e0 : n - 1;
  const int c = (int)((e / HW) % C);
  const float r = act_fwd(fmaf(x[e], scale[c], shift[c]), act);
  if (e0 < n) y[e] = r;
  if (y_amax) block_amax_atomic<NT>(abs_bits(r), y_amax);
}

// ---- train backward --------------------------------------------------------------------------------------------------
// Two passes: bn_partial_kernel<1> + bn_apply_kernel<true> above.  BatchNorm1d: one kernel, the geometry of bn1d_fwd_kernel.
__global__ __launch_bounds__(NT) void bn1d_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                      const float* __restrict__ gamma,
                                                      const float* __restrict__ beta,
                                                      const float* __restrict__ mean,
                                                      const float* __restrict__ invstd, float* __restrict__ gx,
                                                      float* __restrict__ dgamma, float* __restrict__ dbeta, int B,
                                                      int C, int act, int accp, unsigned* __restrict__ gx_amax) {
  __shared__ float s_c1[B1_CH], s_c2[B1_CH];
  const int cl = threadIdx.x % B1_CH, sl = threadIdx.x / B1_CH;
  const int c = blockIdx.x * B1_CH + cl;
  const bool cok = c < C;
  Saved co = {0.f, 0.f, 0.f, 0.f};
  double s1 = 0.0, s2 = 0.0;
  if (cok) {
    co = saved_coefficients(mean, invstd, gamma, beta, c);
    for (int b = sl; b < B; b += B1_SL) {
      const size_t o = (size_t)b * C + c;
      const float xv = x[o];
      add_grad_sums(s1, s2, act_grad(fmaf(xv, co.sc, co.sh), gy[o], act), xv, co.mu, co.is);
    }
  }
  column_sums<B1_CH, B1_SL, false>(s1, s2);
  if (sl == 0 && cok) {
    store_param_grads(dgamma, dbeta, c, s1, s2, accp);
    s_c1[cl] = (float)(s1 / B);
    s_c2[cl] = (float)(s2 / B);
  }
  __syncthreads();
  unsigned am = 0;
  if (cok) {
    const float c1 = s_c1[cl], c2 = s_c2[cl];
    for (int b = sl; b < B; b += B1_SL) {
      const size_t o = (size_t)b * C + c;
      const float xv = x[o];
      const float r = bn_gx(act_grad(fmaf(xv, co.sc, co.sh), gy[o], act), xv, co, c1, c2);
      am = max(am, abs_bits(r));
      gx[o] = r;
    }
  }
  if (gx_amax) block_amax_atomic<NT>(am, gx_amax);
}

// Backward in ONE pass for channels that fit a workgroup's registers (B * HW <= ONE_NT * 4 * NV elements: the 16 x 16 and
// 8 x 8 layers at B = 128): a workgroup of 16 wavefronts owns a channel, holds its (x, gy) in registers (2 * NV float4 per
// lane), sums g_pre and g_pre * xhat in fp64 in a fixed order, and writes gx from the registers -- two reads and one write
// per element where the two-pass form above reads (x, gy) twice.  Same formulas as bn_partial_kernel<1> +
// bn_apply_kernel<true>; only the order of the fp64 sums differs.
constexpr int ONE_NT = 1024;

// The register tile of a 1024-thread workgroup: the ONE_NT * 4 * NV virtual elements of channel c from v_base on, float4 j
// of a lane at v_base + (j * ONE_NT + lane) * 4.  Loads are unconditional at a clamped place; what lies past `total` is
// masked out of the sums and not written.
struct TileGeom {
  int C, HW, hw_shift, total, v_base;
  __device__ __forceinline__ TileGeom(int B, int C_, int HW_, int v_base_)
      : C(C_), HW(HW_), hw_shift(hw_shift_of(HW_)), total(B * HW_), v_base(v_base_) {}
  __device__ __forceinline__ bool live(int j) const { return v_base + (j * ONE_NT + (int)threadIdx.x) * 4 < total; }
  __device__ __forceinline__ size_t offset_of(int c, int j) const {
    const int v = v_base + (j * ONE_NT + (int)threadIdx.x) * 4;
    return plane_offset(min(v, total - 4), C, HW, hw_shift, c);      // clamped, unconditional; masked below
  }
};
// KEEP_OFF: the offsets of the loads are kept for the stores (2 * NV registers) instead of being computed again
template <int NV, bool KEEP_OFF>
struct BwdTile {
  float4 xv[NV], gv[NV];
  size_t off[KEEP_OFF ? NV : 1];

  __device__ __forceinline__ void load(const float* x, const float* gy, const TileGeom& t, int c) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const size_t o = t.offset_of(c, j);
      if constexpr (KEEP_OFF) off[j] = o;
      xv[j] = *reinterpret_cast<const float4*>(x + o);
      gv[j] = *reinterpret_cast<const float4*>(gy + o);
    }
  }
  // g_pre replaces gy; its two sums, in register order
  __device__ __forceinline__ void form_g_pre(const TileGeom& t, const Saved& co, int act, double& s1, double& s2) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const bool ok = t.live(j);
      float* xp = reinterpret_cast<float*>(&xv[j]);
      float* gp = reinterpret_cast<float*>(&gv[j]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float g = ok ? act_grad(fmaf(xp[e], co.sc, co.sh), gp[e], act) : 0.f;
        gp[e] = g;
        add_grad_sums(s1, s2, g, xp[e], co.mu, co.is);
      }
    }
  }
  // gx from the registers; max |gx| joins `am`
  __device__ __forceinline__ void write_gx(float* gx, const TileGeom& t, int c, const Saved& co, float c1, float c2,
                                           unsigned& am) const {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      if (!t.live(j)) continue;
      const float* xp = reinterpret_cast<const float*>(&xv[j]);
      const float* gp = reinterpret_cast<const float*>(&gv[j]);
      float4 o;
      o.x = bn_gx(gp[0], xp[0], co, c1, c2);
      o.y = bn_gx(gp[1], xp[1], co, c1, c2);
      o.z = bn_gx(gp[2], xp[2], co, c1, c2);
      o.w = bn_gx(gp[3], xp[3], co, c1, c2);
      am = max(max(am, abs_bits(o.x)), max(max(abs_bits(o.y), abs_bits(o.z)), abs_bits(o.w)));
      size_t o_off;
      if constexpr (KEEP_OFF)
        o_off = off[j];
      else
        o_off = t.offset_of(c, j);
      *reinterpret_cast<float4*>(gx + o_off) = o;
    }
  }
};

template <int NV>
__global__ __launch_bounds__(ONE_NT) void bn_bwd_onepass_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                                const float* __restrict__ gamma,
                                                                const float* __restrict__ beta,
                                                                const float* __restrict__ mean,
                                                                const float* __restrict__ invstd, float* __restrict__ gx,
                                                                float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                int B, int C, int HW, int act, int accp,
                                                                unsigned* __restrict__ gx_amax) {
  __shared__ double red[ONE_NT / 64];
  __shared__ float s_c[2];
  const int c = blockIdx.x;
  const TileGeom geom(B, C, HW, 0);
  const Saved co = saved_coefficients(mean, invstd, gamma, beta, c);
  BwdTile<NV, true> tile;
  tile.load(x, gy, geom, c);
  double s1 = 0.0, s2 = 0.0;
  tile.form_g_pre(geom, co, act, s1, s2);
  const double t1 = block_sum<ONE_NT>(s1, red);
  const double t2 = block_sum<ONE_NT>(s2, red);
  if (threadIdx.x == 0) {
    const double count = (double)geom.total;
    s_c[0] = (float)(t1 / count);
    s_c[1] = (float)(t2 / count);
    store_param_grads(dgamma, dbeta, c, t1, t2, accp);
  }
  __syncthreads();
  const float c1 = s_c[0], c2 = s_c[1];
  unsigned am = 0;
  tile.write_gx(gx, geom, c, co, c1, c2, am);
  if (gx_amax) block_amax_atomic<ONE_NT>(am, gx_amax);      // max |gx| for the fp16-plane consumers (bn_apply_kernel)
}

// The one pass for channels LARGER than a workgroup's registers (the 32 x 32 and 64 x 64 layers at B = 128: 131 072 and
// 524 288 elements per channel): a TEAM of T workgroups owns a channel.  Member j holds the virtual elements
// [j * cap, (j + 1) * cap), cap = ONE_NT * 4 * NV, exactly as the kernel above holds a whole channel (the same tile),
// forms g_pre in place and its two fp64 sums, publishes them, collects the T pairs of its team,
// adds them in member order 0 .. T - 1 -- every member gets the same c1, c2 bit for bit, whatever the timing -- and writes
// its gx from registers.  Member 0 writes dgamma / dbeta.
//
// The grid is persistent: teams * T <= the device's compute units, one 1024-thread workgroup on each (128 VGPRs x 16
// wavefronts fill a CU's register file), team t works off channels t, t + teams, ... one per round; a team whose round
// has no channel left stops, nobody waits on it.  Every workgroup of the grid is resident at once, so a member only ever
// waits for workgroups that are running (or about to: the grid never exceeds the CUs).
//
// Exchange: "the data is the flag".  A member's two doubles are four 8-byte granules {tag = round + 1, 32 bits of value},
// each ONE relaxed agent-scope atomic store; wavefront 0 of every member re-reads its team's 4 * T (<= 64) granules, one per
// lane, with relaxed agent-scope atomic loads until every tag matches.  No flag, no fence, no plain store or scalar load
// of a handed-off word, nothing that depends on which XCD a member runs on.  Two granule sets per team, by round parity:
// a member stores round r + 1 only after it has seen every team-mate's round r, and a team-mate stores round r only after
// it has read round r - 1 -- the set that round r + 1 overwrites.  xch: [status word, 12 bytes of padding][teams][2][T][4]
// granules, zeroed by the launch function before EVERY launch (team_zero_kernel: a kernel node under capture).
//
// Bounded spin: a sweep gives up after about a second of wall clock (a resident partner answers in microseconds), sets the
// status word, and the workgroup goes on with NaN for c1 / c2: its gx slices, and member 0's dgamma / dbeta, are NaN from
// there on (it sweeps no more, but still publishes, so that it costs its team-mates one bound, not one per round).  The
// trainers' non-finite guard stops the run; the kernel cannot hang.
typedef __attribute__((address_space(1))) unsigned long long gu64;
typedef __attribute__((address_space(1))) unsigned gu32;
constexpr int TEAM_MAX_T = 16;                   // 4 * T granules: one per lane of the sweeping wavefront
constexpr int TEAM_MAX_WGS = 1024;               // the exchange block is sized for grids up to this (vg_bn_workspace_bytes)
constexpr size_t TEAM_HDR = 16;                  // status word, padded: the granules stay 16-byte aligned
constexpr long long TEAM_SPIN_TICKS = 100000000; // wall_clock64() counts at 100 MHz: one second
size_t team_block_bytes(int grid) { return TEAM_HDR + (size_t)grid * 2 * 4 * sizeof(unsigned long long); }

__global__ __launch_bounds__(NT) void team_zero_kernel(unsigned long long* __restrict__ xch, int words) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i < words) xch[i] = 0ull;
}

template <int NV>
__global__ __launch_bounds__(ONE_NT) void bn_bwd_team_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta,
                                                             const float* __restrict__ mean,
                                                             const float* __restrict__ invstd, float* __restrict__ gx,
                                                             float* __restrict__ dgamma, float* __restrict__ dbeta, int B,
                                                             int C, int HW, int act, int accp,
                                                             unsigned* __restrict__ gx_amax, int T, int teams,
                                                             unsigned long long* xch) {
  __shared__ double red[ONE_NT / 64];
  __shared__ float s_c[2];
  __shared__ int s_failed;
  const int team = blockIdx.x / T, member = blockIdx.x - team * T;
  const TileGeom geom(B, C, HW, member * (ONE_NT * 4 * NV));
  const int total = geom.total;
  gu32* status = (gu32*)xch;
  gu64* sets = (gu64*)xch + TEAM_HDR / sizeof(unsigned long long) + (size_t)team * 2 * T * 4;
  unsigned am = 0;
  bool failed = false;
  int round = 0;
  for (int c = team; c < C; c += teams, ++round) {
    const Saved co = saved_coefficients(mean, invstd, gamma, beta, c);
    // the offsets are computed again for the stores: 2 * NV registers of them would not fit next to the 8 * NV of data
    BwdTile<NV, false> tile;
    tile.load(x, gy, geom, c);
    double s1 = 0.0, s2 = 0.0;
    tile.form_g_pre(geom, co, act, s1, s2);
    const double t1 = block_sum<ONE_NT>(s1, red);
    const double t2 = block_sum<ONE_NT>(s2, red);
    if (threadIdx.x < 64) {                                 // wavefront 0: publish, sweep, add in member order
      const int lane = threadIdx.x;
      const unsigned tag = (unsigned)round + 1u;
      gu64* set = sets + (size_t)(round & 1) * T * 4;
      if (lane == 0) {
        const unsigned long long b1 = (unsigned long long)__double_as_longlong(t1);
        const unsigned long long b2 = (unsigned long long)__double_as_longlong(t2);
        const unsigned long long hi = (unsigned long long)tag << 32;
        gu64* mine = set + member * 4;
        __hip_atomic_store(mine + 0, hi | (b1 & 0xffffffffull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(mine + 1, hi | (b1 >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(mine + 2, hi | (b2 & 0xffffffffull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(mine + 3, hi | (b2 >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      bool ok = false;
      unsigned val = 0;
      if (!failed) {                                        // wave-uniform (read back from LDS below)
        const bool has = lane < 4 * T;
        const long long start = wall_clock64();
        for (unsigned spins = 1;; ++spins) {
          const unsigned long long g =
              has ? __hip_atomic_load(set + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : (unsigned long long)tag << 32;
          val = (unsigned)g;
          if (__all((unsigned)(g >> 32) == tag)) {
            ok = true;
            break;
          }
          __builtin_amdgcn_s_sleep(2);
          if ((spins & 63u) == 0 && __any(wall_clock64() - start > TEAM_SPIN_TICKS)) break;
        }
      }
      double a1 = 0.0, a2 = 0.0;
      for (int m = 0; m < T; ++m) {                         // member order: the same sums in every member
        const unsigned l1 = __shfl(val, 4 * m, 64), h1 = __shfl(val, 4 * m + 1, 64);
        const unsigned l2 = __shfl(val, 4 * m + 2, 64), h2 = __shfl(val, 4 * m + 3, 64);
        a1 += __longlong_as_double((long long)(((unsigned long long)h1 << 32) | l1));
        a2 += __longlong_as_double((long long)(((unsigned long long)h2 << 32) | l2));
      }
      if (lane == 0) {
        if (!ok) {
          if (!failed) __hip_atomic_store(status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          a1 = a2 = __longlong_as_double(0x7ff8000000000000ll);
        }
        const double count = (double)total;
        s_c[0] = (float)(a1 / count);
        s_c[1] = (float)(a2 / count);
        s_failed = !ok;
        if (member == 0) store_param_grads(dgamma, dbeta, c, a1, a2, accp);
      }
    }
    __syncthreads();
    const float c1 = s_c[0], c2 = s_c[1];
    failed = s_failed != 0;
    tile.write_gx(gx, geom, c, co, c1, c2, am);
  }
  if (gx_amax) block_amax_atomic<ONE_NT>(am, gx_amax);      // one atomic per workgroup, after its last round
}

size_t part_bytes(int C) { return (size_t)C * NS_MAX * 2 * sizeof(double); }
// the two-stage partials, or (team backward) the exchange block: either one starts at the workspace's first byte
size_t ws_bytes(int C) { return part_bytes(C) + 64 + team_block_bytes(TEAM_MAX_WGS); }

// Compute units of the current device: what a persistent grid is sized by.  Asked of the runtime once per device and kept
// (a write-once cache of a device constant, not state: every caller computes the same value); 0 if it cannot be had.
int device_cus() {
  constexpr int MAX_DEV = 64;
  static std::atomic<int> cus[MAX_DEV];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) return 0;
  int n = cus[dev].load(std::memory_order_relaxed);
  if (n == 0) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 0) n = 0;
    cus[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

VG_KNOB(int, g_team_nv, 0);            // tuning build: 1 / 8 force the team backward with that NV (vg_debug_set_bn_team)
VG_KNOB(int, g_team_max_wgs, 0);       // tuning build: cap of the resident workgroups (0: the device's)

// What vg_bn_act_bwd launches.  One pass when a channel fits a workgroup's registers and there are channels enough to fill
// the chip's memory system (16-byte loads only: a misaligned x / gy / gx goes to the two passes' scalar loops); the team
// form of the one pass for larger channels of up to 16 members where channels x members reach the same 128 workgroups;
// the two passes for everything else.
enum { BWD_1D = 0, BWD_ONE2 = 1, BWD_ONE8 = 2, BWD_TWO = 3, BWD_TEAM = 4 };
struct BwdPlan {
  int path, nv, T, teams, rounds;
};
BwdPlan make_bwd_plan(int B, int C, int HW, int vec) {
  BwdPlan p = {BWD_TWO, 0, 0, 0, 0};
  if (HW == 1) {
    p.path = BWD_1D;
    return p;
  }
  const long per_channel = (long)B * HW;
  const bool forced = g_team_nv != 0;
  if (!forced && vec && per_channel >= 4 && per_channel <= (long)ONE_NT * 4 * 8 && C >= 128) {
    p.path = per_channel <= (long)ONE_NT * 4 * 2 ? BWD_ONE2 : BWD_ONE8;
    return p;
  }
  if (!vec || per_channel < 4 || (!forced && per_channel <= (long)ONE_NT * 4 * 8)) return p;
  const int nv = forced ? g_team_nv : 8;
  const long cap = (long)ONE_NT * 4 * nv;
  const long T = (per_channel + cap - 1) / cap;
  if (T > TEAM_MAX_T || (!forced && (long)C * T < 128)) return p;
  int max_wgs = device_cus();
  if (g_team_max_wgs > 0 && g_team_max_wgs < max_wgs) max_wgs = g_team_max_wgs;
  if (max_wgs > TEAM_MAX_WGS) max_wgs = TEAM_MAX_WGS;
  if (max_wgs < T) return p;            // a channel's members must all be resident at once
  p.path = BWD_TEAM;
  p.nv = nv;
  p.T = (int)T;
  p.teams = (int)(C < max_wgs / T ? C : max_wgs / T);
  p.rounds = (C + p.teams - 1) / p.teams;
  return p;
}

// ---- coefficients from slots -----------------------------------------------------------------------------------------
// Per-channel coefficients of a train-mode BatchNorm from partial sums (slot_sums: fp32 slots written by a convolution
// epilogue, or the fp64 slices of bn_partial_kernel<0>).  Fixed summation order, fp64.
// Writes mean / invstd (saved for backward), scale = gamma * invstd, shift = beta - mean * scale, and updates the
// running statistics exactly as bn_apply_kernel's slice-0 workgroup does.
// act_amax (may be NULL): an upper bound of max |act(BN(x))| over the whole tensor is added to it (atomic maximum of
// the channels' bn_act_bound, delta: the relative error of the partial sums) -- what the fp16-plane convolution that
// applies these coefficients on load scales its input by.
// <T, 32, 8>: 32 channels per workgroup x 8 partial-lanes: consecutive threads read consecutive channels (the convolution's
// slots are [slot][C][2]: 256 contiguous bytes per 32 threads), each partial-lane sums every 8th partial, and the 8
// sums of a channel are added in order.
// <float, 8, 128>: MANY slots in ONE launch (the ring kernels leave 512-2048 of them at B = 128): a workgroup of 1024
// threads owns 8 channels, 128 partial-lanes each -- every lane sums every 128th slot (4-16 independent 8-byte loads), the
// 128 fp64 sums of a channel are added 16 lanes x 8, then 16.  Replaces stats_partial + finalize (two launches of ~5 us and
// a kernel boundary) wherever a channel has <= 4096 slots.
template <typename T, int CH, int KL>
__global__ __launch_bounds__(CH * KL) void bn_finalize_kernel(const T* __restrict__ part, int np, long cs, long ks, int C,
                                                              double count, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta,
                                                              float* __restrict__ running_mean,
                                                              float* __restrict__ running_var, float* __restrict__ mean_out,
                                                              float* __restrict__ invstd_out, float* __restrict__ scale,
                                                              float* __restrict__ shift, float eps, float momentum,
                                                              unsigned* __restrict__ act_amax, double delta) {
  constexpr bool WIDE = KL > 8;
  const int c = blockIdx.x * CH + threadIdx.x % CH;
  double s1, s2;
  slot_sums<CH, KL, WIDE, WIDE>(part, cs, ks, 0, np, c, C, s1, s2);
  if (threadIdx.x / CH == 0 && c < C) {
    const Coeffs co = channel_coefficients(s1, s2, count, eps, gamma[c], beta[c]);
    mean_out[c] = co.mu;
    invstd_out[c] = co.invstd;
    scale[c] = co.scale;
    shift[c] = co.shift;
    if (act_amax)
      atomicMax(act_amax, __float_as_uint(bn_act_bound(s2, co.m, co.var, count, delta, co.mu, co.scale, beta[c])));
    update_running(running_mean, running_var, c, co, count, momentum);
  }
}

// First stage for MANY slots (a 3 -> 32 first layer at B = 128 leaves 16 384 of them for 32 channels): workgroup
// (channel block, split) sums its share of the slots into fp64 partials part[c][split][2], in a fixed order.
__global__ __launch_bounds__(NT) void stats_partial_kernel(const float* __restrict__ stats, int nslots, int C, int nsplit,
                                                           double* __restrict__ part) {
  constexpr int CH = 32, KL = NT / CH;
  const int c = blockIdx.x * CH + threadIdx.x % CH, sp = blockIdx.y;
  const int per = cdiv(nslots, nsplit), k0 = sp * per, k1 = min(k0 + per, nslots);
  double s1, s2;
  slot_sums<CH, KL, false, false>(stats, 1L, (long)C, k0, k1, c, C, s1, s2);
  if (threadIdx.x / CH == 0 && c < C) store_partial(part, c, nsplit, sp, s1, s2);
}

// ---- eval: BatchNorm on RUNNING statistics (nn.BatchNorm*.eval() of the reference's modules, model.py:451-458, 462,
// 468, 492, 496-505, 390-400) -----------------------------------------------------------------------------------------
// Coefficients from the running statistics: scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale,
// invstd for the backward.  The running buffers are read, never written.  With the producing convolution's statistics
// slots (stats[slot][C][2], `count` values per channel) and act_amax: also an upper bound of max |act(scale x + shift)|
// over the tensor the slots were taken of, from the sums alone.  bn_act_bound's argument, centred on the batch mean
// instead of on the BatchNorm's own: with S1, S2 the computed sums, m = S1 / n, q = S2 / n, var = max(q - m^2, 0),
//   |x - T1/n| <= sigma sqrt(n - 1)  (Samuelson, EXACT mean and sigma),  sigma^2 <= var_up = var + (3.01 delta + 2^-50) q,
//   |T1/n - m| <= 1.01 delta sqrt(q)                                      (both derived above bn_act_bound)
//   => |scale x + shift| <= |scale| (sqrt(var_up (n - 1)) + 1.01 delta sqrt(q)) + |scale m + shift|.
// scale m + shift is evaluated in fp64 from the fp32 coefficients WRITTEN (what the consumer multiplies by); 2^-21 of its
// two terms covers that evaluation, the consumer's fmaf and coefficients rounded otherwise (the exact ones differ from
// the written by 2^-23 relative); (1 + 2^-20): the fp64 -> fp32 conversion.  ReLU / LeakyReLU(0.2) only shrink magnitudes.
// A constant channel has sigma = 0 <= var_up; a variance lost to cancellation is covered by the delta q term.
// CH channels per workgroup x KL partial-lanes (slot_sums); the KL sums of a channel are added serially, also the 128.
template <int CH, int KL>
__global__ __launch_bounds__(CH * KL) void bn_eval_coeffs_kernel(const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta,
                                                                 const float* __restrict__ running_mean,
                                                                 const float* __restrict__ running_var,
                                                                 float* __restrict__ scale, float* __restrict__ shift,
                                                                 float* __restrict__ invstd, int C, float eps,
                                                                 const float* __restrict__ stats, int nslots, double count,
                                                                 unsigned* __restrict__ act_amax, double delta) {
  const int c = blockIdx.x * CH + threadIdx.x % CH;
  const bool bound = stats != nullptr && act_amax != nullptr;      // uniform over the grid
  double s1 = 0.0, s2 = 0.0;
  if (bound) slot_sums<CH, KL, false, false>(stats, 1L, (long)C, 0, nslots, c, C, s1, s2);
  if (threadIdx.x / CH != 0 || c >= C) return;
  const float is = (float)(1.0 / sqrt((double)running_var[c] + (double)eps));
  const float sc = gamma[c] * is;
  const float sh = beta[c] - running_mean[c] * sc;
  scale[c] = sc;
  shift[c] = sh;
  invstd[c] = is;
  if (!bound) return;
  double m, var;
  mean_and_variance(s1, s2, count, m, var);
  const double q = s2 / count;
  const double var_up = var + (3.01 * delta + 0x1p-50) * q;
  const double dev = sqrt(var_up * fmax(count - 1.0, 0.0)) + 1.01 * delta * sqrt(q);
  const double asc = fabs((double)sc);
  const double b = asc * dev + fabs((double)sc * m + (double)sh) + 0x1p-21 * (asc * fabs(m) + fabs((double)sh));
  atomicMax(act_amax, __float_as_uint((float)(b * (1.0 + 0x1p-20))));
}

// Backward of y = act(x * sc + sh) with FROZEN coefficients, one pass: gx = gy act'(pre) sc; dbeta = sum gy act'(pre),
// dgamma = sum gy act'(pre) (x - mean) invstd.  Workgroup (c, k) owns slice k of channel c (make_slicing), writes its gx
// and -- part != NULL -- its fp64 partial sums part[c][k][2]; with ONE slice per channel it writes dgamma / dbeta itself.
__global__ __launch_bounds__(NT) void bn_eval_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                         const float* __restrict__ scale, const float* __restrict__ shift,
                                                         const float* __restrict__ mean, const float* __restrict__ invstd,
                                                         float* __restrict__ gx, double* __restrict__ part,
                                                         float* __restrict__ dgamma, float* __restrict__ dbeta, int B,
                                                         int C, int HW, long per, int ns, int act, int accp,
                                                         unsigned* __restrict__ gx_amax, int vec) {
  __shared__ double red[NT / 64];
  const float slope = act_slope_of(act);
  const int c = blockIdx.x, k = blockIdx.y;
  const float sc = scale[c], sh = shift[c], mu = mean[c], is = invstd[c];
  double s1 = 0.0, s2 = 0.0;
  unsigned am = 0;
  plane_walk<true, true>(x, gy, gx, B, C, HW, c, k, per, vec, [&](float xv, float gv) -> float {
    const float g = eval_act_grad(fmaf(xv, sc, sh), gv, slope);
    add_grad_sums(s1, s2, g, xv, mu, is);
    const float r = g * sc;
    am = max(am, abs_bits(r));
    return r;
  });
  if (part || dgamma || dbeta) {               // uniform over the grid
    const double t1 = block_sum<NT>(s1, red);
    const double t2 = block_sum<NT>(s2, red);
    if (threadIdx.x == 0) {
      if (part)
        store_partial(part, c, ns, k, t1, t2);
      else                                     // ns == 1
        store_param_grads(dgamma, dbeta, c, t1, t2, accp);
    }
  }
  if (gx_amax) block_amax_atomic<NT>(am, gx_amax);
}

__global__ __launch_bounds__(NT) void bn_eval_bwd_finalize_kernel(const double* __restrict__ part, int ns, int C,
                                                                  float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                  int accp) {
  const int c = blockIdx.x * NT + threadIdx.x;
  if (c >= C) return;
  double s1 = 0.0, s2 = 0.0;
  sum_partials(part, c, ns, s1, s2);
  store_param_grads(dgamma, dbeta, c, s1, s2, accp);
}

// The same for BatchNorm1d, x [B][C]: the geometry of bn1d_bwd_kernel, one pass.
__global__ __launch_bounds__(NT) void bn1d_eval_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                           const float* __restrict__ scale, const float* __restrict__ shift,
                                                           const float* __restrict__ mean, const float* __restrict__ invstd,
                                                           float* __restrict__ gx, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta, int B, int C, int act, int accp,
                                                           unsigned* __restrict__ gx_amax) {
  const float slope = act_slope_of(act);
  const int cl = threadIdx.x % B1_CH, sl = threadIdx.x / B1_CH;
  const int c = blockIdx.x * B1_CH + cl;
  const bool cok = c < C;
  double s1 = 0.0, s2 = 0.0;
  unsigned am = 0;
  if (cok) {
    const float sc = scale[c], sh = shift[c], mu = mean[c], is = invstd[c];
    for (int b = sl; b < B; b += B1_SL) {
      const size_t o = (size_t)b * C + c;
      const float xv = x[o];
      const float g = eval_act_grad(fmaf(xv, sc, sh), gy[o], slope);
      add_grad_sums(s1, s2, g, xv, mu, is);
      const float r = g * sc;
      am = max(am, abs_bits(r));
      gx[o] = r;
    }
  }
  column_sums<B1_CH, B1_SL, false>(s1, s2);
  if (sl == 0 && cok) store_param_grads(dgamma, dbeta, c, s1, s2, accp);
  if (gx_amax) block_amax_atomic<NT>(am, gx_amax);
}

}  // namespace

// ---- the C entry points ------------------------------------------------------------------------------------------------
extern "C" size_t vg_bn_workspace_bytes(int C) { return C > 0 ? ws_bytes(C) : 0; }

extern "C" int vg_bn_finalize_stats(const float* stats, int nslots, int C, double count, const float* gamma,
                                    const float* beta, float* running_mean, float* running_var, float* save_mean,
                                    float* save_invstd, float* scale, float* shift, float eps, float momentum,
                                    float* act_amax, void* workspace, size_t workspace_bytes, void* stream) {
  unsigned* am = (unsigned*)act_amax;
  if (!stats || nslots <= 0 || C <= 0 || count <= 0 || !gamma || !beta || !save_mean || !save_invstd || !scale || !shift)
    return VG_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  const double delta = slot_sums_delta(nslots);
  // few slots: one launch (a workgroup per 32 channels, 8 partial-lanes: up to 8 dependent loads per lane); more:
  // NS_MAX-way first stage into the BatchNorm workspace.  (The one-launch form on 1024 slots x 32 channels ran 56 us
  // -- one workgroup, 128 dependent loads per lane -- against ~6 us for the two stages.)
  if (nslots <= 64) {
    hipLaunchKernelGGL((bn_finalize_kernel<float, 32, 8>), dim3(cdiv(C, 32)), dim3(NT), 0, st, stats, nslots, 1L, (long)C, C,
                       count, gamma, beta, running_mean, running_var, save_mean, save_invstd, scale, shift, eps,
                       momentum, am, delta);      // stats[slot][C][2]: channel stride 1, slot stride C
    VG_CHECK_LAUNCH();
    return 0;
  }
  if (nslots <= 4096) {
    hipLaunchKernelGGL((bn_finalize_kernel<float, 8, 128>), dim3(cdiv(C, 8)), dim3(1024), 0, st, stats, nslots, 1L, (long)C,
                       C, count, gamma, beta, running_mean, running_var, save_mean, save_invstd, scale, shift, eps,
                       momentum, am, delta);
    VG_CHECK_LAUNCH();
    return 0;
  }
  if (!workspace || workspace_bytes < ws_bytes(C)) return VG_ERR_WORKSPACE;
  double* part = (double*)workspace;
  hipLaunchKernelGGL(stats_partial_kernel, dim3(cdiv(C, 32), NS_MAX), dim3(NT), 0, st, stats, nslots, C, NS_MAX, part);
  VG_CHECK_LAUNCH();
  hipLaunchKernelGGL((bn_finalize_kernel<double, 32, 8>), dim3(cdiv(C, 32)), dim3(NT), 0, st, (const double*)part, NS_MAX,
                     (long)NS_MAX, 1L, C, count, gamma, beta, running_mean, running_var, save_mean, save_invstd, scale,
                     shift, eps, momentum, am, delta);      // part[c][NS_MAX][2]: the fp32 slots' delta
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int vg_bn_stats(const float* x, const float* gamma, const float* beta, float* running_mean,
                           float* running_var, float* save_mean, float* save_invstd, float* scale, float* shift, int B,
                           int C, int HW, float eps, float momentum, float* act_amax, void* workspace,
                           size_t workspace_bytes, void* stream) {
  if (!x || !gamma || !beta || !save_mean || !save_invstd || !scale || !shift || B <= 0 || C <= 0 || HW <= 0)
    return VG_ERR_BAD_ARG;
  if (!workspace || workspace_bytes < ws_bytes(C)) return VG_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  const Slicing s = make_slicing(B, C, HW);
  hipLaunchKernelGGL(bn_partial_kernel<0>, dim3(C, s.ns), dim3(NT), 0, st, x, (const float*)nullptr, (const float*)nullptr,
                     (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, part, B, C, HW, s.per, s.ns, 0,
                     streams_vec(HW, x));
  VG_CHECK_LAUNCH();
  hipLaunchKernelGGL((bn_finalize_kernel<double, 32, 8>), dim3(cdiv(C, 32)), dim3(NT), 0, st, (const double*)part, s.ns,
                     (long)s.ns, 1L, C, (double)B * HW, gamma, beta, running_mean, running_var, save_mean, save_invstd,
                     scale, shift, eps, momentum, (unsigned*)act_amax, fp64_sums_delta((double)B * HW));      // part[c][ns][2]
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int vg_affine_act(const float* x, const float* scale, const float* shift, float* y, int B, int C, int HW,
                             int act, float* y_amax, void* stream) {
  if (!x || !scale || !shift || !y || B <= 0 || C <= 0 || HW <= 0 || !act_ok(act)) return VG_ERR_BAD_ARG;
  if (!streams_vec(HW, x, y)) {      // H*W not a multiple of 4, or a tensor that is not on a 16-byte boundary
    const size_t n = (size_t)B * C * HW;
    if (cdiv((long)n, (long)NT) > 0x7fffffffL) return VG_ERR_BAD_ARG;
    hipLaunchKernelGGL(affine_act_scalar_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, x,
                       scale, shift, y, C, HW, n, act, (unsigned*)y_amax);
    VG_CHECK_LAUNCH();
    return 0;
  }
  const size_t n4 = (size_t)B * C * HW / 4;
  if (cdiv((long)n4, (long)NT) > 0x7fffffffL) return VG_ERR_BAD_ARG;
  const int hw4 = HW / 4;
  int sh = -1;
  if ((hw4 & (hw4 - 1)) == 0 && n4 < (1ULL << 40)) {      // power of two (and plane indices that fit 32 bits after the shift)
    sh = 0;
    while ((1 << sh) < hw4) ++sh;
    if ((n4 >> sh) > 0xffffffffULL) sh = -1;
  }
  const size_t chunks = (n4 + NT * AA_U - 1) / (NT * AA_U);
  hipLaunchKernelGGL(affine_act_kernel, dim3((unsigned)(chunks < 2048 ? chunks : 2048)), dim3(NT), 0, (hipStream_t)stream, x, scale,
                     shift, y, C, HW, n4, act, sh, (unsigned*)y_amax);
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int vg_bn_act_fwd(const float* x, const float* gamma, const float* beta, float* y, float* running_mean,
                             float* running_var, float* save_mean, float* save_invstd, int B, int C, int HW,
                             float eps, float momentum, int act, float* y_amax, void* workspace,
                             size_t workspace_bytes, void* stream) {
  if (!x || !gamma || !beta || !y || !save_mean || !save_invstd || B <= 0 || C <= 0 || HW <= 0 || !act_ok(act))
    return VG_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (HW == 1) {
    hipLaunchKernelGGL(bn1d_fwd_kernel, dim3(cdiv(C, B1_CH)), dim3(NT), 0, st, x, gamma, beta, y, running_mean,
                       running_var, save_mean, save_invstd, B, C, eps, momentum, act);
    VG_CHECK_LAUNCH();
    return 0;
  }
  if (!workspace || workspace_bytes < ws_bytes(C)) return VG_ERR_WORKSPACE;
  double* part = (double*)workspace;
  const int vec = streams_vec(HW, x, y);
  const Slicing s = make_slicing(B, C, HW);
  hipLaunchKernelGGL(bn_partial_kernel<0>, dim3(C, s.ns), dim3(NT), 0, st, x, (const float*)nullptr, gamma, beta,
                     (const float*)nullptr, (const float*)nullptr, part, B, C, HW, s.per, s.ns, act, vec);
  VG_CHECK_LAUNCH();
  const Slicing a = make_apply_slicing(B, C, HW);
  hipLaunchKernelGGL(bn_apply_kernel<false>, dim3(C, a.ns), dim3(NT), 0, st, x, (const float*)nullptr,
                     (const double*)part, s.ns, gamma, beta, save_mean, save_invstd, running_mean, running_var,
                     (float*)nullptr, (float*)nullptr, y, B, C, HW, a.per, eps, momentum, act, 0,
                     reinterpret_cast<unsigned*>(y_amax), vec);
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int vg_bn_act_bwd(const float* gy, const float* x, const float* gamma, const float* beta,
                             const float* save_mean, const float* save_invstd, float* gx, float* dgamma,
                             float* dbeta, int B, int C, int HW, int act, int accumulate_param_grads, float* gx_amax,
                             void* workspace, size_t workspace_bytes, void* stream) {
  unsigned* am = (unsigned*)gx_amax;
  if (!gy || !x || !gamma || !beta || !save_mean || !save_invstd || !gx || B <= 0 || C <= 0 || HW <= 0 || !act_ok(act))
    return VG_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int accp = accumulate_param_grads ? 1 : 0;      // dgamma / dbeta +=
  if (HW == 1) {
    hipLaunchKernelGGL(bn1d_bwd_kernel, dim3(cdiv(C, B1_CH)), dim3(NT), 0, st, gy, x, gamma, beta, save_mean,
                       save_invstd, gx, dgamma, dbeta, B, C, act, accp, am);
    VG_CHECK_LAUNCH();
    return 0;
  }
  const int vec = streams_vec(HW, x, gy, gx);
  const BwdPlan plan = make_bwd_plan(B, C, HW, vec);
  if (plan.path == BWD_TEAM) {
    const int grid = plan.teams * plan.T;
    const size_t xbytes = team_block_bytes(grid);
    if (!workspace || workspace_bytes < xbytes || ((uintptr_t)workspace & 15)) return VG_ERR_WORKSPACE;
    // status word and granules: zeroed before every launch (tags count rounds within a launch, from 1).  By a kernel of
    // our own, not hipMemsetAsync: the memset NODE of a captured call wrote stale bytes instead of zeros from its second
    // replay on whenever other launches had run in between (seen on the status word: profiles/README.md, Round 12)
    unsigned long long* xch = (unsigned long long*)workspace;
    const int words = (int)(xbytes / sizeof(unsigned long long));
    hipLaunchKernelGGL(team_zero_kernel, dim3(cdiv(words, NT)), dim3(NT), 0, st, xch, words);
    VG_CHECK_LAUNCH();
    if (plan.nv == 8)
      hipLaunchKernelGGL(bn_bwd_team_kernel<8>, dim3(grid), dim3(ONE_NT), 0, st, x, gy, gamma, beta, save_mean, save_invstd,
                         gx, dgamma, dbeta, B, C, HW, act, accp, am, plan.T, plan.teams, xch);
#ifdef VG_TUNING
    else if (plan.nv == 1)
      hipLaunchKernelGGL(bn_bwd_team_kernel<1>, dim3(grid), dim3(ONE_NT), 0, st, x, gy, gamma, beta, save_mean, save_invstd,
                         gx, dgamma, dbeta, B, C, HW, act, accp, am, plan.T, plan.teams, xch);
#endif
    else
      return VG_ERR_BAD_ARG;
    VG_CHECK_LAUNCH();
    return 0;
  }
  if (plan.path == BWD_ONE2 || plan.path == BWD_ONE8) {
    if (plan.path == BWD_ONE2)
      hipLaunchKernelGGL(bn_bwd_onepass_kernel<2>, dim3(C), dim3(ONE_NT), 0, st, x, gy, gamma, beta, save_mean, save_invstd,
                         gx, dgamma, dbeta, B, C, HW, act, accp, am);
    else
      hipLaunchKernelGGL(bn_bwd_onepass_kernel<8>, dim3(C), dim3(ONE_NT), 0, st, x, gy, gamma, beta, save_mean, save_invstd,
                         gx, dgamma, dbeta, B, C, HW, act, accp, am);
    VG_CHECK_LAUNCH();
    return 0;
  }
  if (!workspace || workspace_bytes < ws_bytes(C)) return VG_ERR_WORKSPACE;
  double* part = (double*)workspace;
  const Slicing s = make_slicing(B, C, HW);
  hipLaunchKernelGGL(bn_partial_kernel<1>, dim3(C, s.ns), dim3(NT), 0, st, x, gy, gamma, beta, save_mean,
                     save_invstd, part, B, C, HW, s.per, s.ns, act, vec);
  VG_CHECK_LAUNCH();
  const Slicing a = make_apply_slicing(B, C, HW);
  hipLaunchKernelGGL(bn_apply_kernel<true>, dim3(C, a.ns), dim3(NT), 0, st, x, gy, (const double*)part, s.ns, gamma,
                     beta, const_cast<float*>(save_mean), const_cast<float*>(save_invstd), (float*)nullptr,
                     (float*)nullptr, dgamma, dbeta, gx, B, C, HW, a.per, 0.f, 0.f, act, accp, am, vec);
  VG_CHECK_LAUNCH();
  return 0;
}

#ifdef VG_TUNING
extern "C" int vg_debug_set_bn_team(int nv, int max_wgs) {
  if ((nv != 0 && nv != 1 && nv != 8) || max_wgs < 0) return VG_ERR_BAD_ARG;
  g_team_nv = nv;
  g_team_max_wgs = max_wgs;
  return 0;
}

// the plan vg_bn_act_bwd would launch under the current knobs (make_bwd_plan: the launch's own planning code)
extern "C" int vg_debug_bn_bwd_plan(int B, int C, int HW, const void* gy, const void* x, const void* gx, int* out) {
  if (!out || B <= 0 || C <= 0 || HW <= 0) return VG_ERR_BAD_ARG;
  const BwdPlan p = make_bwd_plan(B, C, HW, streams_vec(HW, x, gy, gx));
  out[0] = p.path; out[1] = p.nv; out[2] = p.T; out[3] = p.teams; out[4] = p.rounds;
  return 0;
}
#endif

extern "C" int vg_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean,
                                 const float* running_var, float* scale, float* shift, float* invstd, int C, float eps,
                                 int act, const float* stats, int nslots, double count, float* act_amax, void* stream) {
  if (!gamma || !beta || !running_mean || !running_var || !scale || !shift || !invstd || C <= 0 || !act_ok(act))
    return VG_ERR_BAD_ARG;
  const bool bound = stats != nullptr && act_amax != nullptr;
  if (bound && (nslots <= 0 || !(count > 0))) return VG_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  const double delta = bound ? slot_sums_delta(nslots) : 0.0;
  const float* sp = bound ? stats : nullptr;
  unsigned* am = bound ? (unsigned*)act_amax : nullptr;
  // few slots (or none): 32 channels x 8 partial-lanes; many (the ring kernels leave 512-2048, a thin first layer 16 384):
  // 8 channels x 128 partial-lanes, as bn_finalize_kernel<float, 8, 128> -- ONE launch either way
  if (!bound || nslots <= 64)
    hipLaunchKernelGGL((bn_eval_coeffs_kernel<32, 8>), dim3(cdiv(C, 32)), dim3(256), 0, st, gamma, beta, running_mean,
                       running_var, scale, shift, invstd, C, eps, sp, nslots, count, am, delta);
  else
    hipLaunchKernelGGL((bn_eval_coeffs_kernel<8, 128>), dim3(cdiv(C, 8)), dim3(1024), 0, st, gamma, beta, running_mean,
                       running_var, scale, shift, invstd, C, eps, sp, nslots, count, am, delta);
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int vg_bn_eval_act_bwd(const float* gy, const float* x, const float* scale, const float* shift,
                                  const float* mean, const float* invstd, float* gx, float* dgamma, float* dbeta, int B,
                                  int C, int HW, int act, int accumulate_param_grads, float* gx_amax, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  unsigned* am = (unsigned*)gx_amax;
  if (!gy || !x || !scale || !shift || !mean || !invstd || !gx || B <= 0 || C <= 0 || HW <= 0 || !act_ok(act))
    return VG_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int accp = accumulate_param_grads ? 1 : 0;
  if (HW == 1) {
    hipLaunchKernelGGL(bn1d_eval_bwd_kernel, dim3(cdiv(C, B1_CH)), dim3(NT), 0, st, gy, x, scale, shift, mean, invstd, gx,
                       dgamma, dbeta, B, C, act, accp, am);
    VG_CHECK_LAUNCH();
    return 0;
  }
  const Slicing s = make_slicing(B, C, HW);      // ns <= NS_MAX: the partials fit vg_bn_workspace_bytes(C)
  const bool want_p = dgamma || dbeta;
  double* part = nullptr;
  if (want_p && s.ns > 1) {
    if (!workspace || workspace_bytes < ws_bytes(C)) return VG_ERR_WORKSPACE;
    part = (double*)workspace;
  }
  hipLaunchKernelGGL(bn_eval_bwd_kernel, dim3(C, s.ns), dim3(NT), 0, st, gy, x, scale, shift, mean, invstd, gx, part,
                     dgamma, dbeta, B, C, HW, s.per, s.ns, act, accp, am, streams_vec(HW, x, gy, gx));
  VG_CHECK_LAUNCH();
  if (part) {
    hipLaunchKernelGGL(bn_eval_bwd_finalize_kernel, dim3(cdiv(C, NT)), dim3(NT), 0, st, (const double*)part, s.ns, C,
                       dgamma, dbeta, accp);
    VG_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int vg_channel_sum(const float* g, float* out, int B, int C, int HW, void* workspace,
                              size_t workspace_bytes, void* stream) {
  if (!g || !out || B <= 0 || C <= 0 || HW <= 0) return VG_ERR_BAD_ARG;
  if (!workspace || workspace_bytes < ws_bytes(C)) return VG_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  const Slicing s = make_slicing(B, C, HW);
  hipLaunchKernelGGL(bn_partial_kernel<2>, dim3(C, s.ns), dim3(NT), 0, st, g, (const float*)nullptr,
                     (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr,
                     part, B, C, HW, s.per, s.ns, 0, streams_vec(HW, g));      // a view at an odd offset: scalar loads
  VG_CHECK_LAUNCH();
  hipLaunchKernelGGL(channel_sum_finalize_kernel, dim3(cdiv(C, NT)), dim3(NT), 0, st, (const double*)part, s.ns,
                     C, out);
  VG_CHECK_LAUNCH();
  return 0;
}
