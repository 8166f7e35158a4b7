// Adversarial losses on the discriminator's LOGIT for gfx950: logistic (BCE-with-logits),
// least squares and the three hinge terms, fused with the head -- Linear(2048 -> 1) -- or on a logit vector.
//
// vg_dot_sigmoid_bce_fwd (losses.hip) reproduces nn.BCELoss on p = sigmoid(s) operation for operation; in fp32 that
// gradient is exactly 0 once p rounds to 1 (s >= 17) and vanishes with p below about 1e-12, where the loss still has
// one.  Every loss here is a function of s, so the Sigmoid is off the loss path and nothing saturates spuriously.
// The backward of the head is vg_dot_sigmoid_bce_bwd as it stands: it consumes a generic dlogit.
#include "common.hpp"
#include "vaegan_hip.h"

namespace {

constexpr int NT = 256;

struct GanTerm {
  float loss;      // l(s)
  float dl;        // d l / d s
  float p;         // sigmoid(s): what the iteration logs as D(x), whatever the loss
};

// One row.  Written with compare + select throughout: fmaxf drops a NaN (max(NaN, 0) = 0), and a NaN logit has to come
// out as a NaN loss AND a NaN gradient for every kind, the constant-gradient ones included (the last select).
__device__ __forceinline__ GanTerm gan_term(float s, float t, int kind) {
  GanTerm r;
  const float e = expf(-fabsf(s));                       // in (0, 1]: never overflows
  const float q = 1.f / (1.f + e);
  r.p = s >= 0.f ? q : e * q;                            // sigmoid(s), stable at both ends; NaN stays NaN (e is NaN)
  if (kind == VG_GAN_LOGISTIC) {
    // (1 - t) s + softplus(-s), softplus(-s) = max(-s, 0) + log1p(exp(-|s|))
    r.loss = (1.f - t) * s + (s < 0.f ? -s : 0.f) + log1pf(e);
    r.dl = r.p - t;
  } else if (kind == VG_GAN_LSGAN) {
    const float d = s - t;
    r.loss = 0.5f * d * d;
    r.dl = d;
  } else if (kind == VG_GAN_HINGE_GEN) {
    r.loss = -s;
    r.dl = -1.f;
  } else {                                               // max(0, 1 -+ s): an exact tie has no gradient
    const float d = kind == VG_GAN_HINGE_REAL ? 1.f - s : 1.f + s;
    r.loss = d < 0.f ? 0.f : d;                          // NaN < 0 is false: d, the NaN
    r.dl = d > 0.f ? (kind == VG_GAN_HINGE_REAL ? -1.f : 1.f) : 0.f;
  }
  if (s != s) r.dl = s;
  return r;
}

// The head + loss, structured as dot_sigmoid_bce_fwd_kernel (losses.hip, whose comment has the timing that decided it):
// a wavefront owns a row (16-byte loads when `vec`, one 64-lane shuffle sum), 16 rows per workgroup; lane 0 evaluates
// the loss; the row terms go to the workspace in double and the sum kernel below adds them in index order.  No atomic.
__global__ __launch_bounds__(1024) void dot_gan_loss_fwd_kernel(const float* __restrict__ feat, const float* __restrict__ w,
                                                                const float* __restrict__ bias, int kind, Word target_w,
                                                                float* __restrict__ logit_out, float* __restrict__ p_out,
                                                                double* __restrict__ terms, float* __restrict__ dlogit,
                                                                int B, int K, float inv_div, int vec) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const float target = read_word(target_w);
  const float b0 = bias ? bias[0] : 0.f;
  const int b = blockIdx.x * 16 + wid;                 // one row per wavefront, 16 rows per workgroup
  if (b >= B) return;
  const float* row = feat + (size_t)b * K;
  float s = 0.f;
  if (vec) {                                           // K % 4 == 0, feat and w on 16-byte boundaries (the host decides)
    for (int j = 4 * lane; j < K; j += 256) {
      const float4 x = *reinterpret_cast<const float4*>(row + j);
      const float4 v = *reinterpret_cast<const float4*>(w + j);
      s = fmaf(x.x, v.x, s);
      s = fmaf(x.y, v.y, s);
      s = fmaf(x.z, v.z, s);
      s = fmaf(x.w, v.w, s);
    }
  } else {
    for (int j = lane; j < K; j += 64) s = fmaf(row[j], w[j], s);
  }
  s = wave_allsum(s);
  if (lane == 0) {
    const float logit = s + b0;
    const GanTerm r = gan_term(logit, target, kind);
    logit_out[b] = logit;
    p_out[b] = r.p;
    terms[b] = (double)r.loss;
    if (dlogit) dlogit[b] = inv_div * r.dl;
  }
}

// (sum_finalize_kernel of losses.hip, restated: that file's kernels keep their bits)
__global__ __launch_bounds__(NT) void gan_sum_finalize_kernel(const double* __restrict__ part, int nparts,
                                                              float* __restrict__ out, float scale) {
  __shared__ double red[NT / 64];
  double s = 0.0;
  for (int i = threadIdx.x; i < nparts; i += NT) s += part[i];
  const double t = block_sum<NT>(s, red);
  if (threadIdx.x == 0) out[0] = (float)(scale * t);
}

// The same losses on a logit vector (the unfused route: a hooked head), as bce_kernel serves nn.BCELoss.
__global__ __launch_bounds__(NT) void gan_loss_kernel(const float* __restrict__ logit, int kind, Word target_w,
                                                      float* __restrict__ p_out, float* __restrict__ loss,
                                                      float* __restrict__ glogit, int B, float inv_div, float gscale) {
  __shared__ double red[NT / 64];
  const float target = read_word(target_w);
  double s = 0.0;
  for (int i = threadIdx.x; i < B; i += NT) {
    const GanTerm r = gan_term(logit[i], target, kind);
    s += (double)r.loss;
    if (p_out) p_out[i] = r.p;
    if (glogit) glogit[i] = gscale * (inv_div * r.dl);
  }
  const double t = block_sum<NT>(s, red);
  if (threadIdx.x == 0 && loss) loss[0] = (float)(t * inv_div);
}

inline bool kind_ok(int kind) { return kind >= VG_GAN_LOGISTIC && kind <= VG_GAN_HINGE_GEN; }

}  // namespace

extern "C" size_t vg_dot_gan_loss_workspace_bytes(int B) { return B > 0 ? (size_t)B * sizeof(double) : 0; }

extern "C" int vg_dot_gan_loss_fwd(const float* feat, const float* w, const float* bias, int kind, float target,
                                   const float* target_dev, float* logit, float* p, float* loss, float* dlogit, int B,
                                   int K, float divisor, void* workspace, size_t workspace_bytes, void* stream) {
  if (!feat || !w || !logit || !p || !loss || !kind_ok(kind) || B <= 0 || K <= 0 || !(divisor > 0.f)) return VG_ERR_BAD_ARG;
  if (!workspace || workspace_bytes < vg_dot_gan_loss_workspace_bytes(B)) return VG_ERR_WORKSPACE;
  // a contiguous view 1-3 floats off a 16-byte boundary is a legal argument and takes the scalar loop
  const int vec = ((K & 3) == 0 && ((((uintptr_t)feat | (uintptr_t)w) & 15) == 0)) ? 1 : 0;
  double* terms = (double*)workspace;
  hipLaunchKernelGGL(dot_gan_loss_fwd_kernel, dim3(cdiv(B, 16)), dim3(1024), 0, (hipStream_t)stream, feat, w, bias, kind,
                     word_or(target, target_dev), logit, p, terms, dlogit, B, K, 1.f / divisor, vec);
  VG_CHECK_LAUNCH();
  hipLaunchKernelGGL(gan_sum_finalize_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, (const double*)terms, B, loss,
                     1.f / divisor);
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int vg_gan_loss(const float* logit, int kind, float target, const float* target_dev, float* p, float* loss,
                           float* glogit, int B, float divisor, float gscale, void* stream) {
  if (!logit || !kind_ok(kind) || B <= 0 || !(divisor > 0.f)) return VG_ERR_BAD_ARG;
  hipLaunchKernelGGL(gan_loss_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, logit, kind, word_or(target, target_dev), p,
                     loss, glogit, B, 1.f / divisor, gscale);
  VG_CHECK_LAUNCH();
  return 0;
}
