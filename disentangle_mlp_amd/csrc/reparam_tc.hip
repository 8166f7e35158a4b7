// Reparameterisation fused with the beta-TCVAE decomposition of the KL term (Chen et al. 2018, minibatch-weighted
// sampling) for gfx950: DESIGN.md section 4.17, include/vaegan_hip.h "vg_reparam_tc_*".
//
// Every pair term lq[i,j,d] = log N(z[i,d]; mu[j,d], exp(logvar[j,d])) is needed in two reductions: summed over d and
// then log-sum-exp'ed over j (the joint), and log-sum-exp'ed over j for each d (the product of marginals).  One
// workgroup owns sample i; a wavefront owns a row j at a time with its lanes along d, so
//   * the row sum over d is one 64-lane shuffle reduction (in fp64: the joint term is a difference of large sums);
//   * the per-d log-sum-exp over j is an ONLINE one -- running maximum and rescaled sum -- kept in registers by each
//     lane for its own d, and merged across the workgroup's wavefronts through LDS at the end.
// No pair term is ever stored: nothing is tiled and LDS holds [wavefronts][D] floats whatever B is.  The backward
// recomputes the pair terms the same way from the two saved log-sum-exps: the sums over j in sample i's workgroup (Gz),
// the sums over i in workgroup j (Gmu, Glv).  All cross-wavefront and cross-workgroup sums run in a fixed order and there
// is no floating-point atomic: the same inputs give the same bits.
#include "reparam_common.hpp"
#include "vaegan_hip.h"

namespace {

constexpr int NW = 8;              // wavefronts per workgroup
constexpr int NT = NW * 64;
static_assert(MAX_DIM == 16 * 64, "B and D: 16 elements of a row per lane at most");
constexpr float LOG_2PI = 1.8378770664093453f;

// lq for one (i, j, d): diff = z[i,d] - mu[j,d], lv = logvar[j,d], iv = exp(-lv)
__device__ __forceinline__ float lq_of(float diff, float lv, float iv) { return -0.5f * (LOG_2PI + lv + diff * diff * iv); }

// online log-sum-exp: (m, s) <- (m, s) (+) x with ONE exponential (the other factor is exp(0)); m starts at -inf, s at 0
__device__ __forceinline__ void lse_push(float& m, float& s, float x) {
  const float d = x - m;
  const float e = expf(-fabsf(d));
  s = d > 0.f ? fmaf(s, e, 1.f) : s + e;
  m = d > 0.f ? x : m;
}
__device__ __forceinline__ void lse_push(double& m, double& s, double x) {
  const double d = x - m;
  const double e = exp(-fabs(d));
  s = d > 0.0 ? s * e + 1.0 : s + e;
  m = d > 0.0 ? x : m;
}

// The pair terms of sample i against row j, for the d this lane owns (d = 64 k + lane): q[k] = lq, r[k] = the derivative
// factor diff * iv, df[k] = diff; returns sum_d lq over the whole row (every lane).  diff = z[i,d] - mu[j,d] is formed
// as (mu[i,d] - mu[j,d]) + eps[i,d] exp(logvar[i,d] / 2) (`mi`, `dg`), not from the rounded z: its error is then relative
// to the difference itself -- sigma can be 20 times smaller than |mu|, and near pairs carry the log-sum-exps -- and
// on the diagonal it is eps * sigma exactly.
template <int KMAX>
__device__ __forceinline__ double pair_row(const float (&mi)[KMAX], const float (&dg)[KMAX], const float* __restrict__ mu_j,
                                           const float* __restrict__ lv_j, int D, int lane, float (&q)[KMAX],
                                           float (&r)[KMAX], float (&df)[KMAX]) {
  double rs = 0.0;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    const int d = k * 64 + lane;
    q[k] = r[k] = df[k] = 0.f;
    if (d < D) {
      const float lj = lv_j[d];
      const float diff = (mi[k] - mu_j[d]) + dg[k];
      const float iv = expf(-lj);
      df[k] = diff;
      r[k] = diff * iv;
      q[k] = lq_of(diff, lj, iv);
      rs += (double)q[k];
    }
  }
  return wave_allsum(rs);
}

// ---- forward: workgroup i ------------------------------------------------------------------------------------------
// parts[i] = {lqzx_i - lqz_i, lqz_i - lqprod_i, lqprod_i - lpz_i} in fp64
template <int KMAX>
__global__ __launch_bounds__(NT) void tc_fwd_kernel(const float* __restrict__ mu, const float* __restrict__ lv,
                                                    const float* __restrict__ eps, float* __restrict__ z,
                                                    double* __restrict__ lse_joint, float* __restrict__ lse_dim,
                                                    double* __restrict__ parts, int B, int D, float log_bn_f) {
  extern __shared__ float red[];      // [NW][D]
  __shared__ double jm[NW], js[NW];
  __shared__ double s_diag;
  const int i = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const size_t row_i = (size_t)i * D;
  float zi[KMAX], mi[KMAX], dg[KMAX], cm[KMAX], cs[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    const int d = k * 64 + lane;
    zi[k] = mi[k] = dg[k] = 0.f;
    cm[k] = -INFINITY;
    cs[k] = 0.f;
    if (d < D) {
      const float h = expf(0.5f * lv[row_i + d]);
      mi[k] = mu[row_i + d];
      dg[k] = eps[row_i + d] * h;
      zi[k] = fmaf(eps[row_i + d], h, mi[k]);      // (the expression of reparam_kl_fwd_kernel: the same bits)
      if (wid == 0) z[row_i + d] = zi[k];
    }
  }
  double wm = -INFINITY, ws = 0.0;
  for (int j = wid; j < B; j += NW) {
    float q[KMAX], r[KMAX], df[KMAX];
    const double rs = pair_row<KMAX>(mi, dg, mu + (size_t)j * D, lv + (size_t)j * D, D, lane, q, r, df);
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k * 64 + lane < D) lse_push(cm[k], cs[k], q[k]);
    if (j == i && lane == 0) s_diag = rs;
    lse_push(wm, ws, rs);
  }
  // merge the wavefronts' partial log-sum-exps: the maxima first, then the sums rescaled to the common maximum
  if (lane == 0) {
    jm[wid] = wm;
    js[wid] = ws;
  }
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k * 64 + lane < D) red[wid * D + k * 64 + lane] = cm[k];
  __syncthreads();
  float gm[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    const int d = k * 64 + lane;
    gm[k] = 0.f;
    if (d < D) {
      float m = red[d];
      for (int w = 1; w < NW; ++w) m = fmaxf(m, red[w * D + d]);
      gm[k] = m;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k * 64 + lane < D) red[wid * D + k * 64 + lane] = cs[k] * expf(cm[k] - gm[k]);      // (an idle wavefront: 0 * exp(-inf) = 0)
  __syncthreads();
  if (wid != 0) return;
  double sum_lse = 0.0, lpz = 0.0;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    const int d = k * 64 + lane;
    if (d < D) {
      float s = red[d];
      for (int w = 1; w < NW; ++w) s += red[w * D + d];
      const float l = gm[k] + logf(s);
      lse_dim[row_i + d] = l;
      sum_lse += (double)l;
      lpz += (double)(-0.5f * (LOG_2PI + zi[k] * zi[k]));
    }
  }
  sum_lse = wave_allsum(sum_lse);
  lpz = wave_allsum(lpz);
  if (lane == 0) {
    double m = jm[0];
    for (int w = 1; w < NW; ++w) m = fmax(m, jm[w]);
    double s = 0.0;
    for (int w = 0; w < NW; ++w)
      if (js[w] > 0.0) s += js[w] * exp(jm[w] - m);
    const double lj = m + log(s);
    const double log_bn = (double)log_bn_f;
    const double lqprod = sum_lse - (double)D * log_bn;
    lse_joint[i] = lj;
    parts[3 * i + 0] = s_diag - lj + log_bn;
    parts[3 * i + 1] = lj - log_bn - lqprod;
    parts[3 * i + 2] = lqprod - lpz;
  }
}

// One wavefront: the per-sample parts summed in a fixed order, and the weighted loss.
__global__ __launch_bounds__(64) void tc_sum_kernel(const double* __restrict__ parts, int B, float alpha, Word beta_w,
                                                    float gamma, float* __restrict__ out4) {
  const float beta = read_word(beta_w);
  double mi = 0.0, tc = 0.0, dw = 0.0;
  for (int i = threadIdx.x; i < B; i += 64) {
    mi += parts[3 * i + 0];
    tc += parts[3 * i + 1];
    dw += parts[3 * i + 2];
  }
  mi = wave_sum(mi);
  tc = wave_sum(tc);
  dw = wave_sum(dw);
  if (threadIdx.x == 0) {
    out4[0] = (float)((double)alpha * mi + (double)beta * tc + (double)gamma * dw);
    out4[1] = (float)mi;
    out4[2] = (float)tc;
    out4[3] = (float)dw;
  }
}

// c[i,j,d] = alpha delta_ij + (beta - alpha) w[i,j] + (gamma - beta) v[i,j,d]:  the part that does not depend on d
__device__ __forceinline__ float c_row(double rs, double lse_joint_i, bool diag, float alpha, float beta) {
  const float w = (float)exp(rs - lse_joint_i);
  return fmaf(beta - alpha, w, diag ? alpha : 0.f);
}

// ---- backward, sums over j: workgroup i writes Gz[i,:] ---------------------------------------------------------------
template <int KMAX>
__global__ __launch_bounds__(NT) void tc_bwd_z_kernel(const float* __restrict__ mu, const float* __restrict__ lv,
                                                      const float* __restrict__ eps, const float* __restrict__ z,
                                                      const double* __restrict__ lse_joint,
                                                      const float* __restrict__ lse_dim, float alpha, Word beta_w,
                                                      float gamma, float* __restrict__ Gz, int B, int D) {
  const float beta = read_word(beta_w);
  extern __shared__ float red[];      // [NW][D]
  const int i = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const size_t row_i = (size_t)i * D;
  float zi[KMAX], mi[KMAX], dg[KMAX], ld[KMAX], az[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    const int d = k * 64 + lane;
    zi[k] = mi[k] = dg[k] = ld[k] = az[k] = 0.f;
    if (d < D) {
      zi[k] = z[row_i + d];
      mi[k] = mu[row_i + d];
      dg[k] = eps[row_i + d] * expf(0.5f * lv[row_i + d]);
      ld[k] = lse_dim[row_i + d];
    }
  }
  const double lj = lse_joint[i];
  for (int j = wid; j < B; j += NW) {
    float q[KMAX], r[KMAX], df[KMAX];
    const double rs = pair_row<KMAX>(mi, dg, mu + (size_t)j * D, lv + (size_t)j * D, D, lane, q, r, df);
    const float cw = c_row(rs, lj, j == i, alpha, beta);
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k * 64 + lane < D) az[k] = fmaf(fmaf(gamma - beta, expf(q[k] - ld[k]), cw), -r[k], az[k]);
  }
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k * 64 + lane < D) red[wid * D + k * 64 + lane] = az[k];
  __syncthreads();
  if (wid != 0) return;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    const int d = k * 64 + lane;
    if (d < D) {
      float s = red[d];
      for (int w = 1; w < NW; ++w) s += red[w * D + d];
      Gz[row_i + d] = fmaf(gamma, zi[k], s);
    }
  }
}

// ---- backward, sums over i: workgroup j writes gmu[j,:], glogvar[j,:] ------------------------------------------------
template <int KMAX>
__global__ __launch_bounds__(NT) void tc_bwd_q_kernel(const float* __restrict__ gz, const float* __restrict__ mu,
                                                      const float* __restrict__ lv, const float* __restrict__ eps,
                                                      const double* __restrict__ lse_joint,
                                                      const float* __restrict__ lse_dim, const float* __restrict__ gloss,
                                                      float alpha, Word beta_w, float gamma, const float* __restrict__ Gz,
                                                      float* __restrict__ gmu, float* __restrict__ glv, int B, int D) {
  const float beta = read_word(beta_w);
  extern __shared__ float red[];      // [NW][D], used for Gmu and then for Glv
  const int j = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const size_t row_j = (size_t)j * D;
  float amu[KMAX], alv[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) amu[k] = alv[k] = 0.f;
  for (int i = wid; i < B; i += NW) {
    const size_t row_i = (size_t)i * D;
    float mi[KMAX], dg[KMAX], q[KMAX], r[KMAX], df[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      const int d = k * 64 + lane;
      mi[k] = dg[k] = 0.f;
      if (d < D) {
        mi[k] = mu[row_i + d];
        dg[k] = eps[row_i + d] * expf(0.5f * lv[row_i + d]);
      }
    }
    const double rs = pair_row<KMAX>(mi, dg, mu + row_j, lv + row_j, D, lane, q, r, df);
    const float cw = c_row(rs, lse_joint[i], i == j, alpha, beta);
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      const int d = k * 64 + lane;
      if (d < D) {
        const float c = fmaf(gamma - beta, expf(q[k] - lse_dim[row_i + d]), cw);
        amu[k] = fmaf(c, r[k], amu[k]);
        alv[k] = fmaf(c, fmaf(0.5f * r[k], df[k], -0.5f), alv[k]);
      }
    }
  }
  float smu[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k * 64 + lane < D) red[wid * D + k * 64 + lane] = amu[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    const int d = k * 64 + lane;
    smu[k] = 0.f;
    if (wid == 0 && d < D) {
      float s = red[d];
      for (int w = 1; w < NW; ++w) s += red[w * D + d];
      smu[k] = s;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k * 64 + lane < D) red[wid * D + k * 64 + lane] = alv[k];
  __syncthreads();
  if (wid != 0) return;
  const float gl = gloss[0];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    const int d = k * 64 + lane;
    if (d < D) {
      float slv = red[d];
      for (int w = 1; w < NW; ++w) slv += red[w * D + d];
      const float gzd = Gz[row_j + d];
      // not reparam_bwd_store: the loss has a gradient through z too (gzd), `eh` serves both and rounds unlike g * e * 0.5f * h
      const float g = gz ? gz[row_j + d] : 0.f;
      const float eh = 0.5f * (eps[row_j + d] * expf(0.5f * lv[row_j + d]));      // d z / d logvar = eps * 0.5 * exp(logvar / 2)
      gmu[row_j + d] = fmaf(gl, smu[k] + gzd, g);
      glv[row_j + d] = fmaf(gl, fmaf(gzd, eh, slv), g * eh);
    }
  }
}

size_t parts_bytes(int B) { return (size_t)B * 3 * sizeof(double); }

int tc_fwd(const float* mu, const float* lv, const float* eps, float* z, float* out4, double* lse_joint, float* lse_dim,
           int B, int D, float alpha, Word beta, float gamma, float log_bn, void* workspace, size_t workspace_bytes,
           hipStream_t st) {
  if (!mu || !lv || !eps || !z || !out4 || !lse_joint || !lse_dim || !workspace || !dims_ok(B, D)) return VG_ERR_BAD_ARG;
  if (!words_ok(beta)) return VG_ERR_BAD_ARG;
  if (workspace_bytes < vg_reparam_tc_workspace_bytes(B, D)) return VG_ERR_WORKSPACE;
  double* parts = (double*)workspace;
  const size_t lds = (size_t)NW * D * sizeof(float);
  if (D <= 128)
    hipLaunchKernelGGL(tc_fwd_kernel<2>, dim3(B), dim3(NT), lds, st, mu, lv, eps, z, lse_joint, lse_dim, parts, B, D, log_bn);
  else
    hipLaunchKernelGGL(tc_fwd_kernel<16>, dim3(B), dim3(NT), lds, st, mu, lv, eps, z, lse_joint, lse_dim, parts, B, D, log_bn);
  VG_CHECK_LAUNCH();
  hipLaunchKernelGGL(tc_sum_kernel, dim3(1), dim3(64), 0, st, (const double*)parts, B, alpha, beta, gamma, out4);
  VG_CHECK_LAUNCH();
  return 0;
}

int tc_bwd(const float* gz, const float* mu, const float* lv, const float* eps, const float* z, const double* lse_joint,
           const float* lse_dim, const float* gloss, float alpha, Word beta, float gamma, float* gmu, float* glv, int B, int D,
           void* workspace, size_t workspace_bytes, hipStream_t st) {
  if (!mu || !lv || !eps || !z || !lse_joint || !lse_dim || !gmu || !glv || !workspace || !dims_ok(B, D)) return VG_ERR_BAD_ARG;
  if (!words_ok(beta)) return VG_ERR_BAD_ARG;
  if (workspace_bytes < vg_reparam_tc_workspace_bytes(B, D)) return VG_ERR_WORKSPACE;
  if (!gloss) return reparam_bwd_gz_only(gz, lv, eps, gmu, glv, B, D, st);
  float* Gz = (float*)((char*)workspace + parts_bytes(B));
  const size_t lds = (size_t)NW * D * sizeof(float);
  if (D <= 128) {
    hipLaunchKernelGGL(tc_bwd_z_kernel<2>, dim3(B), dim3(NT), lds, st, mu, lv, eps, z, lse_joint, lse_dim, alpha, beta, gamma,
                       Gz, B, D);
    VG_CHECK_LAUNCH();
    hipLaunchKernelGGL(tc_bwd_q_kernel<2>, dim3(B), dim3(NT), lds, st, gz, mu, lv, eps, lse_joint, lse_dim, gloss, alpha, beta,
                       gamma, (const float*)Gz, gmu, glv, B, D);
  } else {
    hipLaunchKernelGGL(tc_bwd_z_kernel<16>, dim3(B), dim3(NT), lds, st, mu, lv, eps, z, lse_joint, lse_dim, alpha, beta, gamma,
                       Gz, B, D);
    VG_CHECK_LAUNCH();
    hipLaunchKernelGGL(tc_bwd_q_kernel<16>, dim3(B), dim3(NT), lds, st, gz, mu, lv, eps, lse_joint, lse_dim, gloss, alpha, beta,
                       gamma, (const float*)Gz, gmu, glv, B, D);
  }
  VG_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// per-sample parts in fp64, then Gz
extern "C" size_t vg_reparam_tc_workspace_bytes(int B, int D) {
  return dims_ok(B, D) ? parts_bytes(B) + (size_t)B * D * sizeof(float) : 0;
}

extern "C" int vg_reparam_tc_fwd(const float* mu, const float* logvar, const float* eps, float* z, float* out4,
                                 double* lse_joint, float* lse_dim, int B, int D, float alpha, float beta, float gamma,
                                 float log_bn, void* workspace, size_t workspace_bytes, void* stream) {
  return tc_fwd(mu, logvar, eps, z, out4, lse_joint, lse_dim, B, D, alpha, word(beta), gamma, log_bn, workspace, workspace_bytes,
                (hipStream_t)stream);
}

extern "C" int vg_reparam_tc_fwd_dev(const float* mu, const float* logvar, const float* eps, float* z, float* out4,
                                     double* lse_joint, float* lse_dim, int B, int D, float alpha, const float* beta_dev,
                                     float gamma, float log_bn, void* workspace, size_t workspace_bytes, void* stream) {
  return tc_fwd(mu, logvar, eps, z, out4, lse_joint, lse_dim, B, D, alpha, word_at(beta_dev), gamma, log_bn, workspace,
                workspace_bytes, (hipStream_t)stream);
}

extern "C" int vg_reparam_tc_bwd(const float* gz, const float* mu, const float* logvar, const float* eps, const float* z,
                                 const double* lse_joint, const float* lse_dim, const float* gloss, float alpha, float beta,
                                 float gamma, float* gmu, float* glogvar, int B, int D, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  return tc_bwd(gz, mu, logvar, eps, z, lse_joint, lse_dim, gloss, alpha, word(beta), gamma, gmu, glogvar, B, D, workspace,
                workspace_bytes, (hipStream_t)stream);
}

extern "C" int vg_reparam_tc_bwd_dev(const float* gz, const float* mu, const float* logvar, const float* eps,
                                     const float* z, const double* lse_joint, const float* lse_dim, const float* gloss,
                                     float alpha, const float* beta_dev, float gamma, float* gmu, float* glogvar, int B, int D,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  return tc_bwd(gz, mu, logvar, eps, z, lse_joint, lse_dim, gloss, alpha, word_at(beta_dev), gamma, gmu, glogvar, B, D, workspace,
                workspace_bytes, (hipStream_t)stream);
}
