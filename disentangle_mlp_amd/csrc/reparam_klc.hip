// Reparameterisation fused with the controlled KL term -- a capacity (Burgess et al. 2018, "Understanding disentangling in
// beta-VAE"; disentanglement_lib's AnnealedVAE) over per-dimension free bits (Kingma et al. 2016) -- for gfx950: DESIGN.md
// section 4.30, include/vaegan_hip.h "vg_reparam_klc_*".
//
// loss = beta |T - B C| with T the sum over the dimensions of max(K[d], B lambda), K[d] the dimension's KL summed over the
// batch.  Both the sign and the per-dimension gate of the gradient hang on batch-wide sums, so the forward is two launches:
//   cols    one workgroup per 64 rows x 64 columns, a lane per column, four wavefronts over the rows: z, and the block's
//           sum of the elements' terms per column, in fp64, to the fixed slot [row block][d];
//   finish  ONE workgroup, a thread per dimension: the slots of a column in index order -> K[d], the floor, then thread 0
//           adds K and the floored values in index order (fp64), and all write out4, gate[D] and kl_dim[D].
// The backward is ONE elementwise launch that reads gate: sgn(T - B C) where the dimension is above its floor, 0 where it
// is floored, NaN where a NaN went into T.  No floating-point atomic anywhere, every sum in a fixed order: the same inputs
// give the same bits.  beta and the capacity C are floats or device words (the `_dev` twins: a C annealed every iteration
// replays one captured graph); lambda is a frozen argument.
#include "reparam_common.hpp"
#include "vaegan_hip.h"

namespace {

constexpr int KROWS = 64;      // rows of a cols workgroup: 16 per wavefront

// ---- forward 1: z, and per (row block, column) the sum of the elements' terms of -2 KL ----------------------------------
__global__ __launch_bounds__(CNT) void klc_cols_kernel(const float* __restrict__ mu, const float* __restrict__ lv,
                                                       const float* __restrict__ eps, float* __restrict__ z,
                                                       double* __restrict__ slot, int B, int D) {
  __shared__ double red[CNT / 64][STRIP];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int d = blockIdx.x * STRIP + lane, r0 = blockIdx.y * KROWS;
  double s = 0.0;
  if (d < D) {
    const int r1 = min(r0 + KROWS, B);
    for (int b = r0 + wid; b < r1; b += CNT / 64) {
      const size_t o = (size_t)b * D + d;
      const float m = mu[o], l = lv[o];
      z[o] = reparam_z(m, l, eps[o]);
      s += kl_term(m, l);
    }
  }
  red[wid][lane] = s;
  __syncthreads();
  if (wid != 0 || d >= D) return;
  s = 0.0;
  for (int w = 0; w < CNT / 64; ++w) s += red[w][lane];
  slot[(size_t)blockIdx.y * D + d] = s;
}

// ---- forward 2: one workgroup, thread d owns dimension d ------------------------------------------------------------------
__global__ __launch_bounds__(MAX_DIM) void klc_finish_kernel(const double* __restrict__ slot, int nrb, int B, int D,
                                                             Word beta_w, Word capacity_w, float free_bits,
                                                             float* __restrict__ out4, float* __restrict__ gate,
                                                             float* __restrict__ kl_dim) {
  const float beta = read_word(beta_w), capacity = read_word(capacity_w);
  __shared__ double sk[MAX_DIM], sf[MAX_DIM];
  __shared__ double excess;      // T - B C
  const int d = threadIdx.x;
  const double floor_ = (double)B * (double)free_bits;
  double k = 0.0;
  if (d < D) {
    double s = 0.0;
    for (int r = 0; r < nrb; ++r) s += slot[(size_t)r * D + d];
    k = -0.5 * s;
    sk[d] = k;
    sf[d] = k < floor_ ? floor_ : k;      // (a NaN compares false: it stays, as torch.clamp(min=) keeps it)
  }
  __syncthreads();
  if (d == 0) {
    double kl = 0.0, tot = 0.0;
    int above = 0;
    for (int i = 0; i < D; ++i) {
      kl += sk[i];
      tot += sf[i];
      above += sk[i] > floor_ ? 1 : 0;
    }
    const double x = tot - (double)B * (double)capacity;
    out4[0] = (float)((double)beta * fabs(x));
    out4[1] = (float)kl;
    out4[2] = (float)tot;
    out4[3] = (float)above;
    excess = x;
  }
  __syncthreads();
  if (d >= D) return;
  const double x = excess;
  const float sgn = x > 0.0 ? 1.f : x < 0.0 ? -1.f : x == 0.0 ? 0.f : nanf("");      // (NaN: a NaN K[d] went into T)
  gate[d] = sgn != sgn ? sgn : k > floor_ ? sgn : 0.f;
  kl_dim[d] = (float)(k / (double)B);
}

// ---- backward: elementwise, the loss term through gate ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void klc_bwd_kernel(const float* __restrict__ gz, const float* __restrict__ mu,
                                                      const float* __restrict__ lv, const float* __restrict__ eps,
                                                      const float* __restrict__ gate, const float* __restrict__ gloss,
                                                      Word beta_w, float* __restrict__ gmu, float* __restrict__ glv, int D,
                                                      size_t n) {
  const float beta = read_word(beta_w);
  const float gl = gloss[0];
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const float bg = beta * gate[i % (size_t)D];
    const float l = lv[i], el = expf(l);
    const float pmu = bg * mu[i];
    const float plv = bg * 0.5f * (el - 1.f);
    reparam_bwd_store(gz, eps, l, gl, pmu, plv, gmu, glv, i);
  }
}

size_t slots_bytes(int B, int D) { return (size_t)cdiv(B, KROWS) * D * sizeof(double); }

// what both directions refuse before any launch (a capacity given as a float is a weight; of a word the host knows no value)
bool args_ok(int B, int D, Word beta, Word capacity, float free_bits, const void* workspace, size_t workspace_bytes) {
  if (!workspace || !dims_ok(B, D) || !weight_ok(free_bits) || workspace_bytes < slots_bytes(B, D)) return false;
  return words_ok(beta, capacity) && (!is_float(capacity) || weight_ok(capacity.v));
}

int klc_fwd(const float* mu, const float* lv, const float* eps, float* z, float* out4, float* gate, float* kl_dim, int B, int D,
            Word beta, Word capacity, float free_bits, void* workspace, size_t workspace_bytes, hipStream_t st) {
  if (!mu || !lv || !eps || !z || !out4 || !gate || !kl_dim) return VG_ERR_BAD_ARG;
  if (!args_ok(B, D, beta, capacity, free_bits, workspace, workspace_bytes)) return VG_ERR_BAD_ARG;
  double* slot = (double*)workspace;      // [row blocks][D]
  const int nrb = cdiv(B, KROWS);
  hipLaunchKernelGGL(klc_cols_kernel, dim3(cdiv(D, STRIP), nrb), dim3(CNT), 0, st, mu, lv, eps, z, slot, B, D);
  VG_CHECK_LAUNCH();
  hipLaunchKernelGGL(klc_finish_kernel, dim3(1), dim3(cdiv(D, 64) * 64), 0, st, (const double*)slot, nrb, B, D, beta, capacity,
                     free_bits, out4, gate, kl_dim);
  VG_CHECK_LAUNCH();
  return 0;
}

int klc_bwd(const float* gz, const float* mu, const float* lv, const float* eps, const float* gate, const float* gloss,
            Word beta, Word capacity, float free_bits, float* gmu, float* glv, int B, int D, void* workspace,
            size_t workspace_bytes, hipStream_t st) {
  if (!mu || !lv || !eps || !gate || !gmu || !glv) return VG_ERR_BAD_ARG;
  if (!args_ok(B, D, beta, capacity, free_bits, workspace, workspace_bytes)) return VG_ERR_BAD_ARG;
  if (!gloss) return reparam_bwd_gz_only(gz, lv, eps, gmu, glv, B, D, st);
  const size_t n = (size_t)B * D;
  hipLaunchKernelGGL(klc_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, gz, mu, lv, eps, gate, gloss, beta,
                     gmu, glv, D, n);
  VG_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// the column sums per block of 64 rows, fp64
extern "C" size_t vg_reparam_klc_workspace_bytes(int B, int D) { return dims_ok(B, D) ? slots_bytes(B, D) : 0; }

extern "C" int vg_reparam_klc_fwd(const float* mu, const float* logvar, const float* eps, float* z, float* out4, float* gate,
                                  float* kl_dim, int B, int D, float beta, float capacity, float free_bits, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  return klc_fwd(mu, logvar, eps, z, out4, gate, kl_dim, B, D, word(beta), word(capacity), free_bits, workspace,
                 workspace_bytes, (hipStream_t)stream);
}

extern "C" int vg_reparam_klc_fwd_dev(const float* mu, const float* logvar, const float* eps, float* z, float* out4,
                                      float* gate, float* kl_dim, int B, int D, const float* beta_dev,
                                      const float* capacity_dev, float free_bits, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  return klc_fwd(mu, logvar, eps, z, out4, gate, kl_dim, B, D, word_at(beta_dev), word_at(capacity_dev), free_bits, workspace,
                 workspace_bytes, (hipStream_t)stream);
}

extern "C" int vg_reparam_klc_bwd(const float* gz, const float* mu, const float* logvar, const float* eps, const float* gate,
                                  const float* gloss, float beta, float capacity, float free_bits, float* gmu, float* glogvar,
                                  int B, int D, void* workspace, size_t workspace_bytes, void* stream) {
  return klc_bwd(gz, mu, logvar, eps, gate, gloss, word(beta), word(capacity), free_bits, gmu, glogvar, B, D, workspace,
                 workspace_bytes, (hipStream_t)stream);
}

extern "C" int vg_reparam_klc_bwd_dev(const float* gz, const float* mu, const float* logvar, const float* eps,
                                      const float* gate, const float* gloss, const float* beta_dev, const float* capacity_dev,
                                      float free_bits, float* gmu, float* glogvar, int B, int D, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  return klc_bwd(gz, mu, logvar, eps, gate, gloss, word_at(beta_dev), word_at(capacity_dev), free_bits, gmu, glogvar, B, D,
                 workspace, workspace_bytes, (hipStream_t)stream);
}
