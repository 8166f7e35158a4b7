// Reparameterisation fused with the DIP-VAE objectives (Kumar et al. 2018, variants I and II) for gfx950: DESIGN.md
// section 4.21, include/vaegan_hip.h "vg_reparam_dip_*".
//
// The plain KL term plus a penalty that pulls the covariance C of the aggregate posterior towards the identity.  C is
// formed in its CENTRED shape, (1/B) sum_b c_b c_b^T with c = mu - mean: the column means come first, in fp64, and every
// centred element is the fp64 difference rounded once -- a common offset of the means costs nothing, where
// E[mu mu^T] - m m^T in fp32 would lose it all.  Three launches forward:
//   stats   one workgroup per strip of 64 columns, 16 wavefronts over the rows: z, mean[D] (and, variant II, the column
//           means of exp(logvar)) and the strip's KL partial, all summed in fp64 in a fixed order;
//   cov     one workgroup per 32 x 32 tile of C ON OR ABOVE the diagonal, the centred columns staged in LDS 64 rows at a
//           time; each chunk is a chain of fp32 FMAs in row order, the chunk sums are added in fp64; the tile is written
//           to cov[D, D] and mirrored, its od / dg partial goes to a fixed slot in fp64;
//   sum     one wavefront adds the partials in slot order and writes out4.
// The backward is ONE launch: a workgroup per 16 rows x 64 columns forms c_b . G with G built from cov on load (the same
// chunked FMA chains, over i) and applies the elementwise terms.  No floating-point atomic anywhere, every cross-lane,
// cross-wavefront and cross-workgroup sum in a fixed order: the same inputs give the same bits.  Plain FMAs, no MFMA: the
// whole product is 2 B D^2 = 4 MFLOP at (128, 128), and the time is launch and latency.
#include "reparam_common.hpp"
#include "vaegan_hip.h"

namespace {

// The geometry is reparam_common.hpp's: a strip is a stats workgroup's, a tile one of the covariance, BK rows (cov) /
// columns i (backward) of one LDS chunk: the length of an fp32 FMA chain.

// the centred element, formed the same way wherever it is needed: exact in fp64, rounded once
__device__ __forceinline__ float centred(float mu, double mean) { return (float)((double)mu - mean); }

// ---- forward 1: z, column means, KL partial ----------------------------------------------------------------------------
__global__ __launch_bounds__(SNW * 64) void dip_stats_kernel(const float* __restrict__ mu, const float* __restrict__ lv,
                                                             const float* __restrict__ eps, float* __restrict__ z,
                                                             double* __restrict__ mean, double* __restrict__ evar,
                                                             double* __restrict__ klp, int B, int D, int variant) {
  __shared__ double red[3][SNW][STRIP];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int d = blockIdx.x * STRIP + lane;
  double sm = 0.0, se = 0.0, sk = 0.0;
  if (d < D) {
    for (int b = wid; b < B; b += SNW) {
      const size_t o = (size_t)b * D + d;
      const float m = mu[o], l = lv[o];
      z[o] = reparam_z(m, l, eps[o]);
      const float el = expf(l);
      sm += (double)m;
      se += (double)el;
      sk += kl_term(m, l);
    }
  }
  red[0][wid][lane] = sm;
  red[1][wid][lane] = se;
  red[2][wid][lane] = sk;
  __syncthreads();
  if (wid != 0) return;
  sm = se = sk = 0.0;
  for (int w = 0; w < SNW; ++w) {
    sm += red[0][w][lane];
    se += red[1][w][lane];
    sk += red[2][w][lane];
  }
  if (d < D) {
    mean[d] = sm / (double)B;
    if (variant == 2) evar[d] = se / (double)B;
  }
  sk = wave_sum(sk);
  if (lane == 0) klp[blockIdx.x] = -0.5 * sk;
}

// ---- forward 2: one tile of C on or above the diagonal -----------------------------------------------------------------
__global__ __launch_bounds__(CNT) void dip_cov_kernel(const float* __restrict__ mu, const double* __restrict__ mean,
                                                      const double* __restrict__ evar, float* __restrict__ cov,
                                                      double* __restrict__ covp, int B, int D, int variant) {
  __shared__ float sa[BK][TILE], sb[BK][TILE];
  __shared__ double red[2][CNT / 64];
  const auto [tr, tc] = upper_tile(blockIdx.x, tiles_of(D));
  const int i0 = tr * TILE, j0 = tc * TILE;
  const int t = threadIdx.x, ti = t >> 4, tj = t & 15;      // outputs (ti, ti + 16) x (tj, tj + 16) of the tile
  const int lc = t & 31, lr = t >> 5;                        // staging: column lc, rows lr + 8 k
  const bool a_in = i0 + lc < D, b_in = j0 + lc < D;
  const double ma = a_in ? mean[i0 + lc] : 0.0, mb = b_in ? mean[j0 + lc] : 0.0;
  double tot[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  for (int b0 = 0; b0 < B; b0 += BK) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < BK / 8; ++k) {
      const int r = lr + 8 * k, b = b0 + r;
      sa[r][lc] = (b < B && a_in) ? centred(mu[(size_t)b * D + i0 + lc], ma) : 0.f;
      sb[r][lc] = (b < B && b_in) ? centred(mu[(size_t)b * D + j0 + lc], mb) : 0.f;
    }
    __syncthreads();
    const int nb = min(BK, B - b0);
    float a00 = 0.f, a01 = 0.f, a10 = 0.f, a11 = 0.f;
    for (int r = 0; r < nb; ++r) {
      const float x0 = sa[r][ti], x1 = sa[r][ti + 16], y0 = sb[r][tj], y1 = sb[r][tj + 16];
      a00 = fmaf(x0, y0, a00);
      a01 = fmaf(x0, y1, a01);
      a10 = fmaf(x1, y0, a10);
      a11 = fmaf(x1, y1, a11);
    }
    tot[0][0] += (double)a00;
    tot[0][1] += (double)a01;
    tot[1][0] += (double)a10;
    tot[1][1] += (double)a11;
  }
  double part[2] = {0.0, 0.0};      // {od, dg}
  double &od = part[0], &dg = part[1];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int i = i0 + ti + 16 * p, j = j0 + tj + 16 * q;
      if (i < D && j < D) {
        double cd = tot[p][q] / (double)B;
        if (i == j && variant == 2) cd += evar[i];
        const float c = (float)cd;
        cov[(size_t)i * D + j] = c;
        if (tr != tc) cov[(size_t)j * D + i] = c;      // the mirrored tile
        if (i == j)
          dg += ((double)c - 1.0) * ((double)c - 1.0);
        else
          od += (tr != tc ? 2.0 : 1.0) * (double)c * (double)c;
      }
    }
  tile_slot_sums(part, red, covp + 2 * blockIdx.x);
}

// ---- forward 3: one wavefront, the partials in slot order ---------------------------------------------------------------
__global__ __launch_bounds__(64) void dip_sum_kernel(const double* __restrict__ klp, int nstrips,
                                                     const double* __restrict__ covp, int ntiles, int B, Word beta_w,
                                                     float lambda_od, float lambda_d, float* __restrict__ out4) {
  const float beta = read_word(beta_w);
  double kl = 0.0, od = 0.0, dg = 0.0;
  for (int i = threadIdx.x; i < nstrips; i += 64) kl += klp[i];
  for (int i = threadIdx.x; i < ntiles; i += 64) {
    od += covp[2 * i + 0];
    dg += covp[2 * i + 1];
  }
  kl = wave_sum(kl);
  od = wave_sum(od);
  dg = wave_sum(dg);
  if (threadIdx.x == 0) {
    out4[0] = (float)((double)beta * kl + (double)B * ((double)lambda_od * od + (double)lambda_d * dg));
    out4[1] = (float)kl;
    out4[2] = (float)od;
    out4[3] = (float)dg;
  }
}

// ---- backward: rows [RB blockIdx.y, +RB) x columns [64 blockIdx.x, +64) --------------------------------------------------
// G_id = 2 lambda_od C_id (i != d), 2 lambda_d (C_dd - 1) on the diagonal; Gmu[b, d] = 2 sum_i c[b, i] G[i, d].
__global__ __launch_bounds__(CNT) void dip_bwd_kernel(const float* __restrict__ gz, const float* __restrict__ mu,
                                                      const float* __restrict__ lv, const float* __restrict__ eps,
                                                      const float* __restrict__ cov, const double* __restrict__ mean,
                                                      const float* __restrict__ gloss, int variant, Word beta_w,
                                                      float lambda_od, float lambda_d, float* __restrict__ gmu,
                                                      float* __restrict__ glv, int B, int D) {
  const float beta = read_word(beta_w);
  __shared__ float sc[RB][BK];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int d = blockIdx.x * 64 + lane, r0 = blockIdx.y * RB;
  const float two_od = 2.f * lambda_od, two_d = 2.f * lambda_d;
  double tot[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i0 = 0; i0 < D; i0 += BK) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RB / 4; ++k) {
      const int rr = wid + 4 * k, b = r0 + rr, i = i0 + lane;
      sc[rr][lane] = (b < B && i < D) ? centred(mu[(size_t)b * D + i], mean[i]) : 0.f;
    }
    __syncthreads();
    if (d < D) {
      const int ni = min(BK, D - i0);
      float a[4] = {0.f, 0.f, 0.f, 0.f};
      for (int ii = 0; ii < ni; ++ii) {
        const int i = i0 + ii;
        const float cv = cov[(size_t)i * D + d];
        const float g = i == d ? two_d * (cv - 1.f) : two_od * cv;
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] = fmaf(sc[wid * 4 + q][ii], g, a[q]);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) tot[q] += (double)a[q];
    }
  }
  if (d >= D) return;
  const float gl = gloss[0];
  const float gdd = variant == 2 ? two_d * (cov[(size_t)d * D + d] - 1.f) : 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int b = r0 + wid * 4 + q;
    if (b < B) {
      const size_t o = (size_t)b * D + d;
      const float l = lv[o], el = expf(l);
      const float pmu = fmaf(beta, mu[o], (float)(2.0 * tot[q]));
      const float plv = fmaf(beta * 0.5f, el - 1.f, gdd * el);
      reparam_bwd_store(gz, eps, l, gl, pmu, plv, gmu, glv, o);
    }
  }
}

bool variant_ok(int v) { return v == 1 || v == 2; }

int dip_fwd(const float* mu, const float* lv, const float* eps, float* z, float* out4, float* cov, double* mean, int B, int D,
            int variant, Word beta, float lambda_od, float lambda_d, void* workspace, size_t workspace_bytes, hipStream_t st) {
  if (!mu || !lv || !eps || !z || !out4 || !cov || !mean || !workspace || !dims_ok(B, D) || !variant_ok(variant))
    return VG_ERR_BAD_ARG;
  if (!words_ok(beta)) return VG_ERR_BAD_ARG;
  if (workspace_bytes < vg_reparam_dip_workspace_bytes(B, D)) return VG_ERR_WORKSPACE;
  double* klp = (double*)workspace;      // [KL_SLOTS], then evar [D], then {od, dg} per tile
  double* evar = klp + KL_SLOTS;
  double* covp = evar + D;
  const int nstrips = cdiv(D, STRIP), ntiles = upper_tiles(D);
  hipLaunchKernelGGL(dip_stats_kernel, dim3(nstrips), dim3(SNW * 64), 0, st, mu, lv, eps, z, mean, evar, klp, B, D, variant);
  VG_CHECK_LAUNCH();
  hipLaunchKernelGGL(dip_cov_kernel, dim3(ntiles), dim3(CNT), 0, st, mu, (const double*)mean, (const double*)evar, cov, covp,
                     B, D, variant);
  VG_CHECK_LAUNCH();
  hipLaunchKernelGGL(dip_sum_kernel, dim3(1), dim3(64), 0, st, (const double*)klp, nstrips, (const double*)covp, ntiles, B, beta,
                     lambda_od, lambda_d, out4);
  VG_CHECK_LAUNCH();
  return 0;
}

int dip_bwd(const float* gz, const float* mu, const float* lv, const float* eps, const float* cov, const double* mean,
            const float* gloss, int variant, Word beta, float lambda_od, float lambda_d, float* gmu, float* glv, int B, int D,
            void* workspace, size_t workspace_bytes, hipStream_t st) {
  if (!mu || !lv || !eps || !cov || !mean || !gmu || !glv || !workspace || !dims_ok(B, D) || !variant_ok(variant))
    return VG_ERR_BAD_ARG;
  if (!words_ok(beta)) return VG_ERR_BAD_ARG;
  if (workspace_bytes < vg_reparam_dip_workspace_bytes(B, D)) return VG_ERR_WORKSPACE;
  if (!gloss) return reparam_bwd_gz_only(gz, lv, eps, gmu, glv, B, D, st);
  hipLaunchKernelGGL(dip_bwd_kernel, dim3(cdiv(D, 64), cdiv(B, RB)), dim3(CNT), 0, st, gz, mu, lv, eps, cov, mean, gloss,
                     variant, beta, lambda_od, lambda_d, gmu, glv, B, D);
  VG_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// KL partials per strip, the column means of exp(logvar), {od, dg} per tile: all fp64
extern "C" size_t vg_reparam_dip_workspace_bytes(int B, int D) {
  return dims_ok(B, D) ? (size_t)(KL_SLOTS + D + 2 * upper_tiles(D)) * sizeof(double) : 0;
}

extern "C" int vg_reparam_dip_fwd(const float* mu, const float* logvar, const float* eps, float* z, float* out4, float* cov,
                                  double* mean, int B, int D, int variant, float beta, float lambda_od, float lambda_d,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  return dip_fwd(mu, logvar, eps, z, out4, cov, mean, B, D, variant, word(beta), lambda_od, lambda_d, workspace, workspace_bytes,
                 (hipStream_t)stream);
}

extern "C" int vg_reparam_dip_fwd_dev(const float* mu, const float* logvar, const float* eps, float* z, float* out4,
                                      float* cov, double* mean, int B, int D, int variant, const float* beta_dev,
                                      float lambda_od, float lambda_d, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  return dip_fwd(mu, logvar, eps, z, out4, cov, mean, B, D, variant, word_at(beta_dev), lambda_od, lambda_d, workspace,
                 workspace_bytes, (hipStream_t)stream);
}

extern "C" int vg_reparam_dip_bwd(const float* gz, const float* mu, const float* logvar, const float* eps, const float* cov,
                                  const double* mean, const float* gloss, int variant, float beta, float lambda_od,
                                  float lambda_d, float* gmu, float* glogvar, int B, int D, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  return dip_bwd(gz, mu, logvar, eps, cov, mean, gloss, variant, word(beta), lambda_od, lambda_d, gmu, glogvar, B, D, workspace,
                 workspace_bytes, (hipStream_t)stream);
}

extern "C" int vg_reparam_dip_bwd_dev(const float* gz, const float* mu, const float* logvar, const float* eps,
                                      const float* cov, const double* mean, const float* gloss, int variant,
                                      const float* beta_dev, float lambda_od, float lambda_d, float* gmu, float* glogvar,
                                      int B, int D, void* workspace, size_t workspace_bytes, void* stream) {
  return dip_bwd(gz, mu, logvar, eps, cov, mean, gloss, variant, word_at(beta_dev), lambda_od, lambda_d, gmu, glogvar, B, D,
                 workspace, workspace_bytes, (hipStream_t)stream);
}
