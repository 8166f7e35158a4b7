// Reparameterisation fused with the InfoVAE / WAE-MMD objective (Zhao et al. 2019; Tolstikhin et al. 2018) for gfx950:
// DESIGN.md section 4.23, include/vaegan_hip.h "vg_reparam_mmd_*".
//
// The plain KL term plus the unbiased maximum-mean-discrepancy between the aggregate posterior (the B draws z) and the
// prior (B draws zp), under a sum of RBF or inverse-multiquadratic kernels of up to 8 bandwidths.  Every squared distance
// is formed from the DIFFERENCES (a_d - b_d): the Gram form |a|^2 + |b|^2 - 2 a.b cancels for close points, which is
// where the kernel values matter (identical rows give d == 0 and k == 1 to the bit here).  Three launches forward:
//   z       one workgroup per strip of 64 columns, 16 wavefronts over the rows: z and the strip's KL partial in fp64;
//   pairs   one workgroup per 32 x 32 tile of one of the three pair matrices -- zz and pp ON OR ABOVE the diagonal, zp in
//           full -- the two row blocks staged in LDS 64 columns at a time; the distance is chains of 16 fp32 FMAs of the
//           differences in column order, the chain sums added in fp64; k and k' are evaluated once per pair in fp64; the
//           tile's sum of k goes to a fixed fp64 slot, and k'(d) with its prefactor folded in goes to w[2, B, B] (fp32: zz
//           mirrored with a zero diagonal, zp);
//   sum     one wavefront adds the slots in order and writes out4.
// The backward is ONE launch: a workgroup per 16 rows x 64 columns accumulates sum_j w[i, j] (z_id - x_jd) over both
// matrices (chains of 8 fp32 FMAs over j, their sums in fp64: the zz and the zp sum nearly cancel, and the rounding of a
// longer chain comes back multiplied) and applies the elementwise terms.  No floating-point atomic anywhere, every
// cross-lane, cross-wavefront and cross-workgroup sum in a fixed order: the same inputs give the same bits.  Plain VALU
// work, no MFMA: 3 B^2 D subtract-multiply-adds are 6 MFLOP at (128, 128), and the time is launch and latency.
#include "reparam_common.hpp"
#include "vaegan_hip.h"

namespace {

// The geometry is reparam_common.hpp's: a strip is a z workgroup's, a tile one of a pair matrix, BK columns (pairs) / rows j
// (backward) of one LDS chunk.
constexpr int MAX_BW = 8;          // bandwidths of one kernel sum
constexpr int CHAIN_D = 16;        // length of an fp32 FMA chain of squared differences; the chain sums are added in fp64
constexpr int CHAIN_J = 8;         // the same in the backward, where the zz and the zp sums cancel: see mmd_bwd_kernel
static_assert(BK % CHAIN_D == 0 && BK % CHAIN_J == 0, "chains tile a chunk");
constexpr int KIND_RBF = 1, KIND_IMQ = 2;

struct Bandwidths {      // copied into the kernel arguments
  float h[MAX_BW];
  int n;
};

__host__ __device__ constexpr int pair_tiles(int B) { return 2 * upper_tiles(B) + tiles_of(B) * tiles_of(B); }

// ---- forward 1: z and the KL partial of a strip ---------------------------------------------------------------------------
__global__ __launch_bounds__(SNW * 64) void mmd_z_kernel(const float* __restrict__ mu, const float* __restrict__ lv,
                                                         const float* __restrict__ eps, float* __restrict__ z,
                                                         double* __restrict__ klp, int B, int D) {
  __shared__ double red[SNW][STRIP];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int d = blockIdx.x * STRIP + lane;
  double sk = 0.0;
  if (d < D) {
    for (int b = wid; b < B; b += SNW) {
      const size_t o = (size_t)b * D + d;
      const float m = mu[o], l = lv[o];
      z[o] = reparam_z(m, l, eps[o]);
      sk += kl_term(m, l);
    }
  }
  red[wid][lane] = sk;
  __syncthreads();
  if (wid != 0) return;
  sk = 0.0;
  for (int w = 0; w < SNW; ++w) sk += red[w][lane];
  sk = wave_sum(sk);
  if (lane == 0) klp[blockIdx.x] = -0.5 * sk;
}

// k(d) and k'(d) summed over the bandwidths, in bandwidth order.  Once per pair, against D subtract-multiply-adds for its
// distance: evaluated in fp64 (exp and true division, no fast intrinsic), so that the slopes the backward reads carry one
// rounding, their own -- its zz and zp sums cancel, and every relative error of a slope comes back multiplied.
template <int KIND>
__device__ __forceinline__ void kernel_sum(double d, const Bandwidths& bw, double& k, double& dk) {
  k = 0.0;
  dk = 0.0;
  for (int s = 0; s < bw.n; ++s) {
    const double h = (double)bw.h[s];
    if constexpr (KIND == KIND_RBF) {
      const double e = exp(-d / h);
      k += e;
      dk -= e / h;
    } else {
      const double q = h / (h + d);
      k += q;
      dk -= q / (h + d);
    }
  }
}

// ---- forward 2: one tile of zz (slots [0, U)), pp ([U, 2U)) or zp ([2U, 2U + nt^2)) -----------------------------------------
template <int KIND>
__global__ __launch_bounds__(CNT) void mmd_pairs_kernel(const float* __restrict__ z, const float* __restrict__ zp,
                                                        float* __restrict__ w, double* __restrict__ pairp, int B, int D,
                                                        Bandwidths bw) {
  __shared__ float sa[BK][TILE + 1], sb[BK][TILE + 1];      // [column][row]: the pad keeps the staging stores off one bank
  __shared__ double red[1][CNT / 64];
  const int nt = tiles_of(B), U = upper_tiles(B);
  int idx = blockIdx.x, which = 0, tr, tc;      // which: 0 zz, 1 pp, 2 zp
  if (idx >= 2 * U) {
    which = 2;
    idx -= 2 * U;
    tr = idx / nt;
    tc = idx % nt;
  } else {
    if (idx >= U) {
      which = 1;
      idx -= U;
    }
    const TilePair upper = upper_tile(idx, nt);
    tr = upper.tr;
    tc = upper.tc;
  }
  const float* __restrict__ xa = which == 1 ? zp : z;
  const float* __restrict__ xb = which == 0 ? z : zp;
  const int i0 = tr * TILE, j0 = tc * TILE;
  const int t = threadIdx.x, ti = t >> 4, tj = t & 15;      // outputs (ti, ti + 16) x (tj, tj + 16) of the tile
  const int lc = t & 63, lr = t >> 6;                        // staging: column lc, rows lr + 4 k
  double tot[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  for (int c0 = 0; c0 < D; c0 += BK) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < TILE / 4; ++k) {
      const int r = lr + 4 * k, c = c0 + lc;
      sa[lc][r] = (i0 + r < B && c < D) ? xa[(size_t)(i0 + r) * D + c] : 0.f;
      sb[lc][r] = (j0 + r < B && c < D) ? xb[(size_t)(j0 + r) * D + c] : 0.f;
    }
    __syncthreads();
    const int nc = min(BK, D - c0);
    for (int cc = 0; cc < nc; cc += CHAIN_D) {      // (columns past D are staged as zeros on both sides: difference 0)
      float a00 = 0.f, a01 = 0.f, a10 = 0.f, a11 = 0.f;
#pragma unroll
      for (int u = 0; u < CHAIN_D; ++u) {
        const int c = cc + u;
        const float x0 = sa[c][ti], x1 = sa[c][ti + 16], y0 = sb[c][tj], y1 = sb[c][tj + 16];
        const float d00 = x0 - y0, d01 = x0 - y1, d10 = x1 - y0, d11 = x1 - y1;
        a00 = fmaf(d00, d00, a00);
        a01 = fmaf(d01, d01, a01);
        a10 = fmaf(d10, d10, a10);
        a11 = fmaf(d11, d11, a11);
      }
      tot[0][0] += (double)a00;
      tot[0][1] += (double)a01;
      tot[1][0] += (double)a10;
      tot[1][1] += (double)a11;
    }
  }
  // the prefactors of the gradient: 4 / (B (B - 1)) on zz, -4 / B^2 on zp
  const double pref = which == 0 ? 4.0 / ((double)B * (double)(B - 1)) : -4.0 / ((double)B * (double)B);
  const bool mirrored = which != 2 && tr != tc;
  float* __restrict__ wm = w + (which == 2 ? (size_t)B * B : 0);
  double part[1] = {0.0};
  double& ks = part[0];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int i = i0 + ti + 16 * p, j = j0 + tj + 16 * q;
      if (i < B && j < B) {
        const bool self = which != 2 && i == j;      // the U-statistic leaves the i == j terms of zz and pp out
        double k, dk;
        kernel_sum<KIND>(tot[p][q], bw, k, dk);
        if (!self) ks += (mirrored ? 2.0 : 1.0) * k;
        if (which != 1) {
          const float wv = self ? 0.f : (float)(pref * dk);
          wm[(size_t)i * B + j] = wv;
          if (mirrored) wm[(size_t)j * B + i] = wv;
        }
      }
    }
  tile_slot_sums(part, red, pairp + blockIdx.x);
}

// ---- forward 3: one wavefront, the partials in slot order -------------------------------------------------------------------
// BETA_DEV (this kernel and the backward): beta read from the device word.  The other objectives take a `Word` (common.hpp);
// as a Word this file's captured forward + backward at (256, 128) measured 0.78 us above the parent's median with a spread
// of 0.66 us (profiles/scheduled_word.json), so its two kernels keep the compile-time twin.
template <bool BETA_DEV>
__global__ __launch_bounds__(64) void mmd_sum_kernel(const double* __restrict__ klp, int nstrips,
                                                     const double* __restrict__ pairp, int B, float beta,
                                                     const float* __restrict__ beta_dev, float lambda_mmd,
                                                     float* __restrict__ out4) {
  if constexpr (BETA_DEV) beta = beta_dev[0];
  const int nt = tiles_of(B), U = upper_tiles(B);
  double kl = 0.0, szz = 0.0, spp = 0.0, szp = 0.0;
  for (int i = threadIdx.x; i < nstrips; i += 64) kl += klp[i];
  for (int i = threadIdx.x; i < U; i += 64) {
    szz += pairp[i];
    spp += pairp[U + i];
  }
  for (int i = threadIdx.x; i < nt * nt; i += 64) szp += pairp[2 * U + i];
  kl = wave_sum(kl);
  szz = wave_sum(szz);
  spp = wave_sum(spp);
  szp = wave_sum(szp);
  if (threadIdx.x == 0) {
    const double off = (double)B * (double)(B - 1), all = (double)B * (double)B;
    const double kzz = szz / off, kpp = spp / off, kzp = szp / all;
    const double mmd = kzz + kpp - 2.0 * kzp;
    out4[0] = (float)((double)beta * kl + (double)B * (double)lambda_mmd * mmd);
    out4[1] = (float)kl;
    out4[2] = (float)mmd;
    out4[3] = (float)kzz;
  }
}

// ---- backward: rows [RB blockIdx.y, +RB) x columns [64 blockIdx.x, +64) -----------------------------------------------------
// Gz[i, d] = B lambda sum_j (w[0, i, j] (z[i, d] - z[j, d]) + w[1, i, j] (z[i, d] - zp[j, d]))
template <bool BETA_DEV>
__global__ __launch_bounds__(CNT) void mmd_bwd_kernel(const float* __restrict__ gz, const float* __restrict__ mu,
                                                      const float* __restrict__ lv, const float* __restrict__ eps,
                                                      const float* __restrict__ z, const float* __restrict__ zp,
                                                      const float* __restrict__ w, const float* __restrict__ gloss,
                                                      float beta, const float* __restrict__ beta_dev, float lambda_mmd,
                                                      float* __restrict__ gmu, float* __restrict__ glv, int B, int D) {
  if constexpr (BETA_DEV) beta = beta_dev[0];
  __shared__ float sw[RB][BK];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int d = blockIdx.x * 64 + lane, r0 = blockIdx.y * RB;
  float zi[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int b = r0 + wid * 4 + q;
    zi[q] = (b < B && d < D) ? z[(size_t)b * D + d] : 0.f;
  }
  double tot[4] = {0.0, 0.0, 0.0, 0.0};
  for (int m = 0; m < 2; ++m) {
    const float* __restrict__ wm = w + (size_t)m * B * B;
    const float* __restrict__ x = m == 0 ? z : zp;
    for (int j0 = 0; j0 < B; j0 += BK) {
      __syncthreads();
#pragma unroll
      for (int k = 0; k < RB / 4; ++k) {
        const int rr = wid + 4 * k, b = r0 + rr, j = j0 + lane;
        sw[rr][lane] = (b < B && j < B) ? wm[(size_t)b * B + j] : 0.f;
      }
      __syncthreads();
      if (d < D) {
        const int nj = min(BK, B - j0);
        for (int jc = 0; jc < nj; jc += CHAIN_J) {
          float xv[CHAIN_J];      // the chain's loads first, all in flight together (rows past B: w is staged as 0 there)
#pragma unroll
          for (int u = 0; u < CHAIN_J; ++u) xv[u] = jc + u < nj ? x[(size_t)(j0 + jc + u) * D + d] : 0.f;
          float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int u = 0; u < CHAIN_J; ++u) {
#pragma unroll
            for (int q = 0; q < 4; ++q) a[q] = fmaf(sw[wid * 4 + q][jc + u], zi[q] - xv[u], a[q]);
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) tot[q] += (double)a[q];
        }
      }
    }
  }
  if (d >= D) return;
  const float gl = gloss[0];
  const double scale = (double)B * (double)lambda_mmd;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int b = r0 + wid * 4 + q;
    if (b < B) {
      const size_t o = (size_t)b * D + d;
      const float l = lv[o], el = expf(l);
      const float s = eps[o] * 0.5f * expf(0.5f * l);      // dz / dlogvar
      const float Gz = (float)(scale * tot[q]);
      const float pmu = fmaf(beta, mu[o], Gz);
      const float plv = fmaf(beta * 0.5f, el - 1.f, Gz * s);
      // an absent gz takes its whole term out, as in reparam_kl_bwd_kernel.  Not reparam_bwd_store: that adds a zero term,
      // fmaf(gl, pmu, 0.f), and this a bare product -- the two differ in the sign of a zero product
      gmu[o] = gz ? fmaf(gl, pmu, gz[o]) : gl * pmu;
      glv[o] = gz ? fmaf(gl, plv, gz[o] * s) : gl * plv;
    }
  }
}

constexpr int MIN_B = 2;           // the U-statistic divides by B - 1

template <bool BETA_DEV>
int mmd_fwd(const float* mu, const float* lv, const float* eps, const float* zp, float* z, float* out4, float* w, int B, int D,
            int kind, float beta, const float* beta_dev, float lambda_mmd, const float* bandwidths, int n_bandwidths,
            void* workspace, size_t workspace_bytes, hipStream_t st) {
  if (!mu || !lv || !eps || !zp || !z || !out4 || !w || !bandwidths || !workspace || !dims_ok(B, D, MIN_B)) return VG_ERR_BAD_ARG;
  if ((kind != KIND_RBF && kind != KIND_IMQ) || n_bandwidths < 1 || n_bandwidths > MAX_BW || !weight_ok(lambda_mmd))
    return VG_ERR_BAD_ARG;
  if (BETA_DEV && !beta_dev) return VG_ERR_BAD_ARG;
  if (workspace_bytes < vg_reparam_mmd_workspace_bytes(B, D)) return VG_ERR_BAD_ARG;
  Bandwidths bw = {};
  bw.n = n_bandwidths;
  for (int s = 0; s < n_bandwidths; ++s) {
    if (!(isfinite(bandwidths[s]) && bandwidths[s] > 0.f)) return VG_ERR_BAD_ARG;
    bw.h[s] = bandwidths[s];
  }
  double* klp = (double*)workspace;      // [KL_SLOTS], then one sum of k per pair tile
  double* pairp = klp + KL_SLOTS;
  const int nstrips = cdiv(D, STRIP), ntiles = pair_tiles(B);
  hipLaunchKernelGGL(mmd_z_kernel, dim3(nstrips), dim3(SNW * 64), 0, st, mu, lv, eps, z, klp, B, D);
  VG_CHECK_LAUNCH();
  if (kind == KIND_RBF)
    hipLaunchKernelGGL(mmd_pairs_kernel<KIND_RBF>, dim3(ntiles), dim3(CNT), 0, st, (const float*)z, zp, w, pairp, B, D, bw);
  else
    hipLaunchKernelGGL(mmd_pairs_kernel<KIND_IMQ>, dim3(ntiles), dim3(CNT), 0, st, (const float*)z, zp, w, pairp, B, D, bw);
  VG_CHECK_LAUNCH();
  hipLaunchKernelGGL(mmd_sum_kernel<BETA_DEV>, dim3(1), dim3(64), 0, st, (const double*)klp, nstrips, (const double*)pairp, B,
                     beta, beta_dev, lambda_mmd, out4);
  VG_CHECK_LAUNCH();
  return 0;
}

template <bool BETA_DEV>
int mmd_bwd(const float* gz, const float* mu, const float* lv, const float* eps, const float* z, const float* zp,
            const float* w, const float* gloss, float beta, const float* beta_dev, float lambda_mmd, float* gmu, float* glv,
            int B, int D, void* workspace, size_t workspace_bytes, hipStream_t st) {
  if (!mu || !lv || !eps || !z || !zp || !w || !gmu || !glv || !workspace || !dims_ok(B, D, MIN_B) || !weight_ok(lambda_mmd))
    return VG_ERR_BAD_ARG;
  if (BETA_DEV && !beta_dev) return VG_ERR_BAD_ARG;
  if (workspace_bytes < vg_reparam_mmd_workspace_bytes(B, D)) return VG_ERR_BAD_ARG;
  if (!gloss) return reparam_bwd_gz_only(gz, lv, eps, gmu, glv, B, D, st);
  hipLaunchKernelGGL(mmd_bwd_kernel<BETA_DEV>, dim3(cdiv(D, 64), cdiv(B, RB)), dim3(CNT), 0, st, gz, mu, lv, eps, z, zp, w,
                     gloss, beta, beta_dev, lambda_mmd, gmu, glv, B, D);
  VG_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// KL partials per strip, then the sum of k per pair tile (zz, pp, zp): all fp64
extern "C" size_t vg_reparam_mmd_workspace_bytes(int B, int D) {
  return dims_ok(B, D, MIN_B) ? (size_t)(KL_SLOTS + pair_tiles(B)) * sizeof(double) : 0;
}

extern "C" int vg_reparam_mmd_fwd(const float* mu, const float* logvar, const float* eps, const float* zp, float* z,
                                  float* out4, float* w, int B, int D, int kind, float beta, float lambda_mmd,
                                  const float* bandwidths, int n_bandwidths, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  return mmd_fwd<false>(mu, logvar, eps, zp, z, out4, w, B, D, kind, beta, nullptr, lambda_mmd, bandwidths, n_bandwidths,
                        workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int vg_reparam_mmd_fwd_dev(const float* mu, const float* logvar, const float* eps, const float* zp, float* z,
                                      float* out4, float* w, int B, int D, int kind, const float* beta_dev, float lambda_mmd,
                                      const float* bandwidths, int n_bandwidths, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  return mmd_fwd<true>(mu, logvar, eps, zp, z, out4, w, B, D, kind, 0.f, beta_dev, lambda_mmd, bandwidths, n_bandwidths,
                       workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int vg_reparam_mmd_bwd(const float* gz, const float* mu, const float* logvar, const float* eps, const float* z,
                                  const float* zp, const float* w, const float* gloss, float beta, float lambda_mmd,
                                  float* gmu, float* glogvar, int B, int D, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  return mmd_bwd<false>(gz, mu, logvar, eps, z, zp, w, gloss, beta, nullptr, lambda_mmd, gmu, glogvar, B, D, workspace,
                        workspace_bytes, (hipStream_t)stream);
}

extern "C" int vg_reparam_mmd_bwd_dev(const float* gz, const float* mu, const float* logvar, const float* eps, const float* z,
                                      const float* zp, const float* w, const float* gloss, const float* beta_dev,
                                      float lambda_mmd, float* gmu, float* glogvar, int B, int D, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  return mmd_bwd<true>(gz, mu, logvar, eps, z, zp, w, gloss, 0.f, beta_dev, lambda_mmd, gmu, glogvar, B, D, workspace,
                       workspace_bytes, (hipStream_t)stream);
}
