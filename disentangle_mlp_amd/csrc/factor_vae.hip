// FactorVAE (Kim & Mnih 2018, "Disentangling by Factorising"; disentanglement_lib's form) for gfx950: DESIGN.md section
// 4.32, include/vaegan_hip.h "vg_permute_dims", "vg_factor_tc_*", "vg_factor_critic_loss".
//
// The total correlation is estimated by a critic on the latent code that tells z ~ q(z) (class 0) from a z whose
// dimensions were permuted independently across the batch (class 1).  Three small pieces run on this library; the
// critic's GEMMs are the vendor's (model.LatentCritic).
//   permute   z_perm[rank_d(i), d] = z[i, d] with rank_d(i) the position of u[i, d] in the STABLE ascending order of column
//             d of the uniforms u (ties by row index): rank by counting.  A workgroup stages a strip of 16 columns of u, all B
//             rows, in LDS (a lane per column, so a wavefront reads 16 banks and four broadcast rows: no conflict), and each
//             thread counts, for two rows of its column, the rows that sort before them.  No sort network, no atomic, one
//             launch; every output element is written by exactly one thread.
//   tc        the encoder phase's loss from the critic's logits on z: loss = beta kl + gamma sum_b (l0 - l1), fp64, one
//             workgroup; the backward is the constant +-gamma gloss per row and beta gloss to the KL.
//   critic    the critic phase's cross-entropy on the 2B rows [z; z_perm], its gradient and its accuracy in ONE launch.
// Every sum: lanes by wavefront shuffle, the wavefronts' fp64 slots added in index order -- the same inputs give the same
// bits.  beta and gamma are floats or device words (the `_dev` twins: a gamma annealed every iteration replays one graph).
#include "common.hpp"
#include "vaegan_hip.h"

#include <math.h>

namespace {

constexpr int NT = 256;

// ---- permute_dims ---------------------------------------------------------------------------------------------------------------
constexpr int PC = 16;               // columns of a strip: one per lane of a quarter wavefront, 64 contiguous bytes a row
constexpr int PR = NT / PC;          // row slots of a workgroup
constexpr int PROWS = 2 * PR;        // rows a workgroup ranks: two per thread, one LDS read serves both

// The total order of torch.sort on floats -- ascending, -0 == +0, every NaN behind every number and equal to every NaN -- as
// an unsigned integer: the staged image holds keys, and (key, row index) read as ONE 64-bit integer is the stable order, so
// "sorts before, or ties and stands in front" is a single compare per pair.
__device__ __forceinline__ unsigned sort_key(float v) {
  if (v != v) return 0xff800001u;                      // above +inf's key, 0xff800000
  const unsigned b = __float_as_uint(v);
  return (b & 0x80000000u) ? (b == 0x80000000u ? 0x80000000u : ~b) : (b | 0x80000000u);
}
__device__ __forceinline__ unsigned long long stable_key(unsigned key, int row) {
  return ((unsigned long long)key << 32) | (unsigned)row;
}

// CAP: the rows the LDS image holds (CAP * PC keys).  Row i of column d goes to row #{j : (key_j, j) < (key_i, i)} -- row i
// itself never counts, so the target lies in [0, B - 1] whatever u holds.
template <int CAP>
__global__ __launch_bounds__(NT) void permute_dims_kernel(const float* __restrict__ z, const float* __restrict__ u,
                                                          float* __restrict__ z_perm, int B, int D) {
  __shared__ unsigned su[CAP * PC];
  const int c = threadIdx.x % PC, r = threadIdx.x / PC;
  const int d = blockIdx.x * PC + c;
  const bool col = d < D;
#pragma unroll 8
  for (int j = r; j < B; j += PR) su[j * PC + c] = col ? sort_key(u[(size_t)j * D + d]) : 0u;      // (eight loads in flight)
  __syncthreads();
  const int i0 = blockIdx.y * PROWS + r, i1 = i0 + PR;
  const bool on0 = col && i0 < B, on1 = col && i1 < B;
  const unsigned long long k0 = on0 ? stable_key(su[i0 * PC + c], i0) : 0ull, k1 = on1 ? stable_key(su[i1 * PC + c], i1) : 0ull;
  int n0 = 0, n1 = 0;
#pragma unroll 8
  for (int j = 0; j < B; ++j) {
    const unsigned long long kj = stable_key(su[j * PC + c], j);
    n0 += kj < k0 ? 1 : 0;
    n1 += kj < k1 ? 1 : 0;
  }
  if (on0) z_perm[(size_t)n0 * D + d] = z[(size_t)i0 * D + d];
  if (on1) z_perm[(size_t)n1 * D + d] = z[(size_t)i1 * D + d];
}

template <int CAP>
int permute_launch(const float* z, const float* u, float* z_perm, int B, int D, hipStream_t st) {
  hipLaunchKernelGGL(permute_dims_kernel<CAP>, dim3(cdiv(D, PC), cdiv(B, PROWS)), dim3(NT), 0, st, z, u, z_perm, B, D);
  VG_CHECK_LAUNCH();
  return 0;
}

// ---- the encoder phase's loss ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void factor_tc_fwd_kernel(const float* __restrict__ logits, const float* __restrict__ kl,
                                                           float* __restrict__ out4, int B, Word beta_w, Word gamma_w) {
  const float beta = read_word(beta_w), gamma = read_word(gamma_w);
  __shared__ double red[NT / 64];
  double s = 0.0, n = 0.0;
  for (int b = threadIdx.x; b < B; b += NT) {
    const float l0 = logits[2 * (size_t)b], l1 = logits[2 * (size_t)b + 1];
    s += (double)l0 - (double)l1;
    n += l0 > l1 ? 1.0 : 0.0;
  }
  const double tc = block_sum<NT>(s, red);
  const double q = block_sum<NT>(n, red);
  if (threadIdx.x != 0) return;
  const float k = kl[0];
  out4[0] = (float)((double)beta * (double)k + (double)gamma * tc);
  out4[1] = k;
  out4[2] = (float)tc;
  out4[3] = (float)q;
}

__global__ __launch_bounds__(NT) void factor_tc_bwd_kernel(const float* __restrict__ gloss, Word beta_w, Word gamma_w,
                                                           float* __restrict__ glogits, float* __restrict__ gkl, int B) {
  const float beta = read_word(beta_w), gamma = read_word(gamma_w);
  const float gl = gloss[0];
  const float g = gamma * gl;
  const int b = blockIdx.x * NT + threadIdx.x;
  if (b < B) {
    glogits[2 * (size_t)b] = g;
    glogits[2 * (size_t)b + 1] = -g;
  }
  if (b == 0) gkl[0] = beta * gl;
}

// ---- the critic phase's loss, its gradient and its accuracy ----------------------------------------------------------------------
// log(1 + e^x) and 1 / (1 + e^-x) without overflow; compare + select, so a NaN stays a NaN
__device__ __forceinline__ float softplus_safe(float x) { return (x > 0.f ? x : 0.f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float sigmoid_safe(float x) {
  const float e = expf(-fabsf(x));
  return x >= 0.f ? 1.f / (1.f + e) : x < 0.f ? e / (1.f + e) : x;
}

// rows [0, B): class 0, x = l1 - l0; rows [B, 2B): class 1, x = l0 - l1.  term = softplus(x); d term / d x = sigmoid(x); a row
// is on the right side of 0 iff x < 0 (a tie and a NaN are wrong).
__global__ __launch_bounds__(NT) void factor_critic_loss_kernel(const float* __restrict__ logits, float* __restrict__ loss,
                                                                float* __restrict__ glogits, float* __restrict__ acc, int B,
                                                                float divisor) {
  __shared__ double red[NT / 64];
  const float inv_div = 1.f / divisor;
  double s = 0.0, n = 0.0;
  for (int b = threadIdx.x; b < 2 * B; b += NT) {
    const float l0 = logits[2 * (size_t)b], l1 = logits[2 * (size_t)b + 1];
    const bool first = b < B;
    const float x = first ? l1 - l0 : l0 - l1;
    s += (double)softplus_safe(x);
    n += x < 0.f ? 1.0 : 0.0;
    if (glogits) {
      const float g = sigmoid_safe(x) * inv_div;      // d loss / d (the other class's logit); minus that for the row's own
      glogits[2 * (size_t)b] = first ? -g : g;
      glogits[2 * (size_t)b + 1] = first ? g : -g;
    }
  }
  const double t = block_sum<NT>(s, red);
  const double q = block_sum<NT>(n, red);
  if (threadIdx.x != 0) return;
  loss[0] = (float)(t / (double)divisor);
  if (acc) acc[0] = (float)(q / (2.0 * (double)B));
}

constexpr int MAX_ROWS = 1 << 28;      // logits of 2 * MAX_ROWS rows are indexed in int

int tc_fwd(const float* logits, const float* kl, float* out4, int B, Word beta, Word gamma, hipStream_t st) {
  if (!logits || !kl || !out4 || B < 1 || B > MAX_ROWS || !words_ok(beta, gamma)) return VG_ERR_BAD_ARG;
  hipLaunchKernelGGL(factor_tc_fwd_kernel, dim3(1), dim3(NT), 0, st, logits, kl, out4, B, beta, gamma);
  VG_CHECK_LAUNCH();
  return 0;
}

int tc_bwd(const float* gloss, Word beta, Word gamma, float* glogits, float* gkl, int B, hipStream_t st) {
  if (!gloss || !glogits || !gkl || B < 1 || B > MAX_ROWS || !words_ok(beta, gamma)) return VG_ERR_BAD_ARG;
  hipLaunchKernelGGL(factor_tc_bwd_kernel, dim3(cdiv(B, NT)), dim3(NT), 0, st, gloss, beta, gamma, glogits, gkl, B);
  VG_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int vg_permute_dims(const float* z, const float* u, float* z_perm, int B, int D, void* stream) {
  if (!z || !u || !z_perm || z_perm == z || z_perm == u || B < 1 || B > VG_PERMUTE_MAX_BATCH || D < 1) return VG_ERR_BAD_ARG;
  if ((size_t)B * (size_t)D > ((size_t)1 << 40)) return VG_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (B <= 256) return permute_launch<256>(z, u, z_perm, B, D, st);                 // 16 KiB of LDS
  if (B <= 1024) return permute_launch<1024>(z, u, z_perm, B, D, st);               // 64 KiB
  return permute_launch<VG_PERMUTE_MAX_BATCH>(z, u, z_perm, B, D, st);              // 128 KiB of the CU's 160
}

// nothing is staged: the query exists for the one call site of the objectives' entry points
extern "C" size_t vg_factor_tc_workspace_bytes(int B, int D) {
  (void)B, (void)D;
  return 0;
}

extern "C" int vg_factor_tc_fwd(const float* logits, const float* kl, float* out4, int B, float beta, float gamma,
                                void* workspace, size_t workspace_bytes, void* stream) {
  (void)workspace, (void)workspace_bytes;
  return tc_fwd(logits, kl, out4, B, word(beta), word(gamma), (hipStream_t)stream);
}

extern "C" int vg_factor_tc_fwd_dev(const float* logits, const float* kl, float* out4, int B, const float* beta_dev,
                                    const float* gamma_dev, void* workspace, size_t workspace_bytes, void* stream) {
  (void)workspace, (void)workspace_bytes;
  return tc_fwd(logits, kl, out4, B, word_at(beta_dev), word_at(gamma_dev), (hipStream_t)stream);
}

extern "C" int vg_factor_tc_bwd(const float* gloss, float beta, float gamma, float* glogits, float* gkl, int B, void* workspace,
                                size_t workspace_bytes, void* stream) {
  (void)workspace, (void)workspace_bytes;
  return tc_bwd(gloss, word(beta), word(gamma), glogits, gkl, B, (hipStream_t)stream);
}

extern "C" int vg_factor_tc_bwd_dev(const float* gloss, const float* beta_dev, const float* gamma_dev, float* glogits,
                                    float* gkl, int B, void* workspace, size_t workspace_bytes, void* stream) {
  (void)workspace, (void)workspace_bytes;
  return tc_bwd(gloss, word_at(beta_dev), word_at(gamma_dev), glogits, gkl, B, (hipStream_t)stream);
}

extern "C" int vg_factor_critic_loss(const float* logits, float* loss, float* glogits, float* acc, int B, float divisor,
                                     void* stream) {
  if (!logits || !loss || glogits == logits || B < 1 || B > MAX_ROWS / 2 || !(divisor > 0.f) || !(divisor <= 3.402823466e38f))
    return VG_ERR_BAD_ARG;
  hipLaunchKernelGGL(factor_critic_loss_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, logits, loss, glogits, acc, B,
                     divisor);
  VG_CHECK_LAUNCH();
  return 0;
}
