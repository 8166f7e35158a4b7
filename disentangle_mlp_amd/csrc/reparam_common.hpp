// What the reparameterisation kernels fused with an objective of the KL phase -- reparam_tc.hip, reparam_dip.hip,
// reparam_mmd.hip, reparam_klc.hip -- have in common to the letter: DESIGN.md section 4.24.  Only that: a kernel whose
// inner loop differs between two of them (chain lengths, staging layout) stays in its file, and nothing here asks who
// calls it.  What it holds:
//   all four files   MAX_DIM and dims_ok, weight_ok (a float weight: finite and >= 0), the per-element expressions
//                    (reparam_z, kl_term) and the gz-only backward;
//   klc and dip      reparam_bwd_store, the end of their elementwise backward (mmd and tc keep their own stores: each
//                    says why where it stands);
//   dip and mmd      the tile geometry, the tile decode and the slot sums (reparam_klc.hip takes the strip's width and
//                    the workgroup size from it).
// A scheduled value -- beta, the capacity -- is a `Word` (common.hpp).  Everything has internal linkage: each file compiles
// its own copy.
#pragma once
#include "common.hpp"

#include <math.h>

namespace {

constexpr int MAX_DIM = 1024;      // B and D
inline bool dims_ok(int B, int D, int min_b = 1) { return B >= min_b && B <= MAX_DIM && D >= 1 && D <= MAX_DIM; }
// a weight given as a float (lambda, free bits, a capacity): finite and >= 0.  Written as two comparisons, which a NaN
// fails both: the same floats pass as with isfinite(v) && v >= 0.f, and no classification call is needed.
inline bool weight_ok(float v) { return v >= 0.f && v <= 3.402823466e38f; }

// ---- the geometry reparam_dip.hip and reparam_mmd.hip share (their own comments say what a row and a column are) -------
constexpr int STRIP = 64;          // columns of a strip workgroup (z and the KL partial): one per lane
constexpr int SNW = 16;            // its wavefronts
constexpr int TILE = 32;           // a tile of the D x D covariance / a B x B pair matrix is TILE x TILE, 2 x 2 outputs per thread
constexpr int CNT = 256;           // threads of a tile workgroup and of a backward workgroup
constexpr int BK = 64;             // length of one LDS chunk of the tile and backward kernels
constexpr int RB = 16;             // rows of a backward workgroup: 4 per wavefront
constexpr int KL_SLOTS = MAX_DIM / STRIP;

__host__ __device__ constexpr int tiles_of(int n) { return cdiv(n, TILE); }
__host__ __device__ constexpr int upper_tiles(int n) { return tiles_of(n) * (tiles_of(n) + 1) / 2; }

// the idx-th pair (tr <= tc) in row-major order of the upper triangle of nt x nt tiles
struct TilePair {
  int tr, tc;
};
__device__ __forceinline__ TilePair upper_tile(int idx, int nt) {
  int tr = 0;
  while (idx >= nt - tr) {
    idx -= nt - tr;
    ++tr;
  }
  return {tr, tr + idx};
}

// The end of a tile kernel: N fp64 partials summed over the CNT threads, lanes first (wave_sum), then the four wavefronts
// in order; thread 0 writes the sums to the tile's N slots.
template <int N>
__device__ __forceinline__ void tile_slot_sums(const double (&part)[N], double (&red)[N][CNT / 64], double* __restrict__ slot) {
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  double v[N];
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = wave_sum(part[n]);
  if (lane == 0) {
#pragma unroll
    for (int n = 0; n < N; ++n) red[n][wid] = v[n];
  }
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int n = 0; n < N; ++n) v[n] = 0.0;
    for (int w = 0; w < CNT / 64; ++w) {
#pragma unroll
      for (int n = 0; n < N; ++n) v[n] += red[n][w];
    }
#pragma unroll
    for (int n = 0; n < N; ++n) slot[n] = v[n];
  }
}

// ---- per element ------------------------------------------------------------------------------------------------------------
// z (the expression of reparam_kl_fwd_kernel: the same bits)
__device__ __forceinline__ float reparam_z(float mu, float lv, float eps) { return fmaf(eps, expf(0.5f * lv), mu); }
// the element's term of -2 KL, in fp64
__device__ __forceinline__ double kl_term(float mu, float lv) {
  return 1.0 + (double)lv - (double)mu * (double)mu - (double)expf(lv);
}

// The end of an elementwise backward: element o gets gl times the loss term's partials (pmu, plv) plus the decoder's
// gradient through z; l = lv[o].  An absent gz takes its whole term out, every factor of it, as in reparam_kl_bwd_kernel.
__device__ __forceinline__ void reparam_bwd_store(const float* __restrict__ gz, const float* __restrict__ eps, float l, float gl,
                                                  float pmu, float plv, float* __restrict__ gmu, float* __restrict__ glv,
                                                  size_t o) {
  const float g = gz ? gz[o] : 0.f, e = gz ? eps[o] : 0.f, h = gz ? expf(0.5f * l) : 0.f;
  gmu[o] = fmaf(gl, pmu, g);
  glv[o] = fmaf(gl, plv, g * e * 0.5f * h);
}

// ---- backward with gloss absent ---------------------------------------------------------------------------------------------
// The loss term is out as a whole (as in reparam_kl_bwd_kernel); what is left is the decoder's gradient.
__global__ __launch_bounds__(256) void reparam_bwd_gz_only_kernel(const float* __restrict__ gz, const float* __restrict__ lv,
                                                                  const float* __restrict__ eps, float* __restrict__ gmu,
                                                                  float* __restrict__ glv, size_t n) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const float g = gz ? gz[i] : 0.f, e = gz ? eps[i] : 0.f, h = gz ? expf(0.5f * lv[i]) : 0.f;
    gmu[i] = g;
    glv[i] = g * e * 0.5f * h;
  }
}

inline int reparam_bwd_gz_only(const float* gz, const float* lv, const float* eps, float* gmu, float* glv, int B, int D,
                               hipStream_t st) {
  const size_t n = (size_t)B * D;
  hipLaunchKernelGGL(reparam_bwd_gz_only_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, gz, lv, eps, gmu, glv, n);
  VG_CHECK_LAUNCH();
  return 0;
}

}  // namespace
