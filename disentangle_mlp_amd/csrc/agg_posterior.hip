// Log-density of M points under the aggregate posterior q(z) = 1/N sum_j N(mu_j, sigma_j^2), jointly and per dimension,
// at evaluation scale (N, M in the 10^4..10^5 range) for gfx950: DESIGN.md section 4.22, include/vaegan_hip.h
// "vg_agg_posterior_*".  Forward only.
//
// The pair terms are those of reparam_tc.hip, lq[i,j,d] = log N(z[i,d]; mu[j,d], exp(logvar[j,d])), in two reductions: summed
// over d and log-sum-exp'ed over j (the joint), and log-sum-exp'ed over j for each d.  The layout is the transpose of
// reparam_tc.hip's: a LANE owns an evaluation point, a wavefront a tile of 64 of them, and the rows j stream past all 64 as
// wavefront-uniform values -- scalar loads, consumed as scalar operands of the vector instructions.  Then
//   * the (mu, logvar) traffic is divided by the tile height, and it goes through the scalar cache;
//   * the sum over d and both log-sum-exps over j are serial in a lane: there is NO cross-lane operation anywhere;
//   * what depends on the row alone is formed once per row by a prepare pass, transposed so that 8 consecutive rows of
//     one d are one 32-byte scalar load: planes [mu | r | c][d][j] with, in BASE 2 (v_exp_f32 is 2^x),
//         r = sqrt(1/2 log2(e) exp(-logvar))     c = -1/2 log2(e) (log 2 pi + logvar)
//         u = (z - mu) r     lq log2(e) = fma(-u, u, c)
//     i.e. a subtract, a multiply and an FMA per pair term, each with ONE scalar operand (a gfx9 vector instruction
//     reads one scalar register: with exp(-logvar) itself as the factor the FMA would need two and a copy).  A padding
//     row has r = 0, c = -inf: its term is -inf and its exponential exactly 0 against any finite maximum.  For the joint,
//     sum_d c is a per-row constant C[j], summed in fp64 by the prepare pass: the joint kernel accumulates sum_d u^2 alone.
// The state of a per-d log-sum-exp is two registers per (point, d); a wavefront of the `dim` kernel owns 16 dimensions of
// its 64 points (grid: point tiles x chunks of 16 d x splits) and keeps z and the (max, sum) pairs in registers.  The
// joint needs the whole sum over d of a pair before it can exponentiate, so it is a kernel of its own (grid: point tiles x
// splits): 8 rows at a time, 8 fp64 sums of u^2 per lane (one fp64 FMA per pair term), one fp32 exponential of the fp64
// difference to the running maximum per (point, row).  Both log-sum-exps are tile-wise exact: the running maximum moves
// with every block of 8 rows, the sum is rescaled to it, and the first block of a split always holds a real row -- no
// fixed shift anywhere.  Four wavefronts make a workgroup for one reason only: on one CU, reading the same rows at
// nearly the same time, three of them find the rows in the scalar cache; they exchange nothing.
// N is cut into ranges of whole row tiles (a tile is one block of 8 rows); every (point tile, split) writes its (max, sum)
// pairs to the workspace and a merge kernel folds them in split order, in fp64, back to natural logarithms.  The two
// kernels are cut separately when the launcher chooses: the joint's partials are 16 bytes a point and it has no chunks
// of d to spread over the chip, so it takes many more ranges than the per-dimension kernel, whose partials are 8 bytes
// per (point, d).  No atomics: the same bits every run.
#include "common.hpp"
#include "vaegan_hip.h"

#include <float.h>
#include <math.h>

namespace {

constexpr int TM = VG_AGG_POINT_TILE;      // evaluation points per wavefront (one per lane)
constexpr int TR = VG_AGG_ROW_TILE;        // rows per row tile: the unit N is padded to and splits are counted in
constexpr int WG_WAVES = 4;                // wavefronts per workgroup: four point tiles on one CU read the same rows
constexpr int JB = 8;                      // rows per block: one 32-byte scalar load per plane and d
constexpr int DC = 16;                     // dimensions per wavefront of the dim kernel
constexpr int MAX_D = 1024;
constexpr int MAX_N = 1 << 24;
constexpr int MAX_SPLITS = 1024;
constexpr int AUTO_WAVES = 4096;           // splits = 0: each kernel gets wavefronts for four per SIMD (256 CUs x 4 SIMDs)
constexpr int AUTO_MAX_DIM_SPLITS = 64;    // ... the per-dimension kernel at most this many ranges,
constexpr int AUTO_MIN_DIM_ROWS = 64;      // of at least this many rows: its partials are written and read once per range
constexpr double LOG_2PI = 1.8378770664093454836;
constexpr double LOG2E = 1.4426950408889634074;
constexpr double LN2 = 0.69314718055994530942;

static_assert(TM == 64, "a lane owns a point");
static_assert(JB == 8 && TR % JB == 0, "a row tile is whole blocks of eight");

typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef double f64x8 __attribute__((ext_vector_type(8)));

struct Plan {
  size_t Mpad, Npad, Dpad;
  int tiles, row_tiles;
  int splits_d, tps_d;      // the per-dimension kernel: ranges, row tiles per range
  int splits_j, tps_j;      // the joint kernel
  size_t planes_off, rowc_off, zt_off, pdim_off, pjoint_off, bytes;
};

bool dims_ok(int M, int N, int D, int splits) {
  // (the last clause: the elementwise kernels' grids, 256 threads a workgroup, stay below 2^31 workgroups)
  return M >= 1 && N >= 1 && N <= MAX_N && D >= 1 && D <= MAX_D && splits >= 0 && (size_t)M * (size_t)D < ((size_t)1 << 38);
}

// The split count for (M, N, D, requested): a function of the sizes only.  A request above the number of row tiles (or
// above MAX_SPLITS) is CLAMPED; the ranges are then ceil(row_tiles / splits) tiles each and empty ranges are dropped.
Plan make_plan(int M, int N, int D, int splits) {
  Plan p;
  p.tiles = cdiv(M, TM);
  p.row_tiles = cdiv(N, TR);
  p.Mpad = (size_t)p.tiles * TM;
  p.Npad = (size_t)p.row_tiles * TR;
  p.Dpad = (size_t)cdiv(D, DC) * DC;
  int sd = splits, sj = splits;
  if (splits == 0) {
    const int dchunks = (int)(p.Dpad / DC);
    sd = min(cdiv(AUTO_WAVES, (int)min((long long)p.tiles * dchunks, (long long)AUTO_WAVES)),
             min(AUTO_MAX_DIM_SPLITS, max(N / AUTO_MIN_DIM_ROWS, 1)));
    sj = cdiv(AUTO_WAVES, min(p.tiles, AUTO_WAVES));
  }
  sd = min(sd, min(p.row_tiles, MAX_SPLITS));
  sj = min(sj, min(p.row_tiles, MAX_SPLITS));
  p.tps_d = cdiv(p.row_tiles, sd);
  p.splits_d = cdiv(p.row_tiles, p.tps_d);
  p.tps_j = cdiv(p.row_tiles, sj);
  p.splits_j = cdiv(p.row_tiles, p.tps_j);
  const auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  p.planes_off = 0;
  p.rowc_off = p.planes_off + up(3 * p.Dpad * p.Npad * sizeof(float));
  p.zt_off = p.rowc_off + up(p.Npad * sizeof(double));
  p.pdim_off = p.zt_off + up(p.Dpad * p.Mpad * sizeof(float));
  p.pjoint_off = p.pdim_off + up((size_t)p.splits_d * p.Dpad * p.Mpad * sizeof(float2));
  p.bytes = p.pjoint_off + up((size_t)p.splits_j * p.Mpad * sizeof(double2));
  return p;
}

__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }      // v_exp_f32: 2^x, 2^-inf = 0

// ---- prepare: the per-row constants, transposed to [plane][d][j]; z transposed to [d][i] ------------------------------------
__global__ __launch_bounds__(256) void agg_prep_rows_kernel(const float* __restrict__ mu, const float* __restrict__ lv,
                                                            float* __restrict__ planes, int N, int D, size_t Npad,
                                                            size_t Dpad) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, plane = Dpad * Npad;
  if (idx >= plane) return;
  const size_t d = idx / Npad, j = idx % Npad;
  float pm = 0.f, pr = 0.f, pc = j < (size_t)N ? 0.f : -INFINITY;      // a padding d adds 0 to every real row's terms
  if (d < (size_t)D && j < (size_t)N) {
    const double l = (double)lv[j * D + d];
    pm = mu[j * D + d];
    pr = (float)sqrt(0.5 * LOG2E * exp(-l));
    pc = (float)(-0.5 * LOG2E * (LOG_2PI + l));
  }
  planes[idx] = pm;
  planes[plane + idx] = pr;
  planes[2 * plane + idx] = pc;
}

// C[j] = sum_d c[j,d] in fp64 (from logvar itself, not from the rounded plane); -inf for a padding row
__global__ __launch_bounds__(256) void agg_prep_rowc_kernel(const float* __restrict__ lv, double* __restrict__ rowc, int N,
                                                            int D, size_t Npad) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= Npad) return;
  double c = -INFINITY;
  if (j < (size_t)N) {
    c = 0.0;
    for (int d = 0; d < D; ++d) c += -0.5 * LOG2E * (LOG_2PI + (double)lv[j * D + d]);
  }
  rowc[j] = c;
}

__global__ __launch_bounds__(256) void agg_prep_z_kernel(const float* __restrict__ z, float* __restrict__ zt, int M, int D,
                                                         size_t Mpad, size_t Dpad) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= Dpad * Mpad) return;
  const size_t d = idx / Mpad, i = idx % Mpad;
  zt[idx] = (d < (size_t)D && i < (size_t)M) ? z[i * D + d] : 0.f;
}

// ---- per-dimension log-sum-exp: wavefront = (point tile, 16 dimensions, split) -----------------------------------------------
// pdim[split][d][i] = (m, s): sum_j 2^(t_j) = s 2^m over the split's rows, t = lq log2(e)
__global__ __launch_bounds__(WG_WAVES * TM) void agg_dim_kernel(const float* __restrict__ planes,
                                                                const float* __restrict__ zt, float2* __restrict__ pdim,
                                                                size_t Npad, size_t Mpad, size_t Dpad, int row_tiles,
                                                                int tiles_per_split) {
  // (no barrier and no LDS in this kernel: the wavefronts of a workgroup only share the CU, and with it the scalar cache)
  const size_t i = (size_t)blockIdx.x * (WG_WAVES * TM) + threadIdx.x, d0 = (size_t)blockIdx.y * DC, plane = Dpad * Npad;
  if (i >= Mpad) return;      // whole wavefronts: Mpad is a multiple of 64
  const int t0 = blockIdx.z * tiles_per_split, t1 = min(t0 + tiles_per_split, row_tiles);
  const float* __restrict__ pmu = planes;
  const float* __restrict__ pr = planes + plane;
  const float* __restrict__ pc = planes + 2 * plane;
  float zi[DC], m[DC], s[DC];
#pragma unroll
  for (int k = 0; k < DC; ++k) {
    zi[k] = zt[(d0 + k) * Mpad + i];
    m[k] = -FLT_MAX;      // finite: m - max(m, .) is never inf - inf
    s[k] = 0.f;
  }
  for (size_t j = (size_t)t0 * TR; j < (size_t)t1 * TR; j += JB) {
#pragma unroll
    for (int k = 0; k < DC; ++k) {
      const size_t off = (d0 + k) * Npad + j;
      const f32x8 vm = *(const f32x8*)(pmu + off), vr = *(const f32x8*)(pr + off), vc = *(const f32x8*)(pc + off);
      float q[JB];
#pragma unroll
      for (int r = 0; r < JB; ++r) {
        const float u = (zi[k] - vm[r]) * vr[r];
        q[r] = fmaf(-u, u, vc[r]);
      }
      float mb = fmaxf(fmaxf(fmaxf(q[0], q[1]), fmaxf(q[2], q[3])), fmaxf(fmaxf(q[4], q[5]), fmaxf(q[6], q[7])));
      const float mn = fmaxf(m[k], mb);
      float e[JB];
#pragma unroll
      for (int r = 0; r < JB; ++r) e[r] = ex2(q[r] - mn);
      // the block's eight terms are summed among themselves first: one rounding into the long sum per block, not eight
      s[k] = fmaf(s[k], ex2(m[k] - mn), ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7])));
      m[k] = mn;
    }
  }
#pragma unroll
  for (int k = 0; k < DC; ++k) pdim[((size_t)blockIdx.z * Dpad + d0 + k) * Mpad + i] = make_float2(m[k], s[k]);
}

// ---- joint log-sum-exp: wavefront = (point tile, split) ----------------------------------------------------------------------
// pjoint[split][i] = (m, s): sum_j 2^(sum_d t_jd) = s 2^m; sum_d t_jd = C[j] - sum_d u^2, the sum in fp64
__global__ __launch_bounds__(WG_WAVES * TM) void agg_joint_kernel(const float* __restrict__ planes,
                                                                  const double* __restrict__ rowc,
                                                                  const float* __restrict__ zt, double2* __restrict__ pjoint,
                                                                  int D, size_t Npad, size_t Mpad, size_t Dpad, int row_tiles,
                                                                  int tiles_per_split) {
  const size_t i = (size_t)blockIdx.x * (WG_WAVES * TM) + threadIdx.x, plane = Dpad * Npad;
  if (i >= Mpad) return;
  const int t0 = blockIdx.y * tiles_per_split, t1 = min(t0 + tiles_per_split, row_tiles);
  const float* __restrict__ pmu = planes;
  const float* __restrict__ pr = planes + plane;
  double m = -DBL_MAX, s = 0.0;
  for (size_t j = (size_t)t0 * TR; j < (size_t)t1 * TR; j += JB) {
    double rs[JB];
#pragma unroll
    for (int r = 0; r < JB; ++r) rs[r] = 0.0;
    for (int d = 0; d < D; ++d) {
      const size_t off = (size_t)d * Npad + j;
      const float zd = zt[(size_t)d * Mpad + i];
      const f32x8 vm = *(const f32x8*)(pmu + off), vr = *(const f32x8*)(pr + off);
#pragma unroll
      for (int r = 0; r < JB; ++r) {
        const double u = (double)((zd - vm[r]) * vr[r]);
        rs[r] = fma(u, u, rs[r]);
      }
    }
    const f64x8 vc = *(const f64x8*)(rowc + j);
#pragma unroll
    for (int r = 0; r < JB; ++r) rs[r] = vc[r] - rs[r];
    double mb = rs[0];
#pragma unroll
    for (int r = 1; r < JB; ++r) mb = fmax(mb, rs[r]);
    const double mn = fmax(m, mb);
    // the differences are formed in fp64 and are <= 0; rounding one to fp32 is a relative error of 2^-24 in an exponent
    // that is small wherever the term counts
    float e[JB];
#pragma unroll
    for (int r = 0; r < JB; ++r) e[r] = ex2((float)(rs[r] - mn));
    s = s * (double)ex2((float)(m - mn)) + (double)(((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7])));
    m = mn;
  }
  pjoint[(size_t)blockIdx.y * Mpad + i] = make_double2(m, s);
}

// ---- merge: the splits' (max, sum) pairs in split order, in fp64, back to natural logarithms -----------------------------
__global__ __launch_bounds__(256) void agg_merge_kernel(const float2* __restrict__ pdim, const double2* __restrict__ pjoint,
                                                        double* __restrict__ lse_joint, float* __restrict__ lse_dim, int M,
                                                        int D, size_t Mpad, size_t Dpad, int splits, int splits_j) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx < (size_t)M * D) {
    const size_t d = idx / M, i = idx % M;      // points along the threads: the partials are read in whole lines
    float mm = -FLT_MAX;
    for (int k = 0; k < splits; ++k) mm = fmaxf(mm, pdim[((size_t)k * Dpad + d) * Mpad + i].x);
    double ss = 0.0;
    for (int k = 0; k < splits; ++k) {
      const float2 p = pdim[((size_t)k * Dpad + d) * Mpad + i];
      ss += (double)p.y * (double)ex2(p.x - mm);
    }
    lse_dim[i * D + d] = (float)(((double)mm + log2(ss)) * LN2);
  }
  if (idx < (size_t)M) {
    double mm = -DBL_MAX;
    for (int k = 0; k < splits_j; ++k) mm = fmax(mm, pjoint[(size_t)k * Mpad + idx].x);
    double ss = 0.0;
    for (int k = 0; k < splits_j; ++k) {
      const double2 p = pjoint[(size_t)k * Mpad + idx];
      ss += p.y * (double)ex2((float)(p.x - mm));
    }
    lse_joint[idx] = (mm + log2(ss)) * LN2;
  }
}

}  // namespace

extern "C" int vg_agg_posterior_splits(int M, int N, int D, int splits) {
  return dims_ok(M, N, D, splits) ? make_plan(M, N, D, splits).splits_d : 0;
}

extern "C" size_t vg_agg_posterior_workspace_bytes(int M, int N, int D, int splits) {
  return dims_ok(M, N, D, splits) ? make_plan(M, N, D, splits).bytes : 0;
}

extern "C" int vg_agg_posterior_lse(const float* z, const float* mu, const float* logvar, double* lse_joint, float* lse_dim,
                                    int M, int N, int D, int splits, void* workspace, size_t workspace_bytes, void* stream) {
  if (!z || !mu || !logvar || !lse_joint || !lse_dim || !workspace || !dims_ok(M, N, D, splits)) return VG_ERR_BAD_ARG;
  if (((uintptr_t)workspace & 255u) != 0) return VG_ERR_BAD_ARG;
  const Plan p = make_plan(M, N, D, splits);
  if (workspace_bytes < p.bytes) return VG_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float* planes = (float*)((char*)workspace + p.planes_off);
  double* rowc = (double*)((char*)workspace + p.rowc_off);
  float* zt = (float*)((char*)workspace + p.zt_off);
  float2* pdim = (float2*)((char*)workspace + p.pdim_off);
  double2* pjoint = (double2*)((char*)workspace + p.pjoint_off);
  const unsigned dchunks = (unsigned)(p.Dpad / DC);
  hipLaunchKernelGGL(agg_prep_rows_kernel, dim3((unsigned)((p.Dpad * p.Npad + 255) / 256)), dim3(256), 0, st, mu, logvar,
                     planes, N, D, p.Npad, p.Dpad);
  VG_CHECK_LAUNCH();
  hipLaunchKernelGGL(agg_prep_rowc_kernel, dim3((unsigned)((p.Npad + 255) / 256)), dim3(256), 0, st, logvar, rowc, N, D,
                     p.Npad);
  VG_CHECK_LAUNCH();
  hipLaunchKernelGGL(agg_prep_z_kernel, dim3((unsigned)((p.Dpad * p.Mpad + 255) / 256)), dim3(256), 0, st, z, zt, M, D,
                     p.Mpad, p.Dpad);
  VG_CHECK_LAUNCH();
  hipLaunchKernelGGL(agg_dim_kernel, dim3(cdiv(p.tiles, WG_WAVES), dchunks, p.splits_d), dim3(WG_WAVES * TM), 0, st, (const float*)planes,
                     (const float*)zt, pdim, p.Npad, p.Mpad, p.Dpad, p.row_tiles, p.tps_d);
  VG_CHECK_LAUNCH();
  hipLaunchKernelGGL(agg_joint_kernel, dim3(cdiv(p.tiles, WG_WAVES), p.splits_j), dim3(WG_WAVES * TM), 0, st, (const float*)planes,
                     (const double*)rowc, (const float*)zt, pjoint, D, p.Npad, p.Mpad, p.Dpad, p.row_tiles, p.tps_j);
  VG_CHECK_LAUNCH();
  hipLaunchKernelGGL(agg_merge_kernel, dim3((unsigned)(((size_t)M * D + 255) / 256)), dim3(256), 0, st,
                     (const float2*)pdim, (const double2*)pjoint, lse_joint, lse_dim, M, D, p.Mpad, p.Dpad, p.splits_d, p.splits_j);
  VG_CHECK_LAUNCH();
  return 0;
}
