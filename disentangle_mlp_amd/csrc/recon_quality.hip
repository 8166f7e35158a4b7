// Reconstruction quality of an image batch against its originals for gfx950: per image the sum of squared errors, the mean
// of the SSIM map (Wang et al. 2004) and the mean of its contrast-structure map (what MS-SSIM, Wang et al. 2003, takes from
// every scale but the last).  DESIGN.md section 4.26, include/vaegan_hip.h "vg_recon_quality".
//
// A workgroup of 256 threads owns one (image, channel, band of VG_RECON_BAND_ROWS output rows, tile of VG_RECON_TILE_COLS
// output columns).  It stages the two input tiles with their halo of window - 1 rows and columns into LDS as fp32
// (positions past the image read as 0 and are never used by a valid output), runs the horizontal pass of the five window
// moments (x, y, x^2, y^2, xy) for every staged row into LDS as fp64 (a thread owns four adjacent columns of one row: it
// reads their pixels as 16-byte vectors and converts and squares each once), then the vertical pass: a thread owns one
// output column and two adjacent output rows, whose chains share all but one of the rows they read.  Nothing of the
// moments' size goes to global memory.
//
// Arithmetic: the taps are fp64, formed on the host and passed by value.  Each pass is ONE fp64 FMA chain in ascending tap
// order starting from 0; the products x^2, y^2, xy of fp32 inputs are formed in fp64, where they are exact.  So a moment
// of a given pixel has the same bits whichever workgroup, band or tile forms it, and identical inputs give identical
// moments: mu_x == mu_y, E[x^2] == E[y^2] == E[xy] to the bit.  Everything after the moments is fp64 WITHOUT contraction
// (an fma in mu_x^2 + mu_y^2 would break 2 mu_x mu_y == mu_x^2 + mu_y^2 for identical images): x against itself gives
// numerator == denominator and an IEEE quotient of exactly 1.
//
// Reduction: per thread in a fixed order, over the wavefront by shuffles, over the four wavefronts in index order, into
// the workgroup's slot of the workspace ([slot of the image][3][B] fp64); a finalize kernel (a thread per image) adds an
// image's slots in index order.  No atomics: the same bits every run, and -- the slots of an image depend on nothing but
// that image -- the same bits wherever in a batch the image stands.  A NaN stays in its image's slots.
#include "common.hpp"
#include "vaegan_hip.h"

#include <math.h>

namespace {

constexpr int RB = VG_RECON_BAND_ROWS;      // output rows per band
constexpr int CT = VG_RECON_TILE_COLS;      // output columns per tile
constexpr int NT = 256;
constexpr int MAX_WIN = 11;
constexpr int ROWS_PER_THREAD = RB * CT / NT;
constexpr int CPT = 4;                      // output columns per thread of the horizontal pass

static_assert(CT == 32 && NT % CT == 0, "a thread's column is tid % 32: a wavefront reads two whole rows of doubles");
static_assert(ROWS_PER_THREAD == 2 && RB == (NT / CT) * ROWS_PER_THREAD, "a thread owns two adjacent output rows");

struct Params {
  double w[MAX_WIN];
  double c1, c2;
};

struct Plan {
  int OH, OW, bands, tiles;
  long long per_image, blocks;      // workgroups (= slots) per image, per batch
  size_t bytes;
};

bool window_ok(int window) { return window >= 3 && window <= MAX_WIN && (window & 1); }

bool dims_ok(int B, int C, int H, int W, int window) {
  return B >= 1 && C >= 1 && H >= 1 && W >= 1 && window_ok(window) && H >= window && W >= window;
}

// false: the grid (one workgroup per slot, image-major in grid.x) or the workspace would not fit its index types
bool make_plan(int B, int C, int H, int W, int window, Plan& p) {
  p.OH = H - window + 1;
  p.OW = W - window + 1;
  p.bands = cdiv(p.OH, RB);
  p.tiles = cdiv(p.OW, CT);
  p.per_image = (long long)C * p.bands * p.tiles;
  if (p.per_image > 0x7fffffffLL) return false;
  p.blocks = p.per_image * B;
  if (p.blocks > 0x7fffffffLL) return false;
  p.bytes = ((size_t)p.blocks * 3 * sizeof(double) + 255) / 256 * 256;
  return true;
}

template <int WIN>
__global__ __launch_bounds__(NT) void recon_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                   double* __restrict__ slots, int B, int C, int H, int W, int bands,
                                                   int tiles, int per_image, Params prm) {
  constexpr int IN_ROWS = RB + WIN - 1;
  // horizontal pass: a thread owns CPT adjacent output columns of one staged row and reads their WIN + CPT - 1 pixels as
  // NQ 16-byte vectors; PITCH (a multiple of 4 floats, >= the CT + WIN - 1 staged columns) keeps the last thread's
  // last vector inside its row
  constexpr int NQ = (WIN + CPT - 1 + 3) / 4, PITCH = CT - CPT + 4 * NQ;
  static_assert(PITCH >= CT + WIN - 1 && PITCH % 4 == 0 && IN_ROWS * (CT / CPT) <= NT, "one horizontal item per thread");
  __shared__ __attribute__((aligned(16))) float xs[IN_ROWS][PITCH], ys[IN_ROWS][PITCH];
  __shared__ double hs[5][IN_ROWS][CT];
  __shared__ double red[NT / 64];

  const int tid = threadIdx.x;
  const int b = blockIdx.x / per_image, slot = blockIdx.x - b * per_image;
  const int tile = slot % tiles, band = (slot / tiles) % bands, ch = slot / (tiles * bands);
  const int r0 = band * RB, c0 = tile * CT;
  const int OH = H - WIN + 1, OW = W - WIN + 1;
  const int out_rows = min(RB, OH - r0), out_cols = min(CT, OW - c0);
  // the squared error of every input pixel belongs to exactly one workgroup: the band's RB rows (the last band: all
  // it stages, through row H - 1), the tile's CT columns (the last tile: through column W - 1)
  const int own_rows = band == bands - 1 ? H - r0 : RB, own_cols = tile == tiles - 1 ? W - c0 : CT;
  const size_t base = ((size_t)b * C + ch) * H * W;

  double sse = 0.0;
  for (int i = tid; i < IN_ROWS * PITCH; i += NT) {
    const int r = i / PITCH, c = i - r * PITCH;
    const bool in = r0 + r < H && c0 + c < W;
    const size_t at = base + (size_t)(r0 + r) * W + (c0 + c);
    const float xv = in ? x[at] : 0.f, yv = in ? y[at] : 0.f;
    xs[r][c] = xv;
    ys[r][c] = yv;
    if (r < own_rows && c < own_cols) {       // (own_* never reach past the image)
      const double d = (double)xv - (double)yv;
      sse = fma(d, d, sse);
    }
  }
  __syncthreads();

  // horizontal pass: every staged row, the tile's CT output columns
  // A pixel is converted and squared once per thread and feeds tap p - j of column j: per column the taps still arrive
  // in ascending order, each chain is the one a thread per column would form.
  if (tid < IN_ROWS * (CT / CPT)) {
    const int r = tid / (CT / CPT), cg = (tid % (CT / CPT)) * CPT;
    float xr[4 * NQ], yr[4 * NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const f32x4 xv = *(const f32x4*)&xs[r][cg + 4 * q], yv = *(const f32x4*)&ys[r][cg + 4 * q];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        xr[4 * q + e] = xv[e];
        yr[4 * q + e] = yv[e];
      }
    }
    double acc[CPT][5];
#pragma unroll
    for (int j = 0; j < CPT; ++j)
#pragma unroll
      for (int q = 0; q < 5; ++q) acc[j][q] = 0.0;
#pragma unroll
    for (int p = 0; p < WIN + CPT - 1; ++p) {
      const double xv = (double)xr[p], yv = (double)yr[p];
      const double xx = xv * xv, yy = yv * yv, xy = xv * yv;      // (products of two fp32 values: exact in fp64)
#pragma unroll
      for (int j = 0; j < CPT; ++j) {
        const int k = p - j;
        if (k >= 0 && k < WIN) {
          const double wk = prm.w[k];
          acc[j][0] = fma(wk, xv, acc[j][0]);
          acc[j][1] = fma(wk, yv, acc[j][1]);
          acc[j][2] = fma(wk, xx, acc[j][2]);
          acc[j][3] = fma(wk, yy, acc[j][3]);
          acc[j][4] = fma(wk, xy, acc[j][4]);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 5; ++q)
#pragma unroll
      for (int j = 0; j < CPT; ++j) hs[q][r][cg + j] = acc[j][q];
  }
  __syncthreads();

  // vertical pass: column tid % CT, output rows 2 (tid / CT) and 2 (tid / CT) + 1
  const int c = tid % CT, ra = (tid / CT) * ROWS_PER_THREAD;
  double m[ROWS_PER_THREAD][5];
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    double col[WIN + ROWS_PER_THREAD - 1];
#pragma unroll
    for (int k = 0; k < WIN + ROWS_PER_THREAD - 1; ++k) col[k] = hs[q][ra + k][c];
#pragma unroll
    for (int j = 0; j < ROWS_PER_THREAD; ++j) {
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < WIN; ++k) acc = fma(prm.w[k], col[j + k], acc);
      m[j][q] = acc;
    }
  }
  double ssim_sum = 0.0, cs_sum = 0.0;
  {
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < ROWS_PER_THREAD; ++j) {
      const double mx = m[j][0], my = m[j][1];
      const double mxx = mx * mx, myy = my * my, mxy = mx * my;
      const double sxx = m[j][2] - mxx, syy = m[j][3] - myy, sxy = m[j][4] - mxy;
      const double cs_num = 2.0 * sxy + prm.c2, cs_den = (sxx + syy) + prm.c2;
      const double l_num = 2.0 * mxy + prm.c1, l_den = (mxx + myy) + prm.c1;
      const double cs = cs_num / cs_den;
      const double ss = (l_num * cs_num) / (l_den * cs_den);
      const bool valid = ra + j < out_rows && c < out_cols;      // select, not multiply: a NaN outside the map stays out
      ssim_sum = ssim_sum + (valid ? ss : 0.0);
      cs_sum = cs_sum + (valid ? cs : 0.0);
    }
  }

  const double t_sse = block_sum<NT>(sse, red);
  const double t_ssim = block_sum<NT>(ssim_sum, red);
  const double t_cs = block_sum<NT>(cs_sum, red);
  if (tid == 0) {
    double* s = slots + (size_t)slot * 3 * B + b;
    s[0] = t_sse;
    s[(size_t)B] = t_ssim;
    s[2 * (size_t)B] = t_cs;
  }
}

__global__ __launch_bounds__(256) void recon_finalize_kernel(const double* __restrict__ slots, double* __restrict__ out, int B,
                                                             int per_image, double count) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  double sse = 0.0, ssim = 0.0, cs = 0.0;
  for (int s = 0; s < per_image; ++s) {
    const double* p = slots + (size_t)s * 3 * B + b;
    sse += p[0];
    ssim += p[(size_t)B];
    cs += p[2 * (size_t)B];
  }
  out[(size_t)b * 3 + 0] = sse;
  out[(size_t)b * 3 + 1] = ssim / count;
  out[(size_t)b * 3 + 2] = cs / count;
}

template <int WIN>
void launch(const float* x, const float* y, double* slots, int B, int C, int H, int W, const Plan& p, const Params& prm,
            hipStream_t st) {
  hipLaunchKernelGGL(recon_kernel<WIN>, dim3((unsigned)p.blocks), dim3(NT), 0, st, x, y, slots, B, C, H, W, p.bands, p.tiles,
                     (int)p.per_image, prm);
}

}  // namespace

extern "C" size_t vg_recon_quality_workspace_bytes(int B, int C, int H, int W, int window) {
  Plan p;
  return dims_ok(B, C, H, W, window) && make_plan(B, C, H, W, window, p) ? p.bytes : 0;
}

extern "C" int vg_recon_quality(const float* x, const float* y, double* out, int B, int C, int H, int W, int window,
                                double sigma, double data_range, double k1, double k2, void* workspace,
                                size_t workspace_bytes, void* stream) {
  Plan p;
  if (!x || !y || !out || !workspace || !dims_ok(B, C, H, W, window) || !make_plan(B, C, H, W, window, p))
    return VG_ERR_BAD_ARG;
  if (!(sigma > 0.0) || !isfinite(sigma) || !(data_range > 0.0) || !isfinite(data_range) || !(k1 >= 0.0) || !isfinite(k1) ||
      !(k2 >= 0.0) || !isfinite(k2))
    return VG_ERR_BAD_ARG;
  if (((uintptr_t)workspace & 7u) != 0 || ((uintptr_t)out & 7u) != 0) return VG_ERR_BAD_ARG;
  if (workspace_bytes < p.bytes) return VG_ERR_WORKSPACE;

  Params prm;
  double sum = 0.0;
  for (int k = 0; k < MAX_WIN; ++k) {
    const double d = k - (window - 1) / 2;
    prm.w[k] = k < window ? exp(-(d * d) / (2.0 * sigma * sigma)) : 0.0;
    sum += prm.w[k];
  }
  for (int k = 0; k < MAX_WIN; ++k) prm.w[k] /= sum;
  prm.c1 = (k1 * data_range) * (k1 * data_range);
  prm.c2 = (k2 * data_range) * (k2 * data_range);

  hipStream_t st = (hipStream_t)stream;
  double* slots = (double*)workspace;
  switch (window) {
    case 3: launch<3>(x, y, slots, B, C, H, W, p, prm, st); break;
    case 5: launch<5>(x, y, slots, B, C, H, W, p, prm, st); break;
    case 7: launch<7>(x, y, slots, B, C, H, W, p, prm, st); break;
    case 9: launch<9>(x, y, slots, B, C, H, W, p, prm, st); break;
    default: launch<11>(x, y, slots, B, C, H, W, p, prm, st); break;
  }
  VG_CHECK_LAUNCH();
  hipLaunchKernelGGL(recon_finalize_kernel, dim3(cdiv(B, 256)), dim3(256), 0, st, (const double*)slots, out, B,
                     (int)p.per_image, (double)C * p.OH * p.OW);
  VG_CHECK_LAUNCH();
  return 0;
}
