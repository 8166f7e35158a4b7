// Differentiable augmentation of the discriminator's inputs (Zhao et al. 2020, "Differentiable Augmentation for
// Data-Efficient GAN Training") for gfx950: colour, translation, cutout, and the transpose of their linear part.
// DESIGN.md section 4.31, include/vaegan_hip.h "vg_diff_augment_*".
//
// Per image x[C][H][W] and its row u[0..7] of uniforms (decode(): the one place a uniform becomes a factor or an integer):
//   colour       b = u0 - 1/2, s = 2 u1, c = u2 + 1/2:  x1 = x + b;  x2 = (x1 - mean_C x1) s + mean_C x1;
//                x3 = (x2 - m) c + m  with m = mean_CHW x2 = mean_CHW x + b (saturation keeps a pixel's channel mean);
//   translation  y[c][i][j] = x3[c][i + t_r][j + t_c] inside the image, 0 outside;
//   cutout       0 where the row AND the column are cut -- on the translated image;
//   gate         u7 < p, else the output is a copy of the input.  p: a launch argument, or (the _dev entry points) a device
//                word the kernels read when they run -- the one vg_ada_update, the controller at the end of this file, moves.
// Given u the map is affine in x.  The backward is the transpose of its linear part and reads gy and u alone:
//   g3 = gy masked and shifted back;  g2 = c g3 + (1 - c) mean_CHW g3;  gx = s g2 + (1 - s) mean_C g2.
//
// Launches.  Only the colour step needs a sum over the whole image (of x forward, of g3 backward), so with it there are
// two launches each way and without it one:
//   sum     a workgroup per (image, chunk of SUM_CHUNK elements of the image's C H W): the chunk's sum in fp64 -- a thread
//           in a fixed order, the wavefront by shuffles, the four wavefronts in index order -- into the fixed workspace slot
//           [image][chunk].  An image of any size is covered: nothing assumes that one workgroup, or LDS, holds it.
//   apply   a thread per pixel position and all its C channels (the channel mean is then a sum in registers); every thread
//           adds its image's slots in index order (uniform loads: a 3 x 64 x 64 image has three).
// No floating-point atomic, every sum in a fixed order that depends on nothing but the image: the same bits on every run
// and wherever in a batch the image stands.  Without colour the outputs are copies and zeros: exact.  Masks are selects,
// not products: what is dropped is 0 whatever it held.  Both directions are capturable: no host read, no allocation.
#include "common.hpp"
#include "vaegan_hip.h"

#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int SUM_VECS = 4;                           // 16-byte units a thread of the sum pass adds
constexpr int SUM_CHUNK = NT * SUM_VECS * 4;          // elements of an image per sum workgroup (= per slot)
constexpr int PPT = 4;                                // pixel positions per thread of the apply pass
constexpr int MAX_C = VG_DIFF_AUGMENT_MAX_CHANNELS;

static_assert(SUM_CHUNK == VG_DIFF_AUGMENT_SUM_CHUNK, "the header states the chunk the slots are laid out by");

struct Plan {
  long long chw;
  int hw, chunks, tiles;            // per image: slots of the sum pass, workgroups of the apply pass
  long long sum_blocks, apply_blocks;
  size_t bytes;
};

bool dims_ok(int B, int C, int H, int W) { return B >= 1 && C >= 1 && C <= MAX_C && H >= 2 && W >= 2; }

// false: an image, a grid (image-major in grid.x) or the workspace would not fit its index type
bool make_plan(int B, int C, int H, int W, Plan& p) {
  const long long hw = (long long)H * W;
  p.chw = hw * C;
  if (p.chw > 0x7fffffffLL) return false;
  p.hw = (int)hw;
  p.chunks = (int)((p.chw + SUM_CHUNK - 1) / SUM_CHUNK);
  p.tiles = (int)((hw + NT * PPT - 1) / (NT * PPT));
  p.sum_blocks = (long long)p.chunks * B;
  p.apply_blocks = (long long)p.tiles * B;
  if (p.sum_blocks > 0x7fffffffLL || p.apply_blocks > 0x7fffffffLL) return false;
  p.bytes = ((size_t)p.sum_blocks * sizeof(double) + 255) / 256 * 256;
  return true;
}

// One image's transform, decoded from its row of uniforms.  The integer mappings are ONE fp32 multiply, floor, clamp.
struct Xf {
  bool open;
  float b, s, c;
  int tr, tc;                 // y[i][j] = x3[i + tr][j + tc]
  int r0, r1, c0, c1;         // cut rows r0..r1 and columns c0..c1 (r0 > r1: nothing is cut)
};

__device__ __forceinline__ int pick(float u, int n) { return min((int)floorf(u * (float)n), n - 1); }

__device__ __forceinline__ Xf decode(const float* __restrict__ u, int policy, float p, int H, int W) {
  Xf t;
  t.open = u[7] < p;
  t.b = u[0] - 0.5f;
  t.s = 2.f * u[1];
  t.c = u[2] + 0.5f;
  t.tr = t.tc = 0;
  if (policy & VG_AUGMENT_TRANSLATION) {
    const int rh = (H + 4) / 8, rw = (W + 4) / 8;              // int(H / 8 + 0.5)
    t.tr = pick(u[3], 2 * rh + 1) - rh;
    t.tc = pick(u[4], 2 * rw + 1) - rw;
  }
  t.r0 = t.c0 = 1;
  t.r1 = t.c1 = 0;
  if (policy & VG_AUGMENT_CUTOUT) {
    const int kh = (H + 1) / 2, kw = (W + 1) / 2;              // int(H / 2 + 0.5)
    const int orow = pick(u[5], H + 1 - (kh & 1)), ocol = pick(u[6], W + 1 - (kw & 1));
    t.r0 = max(orow - kh / 2, 0);
    t.r1 = min(orow - kh / 2 + kh - 1, H - 1);
    t.c0 = max(ocol - kw / 2, 0);
    t.c1 = min(ocol - kw / 2 + kw - 1, W - 1);
  }
  return t;
}

// whether output position (i, j) takes a source pixel (it is not cut and its source lies inside the image)
__device__ __forceinline__ bool kept(const Xf& t, int i, int j, int H, int W) {
  const bool cut = i >= t.r0 && i <= t.r1 && j >= t.c0 && j <= t.c1;
  const int si = i + t.tr, sj = j + t.tc;
  return !cut && si >= 0 && si < H && sj >= 0 && sj < W;
}

// ---- the sum pass: forward the chunk's sum of x, backward (BWD) of g3 = gy where the output position is kept ------------
template <bool BWD>
__global__ __launch_bounds__(NT) void sum_kernel(const float* __restrict__ v, const float* __restrict__ u,
                                                 double* __restrict__ slots, int H, int W, int hw, int chw, int chunks,
                                                 int policy, Word p) {
  __shared__ double red[NT / 64];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
  const Xf t = decode(u + (size_t)b * 8, policy, read_word(p), H, W);
  double s = 0.0;
  if (t.open) {                                         // (uniform over the workgroup; a closed image's slots are unread)
    const float* img = v + (size_t)b * chw;
    const int first = chunk * SUM_CHUNK;                // (chunk * SUM_CHUNK < chw <= 2^31 - 1)
    const bool vec = (((uintptr_t)(img + first)) & 15) == 0;
    auto term = [&](int e, float val) -> double {
      if constexpr (BWD) {
        const int pix = e % hw, i = pix / W, j = pix - i * W;
        return kept(t, i, j, H, W) ? (double)val : 0.0;
      } else {
        return (double)val;
      }
    };
    // a thread's elements and their order are the same on the 16-byte path and on the element path: the same bits
    // whatever the alignment of the image
#pragma unroll
    for (int k = 0; k < SUM_VECS; ++k) {
      const long long e0 = (long long)first + 4LL * (k * NT + tid);
      if (e0 + 3 < chw && vec) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(img + e0);
#pragma unroll
        for (int e = 0; e < 4; ++e) s += term((int)e0 + e, q[e]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e0 + e < chw) s += term((int)(e0 + e), img[e0 + e]);
      }
    }
  }
  const double tot = block_sum<NT>(s, red);
  if (tid == 0) slots[(size_t)b * chunks + chunk] = tot;
}

// an image's slots in index order (every thread the same loads: uniform)
__device__ __forceinline__ double image_sum(const double* __restrict__ slots, int b, int chunks) {
  const double* sl = slots + (size_t)b * chunks;
  double s = 0.0;
  for (int k = 0; k < chunks; ++k) s += sl[k];
  return s;
}

// ---- apply, forward: a thread per output position, all C channels ------------------------------------------------------
template <int C>
__global__ __launch_bounds__(NT) void fwd_kernel(const float* __restrict__ x, const float* __restrict__ u,
                                                 float* __restrict__ y, const double* __restrict__ slots, int H, int W,
                                                 int hw, int chunks, int tiles, int policy, Word p) {
  const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const Xf t = decode(u + (size_t)b * 8, policy, read_word(p), H, W);
  const size_t base = (size_t)b * C * hw;
  const bool colour = (policy & VG_AUGMENT_COLOR) != 0;
  float m = 0.f;
  if (colour && t.open) m = (float)(image_sum(slots, b, chunks) / ((double)C * (double)hw) + (double)t.b);
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const int pix = (tile * PPT + k) * NT + threadIdx.x;
    if (pix >= hw) break;
    if (!t.open) {
#pragma unroll
      for (int ch = 0; ch < C; ++ch) y[base + (size_t)ch * hw + pix] = x[base + (size_t)ch * hw + pix];
      continue;
    }
    const int i = pix / W, j = pix - i * W;
    float v[C];
    if (kept(t, i, j, H, W)) {
      const int src = (i + t.tr) * W + (j + t.tc);
#pragma unroll
      for (int ch = 0; ch < C; ++ch) v[ch] = x[base + (size_t)ch * hw + src];
      if (colour) {
        float sum = 0.f;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
          v[ch] += t.b;
          sum += v[ch];
        }
        const float mean = sum / (float)C;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
          const float x2 = fmaf(v[ch] - mean, t.s, mean);
          v[ch] = fmaf(x2 - m, t.c, m);
        }
      }
    } else {
#pragma unroll
      for (int ch = 0; ch < C; ++ch) v[ch] = 0.f;
    }
#pragma unroll
    for (int ch = 0; ch < C; ++ch) y[base + (size_t)ch * hw + pix] = v[ch];
  }
}

// ---- apply, backward: a thread per SOURCE position (i', j'), which output (i' - tr, j' - tc) read -- if it is kept ----------
template <int C>
__global__ __launch_bounds__(NT) void bwd_kernel(const float* __restrict__ gy, const float* __restrict__ u,
                                                 float* __restrict__ gx, const double* __restrict__ slots, int H, int W,
                                                 int hw, int chunks, int tiles, int policy, Word p) {
  const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const Xf t = decode(u + (size_t)b * 8, policy, read_word(p), H, W);
  const size_t base = (size_t)b * C * hw;
  const bool colour = (policy & VG_AUGMENT_COLOR) != 0;
  float rest = 0.f;                                     // (1 - c) mean_CHW g3: what every element of g2 gets
  if (colour && t.open) rest = (1.f - t.c) * (float)(image_sum(slots, b, chunks) / ((double)C * (double)hw));
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const int pix = (tile * PPT + k) * NT + threadIdx.x;
    if (pix >= hw) break;
    if (!t.open) {
#pragma unroll
      for (int ch = 0; ch < C; ++ch) gx[base + (size_t)ch * hw + pix] = gy[base + (size_t)ch * hw + pix];
      continue;
    }
    const int si = pix / W, sj = pix - si * W;
    const int i = si - t.tr, j = sj - t.tc;             // the one output position that read this source pixel
    const bool in = i >= 0 && i < H && j >= 0 && j < W;
    float g[C];
    if (in && kept(t, i, j, H, W)) {
#pragma unroll
      for (int ch = 0; ch < C; ++ch) g[ch] = gy[base + (size_t)ch * hw + (i * W + j)];
    } else {
#pragma unroll
      for (int ch = 0; ch < C; ++ch) g[ch] = 0.f;
    }
    if (colour) {
      float sum = 0.f;
#pragma unroll
      for (int ch = 0; ch < C; ++ch) {
        g[ch] = fmaf(t.c, g[ch], rest);                 // g2
        sum += g[ch];
      }
      const float side = (1.f - t.s) * (sum / (float)C);
#pragma unroll
      for (int ch = 0; ch < C; ++ch) g[ch] = fmaf(t.s, g[ch], side);
    }
#pragma unroll
    for (int ch = 0; ch < C; ++ch) gx[base + (size_t)ch * hw + pix] = g[ch];
  }
}

template <bool BWD>
int run(const float* in, const float* u, float* out, int B, int C, int H, int W, int policy, Word p, void* workspace,
        size_t workspace_bytes, hipStream_t st) {
  Plan pl;
  if (!in || !u || !out || in == out || !dims_ok(B, C, H, W) || !make_plan(B, C, H, W, pl)) return VG_ERR_BAD_ARG;
  // (a NaN p fails the comparison; with the word the host knows no p: whatever the word holds is compared with u7)
  if (policy < 1 || policy > 7 || !words_ok(p) || (is_float(p) && !(p.v >= 0.f && p.v <= 1.f))) return VG_ERR_BAD_ARG;
  const bool colour = (policy & VG_AUGMENT_COLOR) != 0;
  double* slots = nullptr;
  if (colour) {
    if (!workspace || ((uintptr_t)workspace & 7u) != 0) return VG_ERR_BAD_ARG;
    if (workspace_bytes < pl.bytes) return VG_ERR_WORKSPACE;
    slots = (double*)workspace;
    hipLaunchKernelGGL(sum_kernel<BWD>, dim3((unsigned)pl.sum_blocks), dim3(NT), 0, st, in, u, slots, H, W, pl.hw,
                       (int)pl.chw, pl.chunks, policy, p);
    VG_CHECK_LAUNCH();
  }
  auto apply = [&](auto cc) {
    constexpr int CC = decltype(cc)::value;
    if constexpr (BWD)
      hipLaunchKernelGGL(bwd_kernel<CC>, dim3((unsigned)pl.apply_blocks), dim3(NT), 0, st, in, u, out, (const double*)slots,
                         H, W, pl.hw, pl.chunks, pl.tiles, policy, p);
    else
      hipLaunchKernelGGL(fwd_kernel<CC>, dim3((unsigned)pl.apply_blocks), dim3(NT), 0, st, in, u, out, (const double*)slots,
                         H, W, pl.hw, pl.chunks, pl.tiles, policy, p);
  };
  switch (C) {
    case 1: apply(IntC<1>{}); break;
    case 2: apply(IntC<2>{}); break;
    case 3: apply(IntC<3>{}); break;
    default: apply(IntC<4>{}); break;
  }
  VG_CHECK_LAUNCH();
  return 0;
}

// ---- the controller of p (Karras et al. 2020, section 3): ONE workgroup -------------------------
// The sign statistic is an integer: a thread's elements, the wavefront by shuffles, the four wavefronts through LDS --
// exact, so no order can show.  Thread 0 then owns the eight words: plain loads and stores, nobody else touches them.
static_assert(sizeof(vg_ada_state) == 32, "eight device words");

__global__ __launch_bounds__(NT) void ada_kernel(const float* __restrict__ d, int B, float threshold, float target,
                                                 float rate, int interval, vg_ada_state* __restrict__ st) {
  __shared__ int red[NT / 64];
  int s = 0;
  for (int i = threadIdx.x; i < B; i += NT) {
    const float v = d[i];
    s += (int)(v > threshold) - (int)(v < threshold);   // (a NaN or a tie: both comparisons fail -- 0, and counted)
  }
  const int tot = block_sum<NT>(s, red);
  if (threadIdx.x != 0) return;
  float p = st->p;
  int sign_sum = st->sign_sum + tot, count = st->count + B, calls = st->calls + 1;
  if (calls >= interval) {                              // (>=, not ==: a state restored under a larger interval still adjusts)
    const float rt = (float)sign_sum / (float)count;
    const int dir = (int)(rt > target) - (int)(rt < target);
    // one rounded product, one rounded sum, never an FMA: three fp32 operations anyone can restate
    const float step = __fmul_rn((float)count, rate);
    if (dir != 0) p = __fadd_rn(p, dir > 0 ? step : -step);
    p = p < 0.f ? 0.f : (p > 1.f ? 1.f : p);            // (a NaN p stays a NaN: it closes every image and shows in the word)
    st->rt = rt;
    st->adjustments += 1;
    sign_sum = count = calls = 0;
  }
  st->p = p;
  st->sign_sum = sign_sum;
  st->count = count;
  st->calls = calls;
  st->reserved[0] = st->reserved[1] = 0;
}

}  // namespace

extern "C" size_t vg_diff_augment_workspace_bytes(int B, int C, int H, int W) {
  Plan pl;
  return dims_ok(B, C, H, W) && make_plan(B, C, H, W, pl) ? pl.bytes : 0;
}

extern "C" int vg_diff_augment_fwd(const float* x, const float* u, float* y, int B, int C, int H, int W, int policy, float p,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  return run<false>(x, u, y, B, C, H, W, policy, word(p), workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int vg_diff_augment_bwd(const float* gy, const float* u, float* gx, int B, int C, int H, int W, int policy, float p,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  return run<true>(gy, u, gx, B, C, H, W, policy, word(p), workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int vg_diff_augment_fwd_dev(const float* x, const float* u, float* y, int B, int C, int H, int W, int policy,
                                       const float* p_dev, void* workspace, size_t workspace_bytes, void* stream) {
  return run<false>(x, u, y, B, C, H, W, policy, word_at(p_dev), workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int vg_diff_augment_bwd_dev(const float* gy, const float* u, float* gx, int B, int C, int H, int W, int policy,
                                       const float* p_dev, void* workspace, size_t workspace_bytes, void* stream) {
  return run<true>(gy, u, gx, B, C, H, W, policy, word_at(p_dev), workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int vg_ada_update(const float* d_real, int B, float threshold, float target, float rate, int interval, void* state,
                             void* stream) {
  if (!d_real || !state || ((uintptr_t)state & 3u) != 0 || B < 1 || interval < 1) return VG_ERR_BAD_ARG;
  if (!isfinite(target) || !isfinite(rate) || rate < 0.f || threshold != threshold) return VG_ERR_BAD_ARG;
  hipLaunchKernelGGL(ada_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, d_real, B, threshold, target, rate, interval,
                     (vg_ada_state*)state);
  VG_CHECK_LAUNCH();
  return 0;
}
